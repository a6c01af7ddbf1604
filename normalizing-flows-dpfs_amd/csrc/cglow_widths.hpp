// cglow_widths.hpp -- THE list of conditional-GLOW hidden sizes (--x_hidden_channels XH,
// --x_hidden_size XS, --y_hidden_channels YH) the width-general forward kernel
// (cglow_wide.hip) takes, and the packed parameter layout of
// nfdpf.pack.cglow_levels_tensors at those sizes: cg::Cond<OUT> and cgl::AffL<C, G>
// (cglow.hpp, cglow_levels.hpp) with the three sizes as values instead of constants.  Every
// combination of the listed values is supported, at K in 1..4, L in 1..2, either learn_top.
// A further value is one more X(...) entry here (XS a multiple of 4: the MFMA k-steps); the
// kernel's LDS areas are sized by the largest listed values and static_assert their fit.
// resize_x's 16 hidden channels are fixed by the reference (nf/cglow/modules.py), not a flag.
#pragma once

#include "cglow_levels.hpp"

#define NFDPF_CGLOW_XH(X) X(8) X(16)
#define NFDPF_CGLOW_XS(X) X(16) X(32)
#define NFDPF_CGLOW_YH(X) X(8) X(16) X(32)

namespace nfdpf {
namespace cgw {

#define NFDPF_W_OR(W) || v == W
#define NFDPF_W_MAX(W) , W
#define NFDPF_W_STR(W) " " #W
constexpr int max_of(int a) { return a; }
template <class... T>
constexpr int max_of(int a, int b, T... r) { return max_of(a > b ? a : b, r...); }
constexpr bool xh_ok(int v) { return false NFDPF_CGLOW_XH(NFDPF_W_OR); }
constexpr bool xs_ok(int v) { return false NFDPF_CGLOW_XS(NFDPF_W_OR); }
constexpr bool yh_ok(int v) { return false NFDPF_CGLOW_YH(NFDPF_W_OR); }
constexpr int kMaxXH = max_of(0 NFDPF_CGLOW_XH(NFDPF_W_MAX));
constexpr int kMaxXS = max_of(0 NFDPF_CGLOW_XS(NFDPF_W_MAX));
constexpr int kMaxYH = max_of(0 NFDPF_CGLOW_YH(NFDPF_W_MAX));
constexpr const char *kWidthsStr = "x_hidden_channels in {" NFDPF_CGLOW_XH(NFDPF_W_STR) " }, x_hidden_size in {"
    NFDPF_CGLOW_XS(NFDPF_W_STR) " }, y_hidden_channels in {" NFDPF_CGLOW_YH(NFDPF_W_STR) " }";
#undef NFDPF_W_OR
#undef NFDPF_W_MAX
#undef NFDPF_W_STR

constexpr bool widths_ok(int xh, int xs, int yh) { return xh_ok(xh) && xs_ok(xs) && yh_ok(yh); }

// conditioning net (x_Con: three 2x2-stride convs 3 -> XH -> XH -> XH; x_Linear XH -> XS -> XS -> out)
struct Cond {
  int c0w, c0b, c2w, c2b, c4w, c4b, l0w, l0b, l2w, l2b, l4w, l4b, size;
  constexpr Cond(int xh, int xs, int out)
      : c0w(0), c0b(c0w + xh * 3 * 4), c2w(c0b + xh), c2b(c2w + xh * xh * 4), c4w(c2b + xh), c4b(c4w + xh * xh * 4),
        l0w(c4b + xh), l0b(l0w + xs * xh), l2w(l0b + xs), l2b(l2w + xs * xs), l4w(l2b + xs), l4b(l4w + out * xs),
        size(l4b + out) {}
};

// CondAffineCoupling on C channels of a G x G grid with f's hidden width yh (cgl::AffL)
struct Aff {
  int r0w, r0b, r2w, r2b, r4w, r4b, f0w, f0ab, f0al, f2w, f2ab, f2al, f4w, f4b, f4l, f4nb, size;
  constexpr Aff(int yh, int C, int G)
      : r0w(0), r0b(r0w + 16 * 3 * 9), r2w(r0b + 16), r2b(r2w + (C / 2) * 16 * (8 / G) * (8 / G)), r4w(r2b + C / 2),
        r4b(r4w + (C / 2) * (C / 2) * 9), f0w(r4b + C / 2), f0ab(f0w + yh * C * 9), f0al(f0ab + yh), f2w(f0al + yh),
        f2ab(f2w + yh * yh), f2al(f2ab + yh), f4w(f2al + yh), f4b(f4w + C * yh * 9), f4l(f4b + C), f4nb(f4l + C),
        size(f4nb + C) {}
};

// one CondGlowStep on C channels: actnorm net (2 C outputs), 1x1-conv net (C C), the coupling
struct Step {
  Cond A, I;
  Aff F;
  int offI, offF, size;
  constexpr Step(int xh, int xs, int yh, int C, int G)
      : A(xh, xs, 2 * C), I(xh, xs, C * C), F(yh, C, G), offI(A.size), offF(A.size + I.size),
        size(A.size + I.size + F.size) {}
};

// floats of the blob: K level-1 steps; at L = 2 Split2d (cgl::kSplit) and K level-2 steps;
// with learn_top [new_mean | new_logs]
constexpr int64_t wide_size(int K, int L, bool top, int xh, int xs, int yh) {
  return (int64_t)K * Step(xh, xs, yh, cg::kC, 4).size +
         (L == 2 ? cgl::kSplit + (int64_t)K * Step(xh, xs, yh, cgl::kC2, 2).size : 0) + (top ? 2 * cgl::top_n(L) : 0);
}

static_assert(Step(cg::kXH, cg::kXS, cg::kYH, cg::kC, 4).size == 7980 && Step(cg::kXH, cg::kXS, cg::kYH, cgl::kC2, 2).size == 21168 &&
                  cgl::kSplit == 660,
              "the default sizes give the layout of cglow.hpp / cglow_levels.hpp");
static_assert(Step(cg::kXH, cg::kXS, cg::kYH, cg::kC, 4).offF == cg::kOffF && Aff(cg::kYH, cg::kC, 4).f4nb == cg::Aff::f4nb &&
                  Cond(cg::kXH, cg::kXS, 24).l4w == cg::CondA::l4w,
              "the default sizes give the offsets of cglow.hpp");
static_assert(wide_size(1, 1, false, 16, 32, 16) == 18300 && wide_size(1, 1, false, 16, 16, 8) == 11548 &&
                  wide_size(2, 2, true, 8, 16, 32) == 94476 && wide_size(1, 2, true, 16, 32, 32) == 71696 &&
                  wide_size(2, 2, true, 8, 16, 8) == cgl::levels_size(2, 2, true),
              "parameter counts of nfdpf.pack.cglow_levels_tensors");

}  // namespace cgw
}  // namespace nfdpf
