// cglow_levels.hpp -- the packed parameter layout of the conditional GLOW with L in 1..2 levels
// and an optional learnt top prior (nfdpf.pack.cglow_levels_tensors), read by cglow_levels.hip.
//
//   [ K level-1 steps, cg::kStep floats each: the layout of cglow.hpp            ]
//   [ L = 2: Split2d conv 6 -> 12, tap-major [3][3][6][12], then its 12 biases   ]
//   [ L = 2: K level-2 steps, kStep2 floats each (y_size 24 x 2 x 2)             ]
//   [ learn_top: new_mean | new_logs, kTopN(L) floats each                       ]
#pragma once

#include "cglow.hpp"

namespace nfdpf {
namespace cgl {
using namespace cg;

// CondAffineCoupling on C channels (half CH = C / 2) of a G x G grid: resize_x is conv 3 -> 16
// (3x3 at 8x8), Conv2dResize 16 -> CH with an R x R kernel, stride R (R = 8 / G), conv CH -> CH
// (3x3 at G x G); f is C -> 8 (3x3), 8 -> 8 (1x1), 8 -> C (3x3).  Convolutions tap-major,
// output channel fastest, as cg::Aff (= AffL<12, 4>).
template <int C, int G>
struct AffL {
  static constexpr int CH = C / 2, R = 8 / G;
  static constexpr int r0w = 0, r0b = r0w + 16 * 3 * 9, r2w = r0b + 16, r2b = r2w + CH * 16 * R * R,
                       r4w = r2b + CH, r4b = r4w + CH * CH * 9, f0w = r4b + CH, f0ab = f0w + kYH * C * 9,
                       f0al = f0ab + kYH, f2w = f0al + kYH, f2ab = f2w + kYH * kYH, f2al = f2ab + kYH,
                       f4w = f2al + kYH, f4b = f4w + C * kYH * 9, f4l = f4b + C, f4nb = f4l + C,
                       size = f4nb + C;
};
static_assert(AffL<kC, 4>::size == Aff::size && AffL<kC, 4>::f4nb == Aff::f4nb && AffL<kC, 4>::r4w == Aff::r4w,
              "level 1 is the layout of cglow.hpp");

// one CondGlowStep on C channels: actnorm net Cond<2 C>, 1x1-conv net Cond<C C>, AffL<C, G>
template <int C, int G>
struct StepL {
  using A = Cond<2 * C>;
  using I = Cond<C * C>;
  using F = AffL<C, G>;
  static constexpr int offA = 0, offI = A::size, offF = offI + I::size, size = offF + F::size;
};
using Step1 = StepL<kC, 4>;
using Step2 = StepL<2 * kC, 2>;
static_assert(Step1::size == kStep && Step1::offI == kOffI && Step1::offF == kOffF, "level 1 is cg::kStep");
static_assert(Step2::size == 21168, "level-2 step: Cond<48> + Cond<576> + AffL<24, 2>");

constexpr int kC2 = 2 * kC;                           // level-2 channels (24 x 2 x 2)
constexpr int kSplitW = 2 * kCh * kCh * 9;            // Split2d conv 6 -> 12
constexpr int kSplit = kSplitW + 2 * kCh;             // + bias: 660
constexpr int kMaxL = 2;
constexpr int top_n(int L) { return L == 2 ? kC2 * 4 : kE; }  // floats of the final z: 96 / 192
constexpr int64_t levels_size(int K, int L, bool top) {
  return (int64_t)K * kStep + (L == 2 ? kSplit + (int64_t)K * Step2::size : 0) + (top ? 2 * top_n(L) : 0);
}
static_assert(levels_size(1, 2, true) == 30000 && levels_size(2, 2, true) == 59148, "parameter counts at L = 2");

}  // namespace cgl

// cglow_levels.hip, for the backward (cglow_levels_bwd.hip): one forward launch that leaves every
// step's output in zmid -- the K level-1 outputs [k][M][192], then at L = 2 the level-2 inputs /
// outputs [k][M][96], k = 0 .. K (k = K the final z).  Arguments as cglow_forward_mid.
int cglow_levels_forward_mid(const float *pe, const float *glow, int K, int L, const float *enc, int64_t enc_rs,
                             const float *x, int64_t x_rs, int B, int N, const float *xin, float *zmid,
                             hipStream_t st);
}  // namespace nfdpf
