// cglow.hpp -- the packed parameter layout of the conditional-GLOW measurement
// (nfdpf.pack.cglow_tensors; nf/cglow/modules.py), shared by the forward kernel (cglow.hip)
// and its backward (cglow_bwd.hip).
#pragma once

#include "flows.hpp"

namespace nfdpf {
namespace cg {

constexpr int kE = 192;       // particle / frame encoding (3 x 8 x 8)
constexpr int kXH = 8;        // x_hidden_channels (arguments.py:63)
constexpr int kXS = 16;       // x_hidden_size (arguments.py:64)
constexpr int kC = 12;        // y channels after the squeeze
constexpr int kCh = 6;        // coupling half
constexpr int kYH = 8;        // y_hidden_channels

// ---- packed parameter layout (nfdpf.pack.cglow_tensors), floats, per CondGlowStep ----
// conditioning net (x_Con: three 2x2-stride convs, x_Linear: 8->16->16->OUT)
template <int OUT>
struct Cond {
  static constexpr int c0w = 0, c0b = c0w + kXH * 3 * 4, c2w = c0b + kXH, c2b = c2w + kXH * kXH * 4,
                       c4w = c2b + kXH, c4b = c4w + kXH * kXH * 4, l0w = c4b + kXH, l0b = l0w + kXS * kXH,
                       l2w = l0b + kXS, l2b = l2w + kXS * kXS, l4w = l2b + kXS, l4b = l4w + OUT * kXS,
                       size = l4b + OUT;
};
using CondA = Cond<2 * kC>;    // actnorm: (logs, bias)
using CondI = Cond<kC * kC>;   // 1x1 conv weight
struct Aff {                   // CondAffineCoupling
  static constexpr int r0w = 0, r0b = r0w + 16 * 3 * 9, r2w = r0b + 16, r2b = r2w + kCh * 16 * 4,
                       r4w = r2b + kCh, r4b = r4w + kCh * kCh * 9, f0w = r4b + kCh,
                       f0ab = f0w + kYH * kC * 9, f0al = f0ab + kYH, f2w = f0al + kYH,
                       f2ab = f2w + kYH * kYH, f2al = f2ab + kYH, f4w = f2al + kYH,
                       f4b = f4w + kC * kYH * 9, f4l = f4b + kC, f4nb = f4l + kC, size = f4nb + kC;
};
constexpr int kOffA = 0, kOffI = CondA::size, kOffF = kOffI + CondI::size;
constexpr int kStep = kOffF + Aff::size;
constexpr int kMaxK = 4;  // flow depths the kernels take: the blob holds K steps, step k at k * kStep

}  // namespace cg

// Host: the grid of a persistent kernel that deals `tiles` tiles to its workgroups: exactly the
// resident workgroups (CUs x wgs_per_cu; 256 CUs where the device does not say) -- more would
// start a second, late round of workgroups and leave the tail unbalanced -- and no more than tiles.
inline int persistent_grid(int64_t tiles, int wgs_per_cu) {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
  }
  const int64_t resident = (int64_t)cus * wgs_per_cu;
  return (int)(tiles < resident ? tiles : resident);
}

// cglow.hip, for the K > 1 backward (cglow_bwd.hip): the first `nsteps` steps' outputs
int cglow_forward_mid(const float *pe, const float *glow, int nsteps, const float *enc, int64_t enc_rs,
                      const float *x, int64_t x_rs, int B, int N, const float *xin, float *zmid, hipStream_t st);

// cglow_bwd.hip, for the chains whose top Gaussian is taken elsewhere (cglow_levels_bwd.hip): the
// K level-1 steps from K-1 down to 0, every one a !TOP launch of cglow_bwd_kernel.  part: the
// measurement form (pe, x particles, enc rows, g_up = g_lik) or the flow form (x = the condition
// [M, 192], enc = y [M, 192], g_up = g_nll), as the arguments of that kernel.  zmid: the steps'
// outputs z_0 .. z_{K-2} ([M, 192] each, (12, 4, 4)).  gzb / gxb: two [M, 192] hand-over buffers
// each; on entry gzb[1] holds dL/dz_{K-1} and gxb[1] the condition's gradient so far.  partial:
// cglow_bwd_partial_floats(M) floats.  g_glow: the K steps' gradients; g_pe may be null.
int64_t cglow_bwd_partial_floats(int64_t M);
int cglow_bwd_below(bool part, const float *pe, const float *glow, int K, const float *zmid, const float *enc,
                    int64_t enc_rs, const float *x, int64_t x_rs, int B, int N, const float *g_up, int64_t gup_rs,
                    float *const *gzb, float *const *gxb, float *g_y, float *g_x, float *g_glow, float *g_pe,
                    float *partial, hipStream_t st);
}  // namespace nfdpf
