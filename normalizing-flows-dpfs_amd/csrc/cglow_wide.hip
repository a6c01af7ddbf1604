// cglow_wide.hip -- the conditional-GLOW measurement at the hidden sizes of cglow_widths.hpp
// (--x_hidden_channels, --x_hidden_size, --y_hidden_channels) and any --y_bins, forward only, one
// launch per call.  It computes what cglow_levels_kernel (cglow_levels.hip) computes -- particle
// encoder or a given x, squeeze, K level-1 steps, at L = 2 Split2d + squeeze + K level-2 steps,
// the top Gaussian, nll -- with the three sizes as run-time values under the compile-time
// maxima of cglow_widths.hpp, and with logdet0 = -log(y_bins) 192 passed in by the host.  The
// default sizes at 256 bins stay on cglow.hip / cglow_levels.hip, whose lane maps have 8 / 16 / 8
// built in; this kernel is not tuned.
//
// Mapping: one workgroup = 256 threads = a tile of 16 particles, persistent over tiles, with
// workgroup barriers between phases; no flags, spin waits, inter-workgroup hand-offs or atomics.
// A convolution layer is a list of jobs (output channel, 64 (particle, position) pairs) dealt to
// the four waves round-robin: the output channel is wave-uniform, so weights are scalar loads,
// and activations lie channel-major in LDS ([channel][pair]), so a wave reads and writes runs of
// consecutive floats.  The conditioning nets' last layer (XS -> 2 C and XS -> C C) is f32 MFMA
// 16x16x4 with the 16 particles as M and XS / 4 k-steps.  Every output is one fmaf chain in a
// fixed order, and sums over a particle go through LDS and are combined in a fixed order by the
// particle's 16 lanes, so a particle's bits do not depend on its place in the batch or on M.
//
// LDS (102 KB, one workgroup per CU): xs 12 KB, y 12 KB, actnorm 3 KB, v1 4 KB and one 70 KB area
// `u`.  What sizes `u` is the coupling at y_hidden_channels 32: resize_x's first conv at 8 x 8
// (16 x 16 x 64 floats = 64 KB) next to its second (6 KB), and later f's two hidden grids (2 x 32
// KB) next to the coupling's condition (6 KB); the conditioning nets' activations (46 KB at
// x_hidden_channels 16) and the per-particle C x C matrix (36 KB) take the same area in turn.
//
// What does not depend on the sizes -- lane helpers, actnorm_invconv, split_squeeze, the tile's
// prologue and tail -- is cglow_tile.hpp's, shared with cglow_levels.hip.
#include <cmath>

#include "cglow_tile.hpp"
#include "cglow_widths.hpp"

namespace nfdpf {
namespace cgw {
using namespace cgl;  // kE, kC, kCh, kC2, kSplit*, kPe*, kMaxK, kMaxL, top_n
using namespace cgt;  // the tile frame: kTileP, kThreads, kWmStride, the lane helpers

constexpr int kWaves = kThreads / 64;
constexpr int kWgs = 1;                   // resident workgroups per CU (LDS)
constexpr int kPairs1 = kTileP * 16;      // (particle, position) pairs of a 4 x 4 grid
// the conditioning nets' activations inside `u`, [net][channel][pair] (dead before the last
// layer writes the matrix): x_Con's three convs, x_Linear's first layer
constexpr int kCv1 = 0, kCv2 = kCv1 + 2 * kMaxXH * kPairs1, kCv3 = kCv2 + 2 * kMaxXH * kTileP * 4,
              kV0 = kCv3 + 2 * kMaxXH * kTileP, kCondEnd = kV0 + 2 * kMaxXS * kTileP;
// the coupling's grids inside `u` (the matrix is dead by then), sized by level 1 (16 positions):
// r0 (16 channels at 8 x 8) | r2; then fin | h0 | h1 with h1's tail over the dead r2; then the
// log-scales over the dead fin
constexpr int kR0 = 0, kR2 = kR0 + 16 * kTileP * 64, kFin = 0, kH0 = kFin + kCh * kPairs1,
              kH1 = kH0 + kMaxYH * kPairs1, kLs = 0, kUEnd = kH1 + kMaxYH * kPairs1;
static_assert(kR2 + kCh * kPairs1 <= kUEnd && kH0 <= kR2, "r2 outlives r0 only, and fin / h0 do not reach it");

struct Lds {
  float xs[kTileP][kE + 1];           // the condition x, [c][8][8]
  float y[kTileP][kE + 1];            // the flow's state, [c][position] (192 or 96 floats)
  float an[kTileP][2 * kC2 + 1];      // actnorm (logs | bias)
  float v1[kTileP][2 * kMaxXS + 1];   // x_Linear's second layer (actnorm net | 1x1-conv net)
  float ld[kTileP];                   // the log-dets so far
  float pxy[kTileP][2];
  int row[kTileP];
  float u[kUEnd];
};
static_assert(kTileP * kWmStride <= kUEnd && kCondEnd <= kUEnd, "the matrix and the conditioning nets fit in u");
static_assert(kTileP * (kPeH1 + kPeH2) <= kUEnd && kTileP * kE <= kUEnd && 2 * kTileP * 16 * kCh <= kUEnd,
              "the encoder's hidden layers, the top Gaussian's terms and Split2d's buffers fit in u");
static_assert(sizeof(Lds) * kWgs <= 160 * 1024, "one workgroup per CU");
static_assert(kMaxXS % 4 == 0, "whole MFMA k-steps");

typedef float f4 __attribute__((ext_vector_type(4)));

static __shared__ Lds S;
struct Tile {  // cglow_tile.hpp's view of this kernel: its S, and split_squeeze's two areas in S.u
  static __device__ __forceinline__ Lds &lds() { return S; }
  static constexpr int kSplitA = 0, kSplitB = kTileP * 16 * kCh;
};

// f(o, pair) for every output channel o < nout and pair < npairs (a multiple of 64): jobs of one
// channel and 64 pairs, dealt to the waves round-robin; o is wave-uniform
template <class F>
__device__ __forceinline__ void for_jobs(int npairs, int nout, int tid, F &&f) {
  const int l = tid & 63, w = uni(tid >> 6), nch = npairs >> 6;
#pragma unroll 1
  for (int j = w; j < nch * nout; j += kWaves) {
    const int o = j / nch;
    f(o, (j - o * nch) * 64 + l);
  }
}

// The two conditioning nets of a step (x_Con: three 2x2 stride-2 convs; x_Linear XH -> XS -> XS
// -> OUT, tanh) -> S.an (2 C) and the C x C matrix in S.u.  `on` counts the outputs of both
// nets: net on / width, output on % width.
template <int C>
__device__ __noinline__ void cond_nets(const float *__restrict__ gA, const float *__restrict__ gI, int xh_, int xs_,
                                       int tid) {
  const int xh = uni(xh_), xs = uni(xs_);
  const Cond A(xh, xs, 2 * C), I(xh, xs, C * C);  // the same offsets up to l4w
  float *cv1 = S.u + kCv1, *cv2 = S.u + kCv2, *cv3 = S.u + kCv3, *v0 = S.u + kV0;
  cfloat *GA = uptr(gA), *GI = uptr(gI);
  const int l = tid & 63, w = uni(tid >> 6);
  {  // conv 3 -> XH, 8x8 -> 4x4: wave w = the pairs (particle, 4x4 position) 64 w .., all outputs
    const int p = tid >> 4, q = tid & 15, qi = q >> 2, qj = q & 3;
    float in[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) in[k] = S.xs[p][(k >> 2) * 64 + (2 * qi + ((k >> 1) & 1)) * 8 + 2 * qj + (k & 1)];
#pragma unroll 1
    for (int on = 0; on < 2 * xh; ++on) {
      const int net = on >= xh, o = on - net * xh;
      cfloat *G = net ? GI : GA;
      float acc = G[A.c0b + o];
#pragma unroll
      for (int k = 0; k < 12; ++k) acc = fmaf(G[A.c0w + k * xh + o], in[k], acc);
      cv1[on * kPairs1 + tid] = relu(acc);
    }
  }
  __syncthreads();
  // conv XH -> XH, 4x4 -> 2x2: lane = (particle, 2x2 position), 64 pairs; k = (input, kh, kw)
  for_jobs(kTileP * 4, 2 * xh, tid, [&](int on, int pair) {
    const int net = on >= xh, o = on - net * xh, p = pair >> 2, pi = (pair >> 1) & 1, pj = pair & 1;
    cfloat *G = net ? GI : GA;
    const float *src = cv1 + net * xh * kPairs1 + p * 16 + 2 * pi * 4 + 2 * pj;
    float acc = G[A.c2b + o];
#pragma unroll 4
    for (int k = 0; k < 4 * xh; ++k)
      acc = fmaf(G[A.c2w + o * 4 * xh + k], src[(k >> 2) * kPairs1 + ((k >> 1) & 1) * 4 + (k & 1)], acc);
    cv2[on * (kTileP * 4) + pair] = relu(acc);
  });
  __syncthreads();
  // conv XH -> XH, 2x2 -> 1x1, then x_Linear's first two layers: one (output, particle) a thread
  for (int i = tid; i < kTileP * 2 * xh; i += kThreads) {
    const int p = i & 15, on = i >> 4, net = on >= xh, o = on - net * xh;
    const float *G = net ? gI : gA;
    float acc = G[A.c4b + o];
    for (int k = 0; k < 4 * xh; ++k)
      acc = fmaf(G[A.c4w + o * 4 * xh + k], cv2[(net * xh + (k >> 2)) * (kTileP * 4) + p * 4 + (k & 3)], acc);
    cv3[on * kTileP + p] = relu(acc);
  }
  __syncthreads();
  for (int i = tid; i < kTileP * 2 * xs; i += kThreads) {
    const int p = i & 15, on = i >> 4, net = on >= xs, o = on - net * xs;
    const float *G = net ? gI : gA;
    float acc = G[A.l0b + o];
    for (int k = 0; k < xh; ++k) acc = fmaf(G[A.l0w + o * xh + k], cv3[(net * xh + k) * kTileP + p], acc);
    v0[on * kTileP + p] = relu(acc);
  }
  __syncthreads();
  for (int i = tid; i < kTileP * 2 * xs; i += kThreads) {
    const int p = i & 15, on = i >> 4, net = on >= xs, o = on - net * xs;
    const float *G = net ? gI : gA;
    float acc = G[A.l2b + o];
    for (int k = 0; k < xs; ++k) acc = fmaf(G[A.l2w + o * xs + k], v0[(net * xs + k) * kTileP + p], acc);
    S.v1[p][on] = relu(acc);
  }
  __syncthreads();  // cv1 .. v0 are dead: the matrix takes their place
  // last layer + tanh as f32 MFMA 16x16x4 tiles (an exact k-ordered fmaf chain): M = the 16
  // particles, N = 16 outputs per tile, XS / 4 k-steps; lane l feeds A[l % 16][4 s + l / 16] and
  // B[4 s + l / 16][l % 16] and gets C rows 4 (l / 16) + i, column l % 16.  Tiles are dealt to
  // the waves round-robin.
  constexpr int NA = 2 * C, NI = C * C, TA = (NA + 15) / 16, NTILE = TA + NI / 16;
  static_assert(NI % 16 == 0, "whole tiles");
  {
    const int r = l & 15, kk = l >> 4, nks = xs >> 2;
#pragma unroll 1
    for (int job = w; job < NTILE; job += kWaves) {
      const bool isI = job >= TA;
      const int n = (isI ? job - TA : job) * 16 + r;
      const bool ok = n < (isI ? NI : NA);
      const int nn = ok ? n : 0;
      const float *G = (isI ? gI : gA) + A.l4w + nn * xs + kk;
      const float *a = &S.v1[r][(isI ? xs : 0) + kk];
      const float bias = isI ? gI[I.l4b + nn] : gA[A.l4b + nn];
      f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
      for (int s2 = 0; s2 < nks; ++s2)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * s2], ok ? G[4 * s2] : 0.f, acc, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float t = tanhf(acc[i] + bias);
        if (ok) {
          if (isI)
            S.u[(4 * kk + i) * kWmStride + n] = t;
          else
            S.an[4 * kk + i][n] = t;
        }
      }
    }
  }
  __syncthreads();
}

// cond-affine coupling of S.y in place; S.ld += sum log scale.  Every layer is for_jobs over its
// output channels and the tile's NP = 16 HW (particle, position) pairs; grids are [channel][pair].
template <int C, int G>
__device__ __noinline__ void coupling(const float *__restrict__ Fp, int yh_, int tid) {
  constexpr int HW = G * G, R = 8 / G, CH = C / 2, NP = kTileP * HW;
  static_assert(NP % 64 == 0 && CH * NP <= kCh * kPairs1, "whole jobs; level 1 sizes the grids");
  const int yh = uni(yh_);
  const Aff A(yh, C, G);
  float *r0 = S.u + kR0, *r2 = S.u + kR2, *fin = S.u + kFin, *h0 = S.u + kH0, *h1 = S.u + kH1, *ls = S.u + kLs;
  cfloat *F = uptr(Fp);
  {  // resize_x: conv 3 -> 16 (3x3, pad 1, at 8x8) ReLU; a wave takes 64 (particle, 8x8 position)
     // pairs at a time, their 27 inputs in registers, and all 16 outputs
    const int l = tid & 63, w = uni(tid >> 6);
#pragma unroll 1
    for (int chunk = w; chunk < kTileP; chunk += kWaves) {  // (64 positions: chunk = particle)
      const int r = l >> 3, s = l & 7;
      float in[27];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int rr = r + t / 3 - 1, ss = s + t % 3 - 1;
        const bool inb = rr >= 0 && rr < 8 && ss >= 0 && ss < 8;
        const float *xr = &S.xs[chunk][inb ? rr * 8 + ss : 0];
#pragma unroll
        for (int c = 0; c < 3; ++c) in[t * 3 + c] = inb ? xr[c * 64] : 0.f;
      }
#pragma unroll 2
      for (int o = 0; o < 16; ++o) {
        float h = F[A.r0b + o];
#pragma unroll
        for (int k = 0; k < 27; ++k) h = fmaf(F[A.r0w + k * 16 + o], in[k], h);
        r0[(o * kTileP + chunk) * 64 + l] = relu(h);
      }
    }
  }
  __syncthreads();
  // the R x R stride-R conv 16 -> CH, ReLU
  for_jobs(NP, CH, tid, [&](int o, int pair) {
    const int p = pair / HW, pos = pair % HW, pi = pos / G, pj = pos % G;
    const float *src = r0 + p * 64 + R * pi * 8 + R * pj;
    float acc = F[A.r2b + o];
#pragma unroll 1
    for (int ab = 0; ab < R * R; ++ab) {
#pragma unroll
      for (int ci = 0; ci < 16; ++ci)
        acc = fmaf(F[A.r2w + (ab * 16 + ci) * CH + o], src[ci * kTileP * 64 + (ab / R) * 8 + ab % R], acc);
    }
    r2[o * NP + pair] = relu(acc);
  });
  __syncthreads();
  // conv CH -> CH (3x3 at G x G), ReLU: the coupling's condition
  for_jobs(NP, CH, tid, [&](int o, int pair) {
    const int p = pair / HW, pos = pair % HW;
    float acc = F[A.r4b + o];
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
      const int nb = nbr<G>(pos, t);
      if (nb >= 0) {
#pragma unroll
        for (int c = 0; c < CH; ++c) acc = fmaf(F[A.r4w + (t * CH + c) * CH + o], r2[c * NP + p * HW + nb], acc);
      }
    }
    fin[o * NP + pair] = relu(acc);
  });
  __syncthreads();
  // f: Conv2dNormy(C -> YH, 3x3) ReLU, Conv2dNormy(YH -> YH, 1x1) ReLU, Conv2dZerosy(YH -> C, 3x3)
  // tanh.  f's input is cat(condition, z1): channels < CH from fin, the others from S.y.
  for_jobs(NP, yh, tid, [&](int o, int pair) {
    const int p = pair / HW, pos = pair % HW;
    float acc = 0.f;
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
      const int nb = nbr<G>(pos, t);
      if (nb >= 0) {
#pragma unroll
        for (int c = 0; c < CH; ++c) acc = fmaf(F[A.f0w + (t * C + c) * yh + o], fin[c * NP + p * HW + nb], acc);
#pragma unroll
        for (int c = 0; c < CH; ++c) acc = fmaf(F[A.f0w + (t * C + CH + c) * yh + o], S.y[p][c * HW + nb], acc);
      }
    }
    h0[o * NP + pair] = relu((acc + F[A.f0ab + o]) * expf(F[A.f0al + o]));
  });
  __syncthreads();
  for_jobs(NP, yh, tid, [&](int o, int pair) {
    float acc = 0.f;
#pragma unroll 4
    for (int c = 0; c < yh; ++c) acc = fmaf(F[A.f2w + c * yh + o], h0[c * NP + pair], acc);
    h1[o * NP + pair] = relu((acc + F[A.f2ab + o]) * expf(F[A.f2al + o]));
  });
  __syncthreads();
  // (shift, scale) = channels (2 c, 2 c + 1) of f's output ("cross"); z2 = (z2 + shift) scale
  for_jobs(NP, CH, tid, [&](int c, int pair) {
    const int p = pair / HW, pos = pair % HW;
    float as = 0.f, ac = 0.f;
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
      const int nb = nbr<G>(pos, t);
      if (nb >= 0) {
#pragma unroll 4
        for (int k = 0; k < yh; ++k) {
          const float g = h1[k * NP + p * HW + nb];
          as = fmaf(F[A.f4w + (t * yh + k) * C + 2 * c], g, as);
          ac = fmaf(F[A.f4w + (t * yh + k) * C + 2 * c + 1], g, ac);
        }
      }
    }
    const float hs = tanhf((as + F[A.f4b + 2 * c] + F[A.f4nb + 2 * c]) * expf(F[A.f4l + 2 * c] * 3.0f));
    const float hc = tanhf((ac + F[A.f4b + 2 * c + 1] + F[A.f4nb + 2 * c + 1]) * expf(F[A.f4l + 2 * c + 1] * 3.0f));
    const float sc = sigmoidf_(hc + 2.0f);
    float *z2 = &S.y[p][(CH + c) * HW + pos];
    *z2 = (*z2 + hs) * sc;
    ls[p * (HW * CH) + c * HW + pos] = logf(sc);  // (fin's last readers are behind two barriers)
  });
  __syncthreads();
  const float lsum = particle_sum(ls, HW * CH, tid);
  if ((tid & 15) == 0) S.ld[tid >> 4] += lsum;
  __syncthreads();
}

template <int C, int G>
__device__ __forceinline__ void glow_step(const float *__restrict__ gs, int xh, int xs, int yh, int tid) {
  const Step st(xh, xs, yh, C, G);
  cond_nets<C>(gs, gs + st.offI, xh, xs, tid);
  actnorm_invconv<Tile, C, G>(tid);
  coupling<C, G>(gs + st.offF, yh, tid);
}

// x: particle (b, i) at x + b * x_rs + 2 i;  enc: row b at enc + b * enc_rs (192 floats);
// lik: (b, i) at lik + b * lik_rs + i = out_sign * (-nll).  xin non-null: the flow form (the
// condition given per sample, N = 1, enc = y).  zout (may be null): the final z, nz floats per
// particle.  top (may be null): [mean | logs] of the top Gaussian, nz floats each.
// logdet0 = -log(y_bins) 192, rounded from double once by the host.
__global__ __launch_bounds__(kThreads, kWgs) void cglow_wide_kernel(
    const float *__restrict__ pe, const float *__restrict__ glow, const float *__restrict__ top,
    const float *__restrict__ enc, int64_t enc_rs, const float *__restrict__ x, int64_t x_rs, int B, int N,
    float *__restrict__ lik, int64_t lik_rs, const float *__restrict__ xin, float *__restrict__ zout, float out_sign,
    int K, int L, int xh, int xs, int yh, float logdet0) {
  const int tid = threadIdx.x;
  const int64_t total = (int64_t)B * N;
  const int64_t ntiles = (total + kTileP - 1) / kTileP;
  const int nz = L == 2 ? kC2 * 4 : kE;
  const int step1 = Step(xh, xs, yh, kC, 4).size, step2 = Step(xh, xs, yh, kC2, 2).size;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t g0 = tile * kTileP;
    tile_load<Tile>(pe, enc, enc_rs, x, x_rs, N, xin, g0, total, tid);
#pragma unroll 1
    for (int k = 0; k < K; ++k) glow_step<kC, 4>(glow + (int64_t)k * step1, xh, xs, yh, tid);
    if (L == 2) {
      const float *g2 = glow + (int64_t)K * step1;
      split_squeeze<Tile>(g2, tid);
#pragma unroll 1
      for (int k = 0; k < K; ++k) glow_step<kC2, 2>(g2 + kSplit + (int64_t)k * step2, xh, xs, yh, tid);
    }
    tile_finish<Tile>(top, nz, logdet0, lik, lik_rs, zout, out_sign, N, g0, total, tid);
  }
}

}  // namespace cgw
}  // namespace nfdpf

using namespace nfdpf;
using namespace nfdpf::cgw;

extern "C" int nfdpf_cglow_wide_supported(int xh, int xs, int yh) { return widths_ok(xh, xs, yh) ? 1 : 0; }

extern "C" int64_t nfdpf_cglow_wide_params_size(int K, int L, int learn_top, int xh, int xs, int yh) {
  return K >= 1 && K <= kMaxK && L >= 1 && L <= kMaxL && widths_ok(xh, xs, yh) ? wide_size(K, L, learn_top != 0, xh, xs, yh)
                                                                                 : -1;
}

#define NFDPF_WIDE_RANGE(fn)                                                                                        \
  NFDPF_REQUIRE(K >= 1 && K <= kMaxK && L >= 1 && L <= kMaxL,                                                       \
                fn ": built for flow_depth K in 1..4 and num_levels L in 1..2 (got K = %d, L = %d)", K, L);         \
  NFDPF_REQUIRE(widths_ok(xh, xs, yh), fn ": built for %s (got %d / %d / %d)", kWidthsStr, xh, xs, yh);             \
  NFDPF_REQUIRE(std::isfinite(logdet0), fn ": logdet0 = -log(y_bins) 192 must be finite")

extern "C" int nfdpf_cglow_wide_measurement(const float *pe_params, const float *glow_params, int K, int L,
                                            const float *top, const float *enc, int64_t enc_rs, const float *x,
                                            int64_t x_rs, int B, int N, float *lik, int64_t lik_rs, int xh, int xs,
                                            int yh, float logdet0, void *stream) {
  NFDPF_REQUIRE(pe_params && glow_params && enc && x && lik, "nfdpf_cglow_wide_measurement: null pointer");
  NFDPF_WIDE_RANGE("nfdpf_cglow_wide_measurement");
  NFDPF_REQUIRE(B >= 0 && N >= 1, "nfdpf_cglow_wide_measurement: bad sizes");
  if (B == 0) return NFDPF_OK;
  const int grid = persistent_grid(((int64_t)B * N + kTileP - 1) / kTileP, kWgs);
  cglow_wide_kernel<<<grid, kThreads, 0, as_stream(stream)>>>(pe_params, glow_params, top, enc, enc_rs, x, x_rs, B, N, lik,
                                                              lik_rs, nullptr, nullptr, 1.0f, K, L, xh, xs, yh, logdet0);
  return launch_status("nfdpf_cglow_wide_measurement");
}

extern "C" int nfdpf_cglow_wide_flow(const float *glow_params, int K, int L, const float *top, const float *x,
                                     const float *y, int64_t M, float *z, float *nll, int xh, int xs, int yh,
                                     float logdet0, void *stream) {
  NFDPF_REQUIRE(glow_params && x && y && nll, "nfdpf_cglow_wide_flow: null pointer");
  NFDPF_WIDE_RANGE("nfdpf_cglow_wide_flow");
  NFDPF_REQUIRE(M >= 0 && M <= (int64_t)INT32_MAX, "nfdpf_cglow_wide_flow: bad size");
  if (M == 0) return NFDPF_OK;
  // B = M rows of N = 1 (y row m is sample m), the condition x given, out_sign -1: nll
  const int grid = persistent_grid((M + kTileP - 1) / kTileP, kWgs);
  cglow_wide_kernel<<<grid, kThreads, 0, as_stream(stream)>>>(glow_params, glow_params, top, y, kE, nullptr, 0, (int)M, 1, nll,
                                                              1, x, z, -1.0f, K, L, xh, xs, yh, logdet0);
  return launch_status("nfdpf_cglow_wide_flow");
}
