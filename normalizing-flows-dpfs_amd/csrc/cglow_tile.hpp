// cglow_tile.hpp -- the tile frame the two persistent-tile CGLOW forward kernels share:
// cglow_levels.hip (L in 1..2, learn_top; hidden 8 / 16 / 8) and cglow_wide.hip (the hidden sizes
// of cglow_widths.hpp, any y_bins).  Both map a workgroup of 256 threads to a tile of 16 particles
// and keep the tile in one `static __shared__ Lds S` of their own with the members
//   xs[16][193]  the condition x          y[16][193]   the flow's state
//   an[16][49]   actnorm (logs | bias)    ld[16]       the log-dets so far
//   pxy[16][2], row[16]                   u[...]       scratch, reused phase by phase
// What differs per kernel -- cond_nets, coupling, the areas inside `u`, the wide kernel's job
// dealing, the levels kernel's mid-state stores -- stays in its file.  Used by both:
//   sigmoidf_, particle_sum, uni, uptr, wave_sync, nbr<G>, kLog2Pi       lane helpers
//   actnorm_invconv<T, C, G>     cond-actnorm, cond-1x1 conv and its log-determinant
//   split_squeeze<T>             Split2d(12) and the squeeze to 24 x 2 x 2 (L = 2)
//   tile_load<T>                 the prologue: inputs -> S.pxy, S.row, S.ld, S.y, S.xs
//   tile_finish<T>               the tail: top Gaussian, sum, lik / zout stores
// T is the kernel's traits type: `static Lds &lds()` returns that file's S (a __forceinline__
// accessor, so every access here is to a compile-time-known LDS object and stays a ds_
// instruction inside the __noinline__ functions too), and kSplitA / kSplitB are split_squeeze's
// two scratch offsets into S.u.  cglow.hip's lane maps are a different design and use none of it.
#pragma once

#include "cglow_levels.hpp"

namespace nfdpf {
namespace cgt {
using namespace cgl;  // kE, kC, kCh, kC2, kSplitW, kPe*

constexpr int kTileP = 16;
constexpr int kThreads = 256;
constexpr int kWmStride = kC2 * kC2 + 1;  // a particle's 1x1-conv matrix in `u`
constexpr float kLog2Pi = 1.8378770664093453f;

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// sum of buf[p * n + i], i < n, for each particle p: lane j of the particle's 16 adds i = j,
// j + 16, ... in order, then the 16 partials meet on a DPP butterfly -- a fixed order.  Every
// lane of the particle returns the sum.
__device__ __forceinline__ float particle_sum(const float *buf, int n, int tid) {
  const int p = tid >> 4, j = tid & 15;
  float s = 0.f;
  for (int i = j; i < n; i += 16) s += buf[p * n + i];
  s += dpp_f<kDppXor1>(s);
  s += dpp_f<kDppXor2>(s);
  s += dpp_f<kDppHalfMirror>(s);
  s += dpp_f<kDppMirror>(s);
  return s;
}

// a wave-uniform value / weight pointer in SGPRs (scalar loads from the constant address space):
// arguments of a non-inlined function arrive in VGPRs, hence the readfirstlane
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ cfloat *uptr(const float *p) {
  const uint64_t v = (uint64_t)p;
  return (cfloat *)(((uint64_t)(uint32_t)uni((int)(v >> 32)) << 32) | (uint32_t)uni((int)(uint32_t)v));
}

// An LDS hand-off between lanes of ONE wave (a particle's 16 lanes): a wave's LDS accesses
// execute in order, so waiting for its own and a compiler fence suffice (as WSYNC, cglow.hip).
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// neighbour (tap t of 3x3, pad 1) of position ps on the G x G grid, -1 outside
template <int G>
__device__ __forceinline__ int nbr(int ps, int t) {
  const int rr = ps / G + t / 3 - 1, ss = ps % G + t % 3 - 1;
  return rr >= 0 && rr < G && ss >= 0 && ss < G ? rr * G + ss : -1;
}

// cond-actnorm and cond-1x1 conv of S.y in place (a thread owns one (particle, position)), then
// log|det W| by Gaussian elimination with partial pivoting in place in LDS: the particle's 16
// lanes share the rows (rows k + j, k + j + 16 of the remaining ones in lane j); they are lanes
// of one wave, so the elimination's hand-offs need no workgroup barrier.
// S.ld += G G (sum logs + log|det W|).
template <class T, int C, int G>
__device__ __noinline__ void actnorm_invconv(int tid) {
  auto &S = T::lds();
  constexpr int HW = G * G;
  if (tid < kTileP * HW) {
    const int p = tid / HW, pos = tid % HW;
    float y[C];
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = (S.y[p][c * HW + pos] + S.an[p][C + c]) * expf(S.an[p][c]);
    const float *w = S.u + p * kWmStride;
#pragma unroll 1
    for (int o = 0; o < C; ++o) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) acc = fmaf(w[o * C + c], y[c], acc);
      S.y[p][o * HW + pos] = acc;
    }
  }
  __syncthreads();
  const int p = tid >> 4, j = tid & 15;
  float *A = S.u + p * kWmStride;
  float ldw = 0.f;
#pragma unroll 1
  for (int k = 0; k < C; ++k) {
    float best = -1.f;
    int br = k;
    for (int r = k + j; r < C; r += 16) {
      const float v = fabsf(A[r * C + k]);
      if (v > best) {
        best = v;
        br = r;
      }
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {  // (|value|, lowest row) max over the particle's lanes
      const float ob = __shfl_xor(best, m, 16);
      const int orow = __shfl_xor(br, m, 16);
      if (ob > best || (ob == best && orow < br)) {
        best = ob;
        br = orow;
      }
    }
    if (br != k)
      for (int c = j; c < C; c += 16) {
        const float t = A[k * C + c];
        A[k * C + c] = A[br * C + c];
        A[br * C + c] = t;
      }
    wave_sync();
    const float piv = A[k * C + k];
    ldw += logf(fabsf(piv));
    for (int r = k + 1 + j; r < C; r += 16) {
      const float f = A[r * C + k] / piv;
      for (int c = k + 1; c < C; ++c) A[r * C + c] = fmaf(-f, A[k * C + c], A[r * C + c]);
    }
    wave_sync();
  }
  if (j == 0) {
    float sl = 0.f;
    for (int c = 0; c < C; ++c) sl += S.an[p][c];
    S.ld[p] += (float)HW * sl + (float)HW * ldw;
  }
  __syncthreads();
}

// Split2d(12) on S.y (12 x 4 x 4): S.ld += GaussianDiag.logp(mean, logs, z2) with (mean, logs)
// the even / odd channels of tanh(conv 6 -> 12 (3x3) of z1); then z1 squeezed to 24 x 2 x 2.
template <class T>
__device__ __noinline__ void split_squeeze(const float *__restrict__ Sp, int tid) {
  auto &S = T::lds();
  float *bufA = S.u + T::kSplitA, *bufB = S.u + T::kSplitB;
  static_assert(T::kSplitA + kTileP * 16 * kCh <= T::kSplitB, "the Gaussian terms end before the squeezed z1");
  for (int i = tid; i < kTileP * 16 * kCh; i += kThreads) {
    const int pp = i / kCh, m = i - pp * kCh, p = pp >> 4, ps = pp & 15;
    float am = Sp[kSplitW + 2 * m], al = Sp[kSplitW + 2 * m + 1];
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
      const int nb = nbr<4>(ps, t);
      if (nb >= 0) {
#pragma unroll
        for (int c = 0; c < kCh; ++c) {
          const float z1 = S.y[p][c * 16 + nb];
          am = fmaf(Sp[(t * kCh + c) * kC + 2 * m], z1, am);
          al = fmaf(Sp[(t * kCh + c) * kC + 2 * m + 1], z1, al);
        }
      }
    }
    const float mean = tanhf(am), logs = tanhf(al), d = S.y[p][(kCh + m) * 16 + ps] - mean;
    bufA[i] = -0.5f * (2.0f * logs + d * d * expf(-2.0f * logs) + kLog2Pi);
  }
  // squeeze: channel c 4 + a 2 + b at (i, j) is z1[c][2 i + a][2 j + b]
  for (int i = tid; i < kTileP * 96; i += kThreads) {
    const int p = i / 96, e = i - p * 96, nc = e >> 2, np = e & 3;
    bufB[i] = S.y[p][(nc >> 2) * 16 + (2 * (np >> 1) + ((nc >> 1) & 1)) * 4 + 2 * (np & 1) + (nc & 1)];
  }
  __syncthreads();
  const float lp = particle_sum(bufA, 16 * kCh, tid);
  if ((tid & 15) == 0) S.ld[tid >> 4] += lp;
  for (int i = tid; i < kTileP * 96; i += kThreads) S.y[i / 96][i % 96] = bufB[i];
  __syncthreads();
}

// The tile's prologue.  x: particle (b, i) at x + b * x_rs + 2 i;  enc: row b at enc + b * enc_rs
// (192 floats).  xin non-null: the flow form (the condition given per sample, N = 1, enc = y).
// Leaves S.pxy / S.row (the particles of tile g0 .. and their rows), S.ld = 0, S.y = the squeezed
// frame encoding and S.xs = the condition, behind a barrier.
template <class T>
__device__ __forceinline__ void tile_load(const float *pe, const float *enc, int64_t enc_rs,
                                          const float *x, int64_t x_rs, int N,
                                          const float *xin, int64_t g0, int64_t total, int tid) {
  auto &S = T::lds();
  if (tid < kTileP) {
    const int64_t gi = g0 + tid;
    float a = 0.f, c = 0.f;
    int rb = 0;
    if (gi < total) {
      rb = (int)(gi / N);
      if (!xin) {
        const int i = (int)(gi - (int64_t)rb * N);
        a = x[rb * x_rs + 2 * i];
        c = x[rb * x_rs + 2 * i + 1];
      }
    }
    S.pxy[tid][0] = a;
    S.pxy[tid][1] = c;
    S.row[tid] = rb;
    S.ld[tid] = 0.f;
  }
  __syncthreads();
  // y = squeeze(frame encoding of the particle's row), [c 4 + a 2 + b][4 i + j]
  for (int i = tid; i < kTileP * kE; i += kThreads) {
    const int p = i / kE, e = i - p * kE, ch = e >> 4, q = e & 15;
    S.y[p][e] = enc[S.row[p] * enc_rs + (ch >> 2) * 64 + (2 * (q >> 2) + ((ch >> 1) & 1)) * 8 + 2 * (q & 3) + (ch & 1)];
  }
  if (xin) {
    for (int i = tid; i < kTileP * kE; i += kThreads) {
      const int p = i / kE, e = i - p * kE;
      S.xs[p][e] = g0 + p < total ? xin[(g0 + p) * kE + e] : 0.f;
    }
  } else {
    // particle encoder 2 -> 16 -> 32 (ReLU) -> 192 (nfdpf.pack.encoder_tensors: W1 row pairs,
    // W2 / W3 input-major)
    float *h1 = S.u, *h2 = S.u + kTileP * kPeH1;
    {
      const int p = tid >> 4, j = tid & 15;
      const float *w1 = pe + (j >> 1) * 4 + (j & 1);
      h1[tid] = relu(fmaf(w1[2], S.pxy[p][1], fmaf(w1[0], S.pxy[p][0], pe[kPeB1 + j])));
    }
    __syncthreads();
    for (int i = tid; i < kTileP * kPeH2; i += kThreads) {
      const int p = i >> 5, o = i & 31;
      float acc = pe[kPeB2 + o];
#pragma unroll
      for (int k = 0; k < kPeH1; ++k) acc = fmaf(pe[kPeW2 + k * kPeH2 + o], h1[p * kPeH1 + k], acc);
      h2[i] = relu(acc);
    }
    __syncthreads();
    for (int i = tid; i < kTileP * kE; i += kThreads) {
      const int p = i / kE, n = i - p * kE;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < kPeH2; ++k) acc = fmaf(pe[kPeW3 + k * kE + n], h2[p * kPeH2 + k], acc);
      S.xs[p][n] = acc + pe[kPeW3 + kE * kPeH2 + n];
    }
  }
  __syncthreads();
}

// The tile's tail: the top Gaussian of the final z in S.y (nz floats per particle; top, may be
// null: [mean | logs], nz floats each), its sum, and the outputs.  lik: (b, i) at lik + b * lik_rs
// + i = out_sign * (-nll), with logdet0 = -log(y_bins) 192 joining the log-dets and the top
// log-prob.  zout (may be null): the final z.
template <class T>
__device__ __forceinline__ void tile_finish(const float *top, int nz, float logdet0,
                                            float *lik, int64_t lik_rs, float *zout,
                                            float out_sign, int N, int64_t g0, int64_t total, int tid) {
  auto &S = T::lds();
  float *bufA = S.u;
  for (int i = tid; i < kTileP * nz; i += kThreads) {
    const int p = i / nz, e = i - p * nz;
    const float z = S.y[p][e], mean = top ? top[e] : 0.f, logs = top ? top[nz + e] : 0.f, d = z - mean;
    bufA[i] = -0.5f * (2.0f * logs + d * d * expf(-2.0f * logs) + kLog2Pi);
    if (zout && g0 + p < total) zout[(g0 + p) * nz + e] = z;
  }
  __syncthreads();
  const float lp = particle_sum(bufA, nz, tid);
  const int p = tid >> 4;
  if ((tid & 15) == 0 && g0 + p < total) {
    const float obj = logdet0 + (S.ld[p] + lp);
    const int rb = S.row[p];
    const int i = (int)(g0 + p - (int64_t)rb * N);
    lik[rb * lik_rs + i] = out_sign * (obj / (0.6931471805599453f * (float)kE));
  }
  __syncthreads();
}

}  // namespace cgt
}  // namespace nfdpf
