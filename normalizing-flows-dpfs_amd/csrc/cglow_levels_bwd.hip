// cglow_levels_bwd.hip -- backward of the conditional-GLOW measurement and flow for the
// configurations cglow_levels.hip takes forward and cglow_bwd.hip does not differentiate:
// flow_depth K in 1..4 with L = 1 and a learnt top prior (--learn_top), or with L = 2 levels
// and either learn_top setting.
//
// The chain, one launch per stage from the top down (the protocol of cglow_bwd.hip's
// launch_chain: dL/dz and the condition's gradient are handed down through alternating
// buffers, one owner thread per element; parameter partial rows are summed in row order):
//   1. one forward launch leaves every step's output in the workspace (L = 1: cglow.hip's
//      cglow_forward_mid with all K steps; L = 2: the MID variant of cglow_levels_kernel);
//   2. cglow_top_bwd_kernel: dL/dz_final = g_z + (the particle's weight on the objective) *
//      d GaussianDiag.logp(mean, logs, z) / dz, and per-block partial rows of the gradients of
//      new_mean / new_logs: block r owns a contiguous range of particles, thread e owns element
//      e of z and adds its particles' terms in particle order; the rows are then summed in row
//      order;
//   3. L = 2: K launches of cglow_l2_step_bwd_kernel (a CondGlowStep on 24 x 2 x 2), from the
//      last step down, then cglow_split_bwd_kernel (Split2d's Gaussian term and the un-squeeze);
//   4. the K level-1 steps as !TOP launches of cglow_bwd_kernel (cglow_bwd_below): their
//      incoming gradient is dL/dz from above plus the upstream weight on their own log-det;
//      step 0 also runs the particle encoder's backward on the summed encoding gradient.
// Every kernel is tile-local and persistent over tiles: no flags, no spin waits, no inter-
// workgroup hand-offs, no atomics; every sum over particles has a fixed order, so the
// gradients are bit-identical from run to run.
//
// cglow_l2_step_bwd_kernel: one workgroup = 256 threads = a tile of 8 particles.  Per tile it
// recomputes the step from its input with every activation in LDS (each phase a loop over its
// outputs strided by the workgroup), inverts every particle's 24 x 24 matrix by Gauss-Jordan
// with partial pivoting on the particle's 32 lanes (lane r holds row r of [W | I];
// d log|det W| / dW = W^-T), and runs the chain backwards in the same style.  Parameter
// gradients: the wide layers (the conditioning nets' convolutions and last layers, the resize
// and f convolutions) are GEMMs over the tile's terms on v_mfma_f32_16x16x4_f32 whose
// accumulators stay in registers across tiles; every other parameter has one owner thread
// (index mod 256 within its layer) that adds the tile's terms, in a fixed order, to the
// workgroup's row of the workspace after every tile.
#include "cglow_levels.hpp"

namespace nfdpf {
namespace cglb {
using namespace cgl;

constexpr float kLn2 = 0.6931471805599453f;

// ------------------------------------------------------------------------------------------
// the top Gaussian
// ------------------------------------------------------------------------------------------
constexpr int kTopThreads = 256;   // >= the final z's floats (192 at L = 1, 96 at L = 2)
constexpr int kTopRows = 1024;     // partial rows of the top prior's gradient, at most
constexpr int kTopChunk = 64;      // particles per row, at least
static_assert(kTopThreads >= kE, "one thread per element of z");

static int top_rows(int64_t M) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(kTopRows, (M + kTopChunk - 1) / kTopChunk));
}

// z, g_z, gz_out: [M, nz]; the upstream weight of particle m = (b, i), b = m / N, at
// g_up[b * gup_rs + i], times sign / (192 ln 2) (lik = obj / (192 ln 2) in the measurement form,
// nll = -lik in the flow form).  top: [mean | logs] (null: zeros, and no parameter gradient).
// partial: [gridDim.x][2 nz] = this block's sums of (d mean | d logs).
__global__ __launch_bounds__(kTopThreads) void cglow_top_bwd_kernel(
    const float *__restrict__ z, const float *__restrict__ top, const float *__restrict__ g_z,
    const float *__restrict__ g_up, int64_t gup_rs, int N, float sign, int64_t M, int nz,
    float *__restrict__ gz_out, float *__restrict__ partial) {
  const int e = threadIdx.x;
  if (e >= nz) return;
  const int64_t per = (M + gridDim.x - 1) / gridDim.x;
  const int64_t m0 = (int64_t)blockIdx.x * per, m1 = m0 + per < M ? m0 + per : M;
  const float mean = top ? top[e] : 0.f, logs = top ? top[nz + e] : 0.f, iv = expf(-2.0f * logs);
  const float scale = sign / (kLn2 * (float)kE);
  float am = 0.f, al = 0.f;
  for (int64_t m = m0; m < m1; ++m) {
    const int64_t b = m / N;
    const float gobj = g_up[b * gup_rs + (m - b * N)] * scale;
    // logp = sum_e -0.5 (2 logs + d^2 exp(-2 logs) + log 2 pi), d = z - mean
    const float d = z[m * nz + e] - mean, t = d * iv;
    gz_out[m * nz + e] = fmaf(-t, gobj, g_z ? g_z[m * nz + e] : 0.f);
    am = fmaf(t, gobj, am);
    al = fmaf(fmaf(d, t, -1.0f), gobj, al);
  }
  if (top) {
    partial[(int64_t)blockIdx.x * 2 * nz + e] = am;
    partial[(int64_t)blockIdx.x * 2 * nz + nz + e] = al;
  }
}

// out[j] = sum over the rows of partial [rows][n], in row order
__global__ __launch_bounds__(256) void cglow_rows_reduce_kernel(const float *__restrict__ partial, int rows, int n,
                                                                float *__restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  float a = 0.f;
  for (int r = 0; r < rows; ++r) a += partial[(int64_t)r * n + j];
  out[j] = a;
}

// ------------------------------------------------------------------------------------------
// Split2d(12) and the squeeze
// ------------------------------------------------------------------------------------------
constexpr int kSpP = 16, kSpThreads = 256, kSpGrid = 512, kSpSlots = (kSplit + kSpThreads - 1) / kSpThreads;

struct SpLds {
  float z[kSpP][kE];        // the level-1 output (12, 4, 4): z1 = channels 0..5, z2 = 6..11
  float gs[kSpP][kC2 * 4];  // dL/d(level-2 input) (24, 2, 2)
  float gp[kSpP][16][kC];   // dL/d(conv output before the tanh), [pos][2 m | 2 m + 1] = (mean, logs)
  float gobj[kSpP];
};
static_assert(sizeof(SpLds) <= 64 * 1024, "cglow_split_bwd_kernel: static LDS");

__device__ __forceinline__ int nbr4(int ps, int dr, int ds) {
  const int rr = (ps >> 2) + dr, ss = (ps & 3) + ds;
  return rr >= 0 && rr < 4 && ss >= 0 && ss < 4 ? rr * 4 + ss : -1;
}

// Sp: the Split2d conv ([3][3][6][12], then 12 biases).  z [M, 192]: the last level-1 step's
// output; gs [M, 96]: dL/d(level-2 step 0's input).  gz_out [M, 192] = dL/dz: channels 0..5 the
// un-squeezed gs plus the prior's gradient through the transposed convolution, channels 6..11 the
// Gaussian term's gradient to z2.  partial [gridDim.x][660]: this workgroup's parameter sums.
// Lane = (particle tid / 16, position tid % 16).
__global__ __launch_bounds__(kSpThreads) void cglow_split_bwd_kernel(
    const float *__restrict__ Sp, const float *__restrict__ z, const float *__restrict__ gs,
    const float *__restrict__ g_up, int64_t gup_rs, int N, float sign, int64_t M, float *__restrict__ gz_out,
    float *__restrict__ partial) {
  __shared__ SpLds S;
  const int tid = threadIdx.x, p = tid >> 4, ps = tid & 15;
  const int64_t ntiles = (M + kSpP - 1) / kSpP;
  const float scale = sign / (kLn2 * (float)kE);
  float acc[kSpSlots];
#pragma unroll
  for (int s = 0; s < kSpSlots; ++s) acc[s] = 0.f;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t g0 = tile * kSpP;
    for (int i = tid; i < kSpP * kE; i += kSpThreads) {
      const int pp = i / kE, e = i - pp * kE;
      const int64_t m = g0 + pp < M ? g0 + pp : M - 1;
      S.z[pp][e] = z[m * kE + e];
    }
    for (int i = tid; i < kSpP * kC2 * 4; i += kSpThreads) {
      const int pp = i / (kC2 * 4), e = i - pp * (kC2 * 4);
      S.gs[pp][e] = g0 + pp < M ? gs[(g0 + pp) * (kC2 * 4) + e] : 0.f;
    }
    if (tid < kSpP) {
      const int64_t m = g0 + tid;
      float g = 0.f;
      if (m < M) {
        const int64_t b = m / N;
        g = g_up[b * gup_rs + (m - b * N)] * scale;
      }
      S.gobj[tid] = g;
    }
    __syncthreads();
    const int64_t m = g0 + p;
    const bool valid = m < M;
    const float gobj = S.gobj[p];
#pragma unroll 1
    for (int c = 0; c < kCh; ++c) {  // (mean, logs) of z2's channel c at this position
      float am = Sp[kSplitW + 2 * c], al = Sp[kSplitW + 2 * c + 1];
#pragma unroll 1
      for (int t = 0; t < 9; ++t) {
        const int nb = nbr4(ps, t / 3 - 1, t % 3 - 1);
        if (nb < 0) continue;
#pragma unroll
        for (int ci = 0; ci < kCh; ++ci) {
          const float z1 = S.z[p][ci * 16 + nb];
          am = fmaf(Sp[(t * kCh + ci) * kC + 2 * c], z1, am);
          al = fmaf(Sp[(t * kCh + ci) * kC + 2 * c + 1], z1, al);
        }
      }
      const float mean = tanhf(am), logs = tanhf(al), d = S.z[p][(kCh + c) * 16 + ps] - mean;
      const float iv = expf(-2.0f * logs), t1 = d * iv;
      // logp = -0.5 (2 logs + d^2 exp(-2 logs) + log 2 pi)
      if (valid) gz_out[m * kE + (kCh + c) * 16 + ps] = -t1 * gobj;
      S.gp[p][ps][2 * c] = t1 * gobj * (1.0f - mean * mean);
      S.gp[p][ps][2 * c + 1] = fmaf(d, t1, -1.0f) * gobj * (1.0f - logs * logs);
    }
    __syncthreads();
    {
      const int r = ps >> 2, s = ps & 3;
#pragma unroll 1
      for (int c = 0; c < kCh; ++c) {
        // un-squeeze: channel c 4 + a 2 + b of the 2 x 2 grid at (i, j) is z1[c][2 i + a][2 j + b]
        float a = S.gs[p][(c * 4 + (r & 1) * 2 + (s & 1)) * 4 + (r >> 1) * 2 + (s >> 1)];
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
          const int po = nbr4(ps, -(t / 3 - 1), -(t % 3 - 1));  // the output whose tap t reads ps
          if (po < 0) continue;
#pragma unroll
          for (int oc = 0; oc < kC; ++oc) a = fmaf(Sp[(t * kCh + c) * kC + oc], S.gp[p][po][oc], a);
        }
        if (valid) gz_out[m * kE + c * 16 + ps] = a;
      }
    }
#pragma unroll
    for (int sl = 0; sl < kSpSlots; ++sl) {  // the parameters' owner threads
      const int j = tid + kSpThreads * sl;
      if (j >= kSplit) break;
      float a = 0.f;
      if (j < kSplitW) {
        const int oc = j % kC, tc = j / kC, c = tc % kCh, t = tc / kCh;
        for (int k = 0; k < kSpP * 16; ++k) {
          const int nb = nbr4(k & 15, t / 3 - 1, t % 3 - 1);
          if (nb >= 0) a = fmaf(S.gp[k >> 4][k & 15][oc], S.z[k >> 4][c * 16 + nb], a);
        }
      } else {
        const int oc = j - kSplitW;
        for (int k = 0; k < kSpP * 16; ++k) a += S.gp[k >> 4][k & 15][oc];
      }
      acc[sl] += a;
    }
    __syncthreads();
  }
#pragma unroll
  for (int sl = 0; sl < kSpSlots; ++sl) {
    const int j = tid + kSpThreads * sl;
    if (j < kSplit) partial[(int64_t)blockIdx.x * kSplit + j] = acc[sl];
  }
}

// ------------------------------------------------------------------------------------------
// a level-2 CondGlowStep (24 x 2 x 2)
// ------------------------------------------------------------------------------------------
namespace l2 {
constexpr int kP = 8;        // particles per tile
constexpr int kT = 256;
constexpr int kGrid = 256;   // partial rows, at most (one resident workgroup per CU)
constexpr int C = kC2, CH = kC2 / 2, HW = 4, NZ = kC2 * 4;
using St = Step2;
using CA = St::A;
using CI = St::I;
using A = St::F;
static_assert(CA::l4w == CI::l4w, "the two conditioning nets share their layout up to the last layer");

typedef float f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

struct Lds {
  float X[kP][kE], gX[kP][kE];  // the condition x (3, 8, 8) and its gradient
  float c1[kP][16][16], c2[kP][4][16], c3[kP][16], l0[kP][32], l1[kP][32];  // conditioning nets A | I
  float an[kP][2 * C], gan[kP][2 * C];   // tanh outputs (logs | bias) and their gradient
  float wm[kP][C * C], gw[kP][C * C];    // W [o][c]; W^-T, then dL/dW, then dL/d(pre-tanh)
  float prow[kP][2 * C];                 // Gauss-Jordan pivot row
  float ya[kP][NZ], yw[kP][NZ], gz[kP][NZ];  // after actnorm; after the 1x1 conv (z1 | z2); dL/d yw, [c][pos]
  float r1[kP][64][16];                  // resize conv 1 (ReLU), then its gradient in place
  float r2[kP][HW][CH], fin[kP][HW][C], g1[kP][HW][kYH], g2[kP][HW][kYH], u[kP][HW][C], h[kP][HW][C];
  float Da[kP][HW][C], Ea[kP][HW][C];    // f conv 4: dL/d(conv output), log-scale terms; later actnorm terms
  float Db[kP][HW][kYH], Eb[kP][HW][kYH], Dc[kP][HW][kYH], Ec[kP][HW][kYH];  // f conv 2, conv 0
  float Dd[kP][HW][CH], De[kP][HW][CH];  // resize conv 4, conv 2
  float Gl1[kP][32], Gl0[kP][32], Gc3[kP][16], Gc2[kP][4][16], Gc1[kP][16][16];
  float h1[kP][kPeH1], h2[kP][kPeH2], pxy[kP][2], gobj[kP];
  float esc[2 * kYH + C];                // exp(f0 logs), exp(f2 logs), exp(3 f4 logs)
  float cmb[2][64][4];                   // r0w: the two particle halves meet
  int64_t m[kP];
  int valid[kP];
};
static_assert(sizeof(Lds) <= 160 * 1024, "cglow_l2_step_bwd_kernel: LDS above 160 KB");

__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ int nbr2(int ps, int dr, int ds) {
  const int rr = (ps >> 1) + dr, ss = (ps & 1) + ds;
  return rr >= 0 && rr < 2 && ss >= 0 && ss < 2 ? rr * 2 + ss : -1;
}
__device__ __forceinline__ int nbr8(int ps, int dr, int ds) {
  const int rr = (ps >> 3) + dr, ss = (ps & 7) + ds;
  return rr >= 0 && rr < 8 && ss >= 0 && ss < 8 ? rr * 8 + ss : -1;
}
#define L2_WFENCE()                                    \
  do {                                                 \
    __builtin_amdgcn_sched_barrier(0);                 \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    __builtin_amdgcn_wave_barrier();                   \
    __builtin_amdgcn_sched_barrier(0);                 \
  } while (0)
#define L2_FOR(i, n) for (int i = (int)threadIdx.x; i < (n); i += kT)

// the owner threads of the layer at row[off .. off + n) add f(j), the tile's sum of parameter
// j's terms, to the workgroup's row (the same thread every tile: program order)
template <class F>
__device__ __forceinline__ void own(float *row, bool first, int off, int n, const F &f) {
  for (int j = (int)threadIdx.x; j < n; j += kT) {
    const float v = f(j);
    row[off + j] = first ? v : row[off + j] + v;
  }
}
// C (16 x 16 tile, this lane: rows 4 (l / 16) + i, column l % 16) into the row: row[idx(m, n)]
// for m < Mr, n = n0 + l % 16 < NC
template <class IDX>
__device__ __forceinline__ void store_tile(const f4 &c, float *row, int Mr, int n0, int NC, const IDX &idx) {
  const int l = threadIdx.x & 63, n = n0 + (l & 15);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = 4 * (l >> 4) + i;
    if (m < Mr && n < NC) row[idx(m, n)] = c[i];
  }
}

// PART: the condition is the particle encoder's output for particle (b, i) at x + b * x_rs + 2 i
// and the upstream weight g_up[b * gup_rs + i] on lik; else the condition is xin [M, 192] and
// the weight g_up[m] on nll.  glow: this step's 21 168 parameters.  zin [M, 96]: the step's
// input; gz_in [M, 96]: dL/d(its output) from the launch above; gx_in [M, 192] (null: zeros):
// the condition's gradient so far.  Out: gz_out [M, 96] = dL/d(input), gx_out [M, 192] = gx_in +
// this step's share, and the workgroup's row of `partial`.
template <bool PART>
__global__ __launch_bounds__(kT, 1) void cglow_l2_step_bwd_kernel(
    const float *__restrict__ pe_, const float *__restrict__ glow, const float *__restrict__ x, int64_t x_rs,
    const float *__restrict__ xin, int B, int N, const float *__restrict__ g_up, int64_t gup_rs,
    const float *__restrict__ zin, const float *__restrict__ gz_in, const float *__restrict__ gx_in,
    float *__restrict__ gz_out, float *__restrict__ gx_out, float *partial) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  Lds &S = *reinterpret_cast<Lds *>(lds_raw);
  const int tid = threadIdx.x, w = tid >> 6, lr = tid & 15, lk = (tid >> 4) & 3;
  const int64_t M = (int64_t)B * N;
  const int64_t ntiles = (M + kP - 1) / kP;
  float *row = partial + (int64_t)blockIdx.x * St::size;
  // MFMA accumulators, persistent across tiles
  f4 cL4I[9] = {}, cL4A = {}, cR2[4] = {}, cR4[2] = {}, cF0[4] = {}, cF4[3] = {}, cF2 = {}, cR0 = {}, cC0 = {}, cC2 = {};
  if (tid < 2 * kYH + C) {
    const float *F = glow + St::offF;
    S.esc[tid] = tid < kYH ? expf(F[A::f0al + tid])
                 : tid < 2 * kYH ? expf(F[A::f2al + tid - kYH]) : expf(F[A::f4l + tid - 2 * kYH] * 3.0f);
  }
  const float *es0 = S.esc, *es2 = S.esc + kYH, *e3 = S.esc + 2 * kYH;

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const bool first = tile == (int64_t)blockIdx.x;
    // weight pointers laundered per tile: the compiler re-reads the weights from the caches in
    // each tile instead of hoisting their loads out of the tile loop (register spills)
    const float *gw_ = glow, *pe = pe_;
    asm volatile("" : "+s"(gw_), "+s"(pe));
    const float *gA = gw_ + St::offA, *gI = gw_ + St::offI, *F = gw_ + St::offF;
    if (tid < kP) {
      const int64_t mr = tile * kP + tid;
      const bool v = mr < M;
      const int64_t m = v ? mr : M - 1;  // invalid slots recompute a real particle, upstream 0
      S.m[tid] = m;
      S.valid[tid] = v;
      const float scale = 1.0f / (kLn2 * (float)kE);
      float g = 0.f;
      if (PART) {
        const int64_t b = m / N, i = m - b * N;
        if (v) g = g_up[b * gup_rs + i] * scale;
        S.pxy[tid][0] = x[b * x_rs + 2 * i];
        S.pxy[tid][1] = x[b * x_rs + 2 * i + 1];
      } else if (v) {
        g = -g_up[m * gup_rs] * scale;
      }
      S.gobj[tid] = g;
    }
    __syncthreads();
    // ---------------- forward recompute ----------------
    if (PART) {  // particle encoder 2 -> 16 -> 32 (ReLU) -> 192 (W1 row pairs, W2 / W3 input-major)
      L2_FOR(i, kP * kPeH1) {
        const int p = i >> 4, j = i & 15;
        const float *w1 = pe + (j >> 1) * 4 + (j & 1);
        S.h1[p][j] = relu(fmaf(w1[2], S.pxy[p][1], fmaf(w1[0], S.pxy[p][0], pe[kPeB1 + j])));
      }
      __syncthreads();
      L2_FOR(i, kP * kPeH2) {
        const int p = i >> 5, o = i & 31;
        float a = pe[kPeB2 + o];
#pragma unroll
        for (int k = 0; k < kPeH1; ++k) a = fmaf(pe[kPeW2 + k * kPeH2 + o], S.h1[p][k], a);
        S.h2[p][o] = relu(a);
      }
      __syncthreads();
    }
    L2_FOR(i, kP * kE) {
      const int p = i / kE, n = i - p * kE;
      float xv;
      if (PART) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < kPeH2; ++k) a = fmaf(pe[kPeW3 + k * kE + n], S.h2[p][k], a);
        xv = a + pe[kPeW3 + kE * kPeH2 + n];
      } else {
        xv = xin[S.m[p] * kE + n];
      }
      S.X[p][n] = xv;
      S.gX[p][n] = gx_in && S.valid[p] ? gx_in[S.m[p] * kE + n] : 0.f;
    }
    L2_FOR(i, kP * NZ) {
      const int p = i / NZ, e = i - p * NZ;
      S.ya[p][e] = zin[S.m[p] * NZ + e];
      S.gz[p][e] = S.valid[p] ? gz_in[S.m[p] * NZ + e] : 0.f;
    }
    __syncthreads();
    // conditioning nets (A: actnorm, I: 1x1 conv): three 2x2 stride-2 convs, 8 -> 16 -> 16 -> OUT
    L2_FOR(i, kP * 256) {
      const int p = i >> 8, q = (i >> 4) & 15, no = i & 15, net = no >> 3, o = no & 7, qi = q >> 2, qj = q & 3;
      const float *G = net ? gI : gA;
      float a = G[CA::c0b + o];
#pragma unroll
      for (int k = 0; k < 12; ++k)
        a = fmaf(G[CA::c0w + k * kXH + o], S.X[p][(k >> 2) * 64 + (2 * qi + ((k >> 1) & 1)) * 8 + 2 * qj + (k & 1)], a);
      S.c1[p][q][no] = relu(a);
    }
    __syncthreads();
    L2_FOR(i, kP * 64) {
      const int p = i >> 6, pos = (i >> 4) & 3, no = i & 15, net = no >> 3, o = no & 7, pi = pos >> 1, pj = pos & 1;
      const float *G = net ? gI : gA;
      float a = G[CA::c2b + o];
#pragma unroll
      for (int k = 0; k < 32; ++k)
        a = fmaf(G[CA::c2w + o * 32 + k], S.c1[p][(2 * pi + ((k >> 1) & 1)) * 4 + 2 * pj + (k & 1)][net * kXH + (k >> 2)], a);
      S.c2[p][pos][no] = relu(a);
    }
    __syncthreads();
    L2_FOR(i, kP * 16) {
      const int p = i >> 4, no = i & 15, net = no >> 3, o = no & 7;
      const float *G = net ? gI : gA;
      float a = G[CA::c4b + o];
#pragma unroll
      for (int k = 0; k < 32; ++k) a = fmaf(G[CA::c4w + o * 32 + k], S.c2[p][k & 3][net * kXH + (k >> 2)], a);
      S.c3[p][no] = relu(a);
    }
    __syncthreads();
    L2_FOR(i, kP * 32) {
      const int p = i >> 5, net = (i >> 4) & 1, o = i & 15;
      const float *G = net ? gI : gA;
      float a = G[CA::l0b + o];
#pragma unroll
      for (int k = 0; k < kXH; ++k) a = fmaf(G[CA::l0w + o * kXH + k], S.c3[p][net * kXH + k], a);
      S.l0[p][net * kXS + o] = relu(a);
    }
    __syncthreads();
    L2_FOR(i, kP * 32) {
      const int p = i >> 5, net = (i >> 4) & 1, o = i & 15;
      const float *G = net ? gI : gA;
      float a = G[CA::l2b + o];
#pragma unroll
      for (int k = 0; k < kXS; ++k) a = fmaf(G[CA::l2w + o * kXS + k], S.l0[p][net * kXS + k], a);
      S.l1[p][net * kXS + o] = relu(a);
    }
    __syncthreads();
    L2_FOR(i, kP * (2 * C + C * C)) {
      const int p = i / (2 * C + C * C), nn = i - p * (2 * C + C * C);
      const bool isI = nn >= 2 * C;
      const int n = isI ? nn - 2 * C : nn;
      const float *G = isI ? gI : gA;
      float a = G[(isI ? CI::l4b : CA::l4b) + n];
#pragma unroll
      for (int k = 0; k < kXS; ++k) a = fmaf(G[CA::l4w + n * kXS + k], S.l1[p][(isI ? kXS : 0) + k], a);
      const float t = tanhf(a);
      if (isI)
        S.wm[p][n] = t;
      else
        S.an[p][n] = t;
    }
    __syncthreads();
    // actnorm (in place in ya)
    L2_FOR(i, kP * NZ) {
      const int p = i / NZ, e = i - p * NZ, c = e >> 2;
      S.ya[p][e] = (S.ya[p][e] + S.an[p][C + c]) * expf(S.an[p][c]);
    }
    // W^-1: Gauss-Jordan with partial pivoting, lane q < 24 of the particle's 32 holding row q of
    // [W | I]; W^-T goes to gw (gw[o][c] = W^-1[c][o])
    {
      const int p = tid >> 5, q = tid & 31;
      float a[2 * C];
      const int qr = q < C ? q : 0;
#pragma unroll
      for (int j = 0; j < C; ++j) {
        a[j] = q < C ? S.wm[p][qr * C + j] : 0.f;
        a[C + j] = (q == j) ? 1.f : 0.f;
      }
      bool done = q >= C;
      int mycol = 0;
      const uint32_t tag = 31u - (uint32_t)q;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        uint32_t key = done ? 0u : ((__float_as_uint(fabsf(a[k])) & ~0x1Fu) | tag);
#pragma unroll
        for (int msk = 1; msk < 32; msk <<= 1) key = max(key, (uint32_t)__shfl_xor((int)key, msk, 32));
        const int who = 31 - (int)(key & 0x1Fu);
        if (q == who)
#pragma unroll
          for (int j = 0; j < 2 * C; ++j) S.prow[p][j] = a[j];
        L2_WFENCE();
        float pr[2 * C];
#pragma unroll
        for (int j = 0; j < 2 * C; ++j) pr[j] = S.prow[p][j];
        const float inv = 1.0f / pr[k];
        if (q == who) {
          done = true;
          mycol = k;
#pragma unroll
          for (int j = 0; j < 2 * C; ++j) a[j] = pr[j] * inv;
        } else if (q < C) {
          const float f = a[k];
#pragma unroll
          for (int j = 0; j < 2 * C; ++j) a[j] = fmaf(-f, pr[j] * inv, a[j]);
        }
        L2_WFENCE();
      }
      if (q < C)
#pragma unroll
        for (int j = 0; j < C; ++j) S.gw[p][j * C + mycol] = a[C + j];
    }
    __syncthreads();
    L2_FOR(i, kP * NZ) {  // the 1x1 conv
      const int p = i / NZ, e = i - p * NZ, o = e >> 2, pos = e & 3;
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) a = fmaf(S.wm[p][o * C + c], S.ya[p][c * HW + pos], a);
      S.yw[p][e] = a;
    }
    // resize_x: conv 3 -> 16 (3x3 at 8x8) ReLU
    L2_FOR(i, kP * 1024) {
      const int p = i >> 10, pos = (i >> 4) & 63, ci = i & 15;
      float a = F[A::r0b + ci];
#pragma unroll 1
      for (int t = 0; t < 9; ++t) {
        const int nb = nbr8(pos, t / 3 - 1, t % 3 - 1);
        if (nb < 0) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) a = fmaf(F[A::r0w + (t * 3 + c) * 16 + ci], S.X[p][c * 64 + nb], a);
      }
      S.r1[p][pos][ci] = relu(a);
    }
    __syncthreads();
    L2_FOR(i, kP * HW * CH) {  // Conv2dResize 16 -> 12, 4x4 stride 4, ReLU
      const int p = i / (HW * CH), rem = i - p * (HW * CH), pos = rem / CH, o = rem - pos * CH, pi = pos >> 1, pj = pos & 1;
      float a = F[A::r2b + o];
#pragma unroll 1
      for (int ab = 0; ab < 16; ++ab) {
        const float *rr = S.r1[p][(4 * pi + (ab >> 2)) * 8 + 4 * pj + (ab & 3)];
#pragma unroll
        for (int ci = 0; ci < 16; ++ci) a = fmaf(F[A::r2w + (ab * 16 + ci) * CH + o], rr[ci], a);
      }
      S.r2[p][pos][o] = relu(a);
    }
    __syncthreads();
    L2_FOR(i, kP * HW * CH) {  // conv 12 -> 12 (3x3) ReLU; fin = cat(that, z1)
      const int p = i / (HW * CH), rem = i - p * (HW * CH), pos = rem / CH, o = rem - pos * CH;
      float a = F[A::r4b + o];
#pragma unroll 1
      for (int t = 0; t < 9; ++t) {
        const int nb = nbr2(pos, t / 3 - 1, t % 3 - 1);
        if (nb < 0) continue;
#pragma unroll
        for (int c = 0; c < CH; ++c) a = fmaf(F[A::r4w + (t * CH + c) * CH + o], S.r2[p][nb][c], a);
      }
      S.fin[p][pos][o] = relu(a);
      S.fin[p][pos][CH + o] = S.yw[p][o * HW + pos];
    }
    __syncthreads();
    L2_FOR(i, kP * HW * kYH) {  // f: Conv2dNormy(24 -> 8, 3x3) ReLU
      const int p = i >> 5, pos = (i >> 3) & 3, o = i & 7;
      float a = 0.f;
#pragma unroll 1
      for (int t = 0; t < 9; ++t) {
        const int nb = nbr2(pos, t / 3 - 1, t % 3 - 1);
        if (nb < 0) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) a = fmaf(F[A::f0w + (t * C + c) * kYH + o], S.fin[p][nb][c], a);
      }
      S.g1[p][pos][o] = relu((a + F[A::f0ab + o]) * es0[o]);
    }
    __syncthreads();
    L2_FOR(i, kP * HW * kYH) {  // Conv2dNormy(8 -> 8, 1x1) ReLU
      const int p = i >> 5, pos = (i >> 3) & 3, o = i & 7;
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < kYH; ++c) a = fmaf(F[A::f2w + c * kYH + o], S.g1[p][pos][c], a);
      S.g2[p][pos][o] = relu((a + F[A::f2ab + o]) * es2[o]);
    }
    __syncthreads();
    L2_FOR(i, kP * HW * C) {  // Conv2dZerosy(8 -> 24, 3x3), tanh
      const int p = i / (HW * C), rem = i - p * (HW * C), pos = rem / C, o = rem - pos * C;
      float a = 0.f;
#pragma unroll 1
      for (int t = 0; t < 9; ++t) {
        const int nb = nbr2(pos, t / 3 - 1, t % 3 - 1);
        if (nb < 0) continue;
#pragma unroll
        for (int k = 0; k < kYH; ++k) a = fmaf(F[A::f4w + (t * kYH + k) * C + o], S.g2[p][nb][k], a);
      }
      const float uu = (a + F[A::f4b + o] + F[A::f4nb + o]) * e3[o];
      S.u[p][pos][o] = uu;
      S.h[p][pos][o] = tanhf(uu);
    }
    __syncthreads();

    // ---------------- backward ----------------
    // the step's log-det: 4 sum logs + 4 log|det W| + sum log sc, weight gobj
    L2_FOR(i, kP * HW * CH) {
      const int p = i / (HW * CH), rem = i - p * (HW * CH), pos = rem / CH, c = rem - pos * CH;
      const float shift = S.h[p][pos][2 * c], hc = S.h[p][pos][2 * c + 1], sc = sigm(hc + 2.0f);
      const float z2 = S.yw[p][(CH + c) * HW + pos], gobj = S.gobj[p];
      const float gz2p = S.gz[p][(CH + c) * HW + pos];
      S.gz[p][(CH + c) * HW + pos] = gz2p * sc;
      const float gsh = gz2p * sc;
      const float gsp = gz2p * (z2 + shift) * sc * (1.0f - sc) + gobj * (1.0f - sc);
      const float gu0 = gsh * (1.0f - shift * shift), gu1 = gsp * (1.0f - hc * hc);
      S.Da[p][pos][2 * c] = gu0 * e3[2 * c];  // dL/d(conv output) = dL/d(bias) = dL/d(newbias)
      S.Da[p][pos][2 * c + 1] = gu1 * e3[2 * c + 1];
      S.Ea[p][pos][2 * c] = 3.0f * gu0 * S.u[p][pos][2 * c];
      S.Ea[p][pos][2 * c + 1] = 3.0f * gu1 * S.u[p][pos][2 * c + 1];
    }
    __syncthreads();
    {
      auto sumD = [&](int j) {
        float a = 0.f;
        for (int k = 0; k < kP * HW; ++k) a += S.Da[k >> 2][k & 3][j];
        return a;
      };
      own(row, first, St::offF + A::f4b, C, sumD);
      own(row, first, St::offF + A::f4nb, C, sumD);
      own(row, first, St::offF + A::f4l, C, [&](int j) {
        float a = 0.f;
        for (int k = 0; k < kP * HW; ++k) a += S.Ea[k >> 2][k & 3][j];
        return a;
      });
    }
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {  // f4w: dW[o][n = (t, k8)] = sum_(p,pos) Da[p][pos][o] g2[p][pos + tap][k8]
      const int job = w + 4 * jj;
      if (job < 10) {
        const int rt = job / 5, ct = job % 5, n = ct * 16 + lr, t = n >> 3, k8 = n & 7, mm = rt * 16 + lr;
        const bool nok = n < 9 * kYH, mok = mm < C;
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
          const int kk = 4 * s2 + lk, p = kk >> 2, pos = kk & 3;
          const int nb = nok ? nbr2(pos, t / 3 - 1, t % 3 - 1) : -1;
          const float av = S.Da[p][pos][mok ? mm : 0], bv = S.g2[p][nb >= 0 ? nb : 0][k8];
          cF4[jj] = mfma4(mok ? av : 0.f, nb >= 0 ? bv : 0.f, cF4[jj]);
        }
      }
    }
    L2_FOR(i, kP * HW * kYH) {  // transposed conv -> dL/dg2; ReLU; actnorm scale es2
      const int p = i >> 5, pos = (i >> 3) & 3, k = i & 7;
      float a = 0.f;
#pragma unroll 1
      for (int t = 0; t < 9; ++t) {
        const int po = nbr2(pos, -(t / 3 - 1), -(t % 3 - 1));  // the output whose tap t reads pos
        if (po < 0) continue;
#pragma unroll
        for (int o = 0; o < C; ++o) a = fmaf(F[A::f4w + (t * kYH + k) * C + o], S.Da[p][po][o], a);
      }
      const float g2v = S.g2[p][pos][k], gv = g2v > 0.f ? a : 0.f;
      S.Db[p][pos][k] = gv * es2[k];
      S.Eb[p][pos][k] = gv * g2v;
    }
    __syncthreads();
    own(row, first, St::offF + A::f2ab, kYH, [&](int j) {
      float a = 0.f;
      for (int k = 0; k < kP * HW; ++k) a += S.Db[k >> 2][k & 3][j];
      return a;
    });
    own(row, first, St::offF + A::f2al, kYH, [&](int j) {
      float a = 0.f;
      for (int k = 0; k < kP * HW; ++k) a += S.Eb[k >> 2][k & 3][j];
      return a;
    });
    if (w == 1) {  // f2w: dW[o][c] = sum Db[p][pos][o] g1[p][pos][c]
      const bool ok = lr < kYH;
      const int o = ok ? lr : 0;
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) {
        const int kk = 4 * s2 + lk, p = kk >> 2, pos = kk & 3;
        const float av = S.Db[p][pos][o], bv = S.g1[p][pos][o];
        cF2 = mfma4(ok ? av : 0.f, ok ? bv : 0.f, cF2);
      }
    }
    L2_FOR(i, kP * HW * kYH) {
      const int p = i >> 5, pos = (i >> 3) & 3, c = i & 7;
      float a = 0.f;
#pragma unroll
      for (int o = 0; o < kYH; ++o) a = fmaf(F[A::f2w + c * kYH + o], S.Db[p][pos][o], a);
      const float g1v = S.g1[p][pos][c], gv = g1v > 0.f ? a : 0.f;
      S.Dc[p][pos][c] = gv * es0[c];
      S.Ec[p][pos][c] = gv * g1v;
    }
    __syncthreads();
    own(row, first, St::offF + A::f0ab, kYH, [&](int j) {
      float a = 0.f;
      for (int k = 0; k < kP * HW; ++k) a += S.Dc[k >> 2][k & 3][j];
      return a;
    });
    own(row, first, St::offF + A::f0al, kYH, [&](int j) {
      float a = 0.f;
      for (int k = 0; k < kP * HW; ++k) a += S.Ec[k >> 2][k & 3][j];
      return a;
    });
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {  // f0w: dW[o][n = (t, c)] = sum Dc[p][pos][o] fin[p][pos + tap][c]
      const int job = w + 4 * jj;
      if (job < 14) {
        const int n = job * 16 + lr, t = n / C, c = n % C;
        const bool nok = n < 9 * C, mok = lr < kYH;
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
          const int kk = 4 * s2 + lk, p = kk >> 2, pos = kk & 3;
          const int nb = nok ? nbr2(pos, t / 3 - 1, t % 3 - 1) : -1;
          const float av = S.Dc[p][pos][mok ? lr : 0], bv = S.fin[p][nb >= 0 ? nb : 0][nok ? c : 0];
          cF0[jj] = mfma4(mok ? av : 0.f, nb >= 0 ? bv : 0.f, cF0[jj]);
        }
      }
    }
    L2_FOR(i, kP * HW * C) {  // dL/dfin: the z1 half joins gz1, the other goes on through the ReLU
      const int p = i / (HW * C), rem = i - p * (HW * C), pos = rem / C, c = rem - pos * C;
      float a = 0.f;
#pragma unroll 1
      for (int t = 0; t < 9; ++t) {
        const int po = nbr2(pos, -(t / 3 - 1), -(t % 3 - 1));
        if (po < 0) continue;
#pragma unroll
        for (int o = 0; o < kYH; ++o) a = fmaf(F[A::f0w + (t * C + c) * kYH + o], S.Dc[p][po][o], a);
      }
      if (c >= CH)
        S.gz[p][(c - CH) * HW + pos] += a;
      else
        S.Dd[p][pos][c] = S.fin[p][pos][c] > 0.f ? a : 0.f;
    }
    __syncthreads();
    own(row, first, St::offF + A::r4b, CH, [&](int j) {
      float a = 0.f;
      for (int k = 0; k < kP * HW; ++k) a += S.Dd[k >> 2][k & 3][j];
      return a;
    });
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {  // r4w: dW[o][n = (t, c)] = sum Dd[p][pos][o] r2[p][pos + tap][c]
      const int job = w + 4 * jj;
      if (job < 7) {
        const int n = job * 16 + lr, t = n / CH, c = n % CH;
        const bool nok = n < 9 * CH, mok = lr < CH;
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
          const int kk = 4 * s2 + lk, p = kk >> 2, pos = kk & 3;
          const int nb = nok ? nbr2(pos, t / 3 - 1, t % 3 - 1) : -1;
          const float av = S.Dd[p][pos][mok ? lr : 0], bv = S.r2[p][nb >= 0 ? nb : 0][nok ? c : 0];
          cR4[jj] = mfma4(mok ? av : 0.f, nb >= 0 ? bv : 0.f, cR4[jj]);
        }
      }
    }
    L2_FOR(i, kP * HW * CH) {
      const int p = i / (HW * CH), rem = i - p * (HW * CH), pos = rem / CH, c = rem - pos * CH;
      float a = 0.f;
#pragma unroll 1
      for (int t = 0; t < 9; ++t) {
        const int po = nbr2(pos, -(t / 3 - 1), -(t % 3 - 1));
        if (po < 0) continue;
#pragma unroll
        for (int o = 0; o < CH; ++o) a = fmaf(F[A::r4w + (t * CH + c) * CH + o], S.Dd[p][po][o], a);
      }
      S.De[p][pos][c] = S.r2[p][pos][c] > 0.f ? a : 0.f;
    }
    __syncthreads();
    own(row, first, St::offF + A::r2b, CH, [&](int j) {
      float a = 0.f;
      for (int k = 0; k < kP * HW; ++k) a += S.De[k >> 2][k & 3][j];
      return a;
    });
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {  // r2w: dW[o][n = (ab, ci)] = sum De[p][pos][o] r1[p][pos's block at ab][ci]
      const int ab = w + 4 * jj;
      const bool mok = lr < CH;
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) {
        const int kk = 4 * s2 + lk, p = kk >> 2, pos = kk & 3;
        const float av = S.De[p][pos][mok ? lr : 0];
        const float bv = S.r1[p][(4 * (pos >> 1) + (ab >> 2)) * 8 + 4 * (pos & 1) + (ab & 3)][lr];
        cR2[jj] = mfma4(mok ? av : 0.f, bv, cR2[jj]);
      }
    }
    __syncthreads();
    L2_FOR(i, kP * 1024) {  // dL/d(resize conv 1 pre-activation), in place of r1
      const int p = i >> 10, pos = (i >> 4) & 63, ci = i & 15, r = pos >> 3, s = pos & 7;
      const int p4 = (r >> 2) * 2 + (s >> 2), ab = (r & 3) * 4 + (s & 3);
      float a = 0.f;
#pragma unroll
      for (int o = 0; o < CH; ++o) a = fmaf(F[A::r2w + (ab * 16 + ci) * CH + o], S.De[p][p4][o], a);
      S.r1[p][pos][ci] = S.r1[p][pos][ci] > 0.f ? a : 0.f;
    }
    __syncthreads();
    own(row, first, St::offF + A::r0b, 16, [&](int j) {
      float a = 0.f;
      for (int k = 0; k < kP * 64; ++k) a += S.r1[k >> 6][k & 63][j];
      return a;
    });
    {  // r0w: dW[ci][n = (t, c)] = sum_(p, 8x8 pos) d1[p][pos][ci] x[p][c][pos + tap]; wave w: column
       // tile w & 1, particles 4 (w >> 1) .. + 3 (the halves are added at the end)
      const int n = (w & 1) * 16 + lr, t = n / 3, c = n % 3;
      const bool nok = n < 27;
#pragma unroll 4
      for (int s2 = 0; s2 < 64; ++s2) {
        const int kk = 4 * s2 + lk, p = 4 * (w >> 1) + (kk >> 6), pos = kk & 63;
        const int nb = nok ? nbr8(pos, t / 3 - 1, t % 3 - 1) : -1;
        const float av = S.r1[p][pos][lr], bv = S.X[p][(nok ? c : 0) * 64 + (nb >= 0 ? nb : 0)];
        cR0 = mfma4(av, nb >= 0 ? bv : 0.f, cR0);
      }
    }
    L2_FOR(i, kP * kE) {  // dL/dx from the resize conv 1
      const int p = i / kE, n = i - p * kE, c = n >> 6, pos = n & 63;
      float a = 0.f;
#pragma unroll 1
      for (int t = 0; t < 9; ++t) {
        const int po = nbr8(pos, -(t / 3 - 1), -(t % 3 - 1));
        if (po < 0) continue;
#pragma unroll
        for (int ci = 0; ci < 16; ++ci) a = fmaf(F[A::r0w + (t * 3 + c) * 16 + ci], S.r1[p][po][ci], a);
      }
      S.gX[p][n] += a;
    }
    // 1x1 conv and actnorm: dL/dyw = gz (z1 | z2)
    L2_FOR(i, kP * C * C) {  // dL/dW[o][c] = sum_pos gz[o] ya[c] + 4 gobj W^-T[o][c], then through the tanh
      const int p = i / (C * C), e = i - p * (C * C), o = e / C, c = e - o * C;
      float a = 0.f;
#pragma unroll
      for (int pos = 0; pos < HW; ++pos) a = fmaf(S.gz[p][o * HW + pos], S.ya[p][c * HW + pos], a);
      a = fmaf((float)HW * S.gobj[p], S.gw[p][e], a);
      const float t = S.wm[p][e];
      S.gw[p][e] = a * (1.0f - t * t);
    }
    L2_FOR(i, kP * NZ) {  // dL/d(input); the actnorm terms per element (Da: logs, Ea: bias)
      const int p = i / NZ, e = i - p * NZ, c = e >> 2, pos = e & 3;
      float a = 0.f;
#pragma unroll
      for (int o = 0; o < C; ++o) a = fmaf(S.wm[p][o * C + c], S.gz[p][o * HW + pos], a);
      const float gy0 = a * expf(S.an[p][c]);
      if (S.valid[p]) gz_out[S.m[p] * NZ + e] = gy0;
      (&S.Da[p][0][0])[e] = a * S.ya[p][e];
      (&S.Ea[p][0][0])[e] = gy0;
    }
    __syncthreads();
    L2_FOR(i, kP * 2 * C) {
      const int p = i / (2 * C), n = i - p * (2 * C), c = n % C;
      const float *src = n < C ? &S.Da[p][0][0] : &S.Ea[p][0][0];
      float v = 0.f;
#pragma unroll
      for (int pos = 0; pos < HW; ++pos) v += src[c * HW + pos];
      if (n < C) v = fmaf((float)HW, S.gobj[p], v);
      const float t = S.an[p][n];
      S.gan[p][n] = v * (1.0f - t * t);
    }
    __syncthreads();
    // ---------------- conditioning nets backward ----------------
    // last layers: dW[n][k] = sum_p g[p][n] l1[p][k] (the 8 particles are the GEMM's K)
#pragma unroll
    for (int jj = 0; jj < 9; ++jj) {
      const int n0 = (w + 4 * jj) * 16;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int kk = 4 * s2 + lk;
        cL4I[jj] = mfma4(S.gw[kk][n0 + lr], S.l1[kk][kXS + lr], cL4I[jj]);
      }
    }
    if (w < 3) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int kk = 4 * s2 + lk;
        cL4A = mfma4(S.gan[kk][w * 16 + lr], S.l1[kk][lr], cL4A);
      }
    }
    own(row, first, St::offA + CA::l4b, 2 * C, [&](int j) {
      float a = 0.f;
      for (int p = 0; p < kP; ++p) a += S.gan[p][j];
      return a;
    });
    own(row, first, St::offI + CI::l4b, C * C, [&](int j) {
      float a = 0.f;
      for (int p = 0; p < kP; ++p) a += S.gw[p][j];
      return a;
    });
    L2_FOR(i, kP * 32) {
      const int p = i >> 5, net = (i >> 4) & 1, k = i & 15;
      float a = 0.f;
      if (net == 0) {
        for (int n = 0; n < 2 * C; ++n) a = fmaf(gA[CA::l4w + n * kXS + k], S.gan[p][n], a);
      } else {
        for (int n = 0; n < C * C; ++n) a = fmaf(gI[CI::l4w + n * kXS + k], S.gw[p][n], a);
      }
      S.Gl1[p][net * kXS + k] = S.l1[p][net * kXS + k] > 0.f ? a : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int net = 0; net < 2; ++net) {
      const int off = net ? St::offI : St::offA;
      own(row, first, off + CA::l2w, kXS * kXS, [&](int j) {
        const int o = j / kXS, k = j % kXS;
        float a = 0.f;
        for (int p = 0; p < kP; ++p) a = fmaf(S.Gl1[p][net * kXS + o], S.l0[p][net * kXS + k], a);
        return a;
      });
      own(row, first, off + CA::l2b, kXS, [&](int j) {
        float a = 0.f;
        for (int p = 0; p < kP; ++p) a += S.Gl1[p][net * kXS + j];
        return a;
      });
    }
    L2_FOR(i, kP * 32) {
      const int p = i >> 5, net = (i >> 4) & 1, k = i & 15;
      const float *G = net ? gI : gA;
      float a = 0.f;
#pragma unroll
      for (int o = 0; o < kXS; ++o) a = fmaf(G[CA::l2w + o * kXS + k], S.Gl1[p][net * kXS + o], a);
      S.Gl0[p][net * kXS + k] = S.l0[p][net * kXS + k] > 0.f ? a : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int net = 0; net < 2; ++net) {
      const int off = net ? St::offI : St::offA;
      own(row, first, off + CA::l0w, kXS * kXH, [&](int j) {
        const int o = j / kXH, k = j % kXH;
        float a = 0.f;
        for (int p = 0; p < kP; ++p) a = fmaf(S.Gl0[p][net * kXS + o], S.c3[p][net * kXH + k], a);
        return a;
      });
      own(row, first, off + CA::l0b, kXS, [&](int j) {
        float a = 0.f;
        for (int p = 0; p < kP; ++p) a += S.Gl0[p][net * kXS + j];
        return a;
      });
    }
    L2_FOR(i, kP * 16) {
      const int p = i >> 4, net = (i >> 3) & 1, k = i & 7;
      const float *G = net ? gI : gA;
      float a = 0.f;
#pragma unroll
      for (int o = 0; o < kXS; ++o) a = fmaf(G[CA::l0w + o * kXH + k], S.Gl0[p][net * kXS + o], a);
      S.Gc3[p][net * kXH + k] = S.c3[p][net * kXH + k] > 0.f ? a : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int net = 0; net < 2; ++net) {
      const int off = net ? St::offI : St::offA;
      own(row, first, off + CA::c4w, kXH * kXH * 4, [&](int j) {  // [o][ci][a][b]
        const int o = j / 32, ci = (j / 4) % kXH, ab = j % 4;
        float a = 0.f;
        for (int p = 0; p < kP; ++p) a = fmaf(S.Gc3[p][net * kXH + o], S.c2[p][ab][net * kXH + ci], a);
        return a;
      });
      own(row, first, off + CA::c4b, kXH, [&](int j) {
        float a = 0.f;
        for (int p = 0; p < kP; ++p) a += S.Gc3[p][net * kXH + j];
        return a;
      });
    }
    L2_FOR(i, kP * 64) {
      const int p = i >> 6, ab = (i >> 4) & 3, net = (i >> 3) & 1, ci = i & 7;
      const float *G = net ? gI : gA;
      float a = 0.f;
#pragma unroll
      for (int o = 0; o < kXH; ++o) a = fmaf(G[CA::c4w + o * 32 + ci * 4 + ab], S.Gc3[p][net * kXH + o], a);
      S.Gc2[p][ab][net * kXH + ci] = S.c2[p][ab][net * kXH + ci] > 0.f ? a : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int net = 0; net < 2; ++net)
      own(row, first, (net ? St::offI : St::offA) + CA::c2b, kXH, [&](int j) {
        float a = 0.f;
        for (int k = 0; k < kP * 4; ++k) a += S.Gc2[k >> 2][k & 3][net * kXH + j];
        return a;
      });
    {  // c2w of net w >> 1, column tile w & 1: dW[o][n = (ci, ab)] = sum_(p, pos) Gc2[p][pos][o] c1[p][..][ci]
      const int net = w >> 1, n = (w & 1) * 16 + lr, ci = n >> 2, ab = n & 3;
      const bool mok = lr < kXH;
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) {
        const int kk = 4 * s2 + lk, p = kk >> 2, pos = kk & 3;
        const float av = S.Gc2[p][pos][net * kXH + (mok ? lr : 0)];
        const float bv = S.c1[p][(2 * (pos >> 1) + (ab >> 1)) * 4 + 2 * (pos & 1) + (ab & 1)][net * kXH + ci];
        cC2 = mfma4(mok ? av : 0.f, bv, cC2);
      }
    }
    L2_FOR(i, kP * 256) {
      const int p = i >> 8, q = (i >> 4) & 15, no = i & 15, net = no >> 3, ci = no & 7, qi = q >> 2, qj = q & 3;
      const int pos = (qi >> 1) * 2 + (qj >> 1), ab = (qi & 1) * 2 + (qj & 1);
      const float *G = net ? gI : gA;
      float a = 0.f;
#pragma unroll
      for (int o = 0; o < kXH; ++o) a = fmaf(G[CA::c2w + o * 32 + ci * 4 + ab], S.Gc2[p][pos][net * kXH + o], a);
      S.Gc1[p][q][no] = S.c1[p][q][no] > 0.f ? a : 0.f;
    }
    __syncthreads();
    if (w == 2) {  // c0w of both nets (rows net * 8 + o): dW[o][k = (ci, a, b)] = sum_(p,q) Gc1 x
      const int n = lr < 12 ? lr : 0, ci = n >> 2, a2 = (n >> 1) & 1, b2 = n & 1;
#pragma unroll 4
      for (int s2 = 0; s2 < 32; ++s2) {
        const int kk = 4 * s2 + lk, p = kk >> 4, q2 = kk & 15;
        const float av = S.Gc1[p][q2][lr];
        const float bv = S.X[p][ci * 64 + (2 * (q2 >> 2) + a2) * 8 + 2 * (q2 & 3) + b2];
        cC0 = mfma4(av, lr < 12 ? bv : 0.f, cC0);
      }
    }
#pragma unroll
    for (int net = 0; net < 2; ++net)
      own(row, first, (net ? St::offI : St::offA) + CA::c0b, kXH, [&](int j) {
        float a = 0.f;
        for (int k = 0; k < kP * 16; ++k) a += S.Gc1[k >> 4][k & 15][net * kXH + j];
        return a;
      });
    L2_FOR(i, kP * kE) {  // dL/dx from both conditioning conv 1s; the condition's gradient goes out
      const int p = i / kE, n = i - p * kE, ci = n >> 6, r = (n >> 3) & 7, s = n & 7;
      const int q = (r >> 1) * 4 + (s >> 1), k = ci * 4 + (r & 1) * 2 + (s & 1);
      float a = 0.f;
#pragma unroll
      for (int no = 0; no < 16; ++no) a = fmaf(((no >> 3) ? gI : gA)[CA::c0w + k * kXH + (no & 7)], S.Gc1[p][q][no], a);
      const float v = S.gX[p][n] + a;
      if (S.valid[p]) gx_out[S.m[p] * kE + n] = v;
    }
    __syncthreads();
  }
  // the MFMA accumulators into this workgroup's row
  const int oF = St::offF;
#pragma unroll
  for (int jj = 0; jj < 3; ++jj) {
    const int job = w + 4 * jj;
    if (job < 10) {
      const int rt = job / 5, ct = job % 5;
      store_tile(cF4[jj], row, C - rt * 16, ct * 16, 9 * kYH,
                 [=](int m, int n) { return oF + A::f4w + n * C + rt * 16 + m; });
    }
  }
  if (w == 1) store_tile(cF2, row, kYH, 0, kYH, [=](int m, int n) { return oF + A::f2w + n * kYH + m; });
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int job = w + 4 * jj;
    if (job < 14) store_tile(cF0[jj], row, kYH, job * 16, 9 * C, [=](int m, int n) { return oF + A::f0w + n * kYH + m; });
  }
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int job = w + 4 * jj;
    if (job < 7) store_tile(cR4[jj], row, CH, job * 16, 9 * CH, [=](int m, int n) { return oF + A::r4w + n * CH + m; });
  }
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int ab = w + 4 * jj;
    store_tile(cR2[jj], row, CH, 0, 16, [=](int m, int n) { return oF + A::r2w + (ab * 16 + n) * CH + m; });
  }
#pragma unroll
  for (int jj = 0; jj < 9; ++jj) {
    const int n0 = (w + 4 * jj) * 16;
    store_tile(cL4I[jj], row, 16, 0, kXS, [=](int m, int n) { return St::offI + CI::l4w + (n0 + m) * kXS + n; });
  }
  if (w < 3) store_tile(cL4A, row, 16, 0, kXS, [=](int m, int n) { return St::offA + CA::l4w + (w * 16 + m) * kXS + n; });
  {
    const int net = w >> 1;
    store_tile(cC2, row, kXH, (w & 1) * 16, 32,
               [=](int m, int n) { return (net ? St::offI : St::offA) + CA::c2w + m * 32 + n; });
  }
  if (w == 2)
    store_tile(cC0, row, 16, 0, 12,
               [=](int m, int n) { return ((m >> 3) ? St::offI : St::offA) + CA::c0w + n * kXH + (m & 7); });
  // r0w: the two particle halves (waves w and w + 2) added in a fixed order
  const int l = tid & 63;
  if (w >= 2)
#pragma unroll
    for (int i = 0; i < 4; ++i) S.cmb[w - 2][l][i] = cR0[i];
  __syncthreads();
  if (w < 2) {
    f4 t = cR0;
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] += S.cmb[w][l][i];
    store_tile(t, row, 16, w * 16, 27, [=](int m, int n) { return oF + A::r0w + n * 16 + m; });
  }
}

static int grid_of(int64_t M) { return (int)std::max<int64_t>(1, std::min<int64_t>((M + kP - 1) / kP, kGrid)); }

}  // namespace l2

static int split_grid(int64_t M) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((M + kSpP - 1) / kSpP, kSpGrid));
}

// Workspace (floats): the steps' partial rows (level 1, or level 2 where that is larger) | the
// forward's outputs (L = 1: z_0 .. z_{K-1}; L = 2: the MID layout of cglow_levels.hip) | two dL/dz
// and two condition-gradient hand-over buffers, [M, 192] each | the top prior's partial rows |
// L = 2: Split2d's partial rows.
static int64_t align64(int64_t n) { return (n + 63) / 64 * 64; }
static int64_t step_partial_floats(int64_t M, int L) {
  const int64_t p1 = cglow_bwd_partial_floats(M);
  return L == 2 ? std::max<int64_t>(p1, align64((int64_t)l2::grid_of(M) * Step2::size)) : p1;
}
static int64_t mid_floats(int64_t M, int K, int L) {
  return (int64_t)K * M * kE + (L == 2 ? (int64_t)(K + 1) * M * (kC2 * 4) : 0);
}
static int64_t top_floats() { return (int64_t)kTopRows * 2 * kE; }
static int64_t workspace_floats(int64_t M, int K, int L) {
  return step_partial_floats(M, L) + mid_floats(M, K, L) + 4 * M * kE + top_floats() +
         (L == 2 ? (int64_t)kSpGrid * kSplit : 0);
}

static int launch(bool part, const float *pe, const float *glow, int K, int L, const float *top, const float *enc,
                  int64_t enc_rs, const float *x, int64_t x_rs, int B, int N, const float *g_up, int64_t gup_rs,
                  const float *g_z, float *g_y, float *g_x, float *g_glow, float *g_pe, void *ws, hipStream_t st,
                  const char *fn) {
  const int64_t M = (int64_t)B * N;
  const int nz = top_n(L);
  float *partial = (float *)ws, *zmid = partial + step_partial_floats(M, L);
  float *hand = zmid + mid_floats(M, K, L);
  float *gzb[2] = {hand, hand + M * kE}, *gxb[2] = {hand + 2 * M * kE, hand + 3 * M * kE};
  float *tpart = hand + 4 * M * kE, *spart = tpart + top_floats();
  const float sign = part ? 1.0f : -1.0f;
  // flow form: x is the condition [M, 192] (xin), enc = y
  int rc;
  if (L == 1)
    rc = part ? cglow_forward_mid(pe, glow, K, enc, enc_rs, x, x_rs, B, N, nullptr, zmid, st)
              : cglow_forward_mid(glow, glow, K, enc, enc_rs, nullptr, 0, B, N, x, zmid, st);
  else
    rc = part ? cglow_levels_forward_mid(pe, glow, K, L, enc, enc_rs, x, x_rs, B, N, nullptr, zmid, st)
              : cglow_levels_forward_mid(glow, glow, K, L, enc, enc_rs, nullptr, 0, B, N, x, zmid, st);
  if (rc != NFDPF_OK) return rc;
  const float *z1last = zmid + (int64_t)(K - 1) * M * kE;  // the last level-1 step's output
  float *g_top = g_glow + levels_size(K, L, false);
  const int rows = top_rows(M);
  if (L == 1) {
    cglow_top_bwd_kernel<<<rows, kTopThreads, 0, st>>>(z1last, top, g_z, g_up, gup_rs, N, sign, M, nz, gzb[1], tpart);
    if (top) cglow_rows_reduce_kernel<<<(2 * nz + 255) / 256, 256, 0, st>>>(tpart, rows, 2 * nz, g_top);
    (void)hipMemsetAsync(gxb[1], 0, sizeof(float) * M * kE, st);  // no condition gradient above step K-1
  } else {
    const float *z2 = zmid + (int64_t)K * M * kE;  // level-2 inputs / outputs [k][M][96]
    // two [M, 96] hand-over buffers inside gzb[0]; launch j (from the top) reads g96[j & 1]
    float *g96[2] = {gzb[0], gzb[0] + M * nz};
    cglow_top_bwd_kernel<<<rows, kTopThreads, 0, st>>>(z2 + (int64_t)K * M * nz, top, g_z, g_up, gup_rs, N, sign, M, nz,
                                                       g96[0], tpart);
    if (top) cglow_rows_reduce_kernel<<<(2 * nz + 255) / 256, 256, 0, st>>>(tpart, rows, 2 * nz, g_top);
    const int grid = l2::grid_of(M);
    const size_t lds = sizeof(l2::Lds);
    ensure_max_dynamic_lds((const void *)l2::cglow_l2_step_bwd_kernel<true>, (int)lds);
    ensure_max_dynamic_lds((const void *)l2::cglow_l2_step_bwd_kernel<false>, (int)lds);
    const float *sp = glow + (int64_t)K * kStep;
    float *g_sp = g_glow + (int64_t)K * kStep;
    for (int j = 0; j < K; ++j) {
      const int k = K - 1 - j;
      // launch j writes the condition's gradient to gxb[(K - j) & 1], so the last one writes gxb[1]
      const float *gx_in = j == 0 ? nullptr : gxb[(K - j + 1) & 1];
      float *gx_out = gxb[(K - j) & 1];
      const float *gl = sp + kSplit + (int64_t)k * Step2::size;
      if (part)
        l2::cglow_l2_step_bwd_kernel<true><<<grid, l2::kT, lds, st>>>(pe, gl, x, x_rs, nullptr, B, N, g_up, gup_rs,
                                                                      z2 + (int64_t)k * M * nz, g96[j & 1], gx_in,
                                                                      g96[(j + 1) & 1], gx_out, partial);
      else
        l2::cglow_l2_step_bwd_kernel<false><<<grid, l2::kT, lds, st>>>(nullptr, gl, nullptr, 0, x, B, N, g_up, gup_rs,
                                                                       z2 + (int64_t)k * M * nz, g96[j & 1], gx_in,
                                                                       g96[(j + 1) & 1], gx_out, partial);
      cglow_rows_reduce_kernel<<<(Step2::size + 255) / 256, 256, 0, st>>>(partial, grid, Step2::size,
                                                                          g_sp + kSplit + (int64_t)k * Step2::size);
    }
    const int sgrid = split_grid(M);
    cglow_split_bwd_kernel<<<sgrid, kSpThreads, 0, st>>>(sp, z1last, g96[K & 1], g_up, gup_rs, N, sign, M, gzb[1], spart);
    cglow_rows_reduce_kernel<<<(kSplit + 255) / 256, 256, 0, st>>>(spart, sgrid, kSplit, g_sp);
  }
  const int rl = launch_status(fn);
  if (rl != NFDPF_OK) return rl;
  const int rb = cglow_bwd_below(part, pe, glow, K, zmid, enc, enc_rs, x, x_rs, B, N, g_up, gup_rs, gzb, gxb, g_y, g_x,
                                 g_glow, g_pe, partial, st);
  return rb != NFDPF_OK ? rb : launch_status(fn);
}

}  // namespace cglb
}  // namespace nfdpf

using namespace nfdpf;
using namespace nfdpf::cgl;

#define NFDPF_LEVELS_BWD_RANGE(fn)                                                                              \
  NFDPF_REQUIRE(K >= 1 && K <= kMaxK && L >= 1 && L <= kMaxL,                                                   \
                fn ": built for flow_depth K in 1..4 and num_levels L in 1..2 (got K = %d, L = %d)", K, L)

extern "C" int64_t nfdpf_cglow_levels_backward_workspace(int64_t M, int K, int L) {
  if (M < 0 || K < 1 || K > kMaxK || L < 1 || L > kMaxL) return -1;
  return cglb::workspace_floats(M, K, L) * (int64_t)sizeof(float);
}

extern "C" int nfdpf_cglow_levels_measurement_backward(const float *pe_params, const float *glow_params, int K, int L,
                                                       const float *top, const float *enc, int64_t enc_rs,
                                                       const float *x, int64_t x_rs, int B, int N, const float *g_lik,
                                                       int64_t glik_rs, float *g_x, float *g_y, float *g_glow,
                                                       float *g_pe, void *workspace, void *stream) {
  NFDPF_LEVELS_BWD_RANGE("nfdpf_cglow_levels_measurement_backward");
  NFDPF_REQUIRE(B >= 0 && N >= 1, "nfdpf_cglow_levels_measurement_backward: bad sizes");
  NFDPF_REQUIRE(g_glow && g_pe, "nfdpf_cglow_levels_measurement_backward: null pointer");
  hipStream_t st = as_stream(stream);
  if (B == 0) {
    (void)hipMemsetAsync(g_glow, 0, sizeof(float) * levels_size(K, L, top != nullptr), st);
    (void)hipMemsetAsync(g_pe, 0, sizeof(float) * pe_size(kE), st);
    return launch_status("nfdpf_cglow_levels_measurement_backward");
  }
  NFDPF_REQUIRE(pe_params && glow_params && enc && x && g_lik && g_x && g_y && workspace,
                "nfdpf_cglow_levels_measurement_backward: null pointer");
  return cglb::launch(true, pe_params, glow_params, K, L, top, enc, enc_rs, x, x_rs, B, N, g_lik, glik_rs, nullptr,
                      g_y, g_x, g_glow, g_pe, workspace, st, "nfdpf_cglow_levels_measurement_backward");
}

extern "C" int nfdpf_cglow_levels_flow_backward(const float *glow_params, int K, int L, const float *top,
                                                const float *x, const float *y, int64_t M, const float *g_z,
                                                const float *g_nll, float *g_x, float *g_y, float *g_glow,
                                                void *workspace, void *stream) {
  NFDPF_LEVELS_BWD_RANGE("nfdpf_cglow_levels_flow_backward");
  NFDPF_REQUIRE(M >= 0 && M <= (int64_t)INT32_MAX, "nfdpf_cglow_levels_flow_backward: bad size");
  NFDPF_REQUIRE(g_glow, "nfdpf_cglow_levels_flow_backward: null pointer");
  hipStream_t st = as_stream(stream);
  if (M == 0) {
    (void)hipMemsetAsync(g_glow, 0, sizeof(float) * levels_size(K, L, top != nullptr), st);
    return launch_status("nfdpf_cglow_levels_flow_backward");
  }
  NFDPF_REQUIRE(glow_params && x && y && g_nll && g_x && g_y && workspace,
                "nfdpf_cglow_levels_flow_backward: null pointer");
  return cglb::launch(false, nullptr, glow_params, K, L, top, y, kE, x, 0, (int)M, 1, g_nll, 1, g_z, g_y, g_x, g_glow,
                      nullptr, workspace, st, "nfdpf_cglow_levels_flow_backward");
}
