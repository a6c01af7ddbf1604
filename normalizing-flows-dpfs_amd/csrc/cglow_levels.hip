// cglow_levels.hip -- the conditional-GLOW measurement with L in 1..2 levels and an optional
// learnt top prior (nf/cglow/CGlowModel.py:54-107, 159-176 of the reference; -L / --num_levels
// and --learn_top), forward only, one launch per call.  cglow.hip stays the kernel of the
// default configuration (L = 1, learn_top off); this file takes what it does not.
//
// Per particle: x = particle_encoder(pos) (or given) as (3,8,8); y squeezed to (12,4,4);
// K CondGlowSteps at level 1; at L = 2 Split2d(12) (z2's Gaussian term under the prior
// tanh(conv(z1)) joins the log-det, z1 goes on), squeeze to (24,2,2), K CondGlowSteps at level 2;
// then the top Gaussian (learnt mean / logs, or zeros) and nll = -(log-dets + logp) / (192 log 2).
//
// Mapping: one workgroup = 256 threads = a tile of 16 particles, persistent over tiles, with
// workgroup barriers between phases; a CondGlowStep is ONE template over (channels C, grid side
// G), instantiated for (12, 4) and (24, 2).  The convolutions run on VALU with lane = (particle,
// position) and, where a particle has fewer than 16 positions, the wave = a group of the layer's
// output channels, so weights are wave-uniform scalar loads; the conditioning nets' last layer
// is f32 MFMA 16x16x4 with the 16 particles as M; the small remaining layers are loops over
// their outputs strided by the workgroup.  Every output is one fmaf chain in a fixed order, and
// sums over a particle (log-dets, Gaussian terms) go through LDS and are combined in a fixed
// order by the particle's 16 lanes, so a particle's result does not depend on its place in the
// batch.  No flags, spin waits, inter-workgroup hand-offs or atomics: a tile is local to its
// workgroup.
//
// LDS (67 KB, two workgroups per CU): xs 12 KB, y 12 KB, actnorm 3 KB, v1 2 KB and one 37 KB
// area `u` that holds, in turn, the encoder's hidden layers; the conditioning nets' activations;
// the per-particle C x C 1x1-conv matrix (16 x 577 floats at C = 24; eliminated in place for its
// log-determinant once the 1x1 conv has read it); the coupling's grids.
//
// The tile frame -- lane helpers, actnorm_invconv, split_squeeze, the tile's prologue and tail --
// is cglow_tile.hpp's, shared with cglow_wide.hip; cond_nets, coupling and the MID stores are here.
#include "cglow_tile.hpp"

namespace nfdpf {
namespace cgl {
using namespace cgt;  // the tile frame: kTileP, kThreads, kWmStride, the lane helpers
constexpr int kWgs = 2;                 // resident workgroups per CU (LDS)
// the coupling's grids inside `u` (the matrix is dead by then)
constexpr int kBufA = 0, kBufB = 3072, kFin = 5120, kUEnd = 8192;
// the conditioning nets' activations inside `u` (dead before the last layer writes the matrix)
constexpr int kCv1 = 0, kCv2 = 4096, kCv3 = 5120, kV0 = 5376;

struct Lds {
  float xs[kTileP][kE + 1];           // the condition x, [c][8][8]
  float y[kTileP][kE + 1];            // the flow's state, [c][position] (192 or 96 floats)
  float an[kTileP][2 * kC2 + 1];      // actnorm (logs | bias)
  float v1[kTileP][2 * kXS + 1];      // x_Linear's second layer (actnorm net | 1x1-conv net)
  float ld[kTileP];                   // the log-dets so far
  float pxy[kTileP][2];
  int row[kTileP];
  float u[kTileP * kWmStride];
};
static_assert(kUEnd <= kTileP * kWmStride && kV0 + kTileP * 2 * kXS <= kTileP * kWmStride, "areas fit in u");
static_assert(sizeof(Lds) * kWgs <= 160 * 1024, "two workgroups per CU");

typedef float f4 __attribute__((ext_vector_type(4)));

static __shared__ Lds S;
struct Tile {  // cglow_tile.hpp's view of this kernel: its S, and split_squeeze's two areas in S.u
  static __device__ __forceinline__ Lds &lds() { return S; }
  static constexpr int kSplitA = kBufA, kSplitB = kBufB;
};

// The two conditioning nets of a step (x_Con: three 2x2 stride-2 convs; x_Linear 8 -> 16 -> 16
// -> OUT, tanh) -> S.an (2 C) and the C x C matrix in S.u.
template <int C>
__device__ __noinline__ void cond_nets(const float *__restrict__ gA, const float *__restrict__ gI, int tid) {
  using CA = Cond<2 * C>;
  using CI = Cond<C * C>;
  float *cv1 = S.u + kCv1, *cv2 = S.u + kCv2, *cv3 = S.u + kCv3, *v0 = S.u + kV0;
  {  // conv 3 -> 8, 8x8 -> 4x4, both nets: lane = (particle, 4x4 position), scalar weights
    const int p = tid >> 4, q = tid & 15, qi = q >> 2, qj = q & 3;
    float in[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) in[k] = S.xs[p][(k >> 2) * 64 + (2 * qi + ((k >> 1) & 1)) * 8 + 2 * qj + (k & 1)];
#pragma unroll
    for (int net = 0; net < 2; ++net) {
      cfloat *G = uptr(net ? gI : gA);
#pragma unroll
      for (int o = 0; o < kXH; ++o) {
        float acc = G[CA::c0b + o];
#pragma unroll
        for (int k = 0; k < 12; ++k) acc = fmaf(G[CA::c0w + k * kXH + o], in[k], acc);
        cv1[tid * 16 + net * kXH + o] = relu(acc);
      }
    }
  }
  __syncthreads();
  {  // conv 8 -> 8, 4x4 -> 2x2: lane = (particle, 2x2 position), wave w takes net w / 2, outputs 4 (w % 2) ..
    const int l = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), p = l >> 2, pos = l & 3;
    const int pi = pos >> 1, pj = pos & 1, net = w >> 1, o0 = (w & 1) * 4;
    cfloat *G = uptr(net ? gI : gA);
    float acc[4];
#pragma unroll
    for (int oo = 0; oo < 4; ++oo) acc[oo] = G[CA::c2b + o0 + oo];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      const float v = cv1[(p * 16 + (2 * pi + ((k >> 1) & 1)) * 4 + 2 * pj + (k & 1)) * 16 + net * kXH + (k >> 2)];
#pragma unroll
      for (int oo = 0; oo < 4; ++oo) acc[oo] = fmaf(G[CA::c2w + (o0 + oo) * 32 + k], v, acc[oo]);
    }
#pragma unroll
    for (int oo = 0; oo < 4; ++oo) cv2[(p * 4 + pos) * 16 + net * kXH + o0 + oo] = relu(acc[oo]);
  }
  __syncthreads();
  {  // conv 8 -> 8, 2x2 -> 1x1
    const int p = tid >> 4, net = (tid >> 3) & 1, o = tid & 7;
    const float *G = net ? gI : gA;
    float acc = G[CA::c4b + o];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc = fmaf(G[CA::c4w + o * 32 + k], cv2[(p * 4 + (k & 3)) * 16 + net * kXH + (k >> 2)], acc);
    cv3[tid] = relu(acc);
  }
  __syncthreads();
  for (int i = tid; i < kTileP * 32; i += kThreads) {
    const int p = i >> 5, net = (i >> 4) & 1, o = i & 15;
    const float *G = net ? gI : gA;
    float acc = G[CA::l0b + o];
#pragma unroll
    for (int k = 0; k < kXH; ++k) acc = fmaf(G[CA::l0w + o * kXH + k], cv3[p * 16 + net * kXH + k], acc);
    v0[i] = relu(acc);
  }
  __syncthreads();
  for (int i = tid; i < kTileP * 32; i += kThreads) {
    const int p = i >> 5, net = (i >> 4) & 1, o = i & 15;
    const float *G = net ? gI : gA;
    float acc = G[CA::l2b + o];
#pragma unroll
    for (int k = 0; k < kXS; ++k) acc = fmaf(G[CA::l2w + o * kXS + k], v0[p * 32 + net * kXS + k], acc);
    S.v1[p][net * kXS + o] = relu(acc);
  }
  __syncthreads();  // cv1 .. v0 are dead: the matrix takes their place
  // last layer + tanh as f32 MFMA 16x16x4 tiles (an exact k-ordered fmaf chain): M = the 16
  // particles, N = 16 outputs per tile, K = 16; lane l feeds A[l % 16][4 s + l / 16] and
  // B[4 s + l / 16][l % 16] and gets C rows 4 (l / 16) + i, column l % 16.  Tiles are dealt to
  // the waves round-robin; a tile's weights are 4 vector loads per lane.
  constexpr int NA = 2 * C, NI = C * C, TA = (NA + 15) / 16, NTILE = TA + NI / 16;
  static_assert(NI % 16 == 0, "whole tiles");
  {
    const int l = tid & 63, w = tid >> 6, r = l & 15, kk = l >> 4;
    float aA[4], aI[4];
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      aA[s2] = S.v1[r][4 * s2 + kk];
      aI[s2] = S.v1[r][kXS + 4 * s2 + kk];
    }
#pragma unroll 1
    for (int job = w; job < NTILE; job += 4) {
      const bool isI = job >= TA;
      const int n = (isI ? job - TA : job) * 16 + r;
      const bool ok = n < (isI ? NI : NA);
      const int nn = ok ? n : 0;
      const float *G = isI ? gI : gA;
      float b[4];
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) b[s2] = G[CA::l4w + nn * kXS + 4 * s2 + kk];
      const float bias = G[(isI ? CI::l4b : CA::l4b) + nn];
      f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(isI ? aI[s2] : aA[s2], ok ? b[s2] : 0.f, acc, 0, 0, 0);
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

// cond-affine coupling of S.y in place; S.ld += sum log scale.
// Lane = (particle, position) and, where the grid has fewer than 16 positions (NQ = 16 / HW > 1),
// the wave takes one of NQ groups of a layer's output channels: the output group is wave-uniform,
// so every weight is a scalar load (constant address space) and a lane keeps its group's
// accumulators in registers.  Level 1: 16 positions, one group; level 2: 4 positions, 4 groups.
template <int C, int G>
__device__ __noinline__ void coupling(const float *__restrict__ Fp, int tid) {
  using A = AffL<C, G>;
  constexpr int HW = G * G, R = 8 / G, CH = C / 2, NQ = 16 / HW, CIQ = 16 / NQ;
  constexpr int Q4 = CH / NQ, Q8 = kYH / NQ;  // outputs per group of the CH-wide and 8-wide layers
  static_assert(CH % NQ == 0 && kYH % NQ == 0, "output groups");
  float *bufA = S.u + kBufA, *bufB = S.u + kBufB, *fin = S.u + kFin;
  static_assert(kTileP * HW * NQ * CH <= kBufB - kBufA && kTileP * HW * kYH <= kFin - kBufB && kTileP * HW * C <= kUEnd - kFin,
                "grids fit");
  const int l = tid & 63, oq = NQ == 1 ? 0 : __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = NQ == 1 ? tid >> 4 : l >> 2, pos = NQ == 1 ? tid & 15 : l & 3, pp = p * HW + pos;
  {
    // resize_x: conv 3 -> 16 (3x3, pad 1, at 8x8) ReLU, then the R x R stride-R conv 16 -> CH,
    // fused: the lane keeps its R x R block of conv-1 outputs in registers one hidden channel at
    // a time; group oq takes hidden channels [oq CIQ, (oq + 1) CIQ), the NQ partial sums meet
    // below in a fixed order
    cfloat *F = uptr(Fp);
    const int pi = pos / G, pj = pos % G;
    float acc[CH];
#pragma unroll
    for (int o = 0; o < CH; ++o) acc[o] = 0.f;
#pragma unroll 1
    for (int ci = oq * CIQ; ci < (oq + 1) * CIQ; ++ci) {
      const float b0 = F[A::r0b + ci];
#pragma unroll 1
      for (int ab = 0; ab < R * R; ++ab) {
        const int r = R * pi + ab / R, s = R * pj + ab % R;
        float h = b0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int rr = r + t / 3 - 1, ss = s + t % 3 - 1;
          const bool in = rr >= 0 && rr < 8 && ss >= 0 && ss < 8;
          const float *xr = &S.xs[p][in ? rr * 8 + ss : 0];
#pragma unroll
          for (int c = 0; c < 3; ++c) h = fmaf(F[A::r0w + (t * 3 + c) * 16 + ci], in ? xr[c * 64] : 0.f, h);
        }
        h = relu(h);
#pragma unroll
        for (int o = 0; o < CH; ++o) acc[o] = fmaf(F[A::r2w + (ab * 16 + ci) * CH + o], h, acc[o]);
      }
    }
#pragma unroll
    for (int o = 0; o < CH; ++o) bufA[(pp * NQ + oq) * CH + o] = acc[o];
  }
  __syncthreads();
  {
    cfloat *F = uptr(Fp);
#pragma unroll
    for (int oo = 0; oo < Q4; ++oo) {
      const int o = oq * Q4 + oo;
      float v = F[A::r2b + o];
#pragma unroll
      for (int q = 0; q < NQ; ++q) v += bufA[(pp * NQ + q) * CH + o];
      bufB[pp * CH + o] = relu(v);
    }
  }
  __syncthreads();
  {  // fin = cat(relu(conv CH -> CH (3x3) of the above), z1)
    cfloat *F = uptr(Fp);
    float acc[Q4];
#pragma unroll
    for (int oo = 0; oo < Q4; ++oo) acc[oo] = F[A::r4b + oq * Q4 + oo];
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
      const int nb = nbr<G>(pos, t);
      if (nb >= 0) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const float v = bufB[(p * HW + nb) * CH + c];
#pragma unroll
          for (int oo = 0; oo < Q4; ++oo) acc[oo] = fmaf(F[A::r4w + (t * CH + c) * CH + oq * Q4 + oo], v, acc[oo]);
        }
      }
    }
#pragma unroll
    for (int oo = 0; oo < Q4; ++oo) {
      fin[pp * C + oq * Q4 + oo] = relu(acc[oo]);
      fin[pp * C + CH + oq * Q4 + oo] = S.y[p][(oq * Q4 + oo) * HW + pos];
    }
  }
  __syncthreads();
  // f: Conv2dNormy(C -> 8, 3x3) ReLU, Conv2dNormy(8 -> 8, 1x1) ReLU, Conv2dZerosy(8 -> C, 3x3) tanh
  {
    cfloat *F = uptr(Fp);
    float acc[Q8];
#pragma unroll
    for (int oo = 0; oo < Q8; ++oo) acc[oo] = 0.f;
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
      const int nb = nbr<G>(pos, t);
      if (nb >= 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float v = fin[(p * HW + nb) * C + c];
#pragma unroll
          for (int oo = 0; oo < Q8; ++oo) acc[oo] = fmaf(F[A::f0w + (t * C + c) * kYH + oq * Q8 + oo], v, acc[oo]);
        }
      }
    }
#pragma unroll
    for (int oo = 0; oo < Q8; ++oo) {
      const int o = oq * Q8 + oo;
      bufA[pp * kYH + o] = relu((acc[oo] + F[A::f0ab + o]) * expf(F[A::f0al + o]));
    }
  }
  __syncthreads();
  {
    cfloat *F = uptr(Fp);
    float acc[Q8];
#pragma unroll
    for (int oo = 0; oo < Q8; ++oo) acc[oo] = 0.f;
#pragma unroll
    for (int c = 0; c < kYH; ++c) {
      const float v = bufA[pp * kYH + c];
#pragma unroll
      for (int oo = 0; oo < Q8; ++oo) acc[oo] = fmaf(F[A::f2w + c * kYH + oq * Q8 + oo], v, acc[oo]);
    }
#pragma unroll
    for (int oo = 0; oo < Q8; ++oo) {
      const int o = oq * Q8 + oo;
      bufB[pp * kYH + o] = relu((acc[oo] + F[A::f2ab + o]) * expf(F[A::f2al + o]));
    }
  }
  __syncthreads();
  {
    // (shift, scale) = channels (2 c, 2 c + 1) of f's output ("cross"); z2 = (z2 + shift) scale;
    // group oq takes the pairs c in [oq Q4, (oq + 1) Q4)
    cfloat *F = uptr(Fp);
    float as[Q4], ac[Q4];
#pragma unroll
    for (int cc = 0; cc < Q4; ++cc) as[cc] = ac[cc] = 0.f;
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
      const int nb = nbr<G>(pos, t);
      if (nb >= 0) {
#pragma unroll
        for (int k = 0; k < kYH; ++k) {
          const float g = bufB[(p * HW + nb) * kYH + k];
#pragma unroll
          for (int cc = 0; cc < Q4; ++cc) {
            as[cc] = fmaf(F[A::f4w + (t * kYH + k) * C + 2 * (oq * Q4 + cc)], g, as[cc]);
            ac[cc] = fmaf(F[A::f4w + (t * kYH + k) * C + 2 * (oq * Q4 + cc) + 1], g, ac[cc]);
          }
        }
      }
    }
#pragma unroll
    for (int cc = 0; cc < Q4; ++cc) {
      const int c = oq * Q4 + cc;
      const float hs = tanhf((as[cc] + F[A::f4b + 2 * c] + F[A::f4nb + 2 * c]) * expf(F[A::f4l + 2 * c] * 3.0f));
      const float hc = tanhf((ac[cc] + F[A::f4b + 2 * c + 1] + F[A::f4nb + 2 * c + 1]) * expf(F[A::f4l + 2 * c + 1] * 3.0f));
      const float sc = sigmoidf_(hc + 2.0f);
      float *z2 = &S.y[p][(CH + c) * HW + pos];
      *z2 = (*z2 + hs) * sc;
      bufA[pp * CH + c] = logf(sc);  // (bufA's last readers are behind the barrier above)
    }
  }
  __syncthreads();
  const float lsum = particle_sum(bufA, HW * CH, tid);
  if ((tid & 15) == 0) S.ld[tid >> 4] += lsum;
  __syncthreads();
}

template <int C, int G>
__device__ __forceinline__ void glow_step(const float *__restrict__ gs, int tid) {
  using St = StepL<C, G>;
  cond_nets<C>(gs + St::offA, gs + St::offI, tid);
  actnorm_invconv<Tile, C, G>(tid);
  coupling<C, G>(gs + St::offF, tid);
}

// the tile's state S.y (n floats per particle) to buf [M][n] (the MID forward)
__device__ __forceinline__ void mid_store(float *__restrict__ buf, int n, int64_t g0, int64_t total, int tid) {
  for (int i = tid; i < kTileP * n; i += kThreads) {
    const int p = i / n, e = i - p * n;
    if (g0 + p < total) buf[(g0 + p) * n + e] = S.y[p][e];
  }
}

// x: particle (b, i) at x + b * x_rs + 2 i;  enc: row b at enc + b * enc_rs (192 floats);
// lik: (b, i) at lik + b * lik_rs + i = out_sign * (-nll).  xin non-null: the flow form (the
// condition given per sample, N = 1, enc = y).  zout (may be null): the final z, nz floats per
// particle.  top (may be null): [mean | logs] of the top Gaussian, nz floats each.
// MID (the backward's forward pass, cglow_levels_bwd.hip; L = 2): no likelihood; zout receives
// every step's output instead -- the K level-1 outputs as [k][M][192] ((12, 4, 4)), then the
// level-2 inputs / outputs [k][M][96] ((24, 2, 2)), k = 0 the squeezed z1 after Split2d, k = K the
// final z.
template <bool MID>
__global__ __launch_bounds__(kThreads, kWgs) void cglow_levels_kernel(
    const float *__restrict__ pe, const float *__restrict__ glow, const float *__restrict__ top,
    const float *__restrict__ enc, int64_t enc_rs, const float *__restrict__ x, int64_t x_rs, int B, int N,
    float *__restrict__ lik, int64_t lik_rs, const float *__restrict__ xin, float *__restrict__ zout, float out_sign,
    int K, int L) {
  const int tid = threadIdx.x;
  const int64_t total = (int64_t)B * N;
  const int64_t ntiles = (total + kTileP - 1) / kTileP;
  const int nz = L == 2 ? kC2 * 4 : kE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t g0 = tile * kTileP;
    tile_load<Tile>(pe, enc, enc_rs, x, x_rs, N, xin, g0, total, tid);
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
      glow_step<kC, 4>(glow + (int64_t)k * kStep, tid);
      if constexpr (MID) mid_store(zout + (int64_t)k * total * kE, kE, g0, total, tid);
    }
    if (L == 2) {
      const float *g2 = glow + (int64_t)K * kStep;
      split_squeeze<Tile>(g2, tid);
      float *z2mid = MID ? zout + (int64_t)K * total * kE : nullptr;
      if constexpr (MID) mid_store(z2mid, kC2 * 4, g0, total, tid);
#pragma unroll 1
      for (int k = 0; k < K; ++k) {
        glow_step<kC2, 2>(g2 + kSplit + (int64_t)k * Step2::size, tid);
        if constexpr (MID) mid_store(z2mid + (int64_t)(k + 1) * total * (kC2 * 4), kC2 * 4, g0, total, tid);
      }
    }
    if constexpr (MID) {
      __syncthreads();
      continue;
    }
    // logdet0 = -log(256) * 192, a constant here
    tile_finish<Tile>(top, nz, -5.545177444479562f * (float)kE, lik, lik_rs, zout, out_sign, N, g0, total, tid);
  }
}

}  // namespace cgl

// The backward's forward pass (cglow_levels_bwd.hip): every step's output into zmid, in the MID
// layout above.  xin null: the measurement form; else the flow form (enc = y, N = 1), as
// cglow_forward_mid.
int cglow_levels_forward_mid(const float *pe, const float *glow, int K, int L, const float *enc, int64_t enc_rs,
                             const float *x, int64_t x_rs, int B, int N, const float *xin, float *zmid,
                             hipStream_t st) {
  const int grid = persistent_grid(((int64_t)B * N + cgl::kTileP - 1) / cgl::kTileP, cgl::kWgs);
  cgl::cglow_levels_kernel<true><<<grid, cgl::kThreads, 0, st>>>(pe, glow, nullptr, enc, enc_rs, x, x_rs, B, N, nullptr, 0,
                                                                xin, zmid, 1.0f, K, L);
  return launch_status("cglow_levels_forward_mid");
}
}  // namespace nfdpf

using namespace nfdpf;
using namespace nfdpf::cgl;

extern "C" int64_t nfdpf_cglow_levels_params_size(int K, int L, int learn_top) {
  return K >= 1 && K <= kMaxK && L >= 1 && L <= kMaxL ? levels_size(K, L, learn_top != 0) : -1;
}

#define NFDPF_LEVELS_RANGE(fn)                                                                                  \
  NFDPF_REQUIRE(K >= 1 && K <= kMaxK && L >= 1 && L <= kMaxL,                                                   \
                fn ": built for flow_depth K in 1..4 and num_levels L in 1..2 (got K = %d, L = %d)", K, L)

extern "C" int nfdpf_cglow_levels_measurement(const float *pe_params, const float *glow_params, int K, int L,
                                              const float *top, const float *enc, int64_t enc_rs, const float *x,
                                              int64_t x_rs, int B, int N, float *lik, int64_t lik_rs, void *stream) {
  NFDPF_REQUIRE(pe_params && glow_params && enc && x && lik, "nfdpf_cglow_levels_measurement: null pointer");
  NFDPF_LEVELS_RANGE("nfdpf_cglow_levels_measurement");
  NFDPF_REQUIRE(B >= 0 && N >= 1, "nfdpf_cglow_levels_measurement: bad sizes");
  if (B == 0) return NFDPF_OK;
  const int grid = persistent_grid(((int64_t)B * N + kTileP - 1) / kTileP, kWgs);
  cglow_levels_kernel<false><<<grid, kThreads, 0, as_stream(stream)>>>(pe_params, glow_params, top, enc, enc_rs, x, x_rs, B, N,
                                                                 lik, lik_rs, nullptr, nullptr, 1.0f, K, L);
  return launch_status("nfdpf_cglow_levels_measurement");
}

extern "C" int nfdpf_cglow_levels_flow(const float *glow_params, int K, int L, const float *top, const float *x,
                                       const float *y, int64_t M, float *z, float *nll, void *stream) {
  NFDPF_REQUIRE(glow_params && x && y && nll, "nfdpf_cglow_levels_flow: null pointer");
  NFDPF_LEVELS_RANGE("nfdpf_cglow_levels_flow");
  NFDPF_REQUIRE(M >= 0 && M <= (int64_t)INT32_MAX, "nfdpf_cglow_levels_flow: bad size");
  if (M == 0) return NFDPF_OK;
  // B = M rows of N = 1 (y row m is sample m), the condition x given, out_sign -1: nll
  const int grid = persistent_grid((M + kTileP - 1) / kTileP, kWgs);
  cglow_levels_kernel<false><<<grid, kThreads, 0, as_stream(stream)>>>(glow_params, glow_params, top, y, kE, nullptr, 0, (int)M,
                                                                 1, nll, 1, x, z, -1.0f, K, L);
  return launch_status("nfdpf_cglow_levels_flow");
}
