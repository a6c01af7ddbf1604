// measure_wide.hpp -- the per-particle measurement models of measure.hpp at a frame-encoding
// width E other than kE (meas_widths.hpp), for the standalone kernel of measure_wide.hip.
// Same arithmetic as measure.hpp's measure<MEAS> with E in place of kE, built from the same
// width-templated helpers (flows.hpp: particle_encode, encode_dot, fold_pair_c,
// coupling_forward); measure.hpp itself is not templated: the tuned step and pass kernels
// include it and their code generation must not move.
#pragma once

#include "measure.hpp"

namespace nfdpf {

template <int E>
struct WideShared {
  alignas(16) float encv[E];  // this row's frame encoding (raw)
  double vinv;                // cos: 1 / max(|encv|, 1e-12), fp64
  float nnrow[kNnH];          // NN: folded first layer of the obs half
  float f[16];
};

// measurement_model_cnf (model/models.py:256-278) at dim = obser_dim = E: see crnvp_lik
template <int E>
__device__ __forceinline__ float crnvp_lik_w(cfloat *pe, cfloat *mp, int n_flows, float prior_std, const float *encv,
                                             float x0, float x1) {
  float e[E];
  particle_encode<E>(pe, x0, x1, e);
  constexpr int HALF = E / 2;
  constexpr int ns = net_size<HALF, kH>(E);
  float lo[HALF], up[HALF];
#pragma unroll
  for (int k = 0; k < HALF; ++k) {
    lo[k] = encv[k];
    up[k] = encv[HALF + k];
  }
  float ld = 0.f;
  for (int f = 0; f < n_flows; ++f) {
    const auto fw = pair_ptr(mp) + f * 2 * ns;
    f2 cb[2 * kH];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < kH; ++j) cb[n * kH + j] = fold_pair_c<HALF, kH, E>(fw + n * ns, j, e);
    ld += coupling_forward<HALF, kH>(fw, E, lo, up, cb);
  }
  // the prior's quadratic form in fp64, as crnvp_lik
  const double is = 1.0 / (double)prior_std;
  double m = 0.0;
#pragma unroll
  for (int k = 0; k < HALF; ++k) {
    const double a = lo[k] * is, c = up[k] * is;
    m = fma(a, a, m);
    m = fma(c, c, m);
  }
  const double lp = -0.5 * (E * 1.8378770664093453 + m) - E * log((double)prior_std);
  return (float)(lp + (double)ld);
}

template <int E, int MEAS>
__device__ __forceinline__ float measure_w(const MeasArgs &d, const WideShared<E> &L, float x0, float x1) {
  if constexpr (MEAS == NFDPF_MEAS_COS) {
    double ss, dot;
    encode_dot<E>(wptr(d.pe_params), x0, x1, L.encv, ss, dot);
    return cos_lik(ss, dot, L.vinv);
  } else if constexpr (MEAS == NFDPF_MEAS_CRNVP) {
    return crnvp_lik_w<E>(wptr(d.pe_params), wptr(d.meas_params), d.n_flows, d.meas_prior_std, L.encv, x0, x1);
  } else if constexpr (MEAS == NFDPF_MEAS_GAUSSIAN) {
    // measurement_model_Gaussian with N(1, 100 I) (DPFs.py:84-86, model/models.py:237-254)
    float e[E];
    particle_encode<E>(wptr(d.pe_params), x0, x1, e);
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const float v = (L.encv[j] - e[j] - 1.0f) * 0.1f;
      m = fmaf(v, v, m);
    }
    return -0.5f * (E * 1.8378770664093453f + m) - E * 2.302585092994046f;
  } else {
    // measurement_model_NN (model/models.py:221-235): W1 [64, 2E] and W2 [64, 64] in row_pairs
    // layout, W3 [1, 64] and biases plain
    static_assert(MEAS == NFDPF_MEAS_NN, "measure_w: cos, CRNVP, gaussian or NN");
    float e[E];
    particle_encode<E>(wptr(d.pe_params), x0, x1, e);
    cfloat *P = wptr(d.meas_params);
    cf2 *W1 = (cf2 *)P;
    f2 h[kNnH / 2];
#pragma unroll
    for (int m = 0; m < kNnH / 2; ++m) {
      f2 a = f2{L.nnrow[2 * m], L.nnrow[2 * m + 1]};
#pragma unroll
      for (int k = 0; k < E; ++k) a = pfma(W1[m * 2 * E + E + k], splat(e[k]), a);
      h[m] = relu2(a);
    }
    cf2 *W2 = (cf2 *)(P + kNnH * 2 * E + kNnH), *b2 = (cf2 *)(P + kNnH * 2 * E + kNnH + kNnH * kNnH);
    cfloat *W3 = P + kNnH * 2 * E + kNnH + kNnH * kNnH + kNnH, *b3 = W3 + kNnH;
    float o = b3[0];
    for (int m = 0; m < kNnH / 2; ++m) {
      f2 a = b2[m];
#pragma unroll
      for (int k = 0; k < kNnH; ++k) a = pfma(W2[m * kNnH + k], splat(k & 1 ? h[k >> 1].y : h[k >> 1].x), a);
      o = fmaf(W3[2 * m], relu(a.x), o);
      o = fmaf(W3[2 * m + 1], relu(a.y), o);
    }
    return logf(1.0f / (1.0f + expf(-o)));
  }
}

// per-row constants of the measurement (frame encoding, NN obs-half fold); all threads call
template <int E, int MEAS>
__device__ __forceinline__ void measure_row_setup_w(const float *enc, const float *meas_params, WideShared<E> &L) {
  static_assert(E <= 64 && E % 2 == 0, "one wave holds the row's frame encoding");
  const int tid = threadIdx.x;
  if (tid < 64) {
    const float v = tid < E ? enc[tid] : 0.f;
    if (MEAS == NFDPF_MEAS_COS) {
      const double nrm = sqrt(wave_sum((double)v * v));
      if (tid == 0) L.vinv = 1.0 / fmax(nrm, 1e-12);
    }
    if (tid < E) L.encv[tid] = v;
  }
  if (MEAS == NFDPF_MEAS_NN && tid < kNnH) {
    // obs half of likelihood_est's first layer (row_pairs layout: [m][k][2], m = tid / 2)
    float a = meas_params[kNnH * 2 * E + tid];
    const float *w = meas_params + (tid >> 1) * 2 * E * 2 + (tid & 1);
    for (int k = 0; k < E; ++k) a = fmaf(w[2 * k], enc[k], a);
    L.nnrow[tid] = a;
  }
}

// nfdpf_measurement at a listed width other than kE (measure_wide.hip); arguments validated
// by the caller.  NFDPF_EINVAL (message set) for an unsupported kind.
int measurement_wide(int kind, const MeasArgs &a, const float *enc, const float *x, int B, int N, int E, float *lik,
                     hipStream_t st);

}  // namespace nfdpf
