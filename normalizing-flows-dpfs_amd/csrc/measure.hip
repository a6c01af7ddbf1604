// measure.hip -- standalone measurement models behind nfdpf_measurement, at every frame-encoding
// width of meas_widths.hpp: cos (model/models.py:206-219), CRNVP (:256-278), NN (:221-235),
// gaussian (:237-254).  One workgroup per batch row (the row max of CRNVP / gaussian is a row
// reduction), one particle per lane, the weights through scalar loads.  At E = 64 the CRNVP
// instance keeps e[64], the two flow halves and one coupling's t / s in registers (478 VGPRs +
// AGPRs): 256 threads per workgroup leave each wave the whole 512-register budget of its SIMD,
// and no instance spills a VGPR (DESIGN.md §3 has the compiler's figures per instance).
#include "meas_widths.hpp"
#include "measure.hpp"

namespace nfdpf {

template <int E>
struct MeasRow {  // measure_row_setup's constants of this workgroup's row
  alignas(16) float encv[E];  // this row's frame encoding (raw)
  double vinv;                // cos: 1 / max(|encv|, 1e-12), fp64
  float nnrow[kNnH];          // NN: folded first layer of the obs half
  float f[16];                // block_max
};

template <int BLK, int E, int MEAS>
__global__ __launch_bounds__(BLK) void measurement_kernel(MeasArgs a, const float *__restrict__ enc,
                                                          const float *__restrict__ x, int N,
                                                          float *__restrict__ lik) {
  __shared__ MeasRow<E> L;
  const int b = blockIdx.x;
  measure_row_setup<MEAS, E>(enc + (int64_t)b * E, a.meas_params, L);
  __syncthreads();
  float m = -INFINITY;
  for (int i = threadIdx.x; i < N; i += BLK) {
    const int64_t o = (int64_t)b * N + i;
    const float v = measure<E, MEAS>(a, L.encv, &L.vinv, L.nnrow, x[2 * o], x[2 * o + 1]);
    lik[o] = v;
    m = fmaxf(m, v);
  }
  if (MEAS == NFDPF_MEAS_CRNVP || MEAS == NFDPF_MEAS_GAUSSIAN) {
    m = block_max(m, L.f);
    for (int i = threadIdx.x; i < N; i += BLK) lik[(int64_t)b * N + i] -= m;
  }
}

}  // namespace nfdpf

using namespace nfdpf;

extern "C" int nfdpf_meas_width_supported(int kind, int E) {
  const bool k = kind == NFDPF_MEAS_COS || kind == NFDPF_MEAS_CRNVP || kind == NFDPF_MEAS_NN ||
                 kind == NFDPF_MEAS_GAUSSIAN;
  return k && meas_width_ok(E) ? 1 : 0;
}

extern "C" int nfdpf_measurement(int kind, const float *pe_params, const float *meas_params,
                                 int n_flows, const float *enc, const float *x, int B, int N,
                                 int E, float prior_std, float *lik, void *stream) {
  NFDPF_REQUIRE(pe_params && enc && x && lik, "nfdpf_measurement: null pointer");
  NFDPF_REQUIRE(B >= 0 && N >= 1, "nfdpf_measurement: bad sizes");
  NFDPF_REQUIRE(meas_width_ok(E), "nfdpf_measurement: frame-encoding width E = %d is not built (%s)", E,
                kMeasWidthsStr);
  NFDPF_REQUIRE(!(kind == NFDPF_MEAS_CRNVP || kind == NFDPF_MEAS_NN) || meas_params,
                "nfdpf_measurement: meas_params missing");
  NFDPF_REQUIRE(kind != NFDPF_MEAS_CRNVP || (n_flows >= 0 && prior_std > 0.f),
                "nfdpf_measurement: bad CRNVP arguments");
  if (B == 0) return NFDPF_OK;
  hipStream_t st = as_stream(stream);
  MeasArgs a{pe_params, meas_params, n_flows, prior_std};
  bool known = true;
  for_meas_width(E, [&](auto w) {  // (E is listed: meas_width_ok above)
    constexpr int W = decltype(w)::value;
    switch (kind) {
      case NFDPF_MEAS_COS:
        measurement_kernel<256, W, NFDPF_MEAS_COS><<<B, 256, 0, st>>>(a, enc, x, N, lik);
        break;
      case NFDPF_MEAS_CRNVP:
        measurement_kernel<256, W, NFDPF_MEAS_CRNVP><<<B, 256, 0, st>>>(a, enc, x, N, lik);
        break;
      case NFDPF_MEAS_NN:
        measurement_kernel<256, W, NFDPF_MEAS_NN><<<B, 256, 0, st>>>(a, enc, x, N, lik);
        break;
      case NFDPF_MEAS_GAUSSIAN:
        measurement_kernel<256, W, NFDPF_MEAS_GAUSSIAN><<<B, 256, 0, st>>>(a, enc, x, N, lik);
        break;
      default:
        known = false;
    }
  });
  if (!known) {
    set_error("nfdpf_measurement: unsupported kind %d", kind);
    return NFDPF_EINVAL;
  }
  return launch_status("nfdpf_measurement");
}
