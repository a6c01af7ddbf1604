// measure_wide.hip -- the standalone measurement kernel of measure.hip at the frame-encoding
// widths of meas_widths.hpp other than kE: cos (model/models.py:206-219), CRNVP (:256-278),
// NN (:221-235), gaussian (:237-254).  One workgroup per batch row, one particle per lane, the
// weights through scalar loads -- measure.hip's layout.  At E = 64 the CRNVP instance keeps
// e[64], the two flow halves and one coupling's t / s in registers (478 VGPRs + AGPRs): 256
// threads per workgroup leave each wave the whole 512-register budget of its SIMD, and no
// instance spills a VGPR (DESIGN.md §3 has the compiler's figures per instance).
#include "meas_widths.hpp"
#include "measure_wide.hpp"

namespace nfdpf {

template <int BLK, int E, int MEAS>
__global__ __launch_bounds__(BLK) void measurement_wide_kernel(MeasArgs a, const float *__restrict__ enc,
                                                               const float *__restrict__ x, int N,
                                                               float *__restrict__ lik) {
  __shared__ WideShared<E> L;
  const int b = blockIdx.x;
  measure_row_setup_w<E, MEAS>(enc + (int64_t)b * E, a.meas_params, L);
  __syncthreads();
  float m = -INFINITY;
  for (int i = threadIdx.x; i < N; i += BLK) {
    const int64_t o = (int64_t)b * N + i;
    const float v = measure_w<E, MEAS>(a, L, x[2 * o], x[2 * o + 1]);
    lik[o] = v;
    m = fmaxf(m, v);
  }
  if (MEAS == NFDPF_MEAS_CRNVP || MEAS == NFDPF_MEAS_GAUSSIAN) {
    m = block_max(m, L.f);
    for (int i = threadIdx.x; i < N; i += BLK) lik[(int64_t)b * N + i] -= m;
  }
}

template <int E>
static int launch_wide(int kind, const MeasArgs &a, const float *enc, const float *x, int B, int N, float *lik,
                       hipStream_t st) {
  switch (kind) {
    case NFDPF_MEAS_COS:
      measurement_wide_kernel<256, E, NFDPF_MEAS_COS><<<B, 256, 0, st>>>(a, enc, x, N, lik);
      break;
    case NFDPF_MEAS_CRNVP:
      measurement_wide_kernel<256, E, NFDPF_MEAS_CRNVP><<<B, 256, 0, st>>>(a, enc, x, N, lik);
      break;
    case NFDPF_MEAS_NN:
      measurement_wide_kernel<256, E, NFDPF_MEAS_NN><<<B, 256, 0, st>>>(a, enc, x, N, lik);
      break;
    case NFDPF_MEAS_GAUSSIAN:
      measurement_wide_kernel<256, E, NFDPF_MEAS_GAUSSIAN><<<B, 256, 0, st>>>(a, enc, x, N, lik);
      break;
    default:
      set_error("nfdpf_measurement: unsupported kind %d", kind);
      return NFDPF_EINVAL;
  }
  return launch_status("nfdpf_measurement");
}

int measurement_wide(int kind, const MeasArgs &a, const float *enc, const float *x, int B, int N, int E, float *lik,
                     hipStream_t st) {
  int rc = NFDPF_EINVAL;
  const bool listed = for_meas_width(E, [&](auto w) {
    constexpr int W = decltype(w)::value;
    if constexpr (W != kE) rc = launch_wide<W>(kind, a, enc, x, B, N, lik, st);
  });
  if (!listed || E == kE) set_error("nfdpf_measurement: no wide kernel for E = %d", E);
  return rc;
}

}  // namespace nfdpf

using namespace nfdpf;

extern "C" int nfdpf_meas_width_supported(int kind, int E) {
  const bool k = kind == NFDPF_MEAS_COS || kind == NFDPF_MEAS_CRNVP || kind == NFDPF_MEAS_NN ||
                 kind == NFDPF_MEAS_GAUSSIAN;
  return k && meas_width_ok(E) ? 1 : 0;
}
