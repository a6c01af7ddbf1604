// meas_widths.hpp -- THE list of frame-encoding widths (--hiddensize) the cos / CRNVP / NN /
// gaussian measurement kernels are built for, forward and backward.  A further width is one
// more X(...) entry here (even, <= 64: the backward kernels hold a row's encoding in one wave).
// The tuned step and pass kernels stay at kE (measure.hpp); the other widths run the standalone
// kernel of measure.hip (the same measure<E, MEAS>) and the width-templated backwards.
#pragma once

#include <type_traits>

#define NFDPF_MEAS_WIDTHS(X) X(16) X(32) X(64)

namespace nfdpf {

#define NFDPF_W_OR(W) || E == W
constexpr bool meas_width_ok(int E) { return false NFDPF_MEAS_WIDTHS(NFDPF_W_OR); }
#undef NFDPF_W_OR

#define NFDPF_W_STR(W) " " #W
constexpr const char *kMeasWidthsStr = "supported widths:" NFDPF_MEAS_WIDTHS(NFDPF_W_STR);
#undef NFDPF_W_STR

// f(std::integral_constant<int, W>{}) for the listed width W == E; false when E is not listed
template <class F>
inline bool for_meas_width(int E, F &&f) {
#define NFDPF_W_CASE(W)                        \
  if (E == W) {                                \
    f(std::integral_constant<int, W>{});       \
    return true;                               \
  }
  NFDPF_MEAS_WIDTHS(NFDPF_W_CASE)
#undef NFDPF_W_CASE
  return false;
}

}  // namespace nfdpf
