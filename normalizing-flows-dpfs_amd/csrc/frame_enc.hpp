// frame_enc.hpp -- layout of the inference-time frame encoder (csrc/frame_enc.hip).
//
// The model is model.models._conv_stack(H): 5 x [Conv2d(4, stride 2, pad 1, no bias) ReLU
// BatchNorm2d] over channels 3 16 32 64 128 256 and sizes 128 64 32 16 8 4, Flatten, Linear(4096, H).
// Every layer is one implicit GEMM on v_mfma_f32_16x16x4_f32:
//   M  output positions (frame, oh, ow) of a chunk of frames, tiles of kBM = 64 rows;
//   N  output channels, blocks of BN = min(cout, 64) columns (the Linear: 16);
//   K  (kh, kw, cin), cin fastest: k = (4 kh + kw) cin_count + c.  The Linear is the same GEMM
//      as a 4 x 4 convolution without padding over conv5's channels-last [4][4][256] output:
//      k = 256 (4 h + w) + c, the host permuting nn.Linear's columns (Flatten is c 16 + 4 h + w).
//
// Parameter blob (floats; nfdpf.pack.frame_encoder_tensors), nfdpf_frame_encoder_params_size(H):
//   per conv layer l = 0..4:  W packed [16 cin cout] | a [cout] | b [cout]
//   the Linear:               W packed [4096 H]      | bias [H]
// with a = gamma / sqrt(running_var + eps), b = beta - running_mean a (the eval-mode BatchNorm
// after the ReLU: y = a relu(conv) + b), and W packed in B-fragment order
//   [cout / BN][K / 16 (q)][BN / 16 (nt)][lane 64][i 4] =
//       W[k = 16 q + 4 (lane >> 4) + i][n = BN nb + 16 nt + (lane & 15)]
// so that a K-slice of one column block is one contiguous run (copied to LDS as it is), lane l
// reads its B operands of four consecutive MFMAs as one 16-byte word, and the A operand of those
// four -- row (l & 15), k = 16 q + 4 (l >> 4) + i -- is one 16-byte word of the row-major A tile.
// The MFMA numbered 4 q + i so multiplies k = 16 q + i, 16 q + 4 + i, 16 q + 8 + i, 16 q + 12 + i
// (its lane groups 0..3 in turn): every output element is ONE fmaf chain over K in that fixed
// order, whatever the number of frames in the call.
//
// Activations between the layers are channels-last [frame][h][w][c] in the workspace, two
// buffers used in turn: layer 1's output (kChunk x 64 x 64 x 16) and layer 2's (kChunk x 32 x 32
// x 32); layers 3 and 5 write into the first again, layer 4 into the second.
#pragma once

#include <stdint.h>

namespace nfdpf {
namespace fe {

constexpr int kConvs = 5;
constexpr int kChan[kConvs + 1] = {3, 16, 32, 64, 128, 256};
constexpr int kSize[kConvs + 1] = {128, 64, 32, 16, 8, 4};
constexpr int kFlat = 256 * 4 * 4;  // the Linear's K
constexpr int kChunk = 256;         // frames per pass over the layers (the workspace holds one chunk)
constexpr int kBM = 64;             // rows of a workgroup's tile: 4 waves x 16
constexpr int kLinBN = 16;          // the Linear's column block (one accumulator per wave: the
                                    // K = 4096 chain is the launch's latency, so spread N over workgroups)

constexpr int kConvBK = 64;         // K-slice of conv layers 2..5 (layer 1: its whole K = 48)
constexpr int kLinBK = 128;         // K-slice of the Linear

constexpr int conv_bn(int cout) { return cout < 64 ? cout : 64; }

inline bool width_built(int H) { return H == 16 || H == 32 || H == 64 || H == 192; }

// floats of conv layer l in the blob, and where it starts
constexpr int64_t conv_floats(int l) { return (int64_t)16 * kChan[l] * kChan[l + 1] + 2 * kChan[l + 1]; }
constexpr int64_t conv_offset(int l) { return l == 0 ? 0 : conv_offset(l - 1) + conv_floats(l - 1); }
constexpr int64_t kLinOffset = conv_offset(kConvs);
inline int64_t params_size(int H) { return kLinOffset + (int64_t)kFlat * H + H; }

// floats of conv layer l's activation for one frame, and of all five (the `layers` output)
constexpr int64_t act_floats(int l) { return (int64_t)kChan[l + 1] * kSize[l + 1] * kSize[l + 1]; }
constexpr int64_t act_offset(int l) { return l == 0 ? 0 : act_offset(l - 1) + act_floats(l - 1); }
constexpr int64_t kActFloats = act_offset(kConvs);  // 126976

// workspace of n <= kChunk frames: the two activation buffers
inline int64_t buf0_floats(int64_t n) { return n * act_floats(0); }
inline int64_t buf1_floats(int64_t n) { return n * act_floats(1); }

}  // namespace fe
}  // namespace nfdpf
