// frame_enc.hip -- the inference-time frame encoder (model.models._conv_stack in eval mode) as
// six implicit GEMMs on v_mfma_f32_16x16x4_f32, one launch per layer per chunk of frames.
// Layout, fragment maps and the fmaf-chain order: csrc/frame_enc.hpp.
//
// Every kernel is tile-local: a workgroup of 4 waves owns a 64-row x BN-column tile of one
// layer's output, walks K in slices (A gathered from the previous layer's activation into LDS
// with the zero padding applied, B copied from the packed weights; the next slice's loads in
// flight under this slice's MFMAs), and writes its tile once.
// No workgroup waits for another; the launch boundary is the only ordering between layers.
#include "common.hpp"
#include "frame_enc.hpp"

namespace nfdpf {
namespace fe {

typedef float f4v __attribute__((ext_vector_type(4)));

enum Kind { kFirst = 0, kMid = 1, kLinear = 2 };

struct LayerArgs {
  const float *in;       // kFirst: the caller's frames (NCHW, strided); else channels-last activation of the chunk
  const float *w;        // packed weights of this layer
  const float *sa, *sb;  // conv: BatchNorm scale / shift per channel; Linear: sb = bias
  float *out;            // conv: channels-last activation of the chunk; Linear: the caller's out
  float *layers;         // nullable: this layer's NCHW activations of ALL frames of the call
  int64_t b_stride, t_stride;          // kFirst: frame (b, t) at in + b b_stride + t t_stride
  int64_t out_b_stride, out_t_stride;  // kLinear: encoding (b, t) at out + b out_b_stride + t out_t_stride
  int j0;                // index of the chunk's first frame in the call (frame j = b T + t)
  int T;
  int nframes;           // frames in this chunk
};

template <int CIN, int COUT, int HI, int PAD, int BN, int BK, int KIND>
__global__ __launch_bounds__(256) void layer_kernel(const LayerArgs a) {
  constexpr int HO = (HI + 2 * PAD - 4) / 2 + 1, P = HO * HO, K = 16 * CIN, NT = BN / 16, LDA = BK + 4;
  static_assert(K % BK == 0 && BK % 16 == 0 && COUT % BN == 0 && BN % 16 == 0, "tile sizes");
  __shared__ __attribute__((aligned(16))) float As[kBM * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[BK * BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r16 = lane & 15;
  const int m0 = blockIdx.x * kBM, nb = blockIdx.y;
  const int M = a.nframes * P;
  const float *wblk = a.w + (size_t)nb * K * BN;

  f4v acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = f4v{0.f, 0.f, 0.f, 0.f};

  // ---- this thread's rows of the A tile (fixed over the K loop) ----
  // kFirst: one row, 12 consecutive k of the 48;  else: float4 columns, kBM / RPP rows
  constexpr int V = BK / 4, RPP = 256 / V, PASSES = (KIND == kFirst) ? 1 : kBM / RPP;
  static_assert(KIND == kFirst || (256 % V == 0 && kBM % RPP == 0), "A loader shape");
  const float *rbase[PASSES];
  int ih0[PASSES], iw0[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int row = (KIND == kFirst) ? (tid & 63) : tid / V + p * RPP;
    const int m = m0 + row;
    const bool valid = m < M;
    const int f = valid ? m / P : 0, pos = valid ? m % P : 0;
    const int oh = pos / HO, ow = pos % HO;
    ih0[p] = valid ? 2 * oh - PAD : -16;  // an invalid row fails every bounds test below: zeros
    iw0[p] = 2 * ow - PAD;
    if (KIND == kFirst) {
      const int j = a.j0 + f;
      rbase[p] = a.in + (int64_t)(j / a.T) * a.b_stride + (int64_t)(j % a.T) * a.t_stride;
    } else {
      rbase[p] = a.in + (size_t)f * (HI * HI * CIN);
    }
  }

  // ---- the K loop, one slice ahead in registers: slice s + 1's global loads are issued before
  // slice s's MFMAs, so the loads' latency runs under them (one LDS buffer, two barriers a slice) ----
  constexpr int NB4 = (BK * BN / 4 + 255) / 256;
  constexpr bool BFULL = BK * BN / 4 % 256 == 0;  // every thread copies NB4 words of the B slice
  float ra[12];        // kFirst
  float4 ra4[PASSES];  // the other kinds
  f4v rb[NB4];
  auto fetch = [&](int k0) __attribute__((always_inline)) {
    if (KIND == kFirst) {  // one row, 12 consecutive k of the 48 (scalar: NCHW input, cin = 3)
      const int kg = tid >> 6;
#pragma unroll
      for (int jj = 0; jj < 12; ++jj) {
        const int k = kg * 12 + jj, tap = k / 3, c = k % 3;
        const int ih = ih0[0] + (tap >> 2), iw = iw0[0] + (tap & 3);
        const bool ok = (unsigned)ih < (unsigned)HI && (unsigned)iw < (unsigned)HI;
        ra[jj] = ok ? rbase[0][c * (HI * HI) + ih * HI + iw] : 0.f;
      }
    } else {  // four consecutive channels of one tap per row
      const int k = k0 + 4 * (tid % V), tap = k / CIN, c = k % CIN;
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int ih = ih0[p] + (tap >> 2), iw = iw0[p] + (tap & 3);
        const bool ok = (unsigned)ih < (unsigned)HI && (unsigned)iw < (unsigned)HI;
        // (an unconditional load from an address that is always the frame's own, then the zero padding)
        const float4 v = *reinterpret_cast<const float4 *>(rbase[p] + (ok ? (ih * HI + iw) * CIN : 0) + c);
        ra4[p] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    // the B slice: BK x BN floats, contiguous in the packed blob
    const f4v *src = reinterpret_cast<const f4v *>(wblk + (size_t)k0 * BN);
#pragma unroll
    for (int i = 0; i < NB4; ++i) {
      if constexpr (BFULL) {
        rb[i] = src[tid + 256 * i];
      } else {
        rb[i] = src[tid + 256 * i < BK * BN / 4 ? tid + 256 * i : 0];  // (surplus threads: word 0, not stored)
      }
    }
  };
  // registers -> LDS: A row-major with LDA = BK + 4 (conflict-free 16-byte reads), B as it is
  auto stash = [&]() __attribute__((always_inline)) {
    if (KIND == kFirst) {
      const int row = tid & 63, kg = tid >> 6;
#pragma unroll
      for (int jj = 0; jj < 12; ++jj) As[row * LDA + kg * 12 + jj] = ra[jj];
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p)
        *reinterpret_cast<float4 *>(&As[(tid / V + p * RPP) * LDA + 4 * (tid % V)]) = ra4[p];
    }
#pragma unroll
    for (int i = 0; i < NB4; ++i)
      if (BFULL || tid + 256 * i < BK * BN / 4) reinterpret_cast<f4v *>(Bs)[tid + 256 * i] = rb[i];
  };

  fetch(0);
  for (int k0 = 0; k0 < K; k0 += BK) {
    stash();
    __syncthreads();
    if (k0 + BK < K) fetch(k0 + BK);
#pragma unroll
    for (int q = 0; q < BK / 16; ++q) {
      const float4 a4 = *reinterpret_cast<const float4 *>(&As[(wave * 16 + r16) * LDA + 16 * q + 4 * g]);
      float4 b4[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) b4[nt] = *reinterpret_cast<const float4 *>(&Bs[((q * NT + nt) * 64 + lane) * 4]);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4[nt].x, acc[nt], 0, 0, 0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4[nt].y, acc[nt], 0, 0, 0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4[nt].z, acc[nt], 0, 0, 0);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4[nt].w, acc[nt], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue: D element (row 4 g + r, column r16) of each 16 x 16 tile ----
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = nb * BN + 16 * nt + r16;
    const float sa = (KIND == kLinear) ? 1.f : a.sa[n], sb = a.sb[n];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wave * 16 + 4 * g + r;
      if (m >= M) continue;
      const int f = m / P, pos = m % P;
      const int64_t j = (int64_t)a.j0 + f;
      float v;
      if (KIND == kLinear) {
        v = acc[nt][r] + sb;
        a.out[(j / a.T) * a.out_b_stride + (j % a.T) * a.out_t_stride + n] = v;
      } else {
        v = fmaf(sa, fmaxf(acc[nt][r], 0.f), sb);
        a.out[(size_t)m * COUT + n] = v;
        if (a.layers) a.layers[(j * COUT + n) * P + pos] = v;
      }
    }
  }
}

template <int L>
void launch_conv(LayerArgs a, hipStream_t st) {
  constexpr int CIN = kChan[L], COUT = kChan[L + 1], HI = kSize[L], BN = conv_bn(COUT);
  constexpr int P = kSize[L + 1] * kSize[L + 1];
  const dim3 grid((unsigned)((a.nframes * P + kBM - 1) / kBM), COUT / BN);
  layer_kernel<CIN, COUT, HI, 1, BN, (L == 0 ? 48 : kConvBK), (L == 0 ? kFirst : kMid)><<<grid, 256, 0, st>>>(a);
}

template <int H>
void launch_linear(LayerArgs a, hipStream_t st) {
  const dim3 grid((unsigned)((a.nframes + kBM - 1) / kBM), H / kLinBN);
  layer_kernel<256, H, 4, 0, kLinBN, kLinBK, kLinear><<<grid, 256, 0, st>>>(a);
}

}  // namespace fe
}  // namespace nfdpf

using namespace nfdpf;

extern "C" int64_t nfdpf_frame_encoder_params_size(int H) { return fe::width_built(H) ? fe::params_size(H) : -1; }

extern "C" int64_t nfdpf_frame_encoder_workspace_bytes(int64_t frames) {
  if (frames < 0) return -1;
  const int64_t n = frames < fe::kChunk ? frames : fe::kChunk;
  return 4 * (fe::buf0_floats(n) + fe::buf1_floats(n)) + 256;
}

extern "C" int nfdpf_frame_encoder(const float *params, int H, const float *frames, int B, int T, int64_t b_stride,
                                   int64_t t_stride, float *out, int64_t out_b_stride, int64_t out_t_stride,
                                   float *layers, void *workspace, void *stream) {
  NFDPF_REQUIRE(fe::width_built(H), "nfdpf_frame_encoder: built for encoding widths H in {16, 32, 64, 192} (got %d)", H);
  NFDPF_REQUIRE(B >= 0 && T >= 0, "nfdpf_frame_encoder: negative size (B = %d, T = %d)", B, T);
  NFDPF_REQUIRE(b_stride >= 0 && t_stride >= 0 && out_b_stride >= 0 && out_t_stride >= 0,
                "nfdpf_frame_encoder: negative stride");
  const int64_t BT = (int64_t)B * T;
  NFDPF_REQUIRE(BT <= (int64_t)1 << 30, "nfdpf_frame_encoder: too many frames (B T = %lld)", (long long)BT);
  if (BT == 0) return NFDPF_OK;
  NFDPF_REQUIRE(params && frames && out && workspace, "nfdpf_frame_encoder: null pointer");
  NFDPF_REQUIRE(((uintptr_t)params & 15) == 0 && ((uintptr_t)workspace & 15) == 0,
                "nfdpf_frame_encoder: params and workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int64_t nmax = BT < fe::kChunk ? BT : fe::kChunk;
  float *buf0 = (float *)workspace, *buf1 = buf0 + fe::buf0_floats(nmax);
  for (int64_t j0 = 0; j0 < BT; j0 += fe::kChunk) {
    fe::LayerArgs a;
    a.b_stride = b_stride, a.t_stride = t_stride, a.out_b_stride = out_b_stride, a.out_t_stride = out_t_stride;
    a.j0 = (int)j0, a.T = T, a.nframes = (int)(BT - j0 < fe::kChunk ? BT - j0 : fe::kChunk);
    auto conv = [&](int l, const float *in, float *o) {
      const float *p = params + fe::conv_offset(l);
      a.in = in, a.out = o, a.w = p;
      a.sa = p + (int64_t)16 * fe::kChan[l] * fe::kChan[l + 1], a.sb = a.sa + fe::kChan[l + 1];
      a.layers = layers ? layers + BT * fe::act_offset(l) : nullptr;
    };
    conv(0, frames, buf0), fe::launch_conv<0>(a, st);
    conv(1, buf0, buf1), fe::launch_conv<1>(a, st);
    conv(2, buf1, buf0), fe::launch_conv<2>(a, st);
    conv(3, buf0, buf1), fe::launch_conv<3>(a, st);
    conv(4, buf1, buf0), fe::launch_conv<4>(a, st);
    const float *p = params + fe::kLinOffset;
    a.in = buf0, a.out = out, a.w = p, a.sa = nullptr, a.sb = p + (int64_t)fe::kFlat * H, a.layers = nullptr;
    switch (H) {
      case 16: fe::launch_linear<16>(a, st); break;
      case 32: fe::launch_linear<32>(a, st); break;
      case 64: fe::launch_linear<64>(a, st); break;
      default: fe::launch_linear<192>(a, st); break;
    }
  }
  return launch_status("nfdpf_frame_encoder");
}
