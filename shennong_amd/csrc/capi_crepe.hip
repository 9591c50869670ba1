// C ABI of libshennong_hip.so (include/shennong_amd.h): the plan-less CREPE entry points - one convolution
// block, the whole network from the resident audio, the decoders.  Each runs on the calling thread's scratch
// and stream (plan.h: Planless).
#include <algorithm>

#include "plan.h"

using namespace snf;

extern "C" {

namespace {
constexpr int kFrame = 1024, kBins = 360, kBlocks = 6, kMaxFilters = 1 << 14;

int crepe_check_offsets(const int64_t* h_off, int64_t n, const char* what) {
  if (n < 0) return set_error(SNF_E_INVALID, "crepe: number of utterances < 0");
  if (!h_off) return set_error(SNF_E_INVALID, std::string("crepe: null ") + what + " offsets table");
  if (h_off[0] != 0) return set_error(SNF_E_INVALID, std::string("crepe: ") + what + " offsets must start at 0");
  for (int64_t u = 0; u < n; ++u)
    if (h_off[u + 1] < h_off[u])
      return set_error(SNF_E_INVALID, std::string("crepe: ") + what + " offsets must not decrease");
  if (h_off[n] > (int64_t(1) << 40)) return set_error(SNF_E_INVALID, "crepe: batch too large");
  return SNF_OK;
}
}  // namespace

namespace {
// the argument checks that snf_crepe_conv and snf_crepe_conv_bf16 share (`d_w`: the kernel or its packed image)
int crepe_conv_check(const void* d_x, int64_t frames, int32_t in_len, int32_t c_in, int32_t width, int32_t stride,
                     int32_t pad_left, int32_t positions, const void* d_w, const float* d_b, const float* d_scale,
                     const float* d_shift, int32_t c_out, int32_t flags, const void* d_y) {
  if (frames < 0) return set_error(SNF_E_INVALID, "crepe conv: number of frames < 0");
  if (in_len < 1 || c_in < 1 || width < 1 || stride < 1 || pad_left < 0 || positions < 1 || c_out < 1)
    return set_error(SNF_E_INVALID, "crepe conv: sizes must be at least 1 (pad_left 0)");
  if (c_in > kMaxFilters || c_out > kMaxFilters || in_len > (1 << 16) || width > (1 << 16) || stride > (1 << 16) ||
      pad_left > (1 << 16) || positions > (1 << 16) || int64_t(width) * c_in > (1 << 24) ||
      int64_t(in_len) * c_in > (1 << 24) || int64_t(positions) * stride * c_in > (int64_t(1) << 30))
    return set_error(SNF_E_INVALID, "crepe conv: sizes out of range");
  if (positions > (in_len + stride - 1) / stride)   // more would be rows of padding alone
    return set_error(SNF_E_INVALID, "crepe conv: more positions than ceil(in_len / stride)");
  if (flags & ~(kConvNorm | kConvPool | kConvSigmoid)) return set_error(SNF_E_INVALID, "crepe conv: unknown flag");
  if ((flags & kConvPool) && positions % 2) return set_error(SNF_E_INVALID, "crepe conv: the pool needs an even number of positions");
  if (!d_w || !d_b) return set_error(SNF_E_INVALID, "crepe conv: null kernel or bias");
  if ((flags & kConvNorm) && (!d_scale || !d_shift)) return set_error(SNF_E_INVALID, "crepe conv: null scale or shift");
  if (frames > 0 && (!d_x || !d_y)) return set_error(SNF_E_INVALID, "crepe conv: null buffer");
  if (frames > (int64_t(1) << 40) / (int64_t(std::max(in_len, positions)) * std::max(c_in, c_out)))
    return set_error(SNF_E_INVALID, "crepe conv: block too large");
  return SNF_OK;
}
}  // namespace

int snf_crepe_conv(int device_id, const float* d_x, int64_t frames, int32_t in_len, int32_t c_in, int32_t width,
                   int32_t stride, int32_t pad_left, int32_t positions, const float* d_w, const float* d_b,
                   const float* d_scale, const float* d_shift, int32_t c_out, int32_t flags, float* d_y,
                   void* stream) {
  int rc = crepe_conv_check(d_x, frames, in_len, c_in, width, stride, pad_left, positions, d_w, d_b, d_scale, d_shift,
                            c_out, flags, d_y);
  if (rc || frames == 0) return rc;
  Planless lay;
  if ((rc = lay.begin(device_id, stream))) return rc;
  rc = launch_crepe_conv(d_x, frames, positions, stride * c_in, pad_left * c_in, in_len * c_in, width * c_in, d_w, d_b,
                         d_scale, d_shift, c_out, flags, d_y, lay.s);
  return lay.finish(rc, "crepe convolution kernel failed");
}

int snf_crepe_conv_bf16(int device_id, const void* d_x, int32_t x_type, int64_t frames, int32_t in_len, int32_t c_in,
                        int32_t width, int32_t stride, int32_t pad_left, int32_t positions, const uint16_t* d_packed,
                        const float* d_b, const float* d_scale, const float* d_shift, int32_t c_out, int32_t flags,
                        void* d_y, int32_t y_type, void* stream) {
  int rc = crepe_conv_check(d_x, frames, in_len, c_in, width, stride, pad_left, positions, d_packed, d_b, d_scale,
                            d_shift, c_out, flags, d_y);
  if (rc) return rc;
  if ((x_type != SNF_TYPE_F32 && x_type != SNF_TYPE_BF16) || (y_type != SNF_TYPE_F32 && y_type != SNF_TYPE_BF16))
    return set_error(SNF_E_INVALID, "crepe conv: unknown element type");
  if (c_in % 8) return set_error(SNF_E_INVALID, "crepe conv: the bfloat16 path needs c_in to be a multiple of 8");
  if (int64_t(width) * c_in > (1 << 20)) return set_error(SNF_E_INVALID, "crepe conv: sizes out of range");
  if (reinterpret_cast<uintptr_t>(d_packed) & 15)
    return set_error(SNF_E_INVALID, "crepe conv: the packed kernel is not 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_x) & 15)   // (a float32 source is read 16 bytes at a time as well)
    return set_error(SNF_E_INVALID, "crepe conv: the input is not 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_y) & (y_type == SNF_TYPE_BF16 ? 1 : 3))
    return set_error(SNF_E_INVALID, "crepe conv: the output is not aligned to its element type");
  if (frames == 0) return SNF_OK;
  Planless lay;
  if ((rc = lay.begin(device_id, stream))) return rc;
  rc = launch_crepe_conv_bf16(d_x, x_type == SNF_TYPE_BF16, frames, positions, stride * c_in, pad_left * c_in,
                              in_len * c_in, width * c_in, d_packed, d_b, d_scale, d_shift, c_out, flags, d_y,
                              y_type == SNF_TYPE_BF16, lay.s);
  return lay.finish(rc, "crepe convolution kernel failed");
}

namespace {
// ingest and the network; `bf16`: the kernels of blocks 2 to 6 are packed bfloat16 images and run on
// crepe_conv_bf16_kernel, the outputs of blocks 2 to 5 are bfloat16 in scratch
int crepe_forward(bool bf16, int device_id, const int16_t* d_wave, const int64_t* h_sample_offsets, int64_t n_utts,
                  int32_t hop, int32_t center, const int32_t* h_filters, const void* const* h_params,
                  float* d_activation, void* stream) {
  int rc = crepe_check_offsets(h_sample_offsets, n_utts, "sample");
  if (rc) return rc;
  if (hop < 1 || hop > (1 << 20)) return set_error(SNF_E_INVALID, "crepe: hop must be in [1, 2^20] samples");
  if (!h_filters || !h_params) return set_error(SNF_E_INVALID, "crepe: null network description");
  for (int l = 0; l < kBlocks; ++l)
    if (h_filters[l] < 1 || h_filters[l] > kMaxFilters)
      return set_error(SNF_E_INVALID, "crepe: filters of block " + std::to_string(l + 1) + " out of range");
  for (int i = 0; i < 4 * kBlocks + 2; ++i)
    if (!h_params[i]) return set_error(SNF_E_INVALID, "crepe: null parameter buffer " + std::to_string(i));
  if (bf16)
    for (int l = 1; l < kBlocks; ++l) {
      if (h_filters[l - 1] % 8)
        return set_error(SNF_E_INVALID, "crepe: the bfloat16 path needs filters of block " + std::to_string(l) + " to be a multiple of 8");
      if (reinterpret_cast<uintptr_t>(h_params[4 * l]) & 15)
        return set_error(SNF_E_INVALID, "crepe: packed kernel " + std::to_string(4 * l) + " is not 16-byte aligned");
    }
  if (n_utts == 0) return SNF_OK;
  std::vector<int64_t> foff(n_utts + 1, 0);
  for (int64_t u = 0; u < n_utts; ++u) {
    const int64_t padded = h_sample_offsets[u + 1] - h_sample_offsets[u] + (center ? kFrame : 0);
    if (padded < kFrame)
      return set_error(SNF_E_INVALID, "crepe: utterance " + std::to_string(u) + " is shorter than one frame of 1024 samples");
    foff[u + 1] = foff[u] + 1 + (padded - kFrame) / hop;
  }
  const int64_t total = foff[n_utts];
  if (!d_wave || !d_activation) return set_error(SNF_E_INVALID, "crepe: null buffer");
  // activations live in scratch, one block of frames at a time (frames are independent of each other):
  // `even` holds the frames and the outputs of blocks 2, 4, 6, `odd` those of blocks 1, 3, 5; sized in bytes
  // per frame, the outputs of blocks 2 to 5 being 2 bytes an element on the bfloat16 path
  const int32_t* C = h_filters;
  int64_t even = 4 * kFrame, odd = 0;
  for (int l = 0, T = 128; l < kBlocks; ++l, T /= 2) {
    int64_t& side = (l % 2) ? even : odd;
    side = std::max(side, int64_t(T) * C[l] * ((bf16 && l >= 1 && l <= 4) ? 2 : 4));
  }
  int64_t chunk = std::max<int64_t>(64, (int64_t(512) << 20) / (even + odd));
  chunk = std::min(chunk, total);
  Planless lay;
  auto d_soff = lay.take<int64_t>(n_utts + 1);
  auto d_foff = lay.take<int64_t>(n_utts + 1);
  auto buf_even = lay.take<char>(chunk * even);
  auto buf_odd = lay.take<char>(chunk * odd);
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemcpyAsync(d_soff, h_sample_offsets, sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  SNF_HIP_CHECK(hipMemcpyAsync(d_foff, foff.data(), sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  const void* const* P = h_params;
  auto F = [](const void* p) { return static_cast<const float*>(p); };
  for (int64_t a = 0; a < total && !rc; a += chunk) {
    const int64_t m = std::min(chunk, total - a);
    char* src = buf_even;
    char* dst = buf_odd;
    rc = launch_crepe_frames(d_wave, d_soff, d_foff, n_utts, a, m, hop, center ? 1 : 0, reinterpret_cast<float*>(src),
                             lay.s);
    // block 1: 512 taps at stride 4 over the 1024 samples, 254 zeros before; blocks 2..6: 64 taps, 31 before
    if (!rc) rc = launch_crepe_conv(reinterpret_cast<const float*>(src), m, 256, 4, 254, kFrame, 512, F(P[0]), F(P[1]),
                                    F(P[2]), F(P[3]), C[0], kConvNorm | kConvPool, reinterpret_cast<float*>(dst), lay.s);
    for (int l = 1, T = 128; l < kBlocks && !rc; ++l, T /= 2) {
      std::swap(src, dst);
      if (bf16)   // block 2 reads block 1's float32 output and rounds it in its loader; block 6 stores float32
        rc = launch_crepe_conv_bf16(src, l > 1, m, T, C[l - 1], 31 * C[l - 1], T * C[l - 1], 64 * C[l - 1],
                                    static_cast<const uint16_t*>(P[4 * l]), F(P[4 * l + 1]), F(P[4 * l + 2]),
                                    F(P[4 * l + 3]), C[l], kConvNorm | kConvPool, dst, l < kBlocks - 1, lay.s);
      else
        rc = launch_crepe_conv(reinterpret_cast<const float*>(src), m, T, C[l - 1], 31 * C[l - 1], T * C[l - 1],
                               64 * C[l - 1], F(P[4 * l]), F(P[4 * l + 1]), F(P[4 * l + 2]), F(P[4 * l + 3]), C[l],
                               kConvNorm | kConvPool, reinterpret_cast<float*>(dst), lay.s);
    }
    // classifier: the 4 positions x C6 channels of a frame are its row, time-major with channels innermost
    if (!rc) rc = launch_crepe_conv(reinterpret_cast<const float*>(dst), m, 1, 4 * C[5], 0, 4 * C[5], 4 * C[5],
                                    F(P[24]), F(P[25]), nullptr, nullptr, kBins, kConvSigmoid,
                                    d_activation + a * kBins, lay.s);
  }
  return lay.finish(rc, "crepe network kernels failed");
}
}  // namespace

int snf_crepe_forward(int device_id, const int16_t* d_wave, const int64_t* h_sample_offsets, int64_t n_utts,
                      int32_t hop, int32_t center, const int32_t* h_filters, const float* const* h_params,
                      float* d_activation, void* stream) {
  return crepe_forward(false, device_id, d_wave, h_sample_offsets, n_utts, hop, center, h_filters,
                       reinterpret_cast<const void* const*>(h_params), d_activation, stream);
}

int snf_crepe_forward_bf16(int device_id, const int16_t* d_wave, const int64_t* h_sample_offsets, int64_t n_utts,
                           int32_t hop, int32_t center, const int32_t* h_filters, const void* const* h_params,
                           float* d_activation, void* stream) {
  return crepe_forward(true, device_id, d_wave, h_sample_offsets, n_utts, hop, center, h_filters, h_params,
                       d_activation, stream);
}

int snf_crepe_decode(int device_id, const float* d_activation, const int64_t* h_frame_offsets, int64_t n_utts,
                     int32_t viterbi, const double* d_tables, double* d_out, int32_t* d_bins, void* stream) {
  int rc = crepe_check_offsets(h_frame_offsets, n_utts, "frame");
  if (rc) return rc;
  if (n_utts == 0 || h_frame_offsets[n_utts] == 0) return SNF_OK;
  const int64_t total = h_frame_offsets[n_utts];
  if (!d_activation || !d_tables || !d_out || !d_bins) return set_error(SNF_E_INVALID, "crepe: null buffer");
  if (reinterpret_cast<uintptr_t>(d_tables) & 7) return set_error(SNF_E_INVALID, "crepe: tables are not 8-byte aligned");
  Planless lay;
  auto d_foff = lay.take<int64_t>(n_utts + 1);
  auto conf = lay.take<float>(total);
  auto psi = lay.take<uint16_t>(viterbi ? total * kBins : 0);
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemcpyAsync(d_foff, h_frame_offsets, sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  rc = launch_crepe_decode(d_activation, d_foff, n_utts, total, viterbi ? 1 : 0, d_tables, conf, psi, d_bins, d_out,
                           lay.s);
  return lay.finish(rc, "crepe decoder kernels failed");
}

int snf_crepe_rows(int device_id, const double* d_in, const int64_t* h_in_offsets, const int64_t* h_out_offsets,
                   int64_t n_utts, double* d_out, void* stream) {
  int rc = crepe_check_offsets(h_in_offsets, n_utts, "input row");
  if (!rc) rc = crepe_check_offsets(h_out_offsets, n_utts, "output row");
  if (rc) return rc;
  constexpr int64_t kMaxRows = int64_t(1) << 20;   // (M N (2K + 1) must fit an int64)
  int64_t n_tiles = 0;
  for (int64_t u = 0; u < n_utts; ++u) {
    const int64_t N = h_in_offsets[u + 1] - h_in_offsets[u], M = h_out_offsets[u + 1] - h_out_offsets[u];
    if (N < 1 || M < 1)
      return set_error(SNF_E_INVALID, "crepe rows: utterance " + std::to_string(u) + " has no input or no output rows");
    if (N > kMaxRows || M > kMaxRows)
      return set_error(SNF_E_INVALID, "crepe rows: utterance " + std::to_string(u) + " has more than 2^20 rows");
    n_tiles += (M + kCrepeRowsTile - 1) / kCrepeRowsTile;
  }
  if (n_tiles > (int64_t(1) << 30)) return set_error(SNF_E_INVALID, "crepe: batch too large");
  if (n_utts == 0) return SNF_OK;
  if (!d_in || !d_out) return set_error(SNF_E_INVALID, "crepe: null buffer");
  if ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 7)
    return set_error(SNF_E_INVALID, "crepe rows: a buffer is not 8-byte aligned");
  std::vector<int64_t> tile_off(n_utts + 1, 0);
  std::vector<int32_t> tile_utt(n_tiles);
  for (int64_t u = 0; u < n_utts; ++u) {
    const int64_t M = h_out_offsets[u + 1] - h_out_offsets[u];
    tile_off[u + 1] = tile_off[u] + (M + kCrepeRowsTile - 1) / kCrepeRowsTile;
    std::fill(tile_utt.begin() + tile_off[u], tile_utt.begin() + tile_off[u + 1], static_cast<int32_t>(u));
  }
  Planless lay;
  auto d_ioff = lay.take<int64_t>(n_utts + 1);
  auto d_ooff = lay.take<int64_t>(n_utts + 1);
  auto d_toff = lay.take<int64_t>(n_utts + 1);
  auto d_tutt = lay.take<int32_t>(n_tiles);
  if ((rc = lay.begin(device_id, stream))) return rc;
  const size_t table = sizeof(int64_t) * (n_utts + 1);
  SNF_HIP_CHECK(hipMemcpyAsync(d_ioff, h_in_offsets, table, hipMemcpyHostToDevice, lay.s));
  SNF_HIP_CHECK(hipMemcpyAsync(d_ooff, h_out_offsets, table, hipMemcpyHostToDevice, lay.s));
  SNF_HIP_CHECK(hipMemcpyAsync(d_toff, tile_off.data(), table, hipMemcpyHostToDevice, lay.s));
  SNF_HIP_CHECK(hipMemcpyAsync(d_tutt, tile_utt.data(), sizeof(int32_t) * n_tiles, hipMemcpyHostToDevice, lay.s));
  rc = launch_crepe_rows(d_in, d_ioff, d_ooff, d_tutt, d_toff, n_tiles, d_out, lay.s);
  // (the wait below also covers the copies out of tile_off / tile_utt, which are pageable)
  return lay.finish(rc, "crepe row resampling kernel failed");
}

int snf_crepe_voicing_convert(int device_id, const double* d_rows, const int64_t* h_offsets, int64_t n_utts,
                              const double* h_model, float* d_out, int32_t* d_status, void* stream) {
  int rc = crepe_check_offsets(h_offsets, n_utts, "row");
  if (rc) return rc;
  if (!h_model) return set_error(SNF_E_INVALID, "crepe voicing: null model");
  for (int i = 0; i < kCrepeVoicingModel; ++i)
    if (!(h_model[i] == h_model[i])) return set_error(SNF_E_INVALID, "crepe voicing: the model holds a NaN");
  if (!(h_model[3] > 0)) return set_error(SNF_E_INVALID, "crepe voicing: the variance must be positive");
  for (int64_t u = 0; u < n_utts; ++u)
    if (h_offsets[u + 1] - h_offsets[u] > (int64_t(1) << 30))
      return set_error(SNF_E_INVALID, "crepe voicing: utterance " + std::to_string(u) + " has more than 2^30 rows");
  if (n_utts > (int64_t(1) << 30)) return set_error(SNF_E_INVALID, "crepe: batch too large");
  if (n_utts == 0) return SNF_OK;
  const int64_t total = h_offsets[n_utts];
  if (!d_status || (total > 0 && (!d_rows || !d_out))) return set_error(SNF_E_INVALID, "crepe: null buffer");
  if ((reinterpret_cast<uintptr_t>(d_rows) & 7) || (reinterpret_cast<uintptr_t>(d_out) & 3) ||
      (reinterpret_cast<uintptr_t>(d_status) & 3))
    return set_error(SNF_E_INVALID, "crepe voicing: a buffer is not aligned to its element type");
  Planless lay;
  auto d_off = lay.take<int64_t>(n_utts + 1);
  auto lattice = lay.take<double>(2 * total);
  auto next_voiced = lay.take<int32_t>(total);
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemcpyAsync(d_off, h_offsets, sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  rc = launch_crepe_voicing(d_rows, d_off, n_utts, h_model, lattice, next_voiced, d_out, d_status, lay.s);
  return lay.finish(rc, "crepe voicing kernel failed");
}

}  // extern "C"
