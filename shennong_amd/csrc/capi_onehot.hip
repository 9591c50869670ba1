// C ABI of libshennong_hip.so (include/shennong_amd.h): the plan-less framed one-hot entry point.  Everything the
// kernels index with is checked here, on the host, before anything is launched; the tables cross the link as
// ONE block.  Runs on the calling thread's scratch and stream (plan.h: Planless).
#include <cmath>
#include <cstring>

#include "plan.h"

using namespace snf;

extern "C" {

int snf_framed_onehot(int device_id, double sample_rate, int32_t frame_length, int32_t frame_shift,
                      int32_t window_type, float blackman_coeff, int64_t n_alignments,
                      const int64_t* h_segment_offsets, const double* h_first_onsets, const double* h_offsets,
                      const int32_t* h_token_ids, const int64_t* h_num_samples, const int64_t* h_num_frames,
                      const int32_t* h_num_tokens, const int64_t* h_row_offsets, int32_t* d_winners,
                      uint8_t* d_onehot, float* kernel_ms, void* stream) {
  const int64_t n = n_alignments;
  if (kernel_ms) *kernel_ms = 0.0f;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_error(SNF_E_NODEVICE, "no HIP device visible: libshennong_hip needs an MI355X (gfx950)");
  if (device_id < 0 || device_id >= ndev) return set_error(SNF_E_INVALID, "bad device id");
  if (n < 0 || n > (int64_t(1) << 31)) return set_error(SNF_E_INVALID, "onehot: number of alignments out of range");
  if (!(sample_rate > 0.0) || !std::isfinite(sample_rate))
    return set_error(SNF_E_INVALID, "onehot: sample rate must be positive");
  if (frame_length < 1 || frame_length > kOneHotMaxFrameLength)
    return set_error(SNF_E_INVALID, "onehot: frame length must be in [1, " + std::to_string(kOneHotMaxFrameLength) +
                                        "] samples");
  if (frame_shift < 1 || frame_shift > (1 << 24))
    return set_error(SNF_E_INVALID, "onehot: frame shift must be in [1, 2^24] samples");
  if (window_type < SNF_WINDOW_HAMMING || window_type > SNF_WINDOW_BLACKMAN)
    return set_error(SNF_E_INVALID, "onehot: unknown window type");
  if (n == 0) return SNF_OK;
  if (!h_segment_offsets || !h_first_onsets || !h_num_samples || !h_num_frames || !h_num_tokens || !h_row_offsets)
    return set_error(SNF_E_INVALID, "onehot: null table");
  if (h_segment_offsets[0] != 0 || h_row_offsets[0] != 0)
    return set_error(SNF_E_INVALID, "onehot: offsets tables must start at 0");
  const int64_t kMaxTotal = int64_t(1) << 36;
  std::vector<int64_t> frame_off(n + 1, 0);
  for (int64_t a = 0; a < n; ++a) {
    const std::string who = "onehot: alignment " + std::to_string(a);
    const int64_t s0 = h_segment_offsets[a], s1 = h_segment_offsets[a + 1];
    const int64_t frames = h_num_frames[a], samples = h_num_samples[a], width = h_num_tokens[a];
    if (s1 < s0 || s1 > kMaxTotal) return set_error(SNF_E_INVALID, who + ": segment offsets must not decrease");
    if (frames < 0 || samples < 0 || width < 0 || samples > kMaxTotal || frames > kMaxTotal || width > (1 << 24))
      return set_error(SNF_E_INVALID, who + ": counts out of range");
    if (frames > 0 && (s1 == s0 || width < 1)) return set_error(SNF_E_INVALID, who + ": frames without tokens");
    if (frames > 0 && (frames - 1) * int64_t(frame_shift) + frame_length > samples)
      return set_error(SNF_E_INVALID, who + ": " + std::to_string(frames) + " frames do not fit in " +
                                          std::to_string(samples) + " samples");
    const int64_t bytes = frames * width, r0 = h_row_offsets[a], r1 = h_row_offsets[a + 1];
    if (r0 % 16 || r1 % 16 || r1 < r0 || r1 - r0 < bytes || r1 > kMaxTotal)
      return set_error(SNF_E_INVALID, who + ": rows must start on 16-byte boundaries and hold frames x tokens bytes");
    if (s1 > s0 && (!h_offsets || !h_token_ids)) return set_error(SNF_E_INVALID, "onehot: null segment table");
    if (s1 > s0 && !std::isfinite(h_first_onsets[a])) return set_error(SNF_E_INVALID, who + ": first onset is not finite");
    for (int64_t k = s0; k < s1; ++k) {
      if (!std::isfinite(h_offsets[k]) || (k > s0 && h_offsets[k] < h_offsets[k - 1]))
        return set_error(SNF_E_INVALID, who + ": offsets must be finite and must not decrease");
      if (frames > 0 && (h_token_ids[k] < 0 || h_token_ids[k] >= width))
        return set_error(SNF_E_INVALID, who + ": token id out of range");
    }
    frame_off[a + 1] = frame_off[a] + frames;
    if (frame_off[a + 1] > kMaxTotal) return set_error(SNF_E_INVALID, "onehot: batch too large");
  }
  const int64_t n_seg = h_segment_offsets[n], total_frames = frame_off[n], total_bytes = h_row_offsets[n];
  if (total_frames == 0) return SNF_OK;
  if (!d_winners || !d_onehot) return set_error(SNF_E_INVALID, "onehot: null output buffer");
  if (reinterpret_cast<uintptr_t>(d_onehot) & 15) return set_error(SNF_E_INVALID, "onehot: rows are not 16-byte aligned");

  // the window of shennong_amd/window.py: the table of a 1 kHz "signal" whose frame lasts frame_length ms,
  // ones in the degenerate cases (reference window.py:97-105)
  std::vector<float> window;
  const bool zero_ends = window_type == SNF_WINDOW_POVEY || window_type == SNF_WINDOW_BLACKMAN ||
                         window_type == SNF_WINDOW_HANNING;
  if (frame_length == 1 || (frame_length == 2 && zero_ends)) {
    window.assign(frame_length, 1.0f);
  } else {
    snf_frame_options fo{};
    fo.samp_freq = 1000.0f;
    fo.frame_length_ms = static_cast<float>(frame_length);
    fo.frame_shift_ms = 1.0f;
    fo.window_type = window_type;
    fo.blackman_coeff = blackman_coeff;
    fo.snip_edges = 1;
    int rc = make_window(fo, &window);
    if (rc) return rc;
    if (static_cast<int64_t>(window.size()) != frame_length)
      return set_error(SNF_E_RUNTIME, "onehot: window table of the wrong length");
  }

  // one block for all the tables: 8-byte entries first
  const size_t n1 = static_cast<size_t>(n + 1), ns = static_cast<size_t>(n_seg);
  const size_t at_seg = 0, at_frame = at_seg + 8 * n1, at_row = at_frame + 8 * n1, at_samples = at_row + 8 * n1,
               at_onset = at_samples + 8 * n1, at_offsets = at_onset + 8 * n1, at_ids = at_offsets + 8 * ns,
               at_width = at_ids + 4 * ns, at_window = at_width + 4 * n1,
               blob_bytes = at_window + 4 * static_cast<size_t>(frame_length);
  std::vector<char> blob(blob_bytes, 0);
  std::memcpy(&blob[at_seg], h_segment_offsets, 8 * n1);
  std::memcpy(&blob[at_frame], frame_off.data(), 8 * n1);
  std::memcpy(&blob[at_row], h_row_offsets, 8 * n1);
  std::memcpy(&blob[at_samples], h_num_samples, 8 * (n1 - 1));
  std::memcpy(&blob[at_onset], h_first_onsets, 8 * (n1 - 1));
  if (ns) std::memcpy(&blob[at_offsets], h_offsets, 8 * ns);
  if (ns) std::memcpy(&blob[at_ids], h_token_ids, 4 * ns);
  std::memcpy(&blob[at_width], h_num_tokens, 4 * (n1 - 1));
  std::memcpy(&blob[at_window], window.data(), 4 * static_cast<size_t>(frame_length));

  Planless lay;
  auto d_blob = lay.take<char>(blob_bytes);
  auto d_ends = lay.take<int64_t>(ns);
  int rc = lay.begin(device_id, stream);
  if (rc) return rc;
  SNF_HIP_CHECK(hipMemcpyAsync(d_blob, blob.data(), blob_bytes, hipMemcpyHostToDevice, lay.s));
  const char* base = d_blob;
  OneHotBatch b{};
  b.n_ali = n;
  b.n_seg = n_seg;
  b.total_frames = total_frames;
  b.total_bytes = total_bytes;
  b.frame_length = frame_length;
  b.frame_shift = frame_shift;
  b.rate = sample_rate;
  b.seg_off = reinterpret_cast<const int64_t*>(base + at_seg);
  b.frame_off = reinterpret_cast<const int64_t*>(base + at_frame);
  b.row_off = reinterpret_cast<const int64_t*>(base + at_row);
  b.nsamples = reinterpret_cast<const int64_t*>(base + at_samples);
  b.onset0 = reinterpret_cast<const double*>(base + at_onset);
  b.offsets = reinterpret_cast<const double*>(base + at_offsets);
  b.ids = reinterpret_cast<const int32_t*>(base + at_ids);
  b.ntokens = reinterpret_cast<const int32_t*>(base + at_width);
  b.window = reinterpret_cast<const float*>(base + at_window);
  b.ends = d_ends;
  b.winner = d_winners;
  b.rows = d_onehot;
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (kernel_ms) {
    if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) {
      if (ev[0]) (void)hipEventDestroy(ev[0]);
      (void)hipStreamSynchronize(lay.s);
      return set_error(SNF_E_HIP, "onehot: cannot create the timing marks");
    }
    (void)hipEventRecord(ev[0], lay.s);
  }
  rc = launch_framed_onehot(b, lay.s);
  if (kernel_ms) (void)hipEventRecord(ev[1], lay.s);
  rc = lay.finish(rc, "one-hot kernels failed");
  if (kernel_ms) {
    if (!rc && hipEventElapsedTime(kernel_ms, ev[0], ev[1]) != hipSuccess)
      rc = set_error(SNF_E_HIP, "onehot: cannot read the timing marks");
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
  }
  return rc;
}

}  // extern "C"
