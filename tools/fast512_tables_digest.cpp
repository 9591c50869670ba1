// Digest of the tables of the 512-point fast path (shennong_amd/csrc/fast512_tables.cpp), on the CPU.
// For a fixed list of configurations that reaches every branch of the builder: the window, mel banks, DCT and
// lifter from host_tables.cpp, then fast512_eligible / fast512_dual_eligible / fast512_build, and one line with
// the return code, every non-pointer field of Fast512Params (floats as their bits), the blob's length and a
// 64-bit FNV-1a of its bytes.  tests/test_fast512_tables.py compares the output with
// profiles/fast512_tables_digest.txt; a change that means to alter the tables records that file again.
//
// Build (host only; from the repository root):
//   hipcc -O1 -std=c++17 -o fast512_tables_digest tools/fast512_tables_digest.cpp \
//       shennong_amd/csrc/fast512_tables.cpp shennong_amd/csrc/host_tables.cpp
// or, instead of the two sources, against a built library: -Lshennong_amd -lshennong_hip -Wl,-rpath,...
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../shennong_amd/csrc/snf_internal.h"

using namespace snf;

namespace {

struct Config {
  const char* name;
  float samp_freq, frame_length_ms;
  int kind, num_bins, num_ceps;
  float warp;      // VTLN warp factor of the mel banks
  int dual;        // 0 / 1: build with that `dual`; -1: twice, with both
  int dct_mfma;    // SNF_DCT_MFMA=1 during the build
};

const Config kConfigs[] = {
    {"fbank40_16k_25ms", 16000, 25, SNF_KIND_FBANK, 40, 0, 1.0f, 0, 0},
    {"fbank23_16k_25ms", 16000, 25, SNF_KIND_FBANK, 23, 0, 1.0f, 0, 0},
    {"fbank64_16k_25ms", 16000, 25, SNF_KIND_FBANK, 64, 0, 1.0f, 0, 0},
    {"mfcc13_23_16k_25ms", 16000, 25, SNF_KIND_MFCC, 23, 13, 1.0f, 0, 0},
    {"mfcc13_23_16k_25ms_dct_mfma", 16000, 25, SNF_KIND_MFCC, 23, 13, 1.0f, 0, 1},
    {"plp23_16k_25ms", 16000, 25, SNF_KIND_PLP, 23, 13, 1.0f, 0, 0},
    {"spectrogram_16k_25ms", 16000, 25, SNF_KIND_SPECTROGRAM, 0, 0, 1.0f, 0, 0},
    {"energy_16k_25ms", 16000, 25, SNF_KIND_ENERGY, 0, 0, 1.0f, 0, 0},
    {"fbank40_16k_32ms", 16000, 32, SNF_KIND_FBANK, 40, 0, 1.0f, 0, 0},
    {"fbank40_16k_odd_window", 16000, 25.07f, SNF_KIND_FBANK, 40, 0, 1.0f, 0, 0},
    {"fbank40_8k_25ms", 8000, 25, SNF_KIND_FBANK, 40, 0, 1.0f, -1, 0},
    {"mfcc13_23_8k_25ms", 8000, 25, SNF_KIND_MFCC, 23, 13, 1.0f, -1, 0},
    {"spectrogram_8k_25ms", 8000, 25, SNF_KIND_SPECTROGRAM, 0, 0, 1.0f, -1, 0},
    {"fbank23_8k_10ms", 8000, 10, SNF_KIND_FBANK, 23, 0, 1.0f, 0, 0},
    {"fbank40_16k_25ms_warp0.85", 16000, 25, SNF_KIND_FBANK, 40, 0, 0.85f, 0, 0},
    {"mfcc13_23_16k_25ms_warp1.2", 16000, 25, SNF_KIND_MFCC, 23, 13, 1.2f, 0, 0},
    {"fbank68_16k_25ms_17_groups", 16000, 25, SNF_KIND_FBANK, 68, 0, 1.0f, 0, 0},
    {"mfcc16_64_8k_25ms_warp1.2_no_lds_room", 8000, 25, SNF_KIND_MFCC, 64, 16, 1.2f, 0, 0},
};

uint64_t fnv1a(const void* data, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(data);
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

uint32_t bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}

int run(const Config& c, bool dual) {
  snf_frame_options fo{};
  fo.samp_freq = c.samp_freq;
  fo.frame_shift_ms = 10;
  fo.frame_length_ms = c.frame_length_ms;
  fo.dither = 0.0f;
  fo.preemph_coeff = 0.97f;
  fo.remove_dc_offset = 1;
  fo.window_type = SNF_WINDOW_POVEY;
  fo.round_to_power_of_two = 1;
  fo.blackman_coeff = 0.42f;
  fo.snip_edges = 1;
  snf_mel_options mo{};
  mo.num_bins = c.num_bins;
  mo.low_freq = 20;
  mo.high_freq = 0;
  mo.vtln_low = 100;
  mo.vtln_high = -500;

  // (the scalar fields as capi_plan.hip mel_options sets them)
  MelParams p{};
  p.win_len = window_size(fo);
  p.win_shift = window_shift(fo);
  p.padded = padded_window_size(fo);
  p.half = p.padded / 2;
  p.pow2 = (p.padded & (p.padded - 1)) == 0;
  p.snip_edges = fo.snip_edges;
  p.remove_dc = fo.remove_dc_offset;
  p.preemph = fo.preemph_coeff;
  p.dither = fo.dither;
  p.seed = 0;
  p.kind = c.kind;
  p.use_log = 1;
  p.use_power = 1;
  p.num_bins = c.num_bins;
  p.num_ceps = c.num_ceps;
  if (c.kind == SNF_KIND_SPECTROGRAM) p.need_post = 1;

  std::vector<float> window, dct, lifter;
  MelBanksHost mb;
  if (make_window(fo, &window) != SNF_OK) return 1;
  if (c.num_bins > 0 && make_mel_banks(mo, fo, c.warp, &mb) != SNF_OK) {
    std::fprintf(stderr, "%s: %s\n", c.name, last_error());
    return 1;
  }
  if (c.kind == SNF_KIND_MFCC) make_dct_matrix(c.num_ceps, c.num_bins, &dct);
  if (c.kind == SNF_KIND_MFCC || c.kind == SNF_KIND_PLP) make_lifter(22.0f, c.num_ceps, &lifter);

  if (c.dct_mfma) setenv("SNF_DCT_MFMA", "1", 1);
  const int eligible = fast512_eligible(p, false), dual_eligible = fast512_dual_eligible(p);
  std::vector<float> blob;
  Fast512Params f{};
  const int rc = fast512_build(p, window, mb, dct, lifter, dual, &blob, &f);
  unsetenv("SNF_DCT_MFMA");

  std::printf("%s dual=%d eligible=%d dual_eligible=%d rc=%d", c.name, dual ? 1 : 0, eligible, dual_eligible, rc);
  std::printf(" win_len=%d win_shift=%d remove_dc=%d snip_edges=%d preemph=%08x dither=%08x seed=%llu kind=%d"
              " out_cols=%d use_energy=%d need_raw=%d need_post=%d htk_compat=%d use_log=%d has_floor=%d"
              " log_energy_floor=%08x num_bins=%d num_ceps=%d compression=%d",
              f.win_len, f.win_shift, f.remove_dc, f.snip_edges, bits(f.preemph), bits(f.dither), f.seed, f.kind,
              f.out_cols, f.use_energy, f.need_raw, f.need_post, f.htk_compat, f.use_log, f.has_floor,
              bits(f.log_energy_floor), f.num_bins, f.num_ceps, f.compression);
  std::printf(" mm_quads=%d mm_levels=%d dd_quads=%d dd_groups=%d dct_mfma=%d dual=%d fused_delta=%d"
              " table_floats=%d table_stride=%d off_mm_a=%d off_mm_lane=%d off_dd_a=%d off_lifter=%d off_dd_v=%d",
              f.mm_quads, f.mm_levels, f.dd_quads, f.dd_groups, f.dct_mfma, f.dual, f.fused_delta, f.table_floats,
              f.table_stride, f.off_mm_a, f.off_mm_lane, f.off_dd_a, f.off_lifter, f.off_dd_v);
  std::printf(" blob_floats=%zu fnv1a=%016" PRIx64 "\n", blob.size(), fnv1a(blob.data(), 4 * blob.size()));
  return 0;
}

}  // namespace

int main() {
  // the knobs the builder reads: only what a configuration of the list sets itself
  unsetenv("SNF_DCT_MFMA");
  unsetenv("SNF_DISABLE_FAST512");
  unsetenv("SNF_DISABLE_DUAL256");
  for (const Config& c : kConfigs) {
    if (c.dual != 1 && run(c, false)) return 1;
    if (c.dual != 0 && run(c, true)) return 1;
  }
  return 0;
}
