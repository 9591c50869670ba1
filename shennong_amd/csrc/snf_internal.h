// Internal declarations of libshennong_hip.so (MI355X / gfx950 speech-features backend).
// Not part of the public ABI (that is include/shennong_amd.h).
#ifndef SNF_INTERNAL_H_
#define SNF_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/shennong_amd.h"

namespace snf {

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
int set_error(int code, const std::string& msg);
const char* last_error();

#define SNF_HIP_CHECK(expr)                                                                  \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return snf::set_error(SNF_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
  } while (0)

// ---------------------------------------------------------------------------------------------
// host-side tables (host_tables.cpp): the product's own restatement of the tables Kaldi
// precomputes in FeatureWindowFunction / MelBanks / MfccComputer / PlpComputer / LinearResample /
// ArbitraryResample (called by the reference at processor/base.py:429-431, plp.py:443-508,
// pitch_kaldi.py:296-299)
// ---------------------------------------------------------------------------------------------
int32_t window_shift(const snf_frame_options& o);
int32_t window_size(const snf_frame_options& o);
int32_t padded_window_size(const snf_frame_options& o);
int64_t num_frames(const snf_frame_options& o, int64_t num_samples);
int64_t first_sample_of_frame(const snf_frame_options& o, int64_t frame);
int make_window(const snf_frame_options& o, std::vector<float>* w);

struct MelBanksHost {
  int num_bins = 0, num_fft_bins = 0;
  std::vector<int> first, size, offset;  // per bin: first fft bin, support length, offset in w
  std::vector<float> w;                  // concatenated supports
  std::vector<float> center_freqs;
};
int make_mel_banks(const snf_mel_options& mo, const snf_frame_options& fo, float vtln_warp,
                   MelBanksHost* out);
// structurally valid banks with zero weights: what a PLP plan holds in place of unwarped banks that the
// options do not allow, until an utterance asks for them (plan.h: snf_plan::base_banks_error)
void make_placeholder_banks(const snf_mel_options& mo, const snf_frame_options& fo, MelBanksHost* out);
void make_dct_matrix(int num_rows, int num_cols, std::vector<float>* m);  // first rows of NxN DCT
void make_lifter(float q, int n, std::vector<float>* c);
void make_equal_loudness(const MelBanksHost& mb, std::vector<float>* out);
void make_idft_bases(int n_bases, int dim, std::vector<float>* m);
void make_delta_scales(int order, int window, std::vector<float>* scales, std::vector<int>* dims);

struct LinearResampleHost {
  int rate_in = 0, rate_out = 0, in_unit = 0, out_unit = 0, num_zeros = 0, max_taps = 0;
  float cutoff = 0;
  std::vector<int> first;       // [out_unit]
  std::vector<int> ntaps;       // [out_unit]
  std::vector<float> weights;   // [out_unit][max_taps] zero padded
  int64_t num_output(int64_t n_in, bool flush) const;
};
void make_linear_resample(int rate_in, int rate_out, float cutoff, int num_zeros,
                          LinearResampleHost* out);
// ... everything but the weights: the phases' first taps and tap counts (what a size check needs)
void make_linear_resample_geometry(int rate_in, int rate_out, float cutoff, int num_zeros,
                                   LinearResampleHost* out);

struct PitchTablesHost {
  int first_lag = 0, last_lag = 0, num_lags = 0, num_states = 0;
  int win_size = 0, win_shift = 0, full_len = 0, max_taps = 0;
  std::vector<float> lags;        // [num_states]
  std::vector<int> ar_first;      // [num_states]
  std::vector<int> ar_n;          // [num_states]
  std::vector<float> ar_w;        // [num_states][max_taps]
  LinearResampleHost resample;
  int64_t frames_available(int64_t n_down, bool input_finished, bool snip_edges) const;
};
int make_pitch_tables(const snf_pitch_options& o, PitchTablesHost* out);

// ---------------------------------------------------------------------------------------------
// device parameter blocks (passed by value to kernels)
// ---------------------------------------------------------------------------------------------
struct MelParams {
  // framing
  int win_len, win_shift, padded, half, log2_half;  // half = padded/2 (complex FFT size)
  int snip_edges, remove_dc, pow2;
  float preemph, dither;
  unsigned long long seed;
  const float* window;       // [win_len]
  const float2* tw_fft;      // [half/2]     exp(-2 pi i k / half)
  const float2* tw_unpack;   // [half/2 + 1] exp(-2 pi i k / padded)
  const float2* tw_dft;      // [padded]     exp(-2 pi i k / padded) (non power-of-two path)
  // epilogue
  int kind, ndims;
  int use_energy, raw_energy, htk_compat, use_log, use_power, need_raw, need_post;
  int has_floor;
  float log_energy_floor;
  int num_bins, num_ceps, compression;
  const int* mel_first;      // [n_warps][num_bins]
  const int* mel_size;       // [n_warps][num_bins]
  const int* mel_offset;     // [n_warps][num_bins] offset into mel_w
  const float* mel_w;
  const float* mel_w32;      // long-frame kernel: the weights with every filter zero-padded to 32-tap slices
  const int* mel_off32;      // [n_warps][num_bins] offset into mel_w32 (slice 0 of mel_w32 is all zeros)
  const float* dct;          // [num_ceps][num_bins]
  const float* lifter;       // [num_ceps] or nullptr
};

// fbank256x2_kernel: one record per frame pair.  Pairs are formed INSIDE an utterance (frames 2 m and
// 2 m + 1 counted from the utterance's first frame; an odd last frame is paired with itself), so the
// features of an utterance do not depend on what else is in the batch.
struct PairRec {
  int64_t start_a, start_b;  // first sample of the two frames (clamped into the utterance)
  int64_t frame_a;           // batch-wide frame index of frame a (frame b, if any, is frame_a + 1)
  int32_t utt1;              // utterance + 1
  int32_t flags;             // bit 0 / 1: frame a / b reflects; bit 2: frame b exists
};

struct BatchArgs {
  const int16_t* wave;
  const int64_t* sample_offsets;  // [n_utts+1]
  const int64_t* frame_offsets;   // [n_utts+1]
  const int32_t* utt_warp;        // [n_utts] index into the plan's warp tables, or nullptr
  const int64_t* frame_start;     // [total_frames] first sample of every frame (fast path only)
  const int32_t* frame_edge;      // [total_frames] snip_edges = false: utterance + 1 of edge frames
  const int32_t* frame_utt;       // [total_frames] utterance of every frame (generic kernel)
  const int32_t* blk_utt;         // [n_blocks] fast path with VTLN warps: utterance of every workgroup
  const int32_t* blk_set0;        // [n_blocks] ... and its first frame set inside that utterance
  const uint8_t* utt_mask;        // [n_utts] generic kernel: when set, only the utterances marked 1 are computed
  const uint64_t* frame_noise;    // [total_frames] fbank512b_kernel with dither: wave_noise_id of every frame
  const uint32_t* utt_noise;      // [n_utts] dither: a hash of 64 samples spread over every utterance (per call)
  const PairRec* pair_tab;        // [n_pairs] fbank256x2_kernel / fbank1024x2_kernel only
  int64_t n_pairs;
  // fbank256x2_kernel: a pair of frames shares the roundings of ONE complex transform - the louder frame sets the
  // error floor of both.  Pairs whose windowed energies differ by more than `split_ratio` are appended here, as two
  // records of one frame each (a frame paired with itself), `fix_count` counting the records; a second launch
  // of the kernel over that list (`n_pairs_dev` = the count, read on the device) rewrites their rows.
  PairRec* fix_tab;
  unsigned int* fix_count;
  const unsigned int* n_pairs_dev;
  float split_ratio;
  int64_t n_blocks;
  int64_t n_utts;
  int64_t total_frames;
  // fbank512b_kernel: the samples of the whole batch where the set-relative 32-bit sample addressing holds for it
  // (fbank512b_rel32_ok, decided by route_mel_batch), 0 where the kernel keeps 64-bit addresses per lane
  int64_t rel32_samples;
};

// The noise stream of a frame (dither, delta-pitch noise) is keyed by what the frame IS, not by where it
// sits in the batch: its index inside its utterance, the utterance's length and 32 bits that stand for the
// utterance (a hash of 64 samples spread over the waveform / the bits of the first pitch value).  An utterance therefore draws the same noise alone and in
// any batch of the same call count (the per-call stream key is in `seed`), and the utterances of a batch draw
// different noise.  The reference draws from C rand(): no stream is "the" Kaldi one.
#if defined(__HIPCC__)
__device__ __forceinline__ uint64_t frame_noise_id(int64_t local_frame, int64_t utt_len, uint32_t first_bits) {
  uint64_t x = static_cast<uint64_t>(local_frame) * 0x9E3779B97F4A7C15ull +
               static_cast<uint64_t>(utt_len) * 0xC2B2AE3D27D4EB4Full + first_bits;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// ... of the frame `local_frame` of utterance `u` of a waveform batch.  What stands for "the utterance" is a
// 32-bit hash of 64 of its samples, spread evenly from its first to its last (launch_build_utt_noise, once
// per call; round 4 - the first two samples alone, as before, made every equal-length utterance that begins
// with digital silence draw the same dither: ADVICE r03).
__device__ __forceinline__ uint64_t wave_noise_id(const BatchArgs& b, int64_t u, int64_t local_frame) {
  const int64_t n = b.sample_offsets[u + 1] - b.sample_offsets[u];
  return frame_noise_id(local_frame, n, b.utt_noise[u]);
}
// Vector types of the matrix-core kernels (gemm_tiles.h, dtw_tiles.h) and the one rounding to bfloat16, which the
// collate kernels use too (v_cvt_pk_bf16_f32: to nearest, ties to even, subnormals kept, a NaN stays a NaN)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint16_t bf16_rne(float f) { return __builtin_bit_cast(uint16_t, static_cast<__bf16>(f)); }
__device__ __forceinline__ uint32_t bf16_pack2(float lo, float hi) {
  f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
#endif

struct PlpParams {
  int num_bins, lpc_order, num_ceps, use_energy, htk_compat, has_floor, rasta;
  int exact_pow;  // SNF_PLP_EXACT_POW=1: the correctly-rounded powf in plp_tail_exact_kernel (A/B runs)
  float compress_factor, cepstral_scale;
  double log_energy_floor;
  const float* eql;     // [n_warps][num_bins]
  const float* idft;    // [lpc_order+1][num_bins+2]
  const float* lifter;  // [num_ceps] or nullptr
};

struct DeltaParams {
  int order, window, n_scales;
  const float* scales;   // concatenated
  const int* dims;       // [order+1]
};

// ---------------------------------------------------------------------------------------------
// kernel launchers (kernels_*.hip)
// ---------------------------------------------------------------------------------------------
// Fused frame extraction -> window -> FFT -> power -> epilogue.  `out` is [total_frames, out_cols];
// for kind PLP it receives linear mel energies [total_frames, num_bins] and `energy_out`
// [total_frames] the linear frame energy (double; plp_tail_kernel floors it and takes the double log).
int launch_mel_features(const MelParams& p, const BatchArgs& b, float* out, int out_cols,
                        double* energy_out, hipStream_t stream);
int launch_rasta(float* mel, const BatchArgs& b, int num_bins, hipStream_t stream);
// `launched`: receives the name of the kernel the rows went to (plp_tail_exact_kernel, plp_tail_small_kernel or
// plp_tail_kernel; nullptr: nothing was launched)
int launch_plp_tail(const PlpParams& p, const BatchArgs& b, const float* mel, const double* energy,
                    float* out, hipStream_t stream, const char** launched = nullptr);
// `tile_info`: scratch of 4 (total_frames / 32 + 2) int64 (nullptr: per-element kernels only), rebuilt
// from the offsets table when `build_info` is set (the caller keeps it while the table stays the same).
// `launched`: receives the name of the kernel that computes the rows (delta_flat_o2w2_kernel,
// delta_tiled_fixed_kernel, delta_tiled_kernel or delta_kernel; nullptr: nothing was launched)
int launch_deltas(const DeltaParams& p, const float* in, int in_cols, const int64_t* frame_offsets,
                  int64_t n_utts, int64_t total_frames, float* out, int64_t* tile_info, bool build_info,
                  hipStream_t stream, const char** launched = nullptr);


// ---- register-resident 512-point fast path: fbank512_kernel (kernels_fbank512.hip), fbank256x2_kernel
// (kernels_fbank256x2.hip), fbank512b_kernel (kernels_fbank512b.hip); their tables: fast512_tables.cpp ----
constexpr int kFast512MaxBins = 64;    // mel bins: 16 MFMA blocks of 4 bins
// The LDS of a workgroup, stated once for the kernels, their launchers and the admission checks of the host
// layer: [table blob, rounded up to 256 bytes | waves x 4 frame tiles | fused deltas: cepstra of the
// workgroup's frame sets and one halo set on each side].
constexpr int kFast512HeaderFloats = 16;  // table header: the mel layout of one warp factor
constexpr int kFast512TileRow = 17;       // complex per transposed row (16 + 1 pad: conflict-free)
constexpr int kFast512TileBytes = 16 * kFast512TileRow * 8;  // wave-private LDS per frame (2176 B)
constexpr int kFast512MaxWaves = 16;    // wavefronts per workgroup: 8 when two workgroups fit the LDS of a CU
constexpr int kFast512MinWaves = 8;     // (measured 5 % faster), else one of 16
constexpr int kFast512FusedWaves = 14;  // fused deltas: 14 waves x 6 sets = 82 sets + one halo set on each side
constexpr int kFast512FusedSets = 82;   // (the +-4 frames the delta-delta reaches); a 3 s utterance (75 sets) is
                                        // one workgroup without any halo
constexpr int kFast512Sets = 64;        // per-utterance schedule: frame sets (of 4 frames) per workgroup
constexpr int kFast512FusedCols = 16;   // cepstra per row of the fused form's LDS buffer (num_ceps <= 16)
constexpr size_t kFast512LdsBytes = 160 * 1024;  // LDS of a CU
constexpr size_t fast512_table_bytes(int table_floats) {
  return (static_cast<size_t>(table_floats) * 4 + 255) & ~static_cast<size_t>(255);
}
constexpr size_t fast512_lds_bytes(int table_floats, int waves, bool fused) {
  return fast512_table_bytes(table_floats) + static_cast<size_t>(waves) * 4 * kFast512TileBytes +
         (fused ? sizeof(float) * 4 * (kFast512FusedSets + 2) * kFast512FusedCols : 0);
}
struct Fast512Params {
  int win_len, win_shift, remove_dc, snip_edges;
  float preemph, dither;
  unsigned long long seed;
  int kind, out_cols, use_energy, need_raw, need_post, htk_compat, use_log, has_floor;
  float log_energy_floor;
  int num_bins, num_ceps, compression;
  // mel filterbank as a chain of v_mfma_f32_4x4x1_16b_f32: 16 blocks of (4 mel bins x 4 frames), one
  // FFT bin per block and instruction; `mm_quads` = chain length / 4, `mm_levels` = the most blocks a
  // group of 4 bins is split into along the FFT bins (partial sums are added through DPP)
  int mm_quads, mm_levels;
  int dd_quads;              // MFCC: DCT-II chain length / 4 (mel bins per K partition / 4)
  int dd_groups;             // MFCC, vector-pipe DCT: groups of 4 mel bins (ceil(num_bins / 4))
  int dct_mfma;              // MFCC: 1 = DCT-II as the MFMA chain (SNF_DCT_MFMA=1; measured slower), 0 = vector pipe
  int dual;                  // frames pad to 256 samples: two frames per 16-lane row (fbank256x2_kernel)
  int fused_delta;           // MFCC: rows are [cepstra | delta | delta-delta] (order 2, window 2)
  const float* delta_scales; // ... composite scales of the three orders, 1 + 5 + 9 floats (device)
  int table_floats;          // total floats of the packed table blob below (warp 1.0)
  int table_stride;          // floats between the blobs of consecutive warp factors (VTLN)
  // one packed blob, copied to LDS at kernel start:
  //   header[16] | float2 win[16][18] | float2 tw16[16][18] | float2 tw512[16][10] |
  //   float4 mm_a[mm_quads][64] | mm_lane[5][64] | float4 dd_a[dd_quads][64] | float lifter[16] |
  //   float4 dd_v[dd_groups][16]
  const float* tables;
  int off_mm_a, off_mm_lane, off_dd_a, off_lifter, off_dd_v;  // float offsets into the blob
};

bool fast512_eligible(const MelParams& mp, bool any_warp);
// frames that pad to 256 samples: the two-frames-per-row form (flat batches without VTLN warps)
bool fast512_dual_eligible(const MelParams& mp);
int fast512_build(const MelParams& mp, const std::vector<float>& window, const MelBanksHost& mb,
                  const std::vector<float>& dct, const std::vector<float>& lifter, bool dual,
                  std::vector<float>* blob, Fast512Params* out);
int launch_build_pair_table(const int64_t* d_frame_offsets, const int64_t* d_sample_offsets,
                            const int64_t* d_pair_offsets, int64_t n_utts, int64_t n_pairs, int win_shift,
                            int win_len, int snip_edges, PairRec* d_pairs, hipStream_t stream);
int launch_build_frame_start(const int64_t* d_frame_offsets, const int64_t* d_sample_offsets,
                             int64_t n_utts, int64_t total_frames, int64_t total_samples, int win_shift,
                             int win_len, int snip_edges, int64_t* d_frame_start, int32_t* d_frame_edge,
                             int32_t* d_frame_utt, hipStream_t stream);
// `launched`: receives the name of the kernel the call went to (fbank512b_kernel, fbank256x2_kernel or
// fbank512_kernel; nullptr: none)
int launch_fbank512(const Fast512Params& p, const BatchArgs& b, float* out, int out_cols,
                    double* energy_out, hipStream_t stream, const char** launched = nullptr);
// the two-frames-per-row half of launch_fbank512 (kernels_fbank256x2.hip; `p.dual` tables, `b` carries the
// pair table): the launch over the pairs and, with a fix-up list, the one over the pairs it put down
int launch_fbank256x2(const Fast512Params& p, const BatchArgs& b, float* out, int out_cols,
                      double* energy_out, hipStream_t stream);
// per-call table of the frames' noise keys (wave_noise_id: the dither of fbank512b_kernel; the keys hold
// the first two samples of the utterance, so they are rebuilt with every batch)
int launch_build_frame_noise(const BatchArgs& b, uint64_t* d_keys, hipStream_t stream);
// per-call table of the utterances' noise words (every dithering kernel reads it through wave_noise_id)
int launch_build_utt_noise(const BatchArgs& b, uint32_t* d_words, hipStream_t stream);
// the occupancy-first form of the same kernel (kernels_fbank512b.hip): flat, snip_edges batches
bool fbank512b_eligible(const Fast512Params& p, const BatchArgs& b);
// ... everything of it that does not depend on the frames' noise key table: whoever makes that table asks this
bool fbank512b_shape_ok(const Fast512Params& p, bool per_utt);
// ... and whether the frame starts of any four consecutive frames of the batch lie less than 2^30 samples apart
// (host offset tables): the kernel's set-relative 32-bit sample addressing
bool fbank512b_rel32_spans_ok(const int64_t* sample_offsets, const int64_t* frame_offsets, int64_t n_utts);
// ... unless SNF_FBANK512B_ADDR64=1 keeps every batch on the 64-bit form (read at every call)
bool fbank512b_addr64_knob();
bool fbank512b_rel32_ok(const int64_t* sample_offsets, const int64_t* frame_offsets, int64_t n_utts);
int launch_fbank512b(const Fast512Params& p, const BatchArgs& b, float* out, int out_cols,
                     double* energy_out, hipStream_t stream);
// fbank512b_kernel deals the frame sets to the waves of a workgroup as they finish (DEAL): workgroup b of
// `blocks` owns the contiguous sets [lo, hi), the shares tile [0, n_sets) in order and differ by at most one
// set: n_sets = blocks * base + rem, and the first `rem` shares hold base + 1.  The quotient is formed once, in
// 64 bits, on the host; the kernel gets (base, rem) and forms its lo and hi in scalar registers.
struct Fast512bShares {
  int64_t base;
  int64_t rem;
};
inline Fast512bShares fbank512b_shares(int64_t n_sets, int64_t blocks) {
  return blocks > 0 ? Fast512bShares{n_sets / blocks, n_sets % blocks} : Fast512bShares{0, 0};
}
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int64_t fbank512b_share_lo(const Fast512bShares& s, int64_t b) {
  return b * s.base + (b < s.rem ? b : s.rem);
}
// ... as a host function of its own (tests/test_fbank512b_share.py through snf_debug_fbank512b_share)
void fbank512b_share(int64_t n_sets, int64_t blocks, int64_t b, int64_t* lo, int64_t* hi);
// workgroups of a launch over n_sets frame sets: one per CU, fewer for a batch of fewer than 16 sets each
int64_t fbank512b_blocks(int64_t n_sets);

// ---- register-resident 2048-point path (kernels_fbank2048.hip): frames that pad to 2048 samples (44.1 / 48 kHz)
bool fbank2048_eligible(const MelParams& mp);
void fbank2048_tables(const MelParams& mp, const std::vector<float>& window, std::vector<float>* blob);
int launch_fbank2048(const MelParams& p, const BatchArgs& b, const float* tables, float* out, int out_cols,
                     double* energy_out, hipStream_t stream);

// ---- two 1024-sample frames per complex transform (kernels_fbank1024x2.hip): 22.05 / 32 kHz frames; `b` carries
// the pair table of launch_build_pair_table
bool fbank1024x2_eligible(const MelParams& mp);
void fbank1024x2_tables(const MelParams& mp, const std::vector<float>& window, std::vector<float>* blob);
int launch_fbank1024x2(const MelParams& p, const BatchArgs& b, const float* tables, float* out, int out_cols,
                       double* energy_out, hipStream_t stream);

// MFCC tail behind the filterbank kernels (kernels_dct.hip): DCT, lifter, energy and htk conventions on rows of
// [log energy |] log-mel energies
int launch_mfcc_dct(const float* in, int in_cols, int num_bins, int num_ceps, const float* dct_t, const float* lifter,
                    int use_energy, int htk_compat, int64_t total_frames, float* out, int out_cols,
                    hipStream_t stream);

struct PitchDevTables {
  int first_lag, last_lag, num_lags, num_states, win_size, win_shift, full_len;
  int ar_max_taps, rs_in_unit, rs_out_unit, rs_max_taps;
  int snip_edges, recompute_frame;
  float soft_min_f0, inter_frame_factor, nccf_ballast;
  const float* lags;      // [num_states]
  const int* ar_first;    // [num_states]
  const int* ar_n;        // [num_states]
  const float* ar_w;      // [num_states][ar_max_taps]
  // the same taps laid out for the matrix pipe (pitch_nccf_kernel): states in groups of 64 = 16 quads;
  // a quad shares a window of ar_quad_taps lags starting at ar_quad_base (zero weight where a state has
  // no tap); ar_groups is even (a zero-weight group pads an odd count)
  int ar_groups, ar_quad_taps;
  const float* ar_quad_w;   // [ar_groups][ar_quad_taps / 4][64 = quad * 4 + state][4]
  const int* ar_quad_base;  // [ar_groups][16]
  const int* rs_first;    // [rs_out_unit]
  const int* rs_ntaps;    // [rs_out_unit]
  const float* rs_w;      // [rs_out_unit][rs_max_taps]
};
struct PitchBatch {
  const int16_t* wave;
  const int64_t* sample_offsets;  // [n_utts+1]
  const int64_t* frame_offsets;   // [n_utts+1]
  const int64_t* down_offsets;    // [n_utts+1] offsets into the downsampled scratch
  const int64_t* down_phase1;     // [n_utts] samples available before the flush
  const int64_t* frames_phase1;   // [n_utts] frames processed before the flush
  const int32_t* order;           // [n_utts] utterance handled by every tracker slot (longest first), or nullptr
  int64_t n_utts, total_frames, total_down;
  int64_t max_down;               // longest downsampled utterance
};
// scratch of one pitch batch (all in HBM, owned by the plan)
struct PitchScratch {
  float* down;       // [total_down]                  signal resampled to resample_freq
  float* ub;         // [n_utts][6]                   NCCF ballasts of every utterance (pitch_stats_kernel)
  float* nccf_res;   // [total_frames][num_states]    NCCF (with ballast) at the lag of every state
  float* pov_nccf;   // [total_frames][num_lags]      NCCF without ballast at the integer lags
  float* anp;        // [total_frames]                average norm product (RecomputeBacktraces)
  int16_t* backptr;  // [total_frames][num_states]
  int32_t* states;   // [total_frames]                traceback
  int4* frame_meta;  // [total_frames]                window start / existing samples / ballast of every frame
};
// resample -> signal statistics -> frame-parallel NCCF + lag resampling -> Viterbi per utterance ->
// traceback + POV output
int launch_pitch(const PitchDevTables& t, const PitchBatch& b, const PitchScratch& w, float* out,
                 hipStream_t stream);
// its pieces (kernels_pitch_front.hip, kernels_pitch_flat.hip), called by launch_pitch alone.  `trace`: the
// SNF_PITCH_TRACE knob - pitch_stage_done waits for the stage, reports it and returns nonzero if the call ends
// behind it; *stop: it ended inside the front stages
int pitch_stage_done(int trace, const char* name, int index, hipStream_t stream);
int launch_pitch_front(const PitchDevTables& t, const PitchBatch& b, const PitchScratch& w, int trace,
                       hipStream_t stream, bool* stop);
int launch_pitch_viterbi_flat(const PitchDevTables& t, const PitchBatch& b, const PitchScratch& w, size_t lds,
                              float* out, hipStream_t stream);

int launch_vad(const snf_vad_options& o, const float* in, int in_cols, const int64_t* frame_offsets,
               int64_t n_utts, int64_t total_frames, float* thr_scratch, float* out,
               hipStream_t stream);
// `launched`: cmvn_stats_kernel or cmvn_stats_wide_kernel (nullptr: nothing was launched)
int launch_cmvn_stats(const float* in, int in_cols, const int64_t* frame_offsets,
                      const float* weights, int64_t n_utts, double* stats, hipStream_t stream,
                      const char** launched = nullptr);
int launch_cmvn_apply(const float* in, int in_cols, const int64_t* frame_offsets, int64_t n_utts,
                      int64_t max_frames, const int32_t* group, const float* norm, int scale_it,
                      float* out, hipStream_t stream);
int launch_concat_columns(const float* a, int cols_a, const int64_t* d_off_a, const float* b, int cols_b,
                          const int64_t* d_off_b, int64_t n_utts, float* out, const int64_t* d_off_out,
                          int64_t total_rows, hipStream_t stream);
int launch_count_nonfinite(const float* x, uint64_t n, unsigned long long* d_count, hipStream_t stream);
// kernels_collate.hip: ragged block -> padded batch (snf_collate_padded)
struct CollateUtt {
  int64_t row0;     // first row of the utterance in the block
  int32_t frames;   // its rows
  int32_t n_out;    // the rows kept of it (snf_collate_num_out)
};
struct CollateShape {
  int32_t dim, width, left, subsample, offset, t_max;   // width = left + 1 + right
  uint32_t row_elems, utt_elems, total, n_utts;         // dim width, t_max row_elems, n_utts utt_elems
};
int launch_collate_padded(const float* in, const CollateUtt* d_utts, const CollateShape& shape, int out_type,
                          float pad_value, void* out, int32_t* lengths, hipStream_t stream);
int launch_sliding_cmvn(const snf_sliding_cmvn_options& o, const float* in, int in_cols,
                        const int64_t* frame_offsets, int64_t n_utts, float* out,
                        hipStream_t stream);
// kernels_dtw.hip: DTW cost and path length of pairs of items (snf_dtw_pairs)
constexpr int kDtwMaxFrames = 4096;   // rows of an item: the seam row of the largest kernel class holds as many columns
constexpr int kDtwMaxDim = 4096;
constexpr int kDtwClasses = 3;        // kernel classes by the columns M of a pair: M <= 32, <= 512, <= kDtwMaxFrames
struct DtwItem {
  int64_t row0;     // first row of the item in the block
  int32_t frames;   // its rows
  int32_t unused;
};
struct DtwPair {
  int32_t x, y;     // item indices: x gives the rows of the lattice, y its columns
  int32_t out;      // where the result goes (the caller's pair order)
  int32_t cells;    // frames(x) frames(y): the sort key
};
int dtw_class_of(int32_t columns);
// floats of `d_aux` for n_rows rows: one per row; symkl: dim + 1 per row (h of the row, then its logarithms)
size_t dtw_aux_floats(int64_t n_rows, int dim, int metric);
// `d_pairs`: the pairs of class 0, then 1, then 2 (`class_count` of each), each class sorted by cells descending;
// `d_aux`: dtw_aux_floats(row_hi - row_lo, dim, metric) floats, written by the pre-pass
int launch_dtw_pairs(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                     const int64_t* class_count, int64_t row_lo, int64_t row_hi, float* d_aux, int metric,
                     int compute_units, float* cost, int32_t* len, hipStream_t stream);
// the pre-pass alone: the norms (symkl: h and the logarithms) of the rows [row_lo, row_hi) into `d_aux`
int launch_dtw_rows(const float* rows, int dim, int64_t row_lo, int64_t row_hi, float* d_aux, int metric,
                    hipStream_t stream);
// kernels_dtw_search.hip: subsequence DTW of a query (x of the pair: the rows of the lattice) in a target (y: its
// columns, which decide the class), free start and free end (snf_dtw_search).  Tables and `d_aux` as above.
struct DtwSearchOut {
  float* cost;                   // [P] in the caller's pair order, as len, start, end
  int32_t *len, *start, *end;
  const int64_t* curve_first;    // device copy of the caller's element offsets [P], or null: no curves
  float* curve_cost;             // C, L, B of every end j of pair p at element curve_first[p] + j
  int32_t *curve_len, *curve_start;
};
int launch_dtw_search(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                      const int64_t* class_count, int64_t row_lo, int64_t row_hi, float* d_aux, int metric,
                      int normalized, int compute_units, const DtwSearchOut& out, hipStream_t stream);
// kernels_dtw_detect.hip: up to `k` detections per pair, a greedy non-maximum suppression over the ends of the same
// lattice, behind it in the same wave (snf_dtw_detect); and the best `t` detections per query of what it left in
// HBM (snf_dtw_topk)
constexpr int kDtwMaxDetections = 64;   // SNF_DTW_MAX_DETECTIONS
constexpr int kDtwMaxTopk = 1024;       // SNF_DTW_MAX_TOPK
struct DtwDetectOut {
  int32_t* count;                // [P] in the caller's pair order
  float* cost;                   // [P * k]: pair p, rank r at p * k + r, as len, start, end
  int32_t *len, *start, *end;
  int32_t k;                     // 1 <= k <= kDtwMaxDetections
  float max_score;               // a detection needs score <= max_score (+inf: every one does)
  const int64_t* curve_first;    // the curves of DtwSearchOut
  float* curve_cost;
  int32_t *curve_len, *curve_start;
};
int launch_dtw_detect(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                      const int64_t* class_count, int64_t row_lo, int64_t row_hi, float* d_aux, int metric,
                      int normalized, int compute_units, const DtwDetectOut& out, hipStream_t stream);
struct DtwTopkIn {
  const int32_t* count;          // the arrays that snf_dtw_detect wrote, k slots per pair
  const float* cost;
  const int32_t *len, *start, *end;
  int32_t k;
  const int32_t* group_pair;     // device: the pair indices grouped by query
  const int64_t* group_first;    // device [Q + 1]: query q owns group_pair[group_first[q] .. group_first[q + 1])
};
struct DtwTopkOut {
  int32_t* count;                // [Q]
  int32_t *pair, *rank;          // [Q * t]: query q, place i at q * t + i, as cost, len, start, end
  float* cost;
  int32_t *len, *start, *end;
};
int launch_dtw_topk(const DtwTopkIn& in, int64_t n_queries, int top_k, int normalized, const DtwTopkOut& out,
                    hipStream_t stream);
// kernels_dtw_align.hip: the warping paths (snf_dtw_align).  The lattices of kernels_dtw.hip and dtw_strips.h, run
// with a record policy, leave the decision of every cell in `rec` (the layout: the top of kernels_dtw_align.hip), and
// a traceback kernel behind them on the same stream walks the records back from the ends that the lattice wrote
struct DtwNoRecords {};          // the record policy of snf_dtw_pairs, snf_dtw_search, snf_dtw_detect: none
struct DtwRecords {
  uint4* rec;                    // the records of the pairs of a launch
  const int64_t* first;          // device: the first record of pair p of the launch (in its sorted order)
};
struct DtwAlignOut : DtwDetectOut {   // the subsequence lattice with the detections' tail and records
  DtwRecords records;
};
constexpr int64_t kDtwRecordBytes = 16;
constexpr int64_t kDtwDefaultScratch = int64_t(1) << 30;
// records of the lattice of N rows and M columns: every strip of R rows has R + M - 1 steps
inline int64_t dtw_record_count(int64_t n, int64_t m) { return n + ((n + 63) / 64) * (m - 1); }
struct DtwPaths {
  const int64_t* first;          // device [P * k] in the caller's order: slot p * k + r owns [first, first + N + M - 1)
  int32_t *x, *y;                // the frames of the path's cells, forward
};
// One run: `d_pairs` are `run_count[c]` pairs of class c = 0, 1, 2 in this order (a stretch of the sorted pairs),
// `records.first` their first records.  `d_aux` is written already (launch_dtw_rows).  Global (`subsequence` 0): cost
// and len [P] as launch_dtw_pairs, one path per pair; else `out` as launch_dtw_detect (no curves), one path per live
// detection.
int launch_dtw_align(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                     const int64_t* run_count, int64_t row_lo, const float* d_aux, int metric, int subsequence,
                     int normalized, int compute_units, const DtwDetectOut& out, const DtwRecords& records,
                     const DtwPaths& paths, hipStream_t stream);

// kernels_abx.hip: ABX triplet counts per cell over a table of distances (snf_abx_cells)
constexpr int kAbxTile = 1024;        // floats of a B-row staged in LDS at a time (4 KB per wave)
struct AbxCell {
  int64_t offA, offB, stride;   // dAX = element offA + x stride + a, dBX = element offB + x stride + b
  int32_t nA, nB, nX, same;     // every one of nA, nB, nX in [1, 2^31): the host has checked
};
struct AbxUnit {
  int32_t cell;       // index into the cell table (the caller's order: where the counts go)
  int32_t x0, x1;     // the stretch of X this unit counts
  int32_t split;      // 1: the cell has other units, the counts are added with 64-bit vector atomics
};
// `d_small`: the cells that one lane counts each; `d_units`: whole cells and stretches of split cells, one wave
// each, sorted by work descending.  `d_counts` [n_cells][3] has been zeroed in stream order when a unit is split.
int launch_abx_cells(const float* cost, const int32_t* len, const AbxCell* d_cells, const int32_t* d_small,
                     int64_t n_small, const AbxUnit* d_units, int64_t n_units, int compute_units,
                     unsigned long long* d_counts, hipStream_t stream);

struct PitchPostParams {
  snf_pitch_post_options o;
  int ndims;
  unsigned long long seed;
};
int launch_pitch_post(const PitchPostParams& p, const float* in, const int64_t* frame_offsets,
                      int64_t n_utts, int64_t total_frames, float* out, hipStream_t stream,
                      const char** launched = nullptr);  // pitch_post_tiled_kernel or pitch_post_kernel

// GMM kernels (kernels_gmm.hip): see that file's header for the design
int64_t gmm_stats_chunks(int64_t F, int C, int D);
int64_t gmm_tiles(int64_t F);
int launch_gmm_loglikes(const float* x, int64_t F, int D, const float* gconst, const float* mi, const float* iv, int C,
                        float* out, hipStream_t stream);
int launch_gmm_accumulate(const float* x, int64_t F, int D, const float* weights, const float* gconst,
                          const float* mi, const float* iv, int C, float* lse, double* tl_part, double* part,
                          double* stats, double* tot_like, hipStream_t stream);
// lse [F] (the E-step's reduction, unit weights; tl_part [gmm_tiles(F)] scratch) and post[f, c] = exp(L[f, c] - lse[f])
int launch_gmm_posteriors(const float* x, int64_t F, int D, const float* gconst, const float* mi, const float* iv,
                          int C, float* lse, double* tl_part, float* post, hipStream_t stream);
int launch_gmm_topn(const float* L, const int32_t* map, int64_t rows, int P, int n, int32_t* out_idx, float* out_lse,
                    hipStream_t stream);
int launch_gmm_sel_loglikes(const float* x, int64_t F, int D, const float* gconst, const float* mi, const float* iv,
                            int C, const int32_t* sel, int P, float* out, int* bad, hipStream_t stream);
int launch_gmm_post(float* post, int64_t F, int n, float min_post, int prune, float* loglike, hipStream_t stream);

// linear-VTLN kernels (kernels_vtln.hip): see that file's header for the design
int64_t vtln_item_frames();
int launch_fmllr_accumulate(const float* x, int64_t F, int D, const int32_t* sel, const float* post, int n,
                            const float* mi, const float* iv, int C, double* rec, int* bad, const int64_t* items,
                            int64_t n_items, int64_t S, double* out, double* part, const int64_t* red, int64_t n_red,
                            hipStream_t stream);
int launch_vtln_gram(const float* x, const float* y, const float* w, int64_t F, int D, double* rec,
                     const int64_t* items, int64_t n_items, double* out, double* part, const int64_t* red,
                     int64_t n_red, hipStream_t stream);
int launch_vtln_gram_rows(const float* const* xb, const float* const* yb, const int32_t* blk, const int64_t* row,
                          const float* w, int64_t F, int D, double* rec, const int64_t* items, int64_t n_items,
                          double* out, double* part, const int64_t* red, int64_t n_red, hipStream_t stream);
int launch_lvtln_select(const double* stats, int64_t S, int D, const double* A, const double* logdets, int C,
                        int norm_type, double logdet_scale, int default_class, double* objf, int32_t* cls,
                        double* impr, double* count, float* transform, hipStream_t stream);
int launch_affine_apply_segments(const float* x, int64_t F, int D, const int64_t* off, int64_t S, const float* W,
                                 float* y, hipStream_t stream);

// bottleneck extractor kernels (kernels_bottleneck.hip): see that file's header for the design
int bn_table_floats();   // floats of the front end's table blob: window[200] | twiddles[256 x 2] | mel[129 x 24]
int bn_max_context();
// y = act(A w + b); `a_row` non-null: A[r][k] = x[(a_row[r] + gs (k / gw)) * gw + k % gw]
int launch_bn_dense(const float* x, int64_t M, int K, const float* w, const float* b, int N, int act, float* y,
                    const int64_t* a_row, int gw, int gs, hipStream_t stream);
// bfloat16 layer: wt[N][Kp] is the packed image of w[K][N], Kp = bn_bf16_padded_k(K), 16-byte aligned
int bn_bf16_padded_k(int K);
int launch_bn_pack_bf16(const float* w, int K, int N, uint16_t* wt, hipStream_t stream);
// y = act(bf16(x) bf16(w) + b), float32 accumulation, float32 y
int launch_bn_dense_bf16(const float* x, int64_t M, int K, const uint16_t* wt, const float* b, int N, int act,
                         float* y, hipStream_t stream);
int launch_bn_row_map(const int64_t* in_off, const int64_t* out_off, int64_t n_utts, int64_t rows, int64_t* a_row,
                      hipStream_t stream);
int launch_bn_fbank(const int16_t* wave, const int64_t* soff, const int64_t* foff, int64_t n_utts,
                    int64_t total_frames, const float* tables, float dither, uint64_t seed, uint32_t* utt_noise,
                    float* out, hipStream_t stream);
int launch_bn_vad(const int16_t* wave, const int64_t* soff, const int64_t* foff, int64_t n_utts, double* energy,
                  uint8_t* mask, int32_t* voiced, hipStream_t stream);
int launch_bn_nn_input(const float* logmel, const uint8_t* mask, const int32_t* voiced, const int64_t* foff,
                       const int64_t* roff, int64_t n_utts, int64_t total_rows, int context, const float* hd,
                       float* mean, float* x, hipStream_t stream);
// status[u] = (voiced[u] == 0) | 2 (a non-finite value in rows out_start[u] .. + ooff[u + 1] - ooff[u] of out[. x 80])
int launch_bn_status(const int32_t* voiced, const float* out, const int64_t* out_start, const int64_t* ooff,
                     int64_t n_utts, int32_t* status, hipStream_t stream);

// CREPE pitch kernels (kernels_crepe.hip): see that file's header for the design
constexpr int kConvNorm = 1, kConvPool = 2, kConvSigmoid = 4;   // epilogue of launch_crepe_conv
int crepe_table_doubles();   // float64 entries of the decoder's table blob
// y = epilogue(A w): row (f, t) of A is the run of K floats from (t * step - lead) inside frame f's block of L
// floats of x, zero outside the block; kConvPool halves the rows (maximum over position pairs)
int launch_crepe_conv(const float* x, int64_t frames, int T, int step, int lead, int L, int K, const float* w,
                      const float* b, const float* scale, const float* shift, int N, int flags, float* y,
                      hipStream_t stream);
// the same block on the bfloat16 matrix cores: wt[N][Kp] the packed image of w (launch_bn_pack_bf16), x and y
// float32 or bfloat16 (`x_bf16`, `y_bf16`); step, lead, L and K multiples of 8, x and wt 16-byte aligned
int launch_crepe_conv_bf16(const void* x, int x_bf16, int64_t frames, int T, int step, int lead, int L, int K,
                           const uint16_t* wt, const float* b, const float* scale, const float* shift, int N,
                           int flags, void* y, int y_bf16, hipStream_t stream);
int launch_crepe_frames(const int16_t* wave, const int64_t* soff, const int64_t* foff, int64_t n_utts, int64_t first,
                        int64_t count, int hop, int center, float* out, hipStream_t stream);
// bins[2 x total]: first argmax per frame, then the decoded bin; out[total x 2] (confidence, Hertz)
int launch_crepe_decode(const float* act, const int64_t* foff, int64_t n_utts, int64_t total, int viterbi,
                        const double* tab, float* conf, uint16_t* psi, int32_t* bins, double* out,
                        hipStream_t stream);

// The tail of the CREPE path (kernels_crepe_tail.hip): see that file's header for the design
constexpr int kCrepeRowsTile = 64;          // output rows of one workgroup of the row resampler (a row per lane)
constexpr int kCrepeRowsStage = 1024;       // input rows it holds in LDS at a time
constexpr int kCrepeVoicingChunk = 1024;    // frames of the voicing lattice staged in LDS at a time
constexpr int kCrepeVoicingModel = 11;      // float64 entries of the voicing model (include/shennong_amd.h)
// tile k (one workgroup) belongs to utterance tile_utt[k], whose first tile is tile_off[utterance]
int launch_crepe_rows(const double* in, const int64_t* in_off, const int64_t* out_off, const int32_t* tile_utt,
                      const int64_t* tile_off, int64_t n_tiles, double* out, hipStream_t stream);
// h_model: HOST; lattice[total x 2] and next_voiced[total] scratch; out[total x 2] (NCCF, pitch), status[n_utts]
int launch_crepe_voicing(const double* rows, const int64_t* off, int64_t n_utts, const double* h_model,
                         double* lattice, int32_t* next_voiced, float* out, int32_t* status, hipStream_t stream);

// Framed one-hot labels (kernels_onehot.hip): see that file's header for the design.  Device pointers; the
// caller (capi_onehot.hip) has checked on the host everything the kernels index with.
constexpr int kOneHotMaxFrameLength = 8192;   // samples per frame: the window sits in LDS
struct OneHotBatch {
  int64_t n_ali, n_seg, total_frames, total_bytes;   // total_bytes: of the dense rows, a multiple of 16
  int frame_length, frame_shift;
  double rate;
  const int64_t *seg_off, *frame_off, *row_off, *nsamples;   // [n_ali + 1] x 3, [n_ali]
  const double *onset0, *offsets;                             // [n_ali], [n_seg]
  const int32_t *ids, *ntokens;                               // [n_seg], [n_ali]
  const float* window;                                        // [frame_length]
  int64_t* ends;                                              // [n_seg] scratch: first sample past every segment
  int32_t* winner;                                            // [total_frames]
  uint8_t* rows;                                              // [total_bytes]
};
int launch_framed_onehot(const OneHotBatch& batch, hipStream_t stream);

// General LinearResample (kernels_resample.hip): see that file's header for the design.  The table blob the
// kernel copies into LDS word for word: first[out_unit] | ntaps[out_unit] | weights[out_unit][stride] (int32,
// int32, float32); `stride` is max_taps made odd, so that the lanes of a wave, each on its own phase, read
// different banks.
constexpr int kResampleChunk = 256;    // outputs a workgroup filters from one staged span
constexpr int kResampleChunks = 4;     // consecutive chunks per workgroup (its run: 1024 outputs)
constexpr int kResampleLdsBytes = 64 * 1024;
struct ResampleTable {
  int in_unit, out_unit, max_taps, stride;
  int table_words;   // 32-bit words of the blob
  int span;          // most input samples any chunk touches: the staged floats
  const int32_t* blob;   // device
};
struct ResampleUtt {   // per utterance, in samples of the element type
  int64_t src, n_in, dst, n_out;
};
// the blob's layout and the span from a table's geometry (`t->blob` stays null); weights may be empty
void resample_layout(const LinearResampleHost& r, ResampleTable* t);
void resample_blob(const LinearResampleHost& r, const ResampleTable& t, std::vector<int32_t>* blob);
// `kind` 0: int16 in and out (rintf, clamped), 1: float32; `d_utts[n_utts]` on the device
int launch_linear_resample(const ResampleTable& t, int kind, const void* src, const ResampleUtt* d_utts,
                           int64_t n_utts, int64_t max_out, void* dst, hipStream_t stream);

}  // namespace snf

#endif  // SNF_INTERNAL_H_
