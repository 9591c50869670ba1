// Which kernel each of the four laddered launchers of the post-processing path takes - launch_plp_tail
// (kernels_plp_tail.hip), launch_deltas (kernels_delta.hip), launch_pitch_post (kernels_pitch_post.hip),
// launch_cmvn_stats (kernels_cmvn.hip) - and the LDS those kernels carve up, stated once.  Plain C++17 - no device,
// no library; the public header is read for the pitch options alone -, so that tests/tools/post_route_dump.cpp
// compiles it alone (tests/test_post_route.py compares it with the ladders as tests/post_layouts.py states them).
#ifndef SNF_POST_ROUTE_H_
#define SNF_POST_ROUTE_H_

#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/shennong_amd.h"

namespace snf {

constexpr int kMaxBins = 126;   // plp_tail_kernel's arrays: mel bins ...
constexpr int kMaxLpc = 63;     // ... and LPC order
constexpr int kDeltaRows = 256;   // output rows per tile of delta_tiled_kernel and delta_tiled_fixed_kernel
constexpr int kPostRows = 256;    // ... of pitch_post_tiled_kernel
constexpr size_t kPostLdsLimit = 48 * 1024;   // dynamic LDS a workgroup of this path asks for at the most
constexpr int kFlatTileBytes = 28 * 1024;     // delta_flat_o2w2_kernel: input tile + output image of one workgroup
constexpr int kFlatCols[] = {13, 23, 40, 43};   // the column counts delta_flat_o2w2_kernel is instantiated for
constexpr bool is_flat_cols(int cols) {
  for (int d : kFlatCols) if (d == cols) return true;
  return false;
}
// rows per tile of delta_flat_o2w2_kernel<D>: a multiple of 4 (16-byte aligned output blocks) that fits the LDS budget
constexpr int flat_rows(int D) {
  int rows = (kFlatTileBytes / 4 - 8 * D - 8) / (4 * D);
  rows &= ~3;
  return rows > 256 ? 256 : rows;
}

// ---- LDS layouts ------------------------------------------------------------------------------------------------
// delta_tiled_kernel: first and last tile row of every output row's utterance (2 x kDeltaRows ints), the scale table
// rounded up to 16 bytes, the tile of kDeltaRows + 2 halo input rows.  delta_tiled_fixed_kernel: the same without
// the table (its scales sit in registers).
constexpr int delta_scales_floats(int n_scales) { return (n_scales + 3) & ~3; }
constexpr int delta_tile_rows(int halo) { return kDeltaRows + 2 * halo; }
constexpr size_t delta_tiled_fixed_lds_bytes(int halo, int cols) {
  return 2 * sizeof(int) * kDeltaRows + sizeof(float) * static_cast<size_t>(delta_tile_rows(halo)) * cols;
}
constexpr size_t delta_tiled_lds_bytes(int n_scales, int halo, int cols) {
  return delta_tiled_fixed_lds_bytes(halo, cols) + sizeof(float) * delta_scales_floats(n_scales);
}
// pitch_post_tiled_kernel: the POV weights, then the log pitches, of kPostRows frames and the halos around them.
// A halo is the larger of the normalisation context and the delta window on its side, and never negative.
struct PitchPostHalos { int left, right; };
constexpr int pitch_post_halo(int context, int delta_window) {
  const int halo = delta_window > context ? delta_window : context;
  return halo < 0 ? 0 : halo;
}
constexpr PitchPostHalos pitch_post_halos(const snf_pitch_post_options& o) {
  return {pitch_post_halo(o.normalization_left_context, o.delta_window),
          pitch_post_halo(o.normalization_right_context, o.delta_window)};
}
constexpr int pitch_post_tile_rows(int halo_l, int halo_r) { return kPostRows + halo_l + halo_r; }
constexpr size_t pitch_post_lds_bytes(int halo_l, int halo_r) {
  return sizeof(float) * 2 * static_cast<size_t>(pitch_post_tile_rows(halo_l, halo_r));
}
// cmvn_stats_kernel: R groups of threads take the rows r, r + R, ... of an utterance, [R][2 cols + 1] doubles
constexpr int cmvn_row_groups(unsigned threads, int cols) { return threads / cols > 0 ? threads / cols : 1; }
constexpr size_t cmvn_stats_lds_bytes(int cols) { return sizeof(double) * cmvn_row_groups(256, cols) * (2 * cols + 1); }

// ---- developer knobs: presence means on, an empty string and "0" included ----------------------------------------
struct PostKnobs {
  bool plp_generic_tail;       // SNF_PLP_GENERIC_TAIL: plp_tail_kernel on every shape
  bool plp_small_tail;         // SNF_PLP_SMALL_TAIL: plp_tail_small_kernel where the exact kernel would run
  bool pitch_post_per_frame;   // SNF_PITCH_POST_PER_FRAME: the kernel of the long windows on any window - the two
                               // are compared bit for bit
};
inline PostKnobs post_knobs_parse(const char* generic_tail, const char* small_tail, const char* per_frame) {
  return {generic_tail != nullptr, small_tail != nullptr, per_frame != nullptr};
}
// The only reader of the environment on this path, on every call: the tests switch the knobs within one process.
inline PostKnobs post_knobs_from_env() {
  return post_knobs_parse(getenv("SNF_PLP_GENERIC_TAIL"), getenv("SNF_PLP_SMALL_TAIL"),
                          getenv("SNF_PITCH_POST_PER_FRAME"));
}

// ---- the ladders --------------------------------------------------------------------------------------------------
enum PostKernel {
  kPlpTailExact, kPlpTailSmall, kPlpTailGeneric, kDeltaFlat, kDeltaTiledFixed, kDeltaTiled, kDeltaPerElement,
  kPitchPostTiled, kPitchPostPerFrame, kCmvnStats, kCmvnStatsWide
};
// what Plan.kernel_name reports, by PostKernel: the only place these names are spelled
constexpr const char* kPostKernelNames[] = {
    "plp_tail_exact_kernel", "plp_tail_small_kernel", "plp_tail_kernel", "delta_flat_o2w2_kernel",
    "delta_tiled_fixed_kernel", "delta_tiled_kernel", "delta_kernel", "pitch_post_tiled_kernel", "pitch_post_kernel",
    "cmvn_stats_kernel", "cmvn_stats_wide_kernel"};
struct PostRoute {
  PostKernel kernel;
  int variant;          // template choice: REF of the exact PLP tail, D of the flat delta kernel, ORDER of the fixed
  int threads;          // per workgroup
  int rows;             // frames per workgroup or tile; row groups R of cmvn_stats_kernel; 0: no tiling by rows
  size_t lds_bytes;     // dynamic LDS
  bool build_records;   // launch_deltas: delta_tile_utt_kernel runs first if the caller's offsets table changed
  const char* refusal;  // nullptr, or why nothing runs
  const char* name() const { return kPostKernelNames[kernel]; }
};

inline PostRoute plp_tail_route(int num_bins, int lpc_order, int num_ceps, float compress_factor,
                                const PostKnobs& knobs) {
  if (num_bins > kMaxBins || lpc_order > kMaxLpc)
    return {kPlpTailGeneric, 0, 64, 64, 0, false, "PLP: num_bins > 126 or lpc_order > 63 not supported"};
  if (num_bins == 23 && lpc_order == 12 && num_ceps == 13 && !knobs.plp_generic_tail && !knobs.plp_small_tail)
    return {kPlpTailExact, compress_factor != 0.33333334f, 256, 256, 0, false, nullptr};
  if (num_bins <= 32 && lpc_order <= 16 && !knobs.plp_generic_tail)
    return {kPlpTailSmall, 0, 64, 64, 0, false, nullptr};
  return {kPlpTailGeneric, 0, 64, 64, 0, false, nullptr};
}

inline PostRoute delta_route(int order, int window, int n_scales, int cols, bool has_tile_info, bool aligned16) {
  // The tile records are rebuilt whenever the caller asks (its offsets table changed), on whichever path this call
  // then takes: the caller remembers the table, not the path, and a later call with 16-byte aligned pointers must
  // not find records of an older table.
  const bool records = order == 2 && window == 2 && has_tile_info && is_flat_cols(cols);
  if (records && aligned16) return {kDeltaFlat, cols, 256, flat_rows(cols), 0, true, nullptr};
  const int halo = order * window;
  const size_t lds = delta_tiled_lds_bytes(n_scales, halo, cols);
  // (the fixed kernel is chosen by the bytes WITH the scale table, which it does not carve: up to 64 bytes early,
  // no column count lies between the two bounds at its orders and window - kept as it was)
  if (lds <= kPostLdsLimit && cols <= 256 && window == 2 && (order == 2 || order == 1))
    return {kDeltaTiledFixed, order, 256, kDeltaRows, delta_tiled_fixed_lds_bytes(halo, cols), records, nullptr};
  if (lds <= kPostLdsLimit && cols <= 256) return {kDeltaTiled, 0, 256, kDeltaRows, lds, records, nullptr};
  return {kDeltaPerElement, 0, 256, 0, 0, records, nullptr};
}

inline PostRoute pitch_post_route(const snf_pitch_post_options& o, const PostKnobs& knobs) {
  const PitchPostHalos h = pitch_post_halos(o);
  const size_t lds = pitch_post_lds_bytes(h.left, h.right);
  if (lds <= kPostLdsLimit && !knobs.pitch_post_per_frame)
    return {kPitchPostTiled, 0, kPostRows, kPostRows, lds, false, nullptr};
  return {kPitchPostPerFrame, 0, 128, 128, 0, false, nullptr};
}

inline PostRoute cmvn_stats_route(int cols) {
  if (cols > 256) return {kCmvnStatsWide, 0, 256, 0, 0, false, nullptr};
  return {kCmvnStats, 0, 256, cmvn_row_groups(256, cols), cmvn_stats_lds_bytes(cols), false, nullptr};
}

}  // namespace snf

#endif  // SNF_POST_ROUTE_H_
