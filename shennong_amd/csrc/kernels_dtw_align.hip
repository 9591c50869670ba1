// The warping paths of DTW pairs and of search hits (snf_dtw_align; an extension, as its siblings are: DESIGN 4.19).
//
// The lattice kernels are those of snf_dtw_pairs and snf_dtw_detect - pair_strips and search_pairs of dtw_strips.h,
// not copies - instantiated with a record policy: besides (C, L) every lane keeps the decision of its cell,
//   0: (i-1, j-1)   1: (i-1, j)   2: (i, j-1)   3: an origin (cell (0, 0); subsequence: the whole of row 0)
// which is the choice the lattice takes anyway (smallest C, ties to the first of that order, a strict <).
//
// Records.  At step t of the strip of rows s0 .. s0 + R - 1, lane l has made the decision of cell (s0 + l, t - l).
// Two ballots, one per bit, are the 64 decisions of the step; lane 0 stores them as one 16-byte record
//   rec[first(pair) + strip (63 + M) + t] = (bit 0 of lanes 0-31, of lanes 32-63, bit 1 of lanes 0-31, of lanes 32-63)
// (every strip but the last has 64 + M - 1 steps; a lane without a cell gives 0).  That is 16 (N + strips (M - 1))
// bytes a pair, no LDS and no barrier beyond what the lattice has, and one store a step.  The predecessors of a cell
// made at step t of a strip were made at step t - 1 (up: lane l - 1; left: lane l) or t - 2 (diagonal: lane l - 1) of
// the same strip; from lane 0 they lie in the strip above, lane 63, step j' + 63.  So the walk back reads the
// records of a strip as one descending stream.
//
// dtw_traceback_kernel: one wavefront per (pair, detection slot), behind the lattice on the same stream.  It takes
// the end cell and L from the result arrays that the lattice wrote (global: the end is (N-1, M-1)), keeps a window
// of 64 consecutive records of the strip in hand in registers - lane q holds record w0 + q, one coalesced 1 KB load
// when the walk leaves the window - and reads the decision of (lane l, step t) with v_readlane from lane t - w0: the
// walk is uniform over the wave, its state (i, j) lives in scalars, and no step waits for a load of its own.  The
// path is written forward: the walk fills cell L - 1 first; lane k & 63 keeps cell k, and every 64 cells the wave
// stores 64 consecutive words of path_x and of path_y.  The walk runs exactly L - 1 steps, L clamped to N + M - 1,
// the end to [0, M), i and j to >= 0: every bound is a frame count that the host has checked, every record index
// lies inside the pair's stretch and every store inside the slot's, whatever the data are (non-finite features give
// undefined paths and nothing worse).  A slot without a detection (L = 0) writes nothing.
#include "dtw_strips.h"

namespace snf {
namespace {

template <int METRIC, int SLOTS, int SEAM>
__global__ __launch_bounds__(64) void dtw_align_pairs_kernel(const float* __restrict__ rows, const int dim,
                                                             const DtwItem* __restrict__ items,
                                                             const DtwPair* __restrict__ pairs, const int64_t n_pairs,
                                                             const float* __restrict__ aux, const int64_t row_lo,
                                                             float* __restrict__ cost, int32_t* __restrict__ len,
                                                             const DtwRecords records) {
  pair_strips<METRIC, SLOTS, SEAM>(rows, dim, items, pairs, n_pairs, aux, row_lo, cost, len, records);
}

template <int METRIC, int SLOTS, int SEAM>
__global__ __launch_bounds__(64) void dtw_align_search_kernel(const float* __restrict__ rows, const int dim,
                                                              const DtwItem* __restrict__ items,
                                                              const DtwPair* __restrict__ pairs, const int64_t n_pairs,
                                                              const float* __restrict__ aux, const int64_t row_lo,
                                                              const int normalized, const DtwAlignOut out) {
  search_pairs<METRIC, SLOTS, SEAM>(rows, dim, items, pairs, n_pairs, aux, row_lo, normalized, out);
}

// `len` [P k], `end` [P k] or null (global: the end is M - 1) in the caller's pair order, as the lattice left them
__global__ __launch_bounds__(64) void dtw_traceback_kernel(const DtwItem* __restrict__ items,
                                                           const DtwPair* __restrict__ pairs, const int64_t n_pairs,
                                                           const int k, const int32_t* __restrict__ len,
                                                           const int32_t* __restrict__ end, const DtwRecords records,
                                                           const DtwPaths paths) {
  const int lane = threadIdx.x;
  const int64_t walks = n_pairs * k;
  for (int64_t w = blockIdx.x; w < walks; w += gridDim.x) {
    const int64_t p = w / k;
    const DtwPair pair = pairs[p];
    const int N = items[pair.x].frames, M = items[pair.y].frames;   // (the host has checked them)
    const int64_t slot = static_cast<int64_t>(pair.out) * k + (w - p * k);
    const int L = min(__builtin_amdgcn_readfirstlane(len[slot]), N + M - 1);
    if (L < 1) continue;   // (no detection in this slot: the same for the whole wave)
    const int e = end ? __builtin_amdgcn_readfirstlane(end[slot]) : M - 1;
    const int64_t first = paths.first[slot];
    const uint4* __restrict__ rec = records.rec + records.first[p];
    const int stride = 63 + M;   // the records of a whole strip
    int i = N - 1, j = min(max(e, 0), M - 1);
    uint4 win = make_uint4(0, 0, 0, 0);   // lane q: record w0 + q of strip ws
    int ws = -1, w0 = 0;
    int px = 0, py = 0;
    for (int cell = L - 1;; --cell) {
      if (lane == (cell & 63)) {
        px = i;
        py = j;
      }
      if ((cell & 63) == 0 && cell + lane < L) {   // the cells cell .. cell + 63 are made
        paths.x[first + cell + lane] = px;
        paths.y[first + cell + lane] = py;
      }
      if (cell == 0) break;
      const int strip = i >> 6, l = i & 63, t = j + l;
      if (strip != ws || t < w0) {   // (the same for the whole wave) t has left the window: the 64 records up to t
        ws = strip;
        w0 = max(t - 63, 0);
        const int have = min(64, N - 64 * strip) + M - 1;   // the steps of this strip: t < have
        win = w0 + lane < have ? rec[static_cast<int64_t>(strip) * stride + w0 + lane] : make_uint4(0, 0, 0, 0);
      }
      const int src = t - w0;   // in [0, 63]
      const unsigned b0 = l < 32 ? __builtin_amdgcn_readlane(win.x, src) : __builtin_amdgcn_readlane(win.y, src);
      const unsigned b1 = l < 32 ? __builtin_amdgcn_readlane(win.z, src) : __builtin_amdgcn_readlane(win.w, src);
      const int made = ((b0 >> (l & 31)) & 1) | (((b1 >> (l & 31)) & 1) << 1);
      // 0: both go back, 1: the row, 2: the column, 3: an origin (none; behind it there is no cell left to fill)
      i = max(i - (made == 0 || made == 1), 0);
      j = max(j - (made == 0 || made == 2), 0);
    }
  }
}

template <int METRIC, int CLASS>
void launch_class(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs, int64_t n,
                  const float* d_aux, int64_t row_lo, int subsequence, int normalized, int compute_units,
                  const DtwDetectOut& out, DtwRecords records, int64_t first_pair, hipStream_t stream) {
  if (n <= 0) return;
  const int64_t waves = static_cast<int64_t>(compute_units) * kWavesPerCu[CLASS];
  const dim3 grid(static_cast<unsigned>(n < waves ? n : waves)), block(64);
  records.first += first_pair;
  if (subsequence) {
    DtwAlignOut with;
    static_cast<DtwDetectOut&>(with) = out;
    with.records = records;
    hipLaunchKernelGGL((dtw_align_search_kernel<METRIC, CLASS == 0 ? 1 : 3, kSeam[CLASS]>), grid, block, 0, stream,
                       rows, dim, d_items, d_pairs + first_pair, n, d_aux, row_lo, normalized, with);
  } else {
    hipLaunchKernelGGL((dtw_align_pairs_kernel<METRIC, CLASS == 0 ? 1 : 3, kSeam[CLASS]>), grid, block, 0, stream,
                       rows, dim, d_items, d_pairs + first_pair, n, d_aux, row_lo, out.cost, out.len, records);
  }
}

template <int METRIC>
void launch_metric(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                   const int64_t* run_count, const float* d_aux, int64_t row_lo, int subsequence, int normalized,
                   int compute_units, const DtwDetectOut& out, const DtwRecords& records, hipStream_t stream) {
  // the long pairs first, as the siblings launch them
  launch_class<METRIC, 2>(rows, dim, d_items, d_pairs, run_count[2], d_aux, row_lo, subsequence, normalized,
                          compute_units, out, records, run_count[0] + run_count[1], stream);
  launch_class<METRIC, 1>(rows, dim, d_items, d_pairs, run_count[1], d_aux, row_lo, subsequence, normalized,
                          compute_units, out, records, run_count[0], stream);
  launch_class<METRIC, 0>(rows, dim, d_items, d_pairs, run_count[0], d_aux, row_lo, subsequence, normalized,
                          compute_units, out, records, 0, stream);
}

}  // namespace

int launch_dtw_align(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                     const int64_t* run_count, int64_t row_lo, const float* d_aux, int metric, int subsequence,
                     int normalized, int compute_units, const DtwDetectOut& out, const DtwRecords& records,
                     const DtwPaths& paths, hipStream_t stream) {
  const int64_t n = run_count[0] + run_count[1] + run_count[2];
  if (n <= 0) return SNF_OK;
  if (metric == SNF_DTW_COSINE)
    launch_metric<SNF_DTW_COSINE>(rows, dim, d_items, d_pairs, run_count, d_aux, row_lo, subsequence, normalized,
                                  compute_units, out, records, stream);
  else if (metric == SNF_DTW_SYMKL)
    launch_metric<SNF_DTW_SYMKL>(rows, dim, d_items, d_pairs, run_count, d_aux, row_lo, subsequence, normalized,
                                 compute_units, out, records, stream);
  else
    launch_metric<SNF_DTW_SQEUCLIDEAN>(rows, dim, d_items, d_pairs, run_count, d_aux, row_lo, subsequence, normalized,
                                       compute_units, out, records, stream);
  SNF_HIP_CHECK(hipGetLastError());
  // the walks: a wave is a few registers and no LDS, so a compute unit holds 32; they stride over the (pair, slot)s
  const int k = subsequence ? out.k : 1;
  const int64_t walks = n * k, waves = static_cast<int64_t>(compute_units) * 32;
  const dim3 grid(static_cast<unsigned>(walks < waves ? walks : waves)), block(64);
  hipLaunchKernelGGL(dtw_traceback_kernel, grid, block, 0, stream, d_items, d_pairs, n, k, out.len,
                     subsequence ? out.end : nullptr, records, paths);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
