// Query-by-example search by subsequence DTW (snf_dtw_search; an extension, as snf_dtw_pairs is): where does the
// query x [N, D] occur in the target y [M, D]?  With d[i][j] the frame distance of kernels_dtw.hip:
//
//   C[0][j] = d[0][j], L[0][j] = 1, B[0][j] = j for every j                                  (free start)
//   i >= 1: C[i][j] = d[i][j] + C[p], L[i][j] = L[p] + 1, B[i][j] = B[p]
//   p = the predecessor of smallest C among (i-1, j-1), (i-1, j), (i, j-1) that exist, ties to the first of that order
//   score[j] = C[N-1][j] / (float)L[N-1][j] if normalized, else C[N-1][j]                    (free end)
//   end = the smallest j of minimal score (a strict < over j ascending); start = B[N-1][end], cost, len of that cell
//
// dtw_search_kernel is dtw_pairs_kernel (kernels_dtw.hip: the strips of 64 query rows on the lanes, the target in
// tiles of 32 columns on v_mfma_f32_32x32x2_f32, the LDS ring, the skewed wavefront, the DPP hand-down, the seam
// row; the tile code is shared through dtw_tiles.h; the body of the kernel below is search_pairs of dtw_strips.h, which
// dtw_detect_kernel shares) with these differences:
//   * every cell of lattice row 0 is an origin;
//   * the start column B travels with (C, L), packed with L in one word W = L | B << 16 (L <= N + M - 1 <= 8191,
//     B <= 4095): the hand-down stays at two DPP moves per step, the seam at 8 bytes per column, the LDS of every
//     class what it is for the pairs; W + 1 is L + 1;
//   * in the last strip the lane of row N - 1 leaves (C, W) of every end j in the seam row, which no later strip
//     needs.  Behind the lattice the 64 lanes share the ends: each takes the float32 quotient and keeps its running
//     best over ascending j, a butterfly of 6 exchanges keeps the smallest score and of equal ones the smallest j -
//     the first arg-min, as one lane going through the ends in order would find it - and lane 0 writes cost, len,
//     start, end of the pair once.  When the caller asked for curves the same loop stores (C, L, B) of every end at
//     the pair's stretch of the three curve arrays, 64 consecutive words at a time.  (A first version ranked the ends
//     in the step loop, in the one lane of row N - 1: the division and three single-lane stores on every step of the
//     last strip, which the whole wave issues - measured 1.16 to 1.28 times the pair kernel: DESIGN 4.17.)
// Nothing loops or addresses on data: every bound and every index is a frame count that the host has checked or the
// pair's own offset, so non-finite features give undefined values and nothing worse.  The class of a pair is that
// of its target's columns: M <= 32, <= 512, <= 4096, the LDS per wave as in kernels_dtw.hip.
#include "dtw_strips.h"

namespace snf {
namespace {

template <int METRIC, int SLOTS, int SEAM>
__global__ __launch_bounds__(64) void dtw_search_kernel(const float* __restrict__ rows, const int dim,
                                                        const DtwItem* __restrict__ items,
                                                        const DtwPair* __restrict__ pairs, const int64_t n_pairs,
                                                        const float* __restrict__ aux, const int64_t row_lo,
                                                        const int normalized, const DtwSearchOut out) {
  search_pairs<METRIC, SLOTS, SEAM>(rows, dim, items, pairs, n_pairs, aux, row_lo, normalized, out);
}

template <int METRIC, int CLASS>
void launch_class(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs, int64_t n,
                  const float* d_aux, int64_t row_lo, int normalized, int compute_units, const DtwSearchOut& out,
                  hipStream_t stream) {
  if (n <= 0) return;
  const int64_t waves = static_cast<int64_t>(compute_units) * kWavesPerCu[CLASS];
  const dim3 grid(static_cast<unsigned>(n < waves ? n : waves)), block(64);
  hipLaunchKernelGGL((dtw_search_kernel<METRIC, CLASS == 0 ? 1 : 3, kSeam[CLASS]>), grid, block, 0, stream, rows, dim,
                     d_items, d_pairs, n, d_aux, row_lo, normalized, out);
}

template <int METRIC>
void launch_metric(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                   const int64_t* class_count, const float* d_aux, int64_t row_lo, int normalized, int compute_units,
                   const DtwSearchOut& out, hipStream_t stream) {
  // the long targets first: the short ones fill the compute units that they leave idle at their end
  const DtwPair* p1 = d_pairs + class_count[0];
  const DtwPair* p2 = p1 + class_count[1];
  launch_class<METRIC, 2>(rows, dim, d_items, p2, class_count[2], d_aux, row_lo, normalized, compute_units, out,
                          stream);
  launch_class<METRIC, 1>(rows, dim, d_items, p1, class_count[1], d_aux, row_lo, normalized, compute_units, out,
                          stream);
  launch_class<METRIC, 0>(rows, dim, d_items, d_pairs, class_count[0], d_aux, row_lo, normalized, compute_units, out,
                          stream);
}

}  // namespace

int launch_dtw_search(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                      const int64_t* class_count, int64_t row_lo, int64_t row_hi, float* d_aux, int metric,
                      int normalized, int compute_units, const DtwSearchOut& out, hipStream_t stream) {
  if (row_hi - row_lo <= 0) return SNF_OK;
  if (const int rc = launch_dtw_rows(rows, dim, row_lo, row_hi, d_aux, metric, stream)) return rc;
  if (metric == SNF_DTW_COSINE)
    launch_metric<SNF_DTW_COSINE>(rows, dim, d_items, d_pairs, class_count, d_aux, row_lo, normalized, compute_units,
                                  out, stream);
  else if (metric == SNF_DTW_SYMKL)
    launch_metric<SNF_DTW_SYMKL>(rows, dim, d_items, d_pairs, class_count, d_aux, row_lo, normalized, compute_units,
                                 out, stream);
  else
    launch_metric<SNF_DTW_SQEUCLIDEAN>(rows, dim, d_items, d_pairs, class_count, d_aux, row_lo, normalized,
                                       compute_units, out, stream);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
