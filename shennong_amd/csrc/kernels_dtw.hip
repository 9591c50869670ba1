// Dynamic time warping between pairs of feature items (snf_dtw_pairs; an extension: the reference's users leave
// the GPU for this step, examples/features_abx/scripts/abx_score.sh:21).  For the items x [N, D] and y [M, D]:
//
//   d[i][j]  cosine:      acos(clamp(x_i . y_j / (|x_i| |y_j|), -1, 1)) / pi; 1 if one of the rows is zero, 0 if both
//            sqeuclidean: max(|x_i|^2 + |y_j|^2 - 2 x_i . y_j, 0)
//            symkl:       max(0.5 (h(x_i) + h(y_j) - x~_i . ln y~_j - ln x~_i . y~_j), 0), r~ = max(r, 2^-40)
//                         element-wise, h(r) = sum_k r~_k ln r~_k: 0.5 sum_k (x~ - y~)(ln x~ - ln y~)
//   C[0][0] = d[0][0], L[0][0] = 1;   C[i][j] = d[i][j] + C[p], L[i][j] = L[p] + 1
//   p = the predecessor of smallest C among (i-1, j-1), (i-1, j), (i, j-1), ties to the first of that order
//   cost = C[N-1][M-1], len = L[N-1][M-1]
//
// Pre-pass (dtw_rows_kernel): one thread per row of the block writes 1 / |row| (0 for a zero row) or |row|^2, the
// sum of squares being one fused chain over k ascending.  For symkl (dtw_log_rows_kernel, one thread per row too)
// it writes D + 1 floats per row: h(row), the same kind of chain over r~_k logf(r~_k), and behind it the row's
// ln r~_k, which the main kernel takes its second operands from.
//
// Main kernel (dtw_pairs_kernel): one wavefront (a workgroup of 64) owns a pair and walks the pairs of its class
// with the stride of the grid; the host has sorted every class by N M descending, so the strided walk hands
// every wave a like share.  Nothing in it loops on data: every bound is a frame count the host has checked.
//   * x is cut into strips of 64 rows, lane = row of the strip.  The columns come in tiles of 32: the 64 x 32
//     dot products of a tile are two v_mfma_f32_32x32x2_f32 chains over k (lane l supplies x[l & 31][k0 + (l >> 5)]
//     and y[l & 31][k0 + (l >> 5)] straight from memory, zeros beyond an odd D; rows and columns beyond the item
//     repeat its last one and are never read back).  The chain is bit for bit fmaf over k ascending from zero.
//     symkl runs the k loop twice into the same accumulators: floored rows of x against log rows of y, then log
//     rows of x against floored rows of y (the floor is an fmaxf on the raw load; the padded k stay zero in both).
//   * The epilogue turns the accumulators (row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31) into distances
//     and writes them to a ring of SLOTS tiles in LDS, row stride S = 32 SLOTS floats: a half-wave writes 32
//     consecutive words of one row.  The norms of the strip's rows sit in LDS (a broadcast read), the column's
//     norm in a register.
//   * The dynamic programme is skewed: at step t lane i does cell (i, t - i), so the tile T is made at step 32 T,
//     when lane 0 first needs it, and the lanes behind still read the tiles T - 1 and T - 2: SLOTS = 3 (one when
//     the pair has at most 32 columns).  The read of lane i is word i S + (t - i) mod S: bank (t - i) mod 32, a
//     bijection over each half-wave.
//   * Lane i gets (C, L) of cell (i - 1, t - i), which lane i - 1 made at step t - 1, through a DPP rotation; what it
//     got one step earlier is its diagonal neighbour; its own last cell is the left one.  C is float32, L int32.
//   * Strip seams: lane 63 leaves (C, L) per column in a seam row in LDS (8 bytes per column); lane 0 of the next
//     strip reads column t at step t, 63 steps before lane 63 overwrites it - in place.
// Three instances by the columns of a pair (LDS per wave): M <= 32 (8.5 KB), M <= 512 (28.3 KB), M <= 4096 (56.3 KB).
// The tile code (frame_distance, from_lane_below, tile_chain, make_tile) lies in dtw_tiles.h: the search kernel
// (kernels_dtw_search.hip) uses the same.  The body of the main kernel is pair_strips of dtw_strips.h, which the
// global lattice of snf_dtw_align (kernels_dtw_align.hip) shares: there it also records the decision of every cell.
#include "dtw_strips.h"

namespace snf {

int dtw_class_of(int32_t columns) { return columns <= 32 ? 0 : columns <= 512 ? 1 : 2; }

size_t dtw_aux_floats(int64_t n_rows, int dim, int metric) {
  return static_cast<size_t>(n_rows) * (metric == SNF_DTW_SYMKL ? static_cast<size_t>(dim) + 1 : 1);
}

namespace {

__global__ __launch_bounds__(256) void dtw_rows_kernel(const float* __restrict__ rows, const int dim,
                                                       const int64_t row_lo, const int64_t n, const int metric,
                                                       float* __restrict__ aux) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= n) return;
  const float* p = rows + (row_lo + r) * dim;
  float s = 0.0f;
  for (int k = 0; k < dim; ++k) s = fmaf(p[k], p[k], s);
  aux[r] = metric == SNF_DTW_COSINE ? (s > 0.0f ? 1.0f / sqrtf(s) : 0.0f) : s;
}

// symkl: dim + 1 floats of aux per row, r~ = max(row, floor): aux[r (dim + 1)] = h(row) = sum_k r~_k ln r~_k (one
// fused chain over k ascending, the accurate logf), and behind it the row's logarithms ln r~_k
__global__ __launch_bounds__(256) void dtw_log_rows_kernel(const float* __restrict__ rows, const int dim,
                                                           const int64_t row_lo, const int64_t n,
                                                           float* __restrict__ aux) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= n) return;
  const float* p = rows + (row_lo + r) * dim;
  float* q = aux + r * (dim + 1);
  float s = 0.0f;
  for (int k = 0; k < dim; ++k) {
    const float v = fmaxf(p[k], kSymklFloor);
    const float l = logf(v);
    q[1 + k] = l;
    s = fmaf(v, l, s);
  }
  q[0] = s;
}

template <int METRIC, int SLOTS, int SEAM>
__global__ __launch_bounds__(64) void dtw_pairs_kernel(const float* __restrict__ rows, const int dim,
                                                       const DtwItem* __restrict__ items,
                                                       const DtwPair* __restrict__ pairs, const int64_t n_pairs,
                                                       const float* __restrict__ aux, const int64_t row_lo,
                                                       float* __restrict__ cost, int32_t* __restrict__ len) {
  pair_strips<METRIC, SLOTS, SEAM>(rows, dim, items, pairs, n_pairs, aux, row_lo, cost, len, DtwNoRecords{});
}

template <int METRIC, int CLASS>
void launch_class(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs, int64_t n,
                  const float* d_aux, int64_t row_lo, int compute_units, float* cost, int32_t* len,
                  hipStream_t stream) {
  if (n <= 0) return;
  const int64_t waves = static_cast<int64_t>(compute_units) * kWavesPerCu[CLASS];
  const dim3 grid(static_cast<unsigned>(n < waves ? n : waves)), block(64);
  hipLaunchKernelGGL((dtw_pairs_kernel<METRIC, CLASS == 0 ? 1 : 3, kSeam[CLASS]>), grid, block, 0, stream, rows, dim,
                     d_items, d_pairs, n, d_aux, row_lo, cost, len);
}

template <int METRIC>
void launch_metric(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                   const int64_t* class_count, const float* d_aux, int64_t row_lo, int compute_units, float* cost,
                   int32_t* len, hipStream_t stream) {
  // the long pairs first: the short ones fill the compute units that they leave idle at their end
  const DtwPair* p1 = d_pairs + class_count[0];
  const DtwPair* p2 = p1 + class_count[1];
  launch_class<METRIC, 2>(rows, dim, d_items, p2, class_count[2], d_aux, row_lo, compute_units, cost, len, stream);
  launch_class<METRIC, 1>(rows, dim, d_items, p1, class_count[1], d_aux, row_lo, compute_units, cost, len, stream);
  launch_class<METRIC, 0>(rows, dim, d_items, d_pairs, class_count[0], d_aux, row_lo, compute_units, cost, len,
                          stream);
}

}  // namespace

int launch_dtw_rows(const float* rows, int dim, int64_t row_lo, int64_t row_hi, float* d_aux, int metric,
                    hipStream_t stream) {
  const int64_t n_rows = row_hi - row_lo;
  if (n_rows <= 0) return SNF_OK;
  const dim3 grid(static_cast<unsigned>((n_rows + 255) / 256)), block(256);
  if (metric == SNF_DTW_SYMKL)   // (dim + 1 floats per row: dtw_aux_floats)
    hipLaunchKernelGGL(dtw_log_rows_kernel, grid, block, 0, stream, rows, dim, row_lo, n_rows, d_aux);
  else
    hipLaunchKernelGGL(dtw_rows_kernel, grid, block, 0, stream, rows, dim, row_lo, n_rows, metric, d_aux);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_dtw_pairs(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                     const int64_t* class_count, int64_t row_lo, int64_t row_hi, float* d_aux, int metric,
                     int compute_units, float* cost, int32_t* len, hipStream_t stream) {
  if (row_hi - row_lo <= 0) return SNF_OK;
  if (const int rc = launch_dtw_rows(rows, dim, row_lo, row_hi, d_aux, metric, stream)) return rc;
  if (metric == SNF_DTW_COSINE)
    launch_metric<SNF_DTW_COSINE>(rows, dim, d_items, d_pairs, class_count, d_aux, row_lo, compute_units, cost, len,
                                  stream);
  else if (metric == SNF_DTW_SYMKL)
    launch_metric<SNF_DTW_SYMKL>(rows, dim, d_items, d_pairs, class_count, d_aux, row_lo, compute_units, cost, len,
                                 stream);
  else
    launch_metric<SNF_DTW_SQEUCLIDEAN>(rows, dim, d_items, d_pairs, class_count, d_aux, row_lo, compute_units, cost,
                                       len, stream);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
