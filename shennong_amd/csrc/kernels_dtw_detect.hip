// Several detections per (query, target) pair and the best few per query (snf_dtw_detect, snf_dtw_topk; extensions, as
// snf_dtw_search is).
//
// dtw_detect_kernel is dtw_search_kernel (kernels_dtw_search.hip) with another tail; both are search_pairs of
// dtw_strips.h, which holds the lattice once and the two tails.  With score[j] = C[N-1][j] / (float)L[N-1][j] if
// normalized, else C[N-1][j], and every end alive at first, up to k rounds:
//   e = the smallest alive j of minimal score (a strict < over ascending j: the arg-min of the search);
//   stop if not score[e] <= max_score; else (C, L, B)[N-1][e] and e are the detection of the next rank;
//   every end j' whose path interval [B[j'], j'] shares a frame with [B[e], e] dies: B[j'] <= e and j' >= B[e].
// The ends lie in the seam row in LDS and lane l owns the ends l, l + 64, ...: in a round it first kills those of its
// ends that the detection of the round before overlaps, then ranks what is left of them, and the butterfly of the
// search picks the wave's first arg-min.  A dead end is marked in its own seam word, L = 0 (a live end has L >= 1; C
// is left alone, it may hold an inf of its own), so a round is one pass over the lane's own words: no barrier, no LDS
// beyond the search kernel's, no scratch.  The winner is taken from lane 0 into scalars, which keeps the loop uniform
// whatever the scores are: every loop is bounded by k and M, which the host has checked, and non-finite features give
// undefined values and nothing worse.  Curves, when asked for, are stored before the first round marks anything.
//
// dtw_topk_kernel: one wavefront per query over the detections of its pairs where snf_dtw_detect left them in HBM;
// t rounds of arg-min over the key (score, pair, rank), each over the keys strictly greater than the one chosen in
// the round before, which needs no marking and is exact.  Only the first count[p] slots of a pair are candidates.
#include "dtw_strips.h"

namespace snf {
namespace {

template <int METRIC, int SLOTS, int SEAM>
__global__ __launch_bounds__(64) void dtw_detect_kernel(const float* __restrict__ rows, const int dim,
                                                        const DtwItem* __restrict__ items,
                                                        const DtwPair* __restrict__ pairs, const int64_t n_pairs,
                                                        const float* __restrict__ aux, const int64_t row_lo,
                                                        const int normalized, const DtwDetectOut out) {
  search_pairs<METRIC, SLOTS, SEAM>(rows, dim, items, pairs, n_pairs, aux, row_lo, normalized, out);
}

__global__ __launch_bounds__(64) void dtw_topk_kernel(const DtwTopkIn in, const int64_t n_queries, const int top_k,
                                                      const int normalized, const DtwTopkOut out) {
  const int lane = threadIdx.x;
  const float inf = __builtin_inff();
  for (int64_t q = blockIdx.x; q < n_queries; q += gridDim.x) {
    const int64_t g0 = in.group_first[q], g1 = in.group_first[q + 1];
    const int64_t first = q * top_k;
    float lastS = 0.0f;   // the key chosen in the round before
    int lastP = -1, lastR = -1;
    int found = 0;
    for (int i = 0; i < top_k; ++i) {
      float bestS = inf;
      int bestP = 0x7fffffff, bestR = 0x7fffffff;   // (no candidate: wins against nothing)
      for (int64_t g = g0 + lane; g < g1; g += 64) {
        const int pair = in.group_pair[g];   // (in [0, P): the host has checked)
        const int n = min(max(in.count[pair], 0), in.k);
        for (int r = 0; r < n; ++r) {
          const int64_t at = static_cast<int64_t>(pair) * in.k + r;
          const float cost = in.cost[at];
          const float s = normalized ? cost / static_cast<float>(in.len[at]) : cost;
          const bool behind = i == 0 || s > lastS || (s == lastS && (pair > lastP || (pair == lastP && r > lastR)));
          const bool better = bestP == 0x7fffffff || s < bestS ||
                              (s == bestS && (pair < bestP || (pair == bestP && r < bestR)));
          if (behind && better) {
            bestS = s;
            bestP = pair;
            bestR = r;
          }
        }
      }
#pragma unroll
      for (int mask = 1; mask < 64; mask <<= 1) {
        const float s = __shfl_xor(bestS, mask);
        const int pr = __shfl_xor(bestP, mask), r = __shfl_xor(bestR, mask);
        if (s < bestS || (s == bestS && (pr < bestP || (pr == bestP && r < bestR)))) {
          bestS = s;
          bestP = pr;
          bestR = r;
        }
      }
      lastS = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, bestS)));
      lastP = __builtin_amdgcn_readfirstlane(bestP);
      lastR = __builtin_amdgcn_readfirstlane(bestR);
      if (lastP == 0x7fffffff) break;
      if (lane == 0) {
        const int64_t at = static_cast<int64_t>(lastP) * in.k + lastR;
        out.pair[first + i] = lastP;
        out.rank[first + i] = lastR;
        out.cost[first + i] = in.cost[at];
        out.len[first + i] = in.len[at];
        out.start[first + i] = in.start[at];
        out.end[first + i] = in.end[at];
      }
      ++found;
    }
    if (lane == 0) out.count[q] = found;
    for (int i = found + lane; i < top_k; i += 64) {
      out.pair[first + i] = -1;
      out.rank[first + i] = -1;
      out.cost[first + i] = inf;
      out.len[first + i] = 0;
      out.start[first + i] = -1;
      out.end[first + i] = -1;
    }
  }
}

template <int METRIC, int CLASS>
void launch_class(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs, int64_t n,
                  const float* d_aux, int64_t row_lo, int normalized, int compute_units, const DtwDetectOut& out,
                  hipStream_t stream) {
  if (n <= 0) return;
  const int64_t waves = static_cast<int64_t>(compute_units) * kWavesPerCu[CLASS];
  const dim3 grid(static_cast<unsigned>(n < waves ? n : waves)), block(64);
  hipLaunchKernelGGL((dtw_detect_kernel<METRIC, CLASS == 0 ? 1 : 3, kSeam[CLASS]>), grid, block, 0, stream, rows, dim,
                     d_items, d_pairs, n, d_aux, row_lo, normalized, out);
}

template <int METRIC>
void launch_metric(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                   const int64_t* class_count, const float* d_aux, int64_t row_lo, int normalized, int compute_units,
                   const DtwDetectOut& out, hipStream_t stream) {
  // the long targets first, as the search launches them
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

int launch_dtw_detect(const float* rows, int dim, const DtwItem* d_items, const DtwPair* d_pairs,
                      const int64_t* class_count, int64_t row_lo, int64_t row_hi, float* d_aux, int metric,
                      int normalized, int compute_units, const DtwDetectOut& out, hipStream_t stream) {
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

int launch_dtw_topk(const DtwTopkIn& in, int64_t n_queries, int top_k, int normalized, const DtwTopkOut& out,
                    hipStream_t stream) {
  if (n_queries <= 0) return SNF_OK;
  const int64_t most = int64_t(1) << 20;   // (the kernel strides over the queries)
  const dim3 grid(static_cast<unsigned>(n_queries < most ? n_queries : most)), block(64);
  hipLaunchKernelGGL(dtw_topk_kernel, grid, block, 0, stream, in, n_queries, top_k, normalized, out);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
