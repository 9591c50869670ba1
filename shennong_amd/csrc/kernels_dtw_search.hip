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
// row; the tile code is shared through dtw_tiles.h) with these differences:
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
#include "dtw_tiles.h"

namespace snf {
namespace {

template <int METRIC, int SLOTS, int SEAM>
__global__ __launch_bounds__(64) void dtw_search_kernel(const float* __restrict__ rows, const int dim,
                                                        const DtwItem* __restrict__ items,
                                                        const DtwPair* __restrict__ pairs, const int64_t n_pairs,
                                                        const float* __restrict__ aux, const int64_t row_lo,
                                                        const int normalized, const DtwSearchOut out) {
  constexpr int S = 32 * SLOTS;
  __shared__ float ring[64 * S];
  __shared__ float xa[64];
  __shared__ float2 seam[SEAM];
  const int lane = threadIdx.x, li = lane & 31, lh = lane >> 5;
  const float inf = __builtin_inff();
  for (int64_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
    const DtwPair pair = pairs[p];
    const DtwItem ix = items[pair.x], iy = items[pair.y];
    const int N = ix.frames, M = iy.frames;   // (1 <= N <= kDtwMaxFrames, 1 <= M <= SEAM: the host has checked)
    const float* X = rows + ix.row0 * dim;
    const float* Y = rows + iy.row0 * dim;
    const int64_t as = METRIC == SNF_DTW_SYMKL ? dim + 1 : 1;
    const float* ax = aux + (ix.row0 - row_lo) * as;
    const float* ay = aux + (iy.row0 - row_lo) * as;
    // (the host has checked that [curve, curve + M) lies in [0, 2^31) and overlaps no other pair's stretch)
    const bool curves = out.curve_first != nullptr;
    const int64_t curve = curves ? out.curve_first[pair.out] : 0;
    float C = 0.0f;
    int W = 0;   // L | B << 16
    for (int s0 = 0; s0 < N; s0 += 64) {
      const int R = min(64, N - s0);
      const bool more = s0 + 64 < N;
      __syncthreads();   // (the last strip's reads of xa are done)
      xa[lane] = ax[min(s0 + lane, N - 1) * as];
      __syncthreads();
      const float* x0 = X + static_cast<int64_t>(min(s0 + li, N - 1)) * dim;
      const float* x1 = X + static_cast<int64_t>(min(s0 + 32 + li, N - 1)) * dim;
      const float *lx0 = nullptr, *lx1 = nullptr;
      if constexpr (METRIC == SNF_DTW_SYMKL) {
        lx0 = ax + 1 + min(s0 + li, N - 1) * as;
        lx1 = ax + 1 + min(s0 + 32 + li, N - 1) * as;
      }
      float dgC = inf;   // (C, W) of cell (i - 1, j - 1): what came from lane i - 1 one step earlier
      int dgW = 0;
      int pos = -lane;   // (t - lane) mod S once t >= lane
      int slot = 0;      // (t / 32) mod SLOTS
      const int steps = R + M - 1;
      for (int t = 0; t < steps; ++t) {
        if ((t & 31) == 0 && t < M) {   // (the same for the whole wave)
          const int col = min(t + li, M - 1);
          const float* yc = Y + static_cast<int64_t>(col) * dim;
          const float ya = ay[col * as];
          const float* lyc = nullptr;
          if constexpr (METRIC == SNF_DTW_SYMKL) lyc = ay + 1 + col * as;
          make_tile<METRIC, S>(x0, x1, yc, lx0, lx1, lyc, dim, R > 32, lh, li, 32 * slot, ya, xa, ring);
          slot = slot + 1 == SLOTS ? 0 : slot + 1;
          __syncthreads();
        }
        float upC = __builtin_bit_cast(float, from_lane_below(__builtin_bit_cast(int, C)));
        int upW = from_lane_below(W);
        if (lane == 0) {
          upC = inf;
          upW = 0;
          if (s0 > 0 && t < M) {
            const float2 above = seam[t];
            upC = above.x;
            upW = __builtin_bit_cast(int, above.y);
          }
        }
        const int j = t - lane;
        if (j >= 0 && j < M && lane < R) {
          const float d = ring[lane * S + pos];
          float prevC = j > 0 ? dgC : inf;
          int prevW = dgW;
          if (upC < prevC) {
            prevC = upC;
            prevW = upW;
          }
          if (j > 0 && C < prevC) {
            prevC = C;
            prevW = W;
          }
          const bool origin = s0 + lane == 0;   // (the whole of row 0: the start is free)
          C = origin ? d : d + prevC;
          W = origin ? (1 | (j << 16)) : prevW + 1;
          dgC = upC;
          dgW = upW;
          // the seam of the next strip; in the last strip the ends, row N - 1 (lane 0 of a strip has read column j
          // at step j, and this write comes at step j + lane, behind that read in the order of the wave)
          if (lane == (more ? 63 : R - 1)) seam[j] = make_float2(C, __builtin_bit_cast(float, W));
        }
        pos = pos + 1 == S ? 0 : pos + 1;
      }
    }
    // The ends (C, W)[N - 1][j] lie in the seam row.  Lane l ranks the ends j = l, l + 64, ... in ascending order,
    // a strict <; then the wave keeps the smallest score and, of equal scores, the smallest j: the first arg-min.
    // (A lane without ends holds (inf, INT_MAX), which wins against nothing, lane 0 always has end 0: whatever the
    // scores are, the end that is written is a column of the pair.)
    __syncthreads();
    float bestS = inf, bestC = 0.0f;
    int bestW = 0, bestJ = 0x7fffffff;
    for (int j = lane; j < M; j += 64) {
      const float2 e = seam[j];
      const int W = __builtin_bit_cast(int, e.y), L = W & 0xffff;
      const float score = normalized ? e.x / static_cast<float>(L) : e.x;
      if (j == lane || score < bestS) {
        bestS = score;
        bestC = e.x;
        bestW = W;
        bestJ = j;
      }
      if (curves) {
        out.curve_cost[curve + j] = e.x;
        out.curve_len[curve + j] = L;
        out.curve_start[curve + j] = static_cast<int>(static_cast<unsigned>(W) >> 16);
      }
    }
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
      const float s = __shfl_xor(bestS, mask), c = __shfl_xor(bestC, mask);
      const int w = __shfl_xor(bestW, mask), j = __shfl_xor(bestJ, mask);
      if (s < bestS || (s == bestS && j < bestJ)) {
        bestS = s;
        bestC = c;
        bestW = w;
        bestJ = j;
      }
    }
    if (lane == 0) {
      out.cost[pair.out] = bestC;
      out.len[pair.out] = bestW & 0xffff;
      out.start[pair.out] = static_cast<int>(static_cast<unsigned>(bestW) >> 16);
      out.end[pair.out] = bestJ;
    }
  }
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
