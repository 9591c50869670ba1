// The body that the subsequence DTW kernels share (kernels_dtw_search.hip: dtw_search_kernel; kernels_dtw_detect.hip:
// dtw_detect_kernel), as one inline device function: the pairs of the block, the lattice of each - the strips of 64
// query rows on the lanes over the tiles of dtw_tiles.h, every cell of row 0 an origin, (C, W = L | B << 16) handed
// down by DPP, as described at the top of kernels_dtw_search.hip - and, once (C, W)[N - 1][j] of every end j < M lies
// in the seam row, the tail that `OUT` asks for: the one best end (DtwSearchOut) or up to k detections (DtwDetectOut,
// described at the top of kernels_dtw_detect.hip).  The search keeps its text, so that its kernels compile to what
// they were.  pair_strips is the body of dtw_pairs_kernel (kernels_dtw.hip) in the same way.  Both take a
// record policy: with DtwRecords (pair_strips) or DtwAlignOut (search_pairs: the detections' tail) the lattice also
// leaves the decision of every cell for the traceback of snf_dtw_align (kernels_dtw_align.hip); with the
// siblings' policies none of that is compiled.
#pragma once
#include <type_traits>

#include "dtw_tiles.h"

namespace snf {
namespace {

// The record of step t of a strip (snf_dtw_align; the layout: the top of kernels_dtw_align.hip): lane l brings `k`,
// the decision of its cell (s0 + l, t - l), 0 where it has none; the two ballots are the two bits of the 64 decisions,
// and lane 0 stores them as one 16-byte word
__device__ __forceinline__ void store_record(uint4* __restrict__ at, const int k, const int lane) {
  const unsigned long long b0 = __ballot(k & 1), b1 = __ballot(k & 2);
  if (lane == 0)
    *at = make_uint4(static_cast<unsigned>(b0), static_cast<unsigned>(b0 >> 32), static_cast<unsigned>(b1),
                     static_cast<unsigned>(b1 >> 32));
}

// The body of dtw_pairs_kernel (kernels_dtw.hip, which describes it) and, with REC = DtwRecords, of the global
// lattice of snf_dtw_align, which also leaves the decision of every cell: 0 (i-1, j-1), 1 (i-1, j), 2 (i, j-1),
// 3 the origin.  With DtwNoRecords nothing of that is compiled.
template <int METRIC, int SLOTS, int SEAM, class REC>
__device__ __forceinline__ void pair_strips(const float* __restrict__ rows, const int dim,
                                            const DtwItem* __restrict__ items, const DtwPair* __restrict__ pairs,
                                            const int64_t n_pairs, const float* __restrict__ aux,
                                            const int64_t row_lo, float* __restrict__ cost,
                                            int32_t* __restrict__ len, const REC records) {
  constexpr bool kRec = std::is_same<REC, DtwRecords>::value;
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
    // one float of aux per row; symkl: dim + 1, h(row) and behind it the row's logarithms (dtw_log_rows_kernel)
    const int64_t as = METRIC == SNF_DTW_SYMKL ? dim + 1 : 1;
    const float* ax = aux + (ix.row0 - row_lo) * as;
    const float* ay = aux + (iy.row0 - row_lo) * as;
    uint4* rec = nullptr;   // the record of step 0 of the strip in hand
    if constexpr (kRec) rec = records.rec + records.first[p];
    float C = 0.0f;
    int L = 0;
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
      float dgC = inf;   // (C, L) of cell (i - 1, j - 1): what came from lane i - 1 one step earlier
      int dgL = 0;
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
        int upL = from_lane_below(L);
        if (lane == 0) {
          upC = inf;
          upL = 0;
          if (s0 > 0 && t < M) {
            const float2 above = seam[t];
            upC = above.x;
            upL = __builtin_bit_cast(int, above.y);
          }
        }
        const int j = t - lane;
        int made = 0;   // (kRec: the decision of this lane's cell)
        if (j >= 0 && j < M && lane < R) {
          const float d = ring[lane * S + pos];
          float bestC = j > 0 ? dgC : inf;
          int bestL = dgL;
          if (upC < bestC) {
            bestC = upC;
            bestL = upL;
            if constexpr (kRec) made = 1;
          }
          if (j > 0 && C < bestC) {
            bestC = C;
            bestL = L;
            if constexpr (kRec) made = 2;
          }
          const bool origin = s0 + lane == 0 && j == 0;
          C = origin ? d : d + bestC;
          L = origin ? 1 : bestL + 1;
          if constexpr (kRec) made = origin ? 3 : made;
          dgC = upC;
          dgL = upL;
          if (more && lane == 63) seam[j] = make_float2(C, __builtin_bit_cast(float, L));
        }
        if constexpr (kRec) store_record(rec + t, made, lane);
        pos = pos + 1 == S ? 0 : pos + 1;
      }
      if constexpr (kRec) rec += steps;
      if (!more && lane == R - 1) {
        cost[pair.out] = C;
        len[pair.out] = L;
      }
    }
  }
}

template <int METRIC, int SLOTS, int SEAM, class OUT>
__device__ __forceinline__ void search_pairs(const float* __restrict__ rows, const int dim,
                                             const DtwItem* __restrict__ items, const DtwPair* __restrict__ pairs,
                                             const int64_t n_pairs, const float* __restrict__ aux,
                                             const int64_t row_lo, const int normalized, const OUT out) {
  constexpr bool kRec = std::is_same<OUT, DtwAlignOut>::value;   // (snf_dtw_align: the detections' tail, and records)
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
    uint4* rec = nullptr;   // (kRec: the record of step 0 of the strip in hand, as in pair_strips)
    if constexpr (kRec) rec = out.records.rec + out.records.first[p];
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
        int made = 0;   // (kRec: the decision of this lane's cell, 3 in the whole of row 0)
        if (j >= 0 && j < M && lane < R) {
          const float d = ring[lane * S + pos];
          float prevC = j > 0 ? dgC : inf;
          int prevW = dgW;
          if (upC < prevC) {
            prevC = upC;
            prevW = upW;
            if constexpr (kRec) made = 1;
          }
          if (j > 0 && C < prevC) {
            prevC = C;
            prevW = W;
            if constexpr (kRec) made = 2;
          }
          const bool origin = s0 + lane == 0;   // (the whole of row 0: the start is free)
          C = origin ? d : d + prevC;
          W = origin ? (1 | (j << 16)) : prevW + 1;
          if constexpr (kRec) made = origin ? 3 : made;
          dgC = upC;
          dgW = upW;
          // the seam of the next strip; in the last strip the ends, row N - 1 (lane 0 of a strip has read column j
          // at step j, and this write comes at step j + lane, behind that read in the order of the wave)
          if (lane == (more ? 63 : R - 1)) seam[j] = make_float2(C, __builtin_bit_cast(float, W));
        }
        if constexpr (kRec) store_record(rec + t, made, lane);
        pos = pos + 1 == S ? 0 : pos + 1;
      }
      if constexpr (kRec) rec += steps;
    }
    if constexpr (std::is_same<OUT, DtwDetectOut>::value || kRec) {
      // Up to k detections (the top of kernels_dtw_detect.hip).  Lane l owns the ends j = l, l + 64, ...: a round is
      // one pass over them - those that the detection of the round before overlaps die (L = 0 in their seam word),
      // the others are ranked as the search ranks them - and the search's butterfly.  The curves go out first.
      __syncthreads();
      if (curves) {
        for (int j = lane; j < M; j += 64) {
          const float2 e = seam[j];
          const int W = __builtin_bit_cast(int, e.y);
          out.curve_cost[curve + j] = e.x;
          out.curve_len[curve + j] = W & 0xffff;
          out.curve_start[curve + j] = static_cast<int>(static_cast<unsigned>(W) >> 16);
        }
      }
      const int64_t first = static_cast<int64_t>(pair.out) * out.k;
      int found = 0;
      int dead_lo = 0, dead_hi = -1;   // [start, end] of the detection of the round before: none yet
      for (int r = 0; r < out.k; ++r) {
        // (a lane without live ends holds (inf, INT_MAX), which wins against nothing)
        float bestS = inf, bestC = 0.0f;
        int bestW = 0, bestJ = 0x7fffffff;
        // (four ends in flight and no branch in a pass: with two or five waves on a compute unit's four SIMDs it
        // is bound by the latency of the read and of the division, not by their issue - DESIGN 4.18; every word is
        // written back, marked or as it was, and the quotient of a dead end, L = 0, is computed and not looked at)
#pragma unroll 4
        for (int j = lane; j < M; j += 64) {
          const float2 e = seam[j];
          const int W = __builtin_bit_cast(int, e.y), L = W & 0xffff;
          const bool dies = static_cast<int>(static_cast<unsigned>(W) >> 16) <= dead_hi && j >= dead_lo;
          seam[j].y = __builtin_bit_cast(float, dies ? W & ~0xffff : W);
          const float score = e.x / (normalized ? static_cast<float>(L) : 1.0f);   // (x / 1 is x)
          const bool take = L != 0 && !dies && (bestJ == 0x7fffffff || score < bestS);
          bestS = take ? score : bestS;
          bestC = take ? e.x : bestC;
          bestW = take ? W : bestW;
          bestJ = take ? j : bestJ;
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
        // lane 0's winner for the whole wave (the lanes agree unless a score is a NaN)
        const float score =
            __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, bestS)));
        const float cost =
            __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, bestC)));
        const int W = __builtin_amdgcn_readfirstlane(bestW), end = __builtin_amdgcn_readfirstlane(bestJ);
        if (end == 0x7fffffff || !(score <= out.max_score)) break;
        dead_lo = static_cast<int>(static_cast<unsigned>(W) >> 16);
        dead_hi = end;
        if (lane == 0) {
          out.cost[first + r] = cost;
          out.len[first + r] = W & 0xffff;
          out.start[first + r] = dead_lo;
          out.end[first + r] = end;
        }
        ++found;
      }
      if (lane == 0) out.count[pair.out] = found;
      for (int r = found + lane; r < out.k; r += 64) {
        out.cost[first + r] = inf;
        out.len[first + r] = 0;
        out.start[first + r] = -1;
        out.end[first + r] = -1;
      }
    } else {
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
}

}  // namespace
}  // namespace snf
