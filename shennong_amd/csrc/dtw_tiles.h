// The device code that the DTW kernels share (kernels_dtw.hip: dtw_pairs_kernel; kernels_dtw_search.hip:
// dtw_search_kernel): the frame distance of a metric, the DPP hand-down from the lane below, and the tile of 64 x 32
// frame distances on v_mfma_f32_32x32x2_f32 with its epilogue into the LDS ring.  The layout of the lattice, the ring
// and the skew is described at the top of kernels_dtw.hip.
#pragma once
#include <math.h>

#include "snf_internal.h"

namespace snf {
namespace {

constexpr int kSeam[kDtwClasses] = {32, 512, kDtwMaxFrames};
constexpr int kWavesPerCu[kDtwClasses] = {16, 5, 2};   // what the LDS of a compute unit (160 KB) holds

constexpr float kSymklFloor = SNF_DTW_SYMKL_FLOOR;

// `dot`: the dot product; for symkl the sum of the two, x~_i . ln y~_j + ln x~_i . y~_j, with xa = h(x_i), ya = h(y_j)
template <int METRIC>
__device__ __forceinline__ float frame_distance(float dot, float xa, float ya) {
  if constexpr (METRIC == SNF_DTW_COSINE) {
    float c = dot * xa * ya;
    c = fminf(fmaxf(c, -1.0f), 1.0f);
    const float d = acosf(c) * 0.31830988618379067f;
    const bool xz = xa == 0.0f, yz = ya == 0.0f;
    return (xz || yz) ? ((xz && yz) ? 0.0f : 1.0f) : d;
  } else if constexpr (METRIC == SNF_DTW_SYMKL) {
    return fmaxf(0.5f * (xa + ya - dot), 0.0f);
  } else {
    return fmaxf(fmaf(-2.0f, dot, xa + ya), 0.0f);
  }
}

// (C, L) of lane - 1: a DPP move with wave_ror:1 (gfx9 keeps the whole-wave rotations: device_fft1024.h), not a
// trip through the LDS crossbar (ds_bpermute measured within 1 % of it: DESIGN 4.14).  Lane 0 gets lane 63's, which
// its caller replaces.
__device__ __forceinline__ int from_lane_below(int v) {
  return __builtin_amdgcn_update_dpp(0, v, 0x13C, 0xf, 0xf, false);
}

// symkl: one pass of the k loop of a tile into `acc0`, `acc1` (make_tile has the loop of the other metrics, which
// this one follows): the dot products of this lane's operand rows `x0`, `x1` (lattice rows l & 31 and 32 + (l & 31))
// and `yc` (column l & 31).  The k loop goes in groups of 4 MFMA steps (8 k) whose 12 operand loads are issued one
// group ahead, before the MFMAs of the group in hand: one wait per group instead of one per step.  FLOOR_A, FLOOR_B:
// the operand is max(load, floor).
template <bool FLOOR_A, bool FLOOR_B>
__device__ __forceinline__ void tile_chain(const float* __restrict__ x0, const float* __restrict__ x1,
                                           const float* __restrict__ yc, const int dim, const bool two, const int lh,
                                           f32x16& acc0, f32x16& acc1) {
  float a0[4], a1[4], b[4], na0[4], na1[4], nb[4];
  auto load = [&](int g, float* A0, float* A1, float* B) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = 8 * g + 2 * s + lh;
      const bool ok = k < dim;
      // (the padded k of an odd D stay zero in both operands)
      const float vb = ok ? yc[k] : 0.0f, v0 = ok ? x0[k] : 0.0f, v1 = (ok && two) ? x1[k] : 0.0f;
      B[s] = (FLOOR_B && ok) ? fmaxf(vb, kSymklFloor) : vb;
      A0[s] = (FLOOR_A && ok) ? fmaxf(v0, kSymklFloor) : v0;
      A1[s] = (FLOOR_A && ok && two) ? fmaxf(v1, kSymklFloor) : v1;
    }
  };
  const int groups = (dim + 7) >> 3;
  load(0, a0, a1, b);
  for (int g = 0; g < groups; ++g) {
    if (g + 1 < groups) load(g + 1, na0, na1, nb);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (8 * g + 2 * s < dim) {   // (the same for the whole wave; an odd D: the last step's second k is zero)
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b[s], acc0, 0, 0, 0);
        if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b[s], acc1, 0, 0, 0);
      }
    }
    if (g + 1 < groups) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        a0[s] = na0[s];
        a1[s] = na1[s];
        b[s] = nb[s];
      }
    }
  }
}

// The distances of the strip's 64 rows (32 unless `two`) against the 32 columns of a tile, into the ring at column
// offset `c_off`.  `x0`, `x1`, `yc`: this lane's operand rows (lattice rows l & 31 and 32 + (l & 31), column l & 31);
// `lx0`, `lx1`, `lyc` (symkl only): the logarithms of the same rows, from `aux`.
template <int METRIC, int S>
__device__ __forceinline__ void make_tile(const float* __restrict__ x0, const float* __restrict__ x1,
                                          const float* __restrict__ yc, const float* __restrict__ lx0,
                                          const float* __restrict__ lx1, const float* __restrict__ lyc, const int dim,
                                          const bool two, const int lh, const int li, const int c_off, const float ya,
                                          const float* xa, float* ring) {
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
  if constexpr (METRIC == SNF_DTW_SYMKL) {
    tile_chain<true, false>(x0, x1, lyc, dim, two, lh, acc0, acc1);    // x~ . ln y~
    tile_chain<false, true>(lx0, lx1, yc, dim, two, lh, acc0, acc1);   // ln x~ . y~
  } else {
    // (cosine and sqeuclidean keep the loop as it stood, not a tile_chain<false, false>: that way their instances
    // compile to the very instructions they had before symkl came: DESIGN 4.16)
    float a0[4], a1[4], b[4], na0[4], na1[4], nb[4];
    auto load = [&](int g, float* A0, float* A1, float* B) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 8 * g + 2 * s + lh;
        const bool ok = k < dim;
        B[s] = ok ? yc[k] : 0.0f;
        A0[s] = ok ? x0[k] : 0.0f;
        A1[s] = (ok && two) ? x1[k] : 0.0f;
      }
    };
    const int groups = (dim + 7) >> 3;
    load(0, a0, a1, b);
    for (int g = 0; g < groups; ++g) {
      if (g + 1 < groups) load(g + 1, na0, na1, nb);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (8 * g + 2 * s < dim) {   // (the same for the whole wave; an odd D: the last step's second k is zero)
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b[s], acc0, 0, 0, 0);
          if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b[s], acc1, 0, 0, 0);
        }
      }
      if (g + 1 < groups) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          a0[s] = na0[s];
          a1[s] = na1[s];
          b[s] = nb[s];
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (r & 3) + 8 * (r >> 2) + 4 * lh;
    ring[i * S + c_off + li] = frame_distance<METRIC>(acc0[r], xa[i], ya);
  }
  if (two) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      ring[i * S + c_off + li] = frame_distance<METRIC>(acc1[r], xa[i], ya);
    }
  }
}

}  // namespace
}  // namespace snf
