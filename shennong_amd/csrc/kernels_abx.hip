// ABX triplet counts per cell over a table of distances (snf_abx_cells; an extension: the reference's users leave
// the GPU for this step, examples/features_abx/scripts/abx_score.sh:22-23, and collapse the scores on the host,
// collapse_abx.py:35-42).  A cell {offA, offB, stride, nA, nB, nX, same} counts, over its triplets (a, b, x) -
// without those with a == x when `same` -, with dAX = v[offA + x stride + a] and dBX = v[offB + x stride + b]:
//
//   less = #{dAX < dBX}, equal = #{dAX == dBX}, bad = #{dAX or dBX not finite}; a bad triplet is in neither other
//
// v[i] = cost[i] / (float)len[i] (the correctly rounded float32 division) or cost[i].  Everything is a compare and
// an integer add: the counts are exact and do not depend on how the work is split.
//
// Two kernels, by the work nA nB nX of a cell (the host sorts the cells; thresholds in capi_abx.hip):
//   * abx_small_kernel: one LANE per cell, three plain loops on loads that the L1 serves.  A task holds hundreds
//     of thousands of cells of a few triplets: a wave each would spend its time on the cell record.
//   * abx_wave_kernel: one wavefront (a workgroup of 64) per unit - a whole cell, or a stretch [x0, x1) of a cell
//     that the host has split -, walking the units, sorted by work descending, with the stride of the grid.  For
//     a fixed x the B-row is staged in LDS in tiles of kAbxTile floats, a non-finite value as NaN (no compare
//     with it holds) and counted with a ballot; lanes go over a, 64 at a time, and every lane reads the tile
//     through float4 loads of one address for the whole wave (a broadcast: no bank conflict).  Per (a, b): two
//     compares and two adds with carry-in.  A lane whose own dAX is not finite compares NaN and adds the tile's
//     length to `bad`.  The lanes' totals are summed by xor-shuffles; lane 0 stores them (a whole cell) or adds
//     them with 64-bit vector atomics (a stretch; the host has zeroed the counts in stream order).
// Counters: per lane and tile pass `cl`, `ce` (uint32, at most kAbxTile = 1024) and the tile's `nbad` (uint32, at
// most 1024); per lane and unit `less`, `equal`, `bad` (uint64, at most the triplets of the cell, which the host
// keeps at or below 2^62); the wave's sum and the cell's total likewise.  The small kernel counts in uint64.
// Nothing loops on data: every bound is a field of a record that the host has checked.
#include <math.h>

#include "snf_internal.h"

namespace snf {

namespace {

constexpr int kWaveUnitsPerCu = 16;   // 4 KB of LDS and few registers per wave: four waves per SIMD

template <bool NORM>
__device__ __forceinline__ float value_at(const float* __restrict__ cost, const int32_t* __restrict__ len,
                                          const int64_t i) {
  if constexpr (NORM)
    return cost[i] / static_cast<float>(len[i]);
  else
    return cost[i];
}

__device__ __forceinline__ bool finite(float v) { return fabsf(v) < __builtin_inff(); }   // (false for NaN)

template <bool NORM>
__global__ __launch_bounds__(256) void abx_small_kernel(const float* __restrict__ cost,
                                                        const int32_t* __restrict__ len,
                                                        const AbxCell* __restrict__ cells,
                                                        const int32_t* __restrict__ small, const int64_t n_small,
                                                        unsigned long long* __restrict__ counts) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= n_small) return;
  const int32_t c = small[t];
  const AbxCell cell = cells[c];
  unsigned long long less = 0, equal = 0, bad = 0;
  for (int x = 0; x < cell.nX; ++x) {
    const int64_t rowA = cell.offA + x * cell.stride, rowB = cell.offB + x * cell.stride;
    for (int a = 0; a < cell.nA; ++a) {
      if (cell.same && a == x) continue;
      const float dA = value_at<NORM>(cost, len, rowA + a);
      const bool okA = finite(dA);
      for (int b = 0; b < cell.nB; ++b) {
        const float dB = value_at<NORM>(cost, len, rowB + b);
        const bool ok = okA && finite(dB);
        less += ok && dA < dB;
        equal += ok && dA == dB;
        bad += !ok;
      }
    }
  }
  counts[3 * static_cast<int64_t>(c)] = less;
  counts[3 * static_cast<int64_t>(c) + 1] = equal;
  counts[3 * static_cast<int64_t>(c) + 2] = bad;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

template <bool NORM>
__global__ __launch_bounds__(64) void abx_wave_kernel(const float* __restrict__ cost,
                                                      const int32_t* __restrict__ len,
                                                      const AbxCell* __restrict__ cells,
                                                      const AbxUnit* __restrict__ units, const int64_t n_units,
                                                      unsigned long long* __restrict__ counts) {
  __shared__ float4 tile4[kAbxTile / 4];
  float* tile = reinterpret_cast<float*>(tile4);
  const int lane = threadIdx.x;
  const float nan = __builtin_nanf("");
  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const AbxUnit unit = units[u];
    const AbxCell cell = cells[unit.cell];
    unsigned long long less = 0, equal = 0, bad = 0;
    for (int x = unit.x0; x < unit.x1; ++x) {
      const int64_t rowA = cell.offA + x * cell.stride, rowB = cell.offB + x * cell.stride;
      // (b0 and a0 in 64 bits: nA and nB reach 2^31 - 1, and a 32-bit counter would pass it on its last step)
      for (int64_t b0 = 0; b0 < cell.nB; b0 += kAbxTile) {
        const int nb = static_cast<int>(min(static_cast<int64_t>(kAbxTile), cell.nB - b0));
        __syncthreads();   // (the last tile's reads are done)
        uint32_t nbad = 0;
        // whole groups of 64: the words from nb to the next multiple of 64 hold NaN, which no compare counts
        for (int i = lane; i < ((nb + 63) & ~63); i += 64) {
          float v = nan;
          bool lost = false;
          if (i < nb) {
            v = value_at<NORM>(cost, len, rowB + b0 + i);
            lost = !finite(v);
            if (lost) v = nan;
          }
          tile[i] = v;
          nbad += static_cast<uint32_t>(__popcll(__ballot(lost)));
        }
        __syncthreads();
        const int quads = (nb + 3) >> 2;
        for (int64_t a0 = 0; a0 < cell.nA; a0 += 64) {
          const int64_t a = a0 + lane;
          const bool mine = a < cell.nA && !(cell.same && a == x);
          float dA = nan;
          bool okA = false;
          if (mine) {
            dA = value_at<NORM>(cost, len, rowA + a);
            okA = finite(dA);
            if (!okA) dA = nan;
          }
          uint32_t cl = 0, ce = 0;
          for (int q = 0; q < quads; ++q) {
            const float4 v = tile4[q];
            cl += dA < v.x;
            ce += dA == v.x;
            cl += dA < v.y;
            ce += dA == v.y;
            cl += dA < v.z;
            ce += dA == v.z;
            cl += dA < v.w;
            ce += dA == v.w;
          }
          if (mine) {
            less += cl;
            equal += ce;
            bad += okA ? nbad : static_cast<uint32_t>(nb);
          }
        }
      }
    }
    less = wave_sum(less);
    equal = wave_sum(equal);
    bad = wave_sum(bad);
    if (lane == 0) {
      unsigned long long* out = counts + 3 * static_cast<int64_t>(unit.cell);
      if (unit.split) {
        atomicAdd(out, less);
        atomicAdd(out + 1, equal);
        atomicAdd(out + 2, bad);
      } else {
        out[0] = less;
        out[1] = equal;
        out[2] = bad;
      }
    }
  }
}

template <bool NORM>
void launch(const float* cost, const int32_t* len, const AbxCell* d_cells, const int32_t* d_small, int64_t n_small,
            const AbxUnit* d_units, int64_t n_units, int compute_units, unsigned long long* d_counts,
            hipStream_t stream) {
  // the wave units first: the small cells fill the compute units that the last long units leave idle
  if (n_units > 0) {
    const int64_t waves = static_cast<int64_t>(compute_units) * kWaveUnitsPerCu;
    hipLaunchKernelGGL(abx_wave_kernel<NORM>, dim3(static_cast<unsigned>(n_units < waves ? n_units : waves)),
                       dim3(64), 0, stream, cost, len, d_cells, d_units, n_units, d_counts);
  }
  if (n_small > 0)
    hipLaunchKernelGGL(abx_small_kernel<NORM>, dim3(static_cast<unsigned>((n_small + 255) / 256)), dim3(256), 0,
                       stream, cost, len, d_cells, d_small, n_small, d_counts);
}

}  // namespace

int launch_abx_cells(const float* cost, const int32_t* len, const AbxCell* d_cells, const int32_t* d_small,
                     int64_t n_small, const AbxUnit* d_units, int64_t n_units, int compute_units,
                     unsigned long long* d_counts, hipStream_t stream) {
  if (len)
    launch<true>(cost, len, d_cells, d_small, n_small, d_units, n_units, compute_units, d_counts, stream);
  else
    launch<false>(cost, len, d_cells, d_small, n_small, d_units, n_units, compute_units, d_counts, stream);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
