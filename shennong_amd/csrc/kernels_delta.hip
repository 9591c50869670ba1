// Delta / delta-delta features (reference postprocessor/delta.py:129-131 -> [KALDI-UPSTREAM] feature-functions.cc
// DeltaFeatures): the per-element kernel, the two tiled kernels, the flat kernel of the reference's defaults with
// the kernel that builds its tile records, and launch_deltas.  Which one runs: delta_route, post_route.h, where
// the tile heights and the LDS layouts of the tiled kernels are stated too.
//
// Pure HBM-streaming kernels over [frames, cols] float32 matrices: each row is read once (plus an edge-clamped
// halo that stays in L2) and each output row written once.
#include "post_route.h"
#include "snf_internal.h"
#include "utt_search.h"

namespace snf {

// ------------------------------------------------------------------------------------------------
// Deltas: out[:, i*D:(i+1)*D] = sum_j scales_i[j] * in[clamp(t + j)]; one thread per (row, column).
// ------------------------------------------------------------------------------------------------
__global__ void delta_kernel(const DeltaParams p, const float* __restrict__ in, const int D,
                             const int64_t* __restrict__ frame_offsets, const int64_t n_utts,
                             const int64_t total_frames, float* __restrict__ out) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= total_frames * D) return;
  const int64_t g = idx / D;
  const int c = static_cast<int>(idx - g * D);
  const int64_t u = find_utt(frame_offsets, n_utts, g);
  const int64_t f0 = frame_offsets[u], f1 = frame_offsets[u + 1];
  const int OD = D * (p.order + 1);
  const float* __restrict__ sc = p.scales;
  for (int i = 0; i <= p.order; ++i) {
    const int dim = p.dims[i], max_off = (dim - 1) / 2;
    float acc = 0.0f;
    for (int j = -max_off; j <= max_off; ++j) {
      int64_t t = g + j;
      t = t < f0 ? f0 : (t >= f1 ? f1 - 1 : t);
      const float s = sc[j + max_off];
      if (s != 0.0f) acc += s * in[t * D + c];
    }
    out[g * OD + static_cast<int64_t>(i) * D + c] = acc;
    sc += dim;
  }
}

// Tiled variant: a workgroup stages kDeltaRows + 2*halo input rows in LDS once (each HBM row is read
// ~1.1x instead of 9x through the caches) and writes its output rows fully coalesced.  The edge clamp
// is per utterance; a clamped neighbour is never farther than the unclamped one, so it is in the tile.
__global__ __launch_bounds__(256) void delta_tiled_kernel(
    const DeltaParams p, const float* __restrict__ in, const int D, const int halo,
    const int64_t* __restrict__ frame_offsets, const int64_t n_utts, const int64_t total_frames,
    float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* row_lo = reinterpret_cast<int*>(smem);   // [kDeltaRows] first row of the utterance (tile-relative)
  int* row_hi = row_lo + kDeltaRows;            // [kDeltaRows] last row of the utterance (tile-relative)
  float* scales = reinterpret_cast<float*>(row_hi + kDeltaRows);  // [n_scales]
  float* tile = scales + delta_scales_floats(p.n_scales);         // [(kDeltaRows + 2 halo), D]
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * kDeltaRows;
  const int64_t t0 = g0 - halo;
  const int tile_rows = delta_tile_rows(halo);
  const int64_t first = t0 * D, limit = total_frames * D;
  for (int i = threadIdx.x; i < tile_rows * D; i += blockDim.x) {
    const int64_t a = first + i;
    tile[i] = (a >= 0 && a < limit) ? in[a] : 0.0f;
  }
  for (int i = threadIdx.x; i < p.n_scales; i += blockDim.x) scales[i] = p.scales[i];
  if (threadIdx.x < kDeltaRows) {
    const int64_t g = g0 + threadIdx.x;
    if (g < total_frames) {
      const int64_t u = find_utt(frame_offsets, n_utts, g);
      const int64_t lo = frame_offsets[u] - t0, hi = frame_offsets[u + 1] - 1 - t0;
      row_lo[threadIdx.x] = lo < 0 ? 0 : static_cast<int>(lo);  // rows outside the tile are never
      row_hi[threadIdx.x] = hi > tile_rows - 1 ? tile_rows - 1 : static_cast<int>(hi);  // reached
    }
  }
  __syncthreads();
  const int OD = D * (p.order + 1);
  const int rows_here = static_cast<int>(total_frames - g0 < kDeltaRows ? total_frames - g0 : kDeltaRows);
  // element e = (row r, column c); advanced without divisions
  int r = threadIdx.x / D, c = threadIdx.x - r * D;
  const int dr = blockDim.x / D, dc = blockDim.x - dr * D;
  float* __restrict__ obase = out + g0 * OD;
  for (; r < rows_here; r += dr, c += dc) {
    if (c >= D) { c -= D; ++r; if (r >= rows_here) break; }
    const int lo = row_lo[r], hi = row_hi[r], centre = r + halo;
    const float* __restrict__ sc = scales;
    float* __restrict__ orow = obase + static_cast<int64_t>(r) * OD + c;
    for (int i = 0; i <= p.order; ++i) {
      const int max_off = i * p.window;
      float acc = 0.0f;
      for (int j = -max_off; j <= max_off; ++j) {
        int t = centre + j;
        t = t < lo ? lo : (t > hi ? hi : t);
        const float s = sc[j + max_off];
        if (s != 0.0f) acc += s * tile[t * D + c];
      }
      orow[i * D] = acc;
      sc += 2 * max_off + 1;
    }
  }
}

// The same tile with the order and window known at compile time (the reference's defaults, order 2 /
// window 2, and order 1): the 2*halo+1 clamped neighbours of an element are read from LDS ONCE for all
// the orders, the composite scales sit in scalar registers, the tap loops are unrolled.  Same products
// in the same order as the generic kernel above.
template <int ORDER, int WINDOW>
__global__ __launch_bounds__(256) void delta_tiled_fixed_kernel(
    const DeltaParams p, const float* __restrict__ in, const int D,
    const int64_t* __restrict__ frame_offsets, const int64_t n_utts, const int64_t total_frames,
    float* __restrict__ out) {
  constexpr int kHalo = ORDER * WINDOW;
  constexpr int kTaps = 2 * kHalo + 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* row_lo = reinterpret_cast<int*>(smem);
  int* row_hi = row_lo + kDeltaRows;
  float* tile = reinterpret_cast<float*>(row_hi + kDeltaRows);  // [(kDeltaRows + 2 kHalo), D]
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * kDeltaRows;
  const int64_t t0 = g0 - kHalo;
  constexpr int tile_rows = delta_tile_rows(kHalo);
  const int64_t first = t0 * D, limit = total_frames * D;
  for (int i = threadIdx.x; i < tile_rows * D; i += blockDim.x) {
    const int64_t a = first + i;
    tile[i] = (a >= 0 && a < limit) ? in[a] : 0.0f;
  }
  if (threadIdx.x < kDeltaRows) {
    const int64_t g = g0 + threadIdx.x;
    if (g < total_frames) {
      const int64_t u = find_utt(frame_offsets, n_utts, g);
      const int64_t lo = frame_offsets[u] - t0, hi = frame_offsets[u + 1] - 1 - t0;
      row_lo[threadIdx.x] = lo < 0 ? 0 : static_cast<int>(lo);
      row_hi[threadIdx.x] = hi > tile_rows - 1 ? tile_rows - 1 : static_cast<int>(hi);
    }
  }
  // composite scales of every order, concatenated like DeltaParams::scales (uniform: scalar loads)
  constexpr int kScales = (ORDER + 1) * (ORDER * WINDOW + 1);  // sum of 2 i WINDOW + 1, i <= ORDER
  float sc[kScales];
#pragma unroll
  for (int i = 0; i < kScales; ++i) sc[i] = p.scales[i];
  __syncthreads();
  const int OD = D * (ORDER + 1);
  const int rows_here = static_cast<int>(total_frames - g0 < kDeltaRows ? total_frames - g0 : kDeltaRows);
  int r = threadIdx.x / D, c = threadIdx.x - r * D;
  const int dr = blockDim.x / D, dc = blockDim.x - dr * D;
  float* __restrict__ obase = out + g0 * OD;
  for (; r < rows_here; r += dr, c += dc) {
    if (c >= D) { c -= D; ++r; if (r >= rows_here) break; }
    const int lo = row_lo[r], hi = row_hi[r], centre = r + kHalo;
    float x[kTaps];
#pragma unroll
    for (int j = 0; j < kTaps; ++j) {
      int t = centre + j - kHalo;
      t = t < lo ? lo : (t > hi ? hi : t);
      x[j] = tile[t * D + c];
    }
    float* __restrict__ orow = obase + static_cast<int64_t>(r) * OD + c;
    int soff = 0;
#pragma unroll
    for (int i = 0; i <= ORDER; ++i) {
      const int max_off = i * WINDOW;
      float acc = 0.0f;
#pragma unroll
      for (int j = -max_off; j <= max_off; ++j) {
        const float s = sc[soff + j + max_off];
        if (s != 0.0f) acc += s * x[j + kHalo];
      }
      orow[i * D] = acc;
      soff += 2 * max_off + 1;
    }
  }
}

// The reference's defaults (order 2, window 2) as a flat stream: the [T, D] input and the [T, 3 D] output
// are both contiguous.  A tile of rows is staged with 16-byte loads; thread i computes the elements
// (row, column) i, i + 256, ... for all three orders from ONE read of the 9 clamped neighbours
// (consecutive lanes -> consecutive columns: conflict-free; the division by D is by a compile-time
// constant) into an LDS image of the output block, which is then copied out as dwordx4: loads and
// stores are fully coalesced 16-byte accesses (the per-(row, column) form above writes 4-byte elements in runs of D).  The utterance of a
// tile's first row comes from a table built by one thread per tile (a binary search of dependent loads
// at the head of every workgroup costs more than its arithmetic); rows walk forward from it.  Same
// products in the same order as the kernels above.
typedef float f4v __attribute__((ext_vector_type(4)));
// one 32-byte record per tile: the utterance of its first row and the frame offsets of that utterance and
// the next two, so that a workgroup learns the utterance boundaries of its rows from ONE load (a chain of
// dependent loads per row used to be most of a workgroup's life)
__global__ void delta_tile_utt_kernel(const int64_t* __restrict__ frame_offsets, int64_t n_utts,
                                      int64_t total_frames, int rows_per_tile,
                                      int64_t* __restrict__ tile_info) {
  const int64_t tile = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t g = tile * rows_per_tile;
  if (g >= total_frames) return;
  const int64_t u = find_utt(frame_offsets, n_utts, g);
  int64_t* __restrict__ rec = tile_info + 4 * tile;
  rec[0] = u;
  rec[1] = frame_offsets[u];
  rec[2] = frame_offsets[u + 1];
  rec[3] = frame_offsets[u + 2 <= n_utts ? u + 2 : n_utts];
}

template <int D>
__global__ __launch_bounds__(256) void delta_flat_o2w2_kernel(
    const DeltaParams p, const float* __restrict__ in, const int64_t* __restrict__ frame_offsets,
    const int64_t* __restrict__ tile_info, const int64_t n_utts, const int64_t total_frames,
    float* __restrict__ out) {
  constexpr int kRows = flat_rows(D);
  constexpr int kHalo = 4, OD = 3 * D, kTileRows = kRows + 2 * kHalo;
  constexpr int kTileFloats = (kTileRows * D + 3) & ~3;
  __shared__ __attribute__((aligned(16))) float tile[kTileFloats + 4];
  __shared__ __attribute__((aligned(16))) float image[kRows * OD];
  __shared__ int row_lo[kRows], row_hi[kRows];
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * kRows;
  const int64_t t0 = g0 - kHalo;
  const int64_t first = t0 * D, limit = total_frames * D;
  // the tile starts at float `first` of the input, which is 16-byte aligned only for some tiles: stage
  // from the aligned float4 at or below it (`skew` floats earlier)
  const int skew = static_cast<int>(((first % 4) + 4) % 4);
  const int64_t base = first - skew;
  // the tile is requested first (registers), the utterance bookkeeping below overlaps its latency
  constexpr int kStage = (kTileFloats / 4 + 1 + 255) / 256;
  float4 staged[kStage];
#pragma unroll
  for (int k = 0; k < kStage; ++k) {
    const int i = threadIdx.x + 256 * k;
    const int64_t a = base + 4 * static_cast<int64_t>(i);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i * 4 < kTileFloats + 4) {
      if (a >= 0 && a + 3 < limit) {
        v = *reinterpret_cast<const float4*>(in + a);
      } else {
        if (a >= 0 && a < limit) v.x = in[a];
        if (a + 1 >= 0 && a + 1 < limit) v.y = in[a + 1];
        if (a + 2 >= 0 && a + 2 < limit) v.z = in[a + 2];
        if (a + 3 >= 0 && a + 3 < limit) v.w = in[a + 3];
      }
    }
    staged[k] = v;
  }
  const int rows_here = static_cast<int>(total_frames - g0 < kRows ? total_frames - g0 : kRows);
  bool interior = rows_here == kRows;
  {
    const int64_t* __restrict__ rec = tile_info + 4 * static_cast<int64_t>(blockIdx.x);
    const int64_t u0 = rec[0], o0 = rec[1], o1 = rec[2], o2 = rec[3];
    for (int r = threadIdx.x; r < kRows; r += blockDim.x) {
      const int64_t g = g0 + r;
      if (g < total_frames) {
        int64_t lo_f = o0, hi_f = o1;          // [first, end) frames of the row's utterance
        if (g >= o1) {
          lo_f = o1;
          hi_f = o2;
          if (g >= o2) {                       // more than two boundaries inside the tile (rare)
            int64_t u = u0 + 2;
            while (frame_offsets[u + 1] <= g) ++u;
            lo_f = frame_offsets[u];
            hi_f = frame_offsets[u + 1];
          }
        }
        const int64_t lo = lo_f - t0, hi = hi_f - 1 - t0;
        row_lo[r] = lo < 0 ? 0 : static_cast<int>(lo);
        row_hi[r] = hi > kTileRows - 1 ? kTileRows - 1 : static_cast<int>(hi);
        interior = interior && lo <= r && hi >= r + 2 * kHalo;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kStage; ++k) {
    const int i = threadIdx.x + 256 * k;
    if (i * 4 < kTileFloats + 4) reinterpret_cast<float4*>(tile)[i] = staged[k];
  }
  float sc[15];  // scales of the three orders, concatenated like DeltaParams::scales: 1 + 5 + 9
#pragma unroll
  for (int i = 0; i < 15; ++i) sc[i] = p.scales[i];
  // interior tile: every row and its +-4 neighbours lie inside one utterance (3 tiles out of 4 on 3 s
  // utterances) -> no clamping, and a thread walks down one column of a strip of rows with the 9-row
  // window in registers: one LDS read per element instead of nine
  interior = __syncthreads_and(interior);
  const int n_out = rows_here * OD;
  const float* __restrict__ tl = tile + skew;
  if (interior) {
    constexpr int kStrips = 256 / D, kStripRows = (kRows + kStrips - 1) / kStrips;
    const int c = threadIdx.x % D, strip = threadIdx.x / D;
    if (strip < kStrips) {
      const int r0 = strip * kStripRows;
      float v[kStripRows + 2 * kHalo];
#pragma unroll
      for (int i = 0; i < kStripRows + 2 * kHalo; ++i)
        v[i] = r0 + i < kTileRows ? tl[(r0 + i) * D + c] : 0.0f;
#pragma unroll
      for (int rr = 0; rr < kStripRows; ++rr) {
        if (r0 + rr < kRows) {
          float* __restrict__ orow = image + (r0 + rr) * OD + c;
          int soff = 0;
#pragma unroll
          for (int i = 0; i <= 2; ++i) {
            const int max_off = 2 * i;
            float acc = 0.0f;
#pragma unroll
            for (int j = -max_off; j <= max_off; ++j) {
              const float w = sc[soff + j + max_off];
              if (w != 0.0f) acc += w * v[rr + j + kHalo];
            }
            orow[i * D] = acc;
            soff += 2 * max_off + 1;
          }
        }
      }
    }
  }
  // element (row r, column c): its 9 clamped neighbours are read ONCE for the three orders (every lane
  // runs the same taps: no divergence), the three results go to the output image
  for (int idx = threadIdx.x; !interior && idx < rows_here * D; idx += blockDim.x) {
    const int r = idx / D, c = idx - r * D;
    const int lo = row_lo[r], hi = row_hi[r], centre = r + kHalo;
    float x[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      int t = centre + j - kHalo;
      t = t < lo ? lo : (t > hi ? hi : t);
      x[j] = tl[t * D + c];
    }
    float* __restrict__ orow = image + r * OD + c;
    int soff = 0;
#pragma unroll
    for (int i = 0; i <= 2; ++i) {
      const int max_off = 2 * i;
      float acc = 0.0f;
#pragma unroll
      for (int j = -max_off; j <= max_off; ++j) {
        const float w = sc[soff + j + max_off];
        if (w != 0.0f) acc += w * x[j + kHalo];
      }
      orow[i * D] = acc;
      soff += 2 * max_off + 1;
    }
  }
  __syncthreads();
  float* __restrict__ obase = out + g0 * OD;   // (g0 * OD * 4 bytes is a multiple of 16: kRows % 4 == 0)
  for (int e0 = 4 * threadIdx.x; e0 < n_out; e0 += 4 * blockDim.x) {
    if (e0 + 3 < n_out) {
      __builtin_nontemporal_store(*reinterpret_cast<const f4v*>(image + e0), reinterpret_cast<f4v*>(obase + e0));
    } else {
      for (int k = 0; k < 4 && e0 + k < n_out; ++k) obase[e0 + k] = image[e0 + k];
    }
  }
}

int launch_deltas(const DeltaParams& p, const float* in, int in_cols, const int64_t* frame_offsets,
                  int64_t n_utts, int64_t total_frames, float* out, int64_t* tile_info, bool build_info,
                  hipStream_t stream, const char** launched) {
  if (launched) *launched = nullptr;
  const int64_t total = total_frames * in_cols;
  if (total <= 0) return SNF_OK;
  const bool aligned16 = (reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const PostRoute r = delta_route(p.order, p.window, p.n_scales, in_cols, tile_info != nullptr, aligned16);
  if (r.build_records && build_info) {
    const int rows = flat_rows(in_cols);
    const unsigned tiles = static_cast<unsigned>((total_frames + rows - 1) / rows);
    hipLaunchKernelGGL(delta_tile_utt_kernel, dim3((tiles + 255) / 256), dim3(256), 0, stream, frame_offsets,
                       n_utts, total_frames, rows, tile_info);
    SNF_HIP_CHECK(hipGetLastError());
  }
  // a workgroup per tile of r.rows frames; the per-element kernel: a thread per (row, column)
  const dim3 grid(static_cast<unsigned>(r.rows ? (total_frames + r.rows - 1) / r.rows
                                               : (total + r.threads - 1) / r.threads));
  const dim3 block(r.threads);
  switch (r.kernel) {
    case kDeltaFlat: {
      const auto flat = r.variant == 13   ? delta_flat_o2w2_kernel<13>
                        : r.variant == 23 ? delta_flat_o2w2_kernel<23>
                        : r.variant == 40 ? delta_flat_o2w2_kernel<40>
                                          : delta_flat_o2w2_kernel<43>;
      hipLaunchKernelGGL(flat, grid, block, 0, stream, p, in, frame_offsets, tile_info, n_utts, total_frames, out);
      break;
    }
    case kDeltaTiledFixed: {
      const auto fixed = r.variant == 2 ? delta_tiled_fixed_kernel<2, 2> : delta_tiled_fixed_kernel<1, 2>;
      hipLaunchKernelGGL(fixed, grid, block, r.lds_bytes, stream, p, in, in_cols, frame_offsets, n_utts,
                         total_frames, out);
      break;
    }
    case kDeltaTiled:
      hipLaunchKernelGGL(delta_tiled_kernel, grid, block, r.lds_bytes, stream, p, in, in_cols, p.order * p.window,
                         frame_offsets, n_utts, total_frames, out);
      break;
    default:
      hipLaunchKernelGGL(delta_kernel, grid, block, 0, stream, p, in, in_cols, frame_offsets, n_utts, total_frames,
                         out);
  }
  SNF_HIP_CHECK(hipGetLastError());
  if (launched) *launched = r.name();
  return SNF_OK;
}

}  // namespace snf
