// Framed one-hot labels of time alignments (reference processor/onehot.py:215-267 over alignment.py:321-337).
//
// An alignment is a run of segments (offset in seconds, token id); sample i sits at t(i) = i / rate + onset0,
// float64, one IEEE division then one addition, and carries the first token whose offset is greater than t(i).
// The label of a frame is the token all its samples carry or, in a frame with several, the token with the
// largest window weight: per token the float32 sum of the window coefficients of its samples, accumulated in
// sample order from zero (one accumulator per token, however often it comes back within the frame); an exact tie
// goes to the token that appears first.  Three launches per batch, whatever the number of alignments:
//
//  1. onehot_bounds_kernel, one lane per segment: the first sample at or past the segment's offset.  t(i) does
//     not decrease with i, so that sample is found from ceil((offset - onset0) * rate) by stepping while the
//     exact comparison asks for it, at most kSteps either way (the guess is off by rounding alone: a fraction of
//     a sample as long as a sample is many ulps of t, which holds far beyond any speech corpus) - no walk over
//     the samples.  The last segment of an alignment ends at the sample count: a last sample that rounding
//     puts at or past the final offset takes the last token.
//  2. onehot_winner_kernel, one lane per frame, the window in LDS.  A binary search over the segment ends finds
//     the segment of the frame's first sample; when that segment reaches the end of the frame the lane is done
//     (three frames in four of forced-aligned speech).  A mixed frame runs the sums: for every token in order
//     of first appearance, its samples in order - every coefficient is added once per frame, the lanes of a wave
//     with a mixed frame walk over L coefficients at the pace of the slowest.  Sums are sequential float32 adds:
//     a frame split at the centre of a symmetric window compares an ascending with a descending sum of the
//     same numbers, the last bit decides, and a tree or a wider accumulator would decide otherwise.
//  3. onehot_rows_kernel, one lane per 16 bytes of the dense uint8 rows: the rows of an alignment are one
//     run of bytes that starts on a 16-byte boundary, a lane forms 16 of them in registers - zeros and the set
//     byte alike - and stores them once (global_store_dwordx4, a wave covers 1 KiB of consecutive addresses).
//
// Nothing depends on where an alignment sits in the batch: its rows are the same bits alone and in any batch.
#include "snf_internal.h"

namespace snf {
namespace {

constexpr int kThreads = 256;
constexpr int kSteps = 2;

// the last a in [0, n) with table[a] <= x, for a table of n + 1 non-decreasing entries with table[0] <= x <
// table[n] (entries that repeat - empty alignments - are stepped over)
__device__ inline int64_t owner_of(const int64_t* table, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (table[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ inline double sample_time(int64_t i, double rate, double onset0) { return double(i) / rate + onset0; }

__global__ void __launch_bounds__(kThreads)
onehot_bounds_kernel(const int64_t* __restrict__ seg_off, int64_t n_ali, int64_t n_seg,
                     const double* __restrict__ onset0, const double* __restrict__ offsets,
                     const int64_t* __restrict__ nsamples, double rate, int64_t* __restrict__ ends) {
  const int64_t k = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (k >= n_seg) return;
  const int64_t a = owner_of(seg_off, n_ali, k);
  const int64_t n = nsamples[a];
  if (k == seg_off[a + 1] - 1) {
    ends[k] = n;
    return;
  }
  const double offset = offsets[k], first = onset0[a];
  double guess = ceil((offset - first) * rate);
  guess = guess > 0.0 ? guess : 0.0;
  int64_t g = guess < double(n) ? int64_t(guess) : n;
  for (int step = 0; step < kSteps; ++step)
    if (g > 0 && sample_time(g - 1, rate, first) >= offset) --g;
  for (int step = 0; step < kSteps; ++step)
    if (g < n && sample_time(g, rate, first) < offset) ++g;
  ends[k] = g;
}

// samples [lo, hi) of the frame [s, e) that segment q holds (q0: the segment of the frame's first sample);
// empty when hi <= lo.  Whatever `ends` holds, s <= lo and hi <= e: the window is read inside [0, L).
__device__ inline void run_of(const int64_t* ends, int64_t q0, int64_t q, int64_t s, int64_t e, int64_t* lo,
                              int64_t* hi) {
  const int64_t begin = q == q0 ? s : ends[q - 1], end = ends[q];
  *lo = begin > s ? begin : s;
  *hi = end < e ? end : e;
}

__global__ void __launch_bounds__(kThreads)
onehot_winner_kernel(const int64_t* __restrict__ frame_off, int64_t n_ali, int64_t total_frames,
                     const int64_t* __restrict__ seg_off, const int64_t* __restrict__ ends,
                     const int32_t* __restrict__ ids, const float* __restrict__ window, int L, int shift,
                     int32_t* __restrict__ winner) {
  extern __shared__ float win[];
  for (int j = threadIdx.x; j < L; j += kThreads) win[j] = window[j];
  __syncthreads();
  const int64_t f = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= total_frames) return;
  const int64_t a = owner_of(frame_off, n_ali, f);
  const int64_t s = (f - frame_off[a]) * shift, e = s + L;
  const int64_t last = seg_off[a + 1] - 1;   // ends[last] is the sample count: >= e
  int64_t lo = seg_off[a], hi = last;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (ends[mid] > s) hi = mid; else lo = mid + 1;
  }
  const int64_t q0 = lo;
  int32_t best_id = ids[q0];
  if (q0 < last && ends[q0] < e) {
    int64_t q1 = q0 + 1;   // the segment of the frame's last sample
    while (q1 < last && ends[q1] < e) ++q1;
    bool have = false;
    float best = 0.0f;
    for (int64_t r = q0; r <= q1; ++r) {
      int64_t a0, a1;
      run_of(ends, q0, r, s, e, &a0, &a1);
      if (a1 <= a0) continue;
      const int32_t token = ids[r];
      bool seen = false;
      for (int64_t q = q0; q < r && !seen; ++q) {
        if (ids[q] != token) continue;
        run_of(ends, q0, q, s, e, &a0, &a1);
        seen = a1 > a0;
      }
      if (seen) continue;
      float weight = 0.0f;
      for (int64_t q = r; q <= q1; ++q) {
        if (ids[q] != token) continue;
        run_of(ends, q0, q, s, e, &a0, &a1);
        for (int64_t i = a0; i < a1; ++i) weight += win[i - s];
      }
      if (!have || weight > best) {
        have = true;
        best = weight;
        best_id = token;
      }
    }
  }
  winner[f] = best_id;
}

__global__ void __launch_bounds__(kThreads)
onehot_rows_kernel(const int64_t* __restrict__ row_off, int64_t n_ali, int64_t total_chunks,
                   const int64_t* __restrict__ frame_off, const int32_t* __restrict__ ntokens,
                   const int32_t* __restrict__ winner, uint4* __restrict__ out) {
  const int64_t c = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (c >= total_chunks) return;
  const int64_t a = owner_of(row_off, n_ali, c * 16);
  const int64_t local = c * 16 - row_off[a];
  const int64_t frames = frame_off[a + 1] - frame_off[a];
  const int32_t width = ntokens[a];
  uint32_t word[4] = {0u, 0u, 0u, 0u};
  if (width > 0) {
    const int32_t* mine = winner + frame_off[a];
    int64_t row = local / width;
    int32_t col = int32_t(local - row * width);
    int32_t hot = row < frames ? mine[row] : -1;   // (past the last row: padding up to the 16-byte boundary)
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      if (col == hot) word[b >> 2] |= 1u << (8 * (b & 3));
      if (++col == width) {
        col = 0;
        ++row;
        hot = row < frames ? mine[row] : -1;
      }
    }
  }
  out[c] = make_uint4(word[0], word[1], word[2], word[3]);
}

}  // namespace

int launch_framed_onehot(const OneHotBatch& b, hipStream_t stream) {
  const auto blocks = [](int64_t n) { return dim3(static_cast<unsigned>((n + kThreads - 1) / kThreads)); };
  if (b.total_frames <= 0) return SNF_OK;
  hipLaunchKernelGGL(onehot_bounds_kernel, blocks(b.n_seg), dim3(kThreads), 0, stream, b.seg_off, b.n_ali, b.n_seg,
                     b.onset0, b.offsets, b.nsamples, b.rate, b.ends);
  hipLaunchKernelGGL(onehot_winner_kernel, blocks(b.total_frames), dim3(kThreads), sizeof(float) * b.frame_length,
                     stream, b.frame_off, b.n_ali, b.total_frames, b.seg_off, b.ends, b.ids, b.window,
                     b.frame_length, b.frame_shift, b.winner);
  const int64_t chunks = b.total_bytes / 16;
  if (chunks > 0)
    hipLaunchKernelGGL(onehot_rows_kernel, blocks(chunks), dim3(kThreads), 0, stream, b.row_off, b.n_ali, chunks,
                       b.frame_off, b.ntokens, b.winner, reinterpret_cast<uint4*>(b.rows));
  if (hipGetLastError() != hipSuccess) return set_error(SNF_E_HIP, "one-hot kernel launch failed");
  return SNF_OK;
}

}  // namespace snf
