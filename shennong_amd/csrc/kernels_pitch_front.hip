// Kaldi pitch tracker on gfx950: the reference reaches it through
// kaldi.feat.pitch.compute_kaldi_pitch (shennong/processor/pitch_kaldi.py:296-299).
//
// Restates [KALDI-UPSTREAM] pitch-functions.cc (OnlinePitchFeatureImpl::AcceptWaveform /
// InputFinished / RecomputeBacktraces, ComputeCorrelation, ComputeNccf, ComputeLocalCost,
// PitchFrameInfo::ComputeBacktraces) and resample.cc (LinearResample, ArbitraryResample) for the
// offline single-chunk call the reference makes (frames_per_chunk = 0).
//
// Four stages per batch (launch_pitch, kernels_pitch_viterbi.hip); this file holds the first three and their
// launcher, pitch_wave.h the cross-lane helpers every stage shares:
//   1. pitch_resample_kernel one thread per downsampled sample: 16 kHz -> 4 kHz windowed-sinc FIR (a
//                             workgroup filters 4 chunks of 256 samples, the next chunk's input in flight)
//   2. pitch_stats_kernel     one workgroup per utterance: signal sum / sum of squares, from which
//                             one thread derives the NCCF ballasts of the utterance
//   3. pitch_nccf_kernel      FRAME-parallel (nothing in it depends on the previous frame): wave64 =
//                             4 frames x 16 lanes; lane l correlates the lags 5 l .. 5 l + 4 against
//                             the frame's window in LDS (5 x 5 register blocks), NCCF with and
//                             without ballast, then the NCCF is resampled to the log-spaced lags of the
//                             Viterbi states on the matrix pipe (v_mfma_f32_4x4x1: 4 states x 4 frames
//                             per block, one exact fused multiply-add per tap) -> [frames, states] in HBM
//   4. pitch_viterbi_kernel   the only sequential part: one wavefront per utterance walks the frames,
//                             local cost from the row of 3, exact argmin of the transition cost with
//                             the monotone divide-and-conquer search, backpointers to HBM, traceback.
//                             (kernels_pitch_viterbi.hip; small batches: pitch_viterbi_team_kernel there, a team
//                             of waves per utterance; large ones: pitch_viterbi_flat_kernel, a lane per candidate,
//                             kernels_pitch_flat.hip; pitch_route.h has the ladder)
//
// Arithmetic contract.  Kaldi hands the sums of this algorithm to BLAS, whose summation order depends
// on the library build; the CPU oracle (oracle/kaldi_oracle.c, chain_dot / tree16) fixes ONE order and
// these kernels implement exactly that order, so the tracker agrees with the oracle bit for bit and the
// Viterbi paths are identical (a one-ulp difference in a cost flips near-ties in unvoiced regions):
//   - FIR taps, lag correlations, sinc resampling: s = fmaf(a[i], b[i], s), i ascending, from 0 (the
//     matrix-pipe form of the sinc resampling is the same chain: K = 1 per instruction, lags ascending,
//     zero weights outside a state's taps);
//   - frame mean / frame energy / norm average: lane l of 16 sums its elements l, l + 16, ...
//     ascending, the 16 partial sums are added as a balanced tree of neighbours (DPP quad_perm xor 1,
//     xor 2, row_half_mirror, row_mirror: every lane ends with the same bits);
//   - divisions and square roots are IEEE correctly rounded; nothing else is fused: the three kernels_pitch_*
//     files are compiled with -ffp-contract=off and every fused multiply-add is written as one.
#include <cstdio>
#include <type_traits>

#include "device_fft.h"
#include "pitch_wave.h"

namespace snf {

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

}  // namespace

// ---- 1. LinearResample ---------------------------------------------------------------------------
// A workgroup computes 256 consecutive output samples of one utterance: the input span they touch
// (256 x in_unit / out_unit samples + one filter length) is staged into LDS as floats with coalesced
// loads - zeros outside the utterance: fmaf(w, 0, s) = s exactly, the accumulator never being -0 - and
// every thread then runs Kaldi's tap loop (one sequential fmaf chain) from LDS.  The per-output gather
// of 2-byte samples from global memory that this replaces took 0.68 ms per 192 M input samples.
constexpr int kRsChunks = 4;   // 256-output chunks per workgroup of the resampler
constexpr int kRsMaxPer = 6;   // staged samples per thread and chunk that travel through registers

__global__ __launch_bounds__(256) void pitch_resample_kernel(const PitchDevTables t, const PitchBatch b,
                                                             float* __restrict__ down) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xs = reinterpret_cast<float*>(smem);
  // blockIdx.y = utterance (no per-thread search), blockIdx.x = kRsChunks consecutive 256-sample chunks of
  // its output.  A workgroup that handles one chunk is a chain of four dependent memory round trips
  // (offsets, samples, taps, store: 4 us for 250 instructions per wave, 0.375 ms per 192 M samples);
  // here the offsets are read once and the samples of chunk c + 1 are in flight, in registers, while
  // chunk c is filtered.
  const int64_t u = blockIdx.y;
  const int64_t d0 = b.down_offsets[u], nd = b.down_offsets[u + 1] - d0;
  const int64_t k_begin = static_cast<int64_t>(blockIdx.x) * (256 * kRsChunks);
  if (k_begin >= nd) return;
  const int64_t s0 = b.sample_offsets[u], n = b.sample_offsets[u + 1] - s0;
  const int16_t* __restrict__ w = b.wave + s0;
  // (32-bit index arithmetic: a 64-bit division costs ~100 instructions, three of them per output was
  // more than the filter itself; an utterance has fewer than 2^31 samples)
  const int out_unit = t.rs_out_unit, in_unit = t.rs_in_unit;
  const int tid = static_cast<int>(threadIdx.x);
  auto first_of = [&](int k) -> int64_t {
    const int unit = k / out_unit;
    return t.rs_first[k - unit * out_unit] + static_cast<int64_t>(unit) * in_unit;
  };
  // input span of the chunk that starts at output k0: [base, base + span)
  auto geometry = [&](int64_t k0, int64_t* base, int* span) {
    const int k_first = static_cast<int>(k0);
    const int k_last = k0 + 255 < nd - 1 ? k_first + 255 : static_cast<int>(nd) - 1;
    *base = first_of(k_first);                               // (first inputs are non-decreasing in k)
    *span = static_cast<int>(first_of(k_last) + t.rs_max_taps - *base);
  };
  auto sample = [&](int64_t j) -> float { return (j >= 0 && j < n) ? static_cast<float>(w[j]) : 0.0f; };
  // samples in flight: raw 16-bit values from clamped (always valid) addresses, no branch and no
  // conversion until they are staged - a conversion here would wait for every load on the spot
  auto fetch = [&](int64_t j) -> int {
    const int64_t jc = j < 0 ? 0 : (j < n ? j : n - 1);
    return w[jc];
  };
  int pre[kRsMaxPer];
  int64_t base;
  int span;
  geometry(k_begin, &base, &span);
#pragma unroll
  for (int q = 0; q < kRsMaxPer; ++q) pre[q] = fetch(base + tid + 256 * q);
  for (int c = 0; c < kRsChunks; ++c) {
    const int64_t k0 = k_begin + 256 * c;
    if (k0 >= nd) break;
    // stage the chunk: zeros outside the utterance (fmaf(w, 0, s) = s exactly, s never being -0)
#pragma unroll
    for (int q = 0; q < kRsMaxPer; ++q) {
      const int64_t j = base + tid + 256 * q;
      if (tid + 256 * q < span) xs[tid + 256 * q] = (j >= 0 && j < n) ? static_cast<float>(pre[q]) : 0.0f;
    }
    for (int i = tid + 256 * kRsMaxPer; i < span; i += 256) xs[i] = sample(base + i);  // (rate ratios above 5)
    __syncthreads();
    const int64_t base_cur = base;
    if (c + 1 < kRsChunks && k0 + 256 < nd) {
      geometry(k0 + 256, &base, &span);
#pragma unroll
      for (int q = 0; q < kRsMaxPer; ++q) pre[q] = fetch(base + tid + 256 * q);
    }
    const int k = static_cast<int>(k0) + tid;
    if (k < nd) {
      float s = 0.0f;
      if (out_unit == 1) {
        // one filter for every output (integer rate ratios, e.g. 16 kHz -> 4 kHz): uniform weights.  (A
        // de-interleaved LDS layout that makes the tap reads conflict-free was measured: slower, 0.63 ms
        // against 0.375 - the strided staging costs more than the conflicts)
        const float* __restrict__ x = xs + (t.rs_first[0] + static_cast<int64_t>(k) * in_unit - base_cur);
        const int ntaps = t.rs_ntaps[0];
        for (int i = 0; i < ntaps; ++i) s = __builtin_fmaf(t.rs_w[i], x[i], s);
      } else {
        const int unit = k / out_unit, wrapped = k - unit * out_unit;
        const float* __restrict__ x =
            xs + (t.rs_first[wrapped] + static_cast<int64_t>(unit) * in_unit - base_cur);
        const float* __restrict__ wt = t.rs_w + wrapped * t.rs_max_taps;
        const int ntaps = t.rs_ntaps[wrapped];
        for (int i = 0; i < ntaps; ++i) s = __builtin_fmaf(wt[i], x[i], s);
      }
      down[d0 + k] = s;
    }
    __syncthreads();  // (the next chunk overwrites the staged span)
  }
}

// ---- 2. signal statistics for the NCCF ballast -----------------------------------------------------
// Kaldi accumulates the float BLAS dot / sum of each chunk into doubles; phase 1 = what the resampler
// emitted before the flush.  ub[u] = {ballast of the frames of phase 1, of phase 2, the two "old"
// ballasts RecomputeBacktraces derives from the float mean squares, the new ballast, 1 if
// RecomputeBacktraces has to run (utterance shorter than recompute_frame whose phase-1 mean square is
// more than 1 % away from the final one)}
__global__ void pitch_stats_kernel(const PitchDevTables t, const PitchBatch b,
                                   const float* __restrict__ down, float* __restrict__ ub) {
  const int64_t u = blockIdx.x;
  const int64_t d0 = b.down_offsets[u], nd = b.down_offsets[u + 1] - d0, nd1 = b.down_phase1[u];
  const float* __restrict__ x = down + d0;
  double sq1 = 0, s1 = 0, sq2 = 0, s2 = 0;
  for (int64_t i = threadIdx.x; i < nd; i += blockDim.x) {
    const double v = x[i];
    if (i < nd1) { sq1 += v * v; s1 += v; } else { sq2 += v * v; s2 += v; }
  }
  __shared__ double red[4][16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  sq1 = wave_sum_d(sq1); s1 = wave_sum_d(s1); sq2 = wave_sum_d(sq2); s2 = wave_sum_d(s2);
  if (lane == 0) { red[0][wid] = sq1; red[1][wid] = s1; red[2][wid] = sq2; red[3][wid] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0, c = 0, d = 0, e = 0;
    for (int i = 0; i < nw; ++i) { a += red[0][i]; c += red[1][i]; d += red[2][i]; e += red[3][i]; }
    // each chunk's BLAS result is a float that is then added to a double accumulator
    const double fsq1 = static_cast<float>(a), fs1 = static_cast<float>(c);
    const double sumsq2 = fsq1 + static_cast<double>(static_cast<float>(d));
    const double sum2 = fs1 + static_cast<double>(static_cast<float>(e));
    const double n1 = static_cast<double>(nd1), n2 = static_cast<double>(nd);
    const double m1 = nd1 > 0 ? fs1 / n1 : 0.0, m2 = nd > 0 ? sum2 / n2 : 0.0;
    const double ms1 = nd1 > 0 ? fsq1 / n1 - m1 * m1 : 0.0;
    const double ms2 = nd > 0 ? sumsq2 / n2 - m2 * m2 : 0.0;
    const double W = t.win_size, bal = t.nccf_ballast;
    float* __restrict__ o = ub + u * 6;
    o[0] = static_cast<float>((ms1 * W) * (ms1 * W) * bal);
    o[1] = static_cast<float>((ms2 * W) * (ms2 * W) * bal);
    const float f1 = static_cast<float>(ms1), f2 = static_cast<float>(ms2);
    o[2] = static_cast<float>((static_cast<double>(f1) * W) * (static_cast<double>(f1) * W) * bal);
    o[3] = static_cast<float>((static_cast<double>(f2) * W) * (static_cast<double>(f2) * W) * bal);
    o[4] = o[3];
    // ApproxEqual(a, b, 0.01): |a - b| <= 0.01 (|a| + |b|); frames of phase 2 compare equal
    const bool differ = b.frames_phase1[u] > 0 && !(fabsf(f1 - f2) <= 0.01f * (fabsf(f1) + fabsf(f2)));
    o[5] = differ ? 1.0f : 0.0f;
  }
}

namespace {

constexpr int kLagGroup = 5;   // lags per lane and pass of the correlation
constexpr int kNccfWaves = 12;  // 48 frames per workgroup: two workgroups per CU (LDS) = 6 waves per SIMD

// LDS layout of one frame of an NCCF wave: the window (wl floats), then the NCCF at the integer lags.
// When one pass of the correlation covers every lag (num_lags <= 80: the window is dead by the time the
// NCCF is written) the NCCF overlays the head of the window.  The frames of a wave sit 16 mod 32 floats
// apart, so that the two 16-lane rows of a ds_read_b32 lane group (banks = dword address mod 32) never
// meet in the correlation - lane l of a row reads dword base + 5 l (banks 0, 5, .., 30, 3, .., 28, 1, 6,
// 11) and that set shifted by 16 is its complement -, and frames 2 and 3 keep their NCCF 8 floats
// further in, which spreads the four frames of the matrix-pipe resampler over the banks 0, 16, 8, 24.
struct NccfLayout {
  int nccf_off;  // floats from the window to the NCCF of frames 0, 1 (frames 2, 3: + 8)
  int pitch;     // floats between frames
};
__host__ __device__ inline NccfLayout nccf_layout(int wl, int ln, int num_lags) {
  NccfLayout y;
  const bool overlay = num_lags <= kLagGroup * 16 && ln + 8 <= wl;
  y.nccf_off = overlay ? 0 : wl;
  const int n = overlay ? wl : wl + ln + 8;
  y.pitch = n + ((16 - n % 32) + 32) % 32;
  return y;
}

}  // namespace

// one thread per frame: where its window starts in the resampled batch, which of the window's samples exist, and
// the frame's NCCF ballast - 16 bytes that the NCCF kernel reads with ONE load per frame (it used to walk
// frame -> utterance -> offsets -> samples: three dependent trips to HBM at the head of every set of frames,
// half of its wave cycles, profiles/r05_pmc_pitch10k_after_summary.txt)
__global__ void pitch_frame_meta_kernel(const PitchDevTables t, const PitchBatch b, const float* __restrict__ ub,
                                        int4* __restrict__ frame_meta) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= b.total_frames) return;
  const int64_t u = find_utt(b.frame_offsets, b.n_utts, g);
  const int64_t frame = g - b.frame_offsets[u];
  const int64_t d0 = b.down_offsets[u], nd = b.down_offsets[u + 1] - d0;
  int64_t start;
  if (t.snip_edges) start = frame * t.win_shift;
  else start = static_cast<int64_t>((static_cast<double>(frame) + 0.5) * t.win_shift) - t.full_len / 2;
  // window sample i is signal sample start + i: it exists for lo <= i < hi (everything else reads as zero)
  const int64_t lo = start < 0 ? (-start < t.full_len ? -start : t.full_len) : 0;
  const int64_t room = nd - start;
  const int64_t hi = room < 0 ? 0 : (room < t.full_len ? room : t.full_len);
  const int64_t first = d0 + start;   // (may lie in front of the batch for a centred first frame: masked by lo)
  const float ballast = frame < b.frames_phase1[u] ? ub[u * 6 + 0] : ub[u * 6 + 1];
  frame_meta[g] = make_int4(static_cast<int>(static_cast<uint32_t>(first)), static_cast<int>(first >> 32),
                            static_cast<int>(lo | (hi << 16)), __builtin_bit_cast(int, ballast));
}

// ---- 3. NCCF at the integer lags, resampled to the lags of the Viterbi states ------------------------
__global__ __launch_bounds__(kNccfWaves * 64, 6) void pitch_nccf_kernel(
    const PitchDevTables t, const PitchBatch b, const float* __restrict__ down,
    const int4* __restrict__ frame_meta, float* __restrict__ nccf_res,
    float* __restrict__ pov_nccf, float* __restrict__ anp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int S = t.num_states, L = t.num_lags, W = t.win_size;
  const int KQ = t.ar_quad_taps >> 2, G = t.ar_groups;
  // sinc taps of every state quad in matrix-pipe order (PitchDevTables), shared by the workgroup
  float4* quad_w = reinterpret_cast<float4*>(smem);
  int* quad_base = reinterpret_cast<int*>(quad_w + static_cast<size_t>(G) * KQ * 64);
  for (int i = threadIdx.x; i < G * KQ * 64; i += blockDim.x)
    quad_w[i] = reinterpret_cast<const float4*>(t.ar_quad_w)[i];
  for (int i = threadIdx.x; i < G * 16; i += blockDim.x) quad_base[i] = t.ar_quad_base[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l = lane & 15, q = lane >> 4;
  const int WL = (t.full_len + 16 + 3) & ~3, LN = (L + t.ar_quad_taps + 3) & ~3;
  const NccfLayout lay = nccf_layout(WL, LN, L);
  float* frames0 = reinterpret_cast<float*>(quad_base + G * 16) + wid * 4 * lay.pitch;
  float* win = frames0 + q * lay.pitch;
  float* nccf = win + lay.nccf_off + (q >> 1) * 8;
  // matrix-pipe view of the wave: lane 4 b + j -> state quad b of a group (A operand: state 4 b + j),
  // frame j of the set (B operand and the four results of the lane)
  const int mb = lane >> 2, mj = lane & 3;
  const float* __restrict__ nccf_m = frames0 + mj * lay.pitch + lay.nccf_off + (mj >> 1) * 8;
  const int64_t n_sets = (b.total_frames + 3) >> 2;
  for (int64_t set = static_cast<int64_t>(blockIdx.x) * kNccfWaves + wid; set < n_sets;
       set += static_cast<int64_t>(gridDim.x) * kNccfWaves) {
    const int64_t g = set * 4 + q;
    const bool valid = g < b.total_frames;
    const int4 meta = frame_meta[valid ? g : b.total_frames - 1];
    const float ballast = __builtin_bit_cast(float, meta.w);
    // ---- window (zero beyond the signal and in the read-ahead padding), mean removal, e1 -----------
    wave_sync();
    {
      const float* __restrict__ x = down + ((static_cast<int64_t>(meta.y) << 32) | static_cast<uint32_t>(meta.x));
      // (hi < lo never happens: both are clamped to [0, full_len]; hi == lo: no sample of the window exists)
      const unsigned lo = static_cast<unsigned>(meta.z) & 0xffffu, span = (static_cast<unsigned>(meta.z) >> 16) - lo;
      for (int i = l; i < WL; i += 16) win[i] = static_cast<unsigned>(i) - lo < span ? x[i] : 0.0f;
    }
    float part = 0.0f;
    for (int i = l; i < W; i += 16) part += win[i];
    const float neg_mean = -tree16(part) / static_cast<float>(W);
    for (int i = l; i < t.full_len; i += 16) win[i] += neg_mean;
    float pe = 0.0f;
    for (int i = l; i < W; i += 16) pe = __builtin_fmaf(win[i], win[i], pe);
    const float e1 = tree16(pe);
    wave_sync();
    // ---- lag correlation: 5 x 5 (sample, lag) blocks out of 9 window values in registers ---------
    float pnorm = 0.0f;
    for (int g0 = 0; kLagGroup * 16 * g0 < L; ++g0) {
      const int lb = kLagGroup * (l + 16 * g0);
      float e2[kLagGroup], ip[kLagGroup];
#pragma unroll
      for (int d = 0; d < kLagGroup; ++d) e2[d] = ip[d] = 0.0f;
      if (lb < L) {
        const float* __restrict__ a = win;
        const float* __restrict__ cw = win + t.first_lag + lb;
        // blocks of 5 samples x 5 lags out of 9 window values; the 10 LDS values of the next block are
        // requested before the 50 multiply-adds of the current one (two register sets, A and B; the
        // reads past the last block land in the window's zero padding and are dropped)
        float c[kLagGroup - 1];
#pragma unroll
        for (int k = 0; k < kLagGroup - 1; ++k) c[k] = cw[k];
        float av_a[kLagGroup], cn_a[kLagGroup], av_b[kLagGroup], cn_b[kLagGroup];
        auto fetch = [&](float (&av)[kLagGroup], float (&cn)[kLagGroup], int at) {
#pragma unroll
          for (int k = 0; k < kLagGroup; ++k) {
            av[k] = a[at + k];
            cn[k] = cw[at + kLagGroup - 1 + k];
          }
        };
        auto block = [&](const float (&av)[kLagGroup], const float (&cn)[kLagGroup]) {
          float cc[2 * kLagGroup - 1];
#pragma unroll
          for (int k = 0; k < kLagGroup - 1; ++k) cc[k] = c[k];
#pragma unroll
          for (int k = 0; k < kLagGroup; ++k) cc[kLagGroup - 1 + k] = cn[k];
#pragma unroll
          for (int k = 0; k < kLagGroup; ++k)
#pragma unroll
            for (int d = 0; d < kLagGroup; ++d) {
              ip[d] = __builtin_fmaf(av[k], cc[k + d], ip[d]);
              e2[d] = __builtin_fmaf(cc[k + d], cc[k + d], e2[d]);
            }
#pragma unroll
          for (int k = 0; k < kLagGroup - 1; ++k) c[k] = cc[kLagGroup + k];
        };
        fetch(av_a, cn_a, 0);
        int i = 0;
        for (; i + 2 * kLagGroup <= W; i += 2 * kLagGroup) {
          fetch(av_b, cn_b, i + kLagGroup);
          block(av_a, cn_a);
          fetch(av_a, cn_a, i + 2 * kLagGroup);
          block(av_b, cn_b);
        }
        if (i + kLagGroup <= W) {
          block(av_a, cn_a);
          i += kLagGroup;
        }
        for (; i < W; ++i) {  // windows that are not a multiple of 5 samples
          const float ai = a[i];
#pragma unroll
          for (int d = 0; d < kLagGroup; ++d) {
            const float vc = cw[i + d];
            ip[d] = __builtin_fmaf(ai, vc, ip[d]);
            e2[d] = __builtin_fmaf(vc, vc, e2[d]);
          }
        }
      }
#pragma unroll
      for (int d = 0; d < kLagGroup; ++d) {
        const int lag = lb + d;
        if (lag < L) {
          const float norm = e1 * e2[d];
          const float den = sqrtf(norm + ballast);
          nccf[lag] = den != 0.0f ? ip[d] / den : 0.0f;
          // the POV feature uses the NCCF without ballast; only the lags around the state chosen by
          // the traceback are read back
          const float den0 = sqrtf(norm);
          if (valid) pov_nccf[g * L + lag] = den0 != 0.0f ? ip[d] / den0 : 0.0f;
          pnorm += norm;
        }
      }
    }
    const float avg_norm_prod = tree16(pnorm) / static_cast<float>(L);  // (RecomputeBacktraces)
    if (valid && l == 0) anp[g] = avg_norm_prod;
    for (int i = L + l; i < LN; i += 16) nccf[i] = 0.0f;  // (taps are zero padded)
    wave_sync();
    // ---- ArbitraryResample: NCCF at the lag of every state, on the matrix pipe.  One
    // v_mfma_f32_4x4x1_16b_f32 = 16 blocks of (4 states) x (4 frames) += w[state][lag] * nccf[frame][lag]:
    // a fused multiply-add per element, lags ascending = Kaldi's tap order (zero weights in front of
    // and behind a state's taps leave its sum unchanged); two groups of 64 states run as independent
    // chains.  12 steps per group instead of 27 x 12 multiply-adds (+ as many LDS reads) per lane. ------
    {
      const int64_t gm = set * 4 + mj;
      const bool valid_m = gm < b.total_frames;
      float* __restrict__ row = nccf_res + gm * static_cast<int64_t>(S);
      // (the usual 12-lag quad window as straight-line code: a loop over a run-time step count makes the
      // register allocator rotate the two accumulators through v_accvgpr moves every iteration)
      auto groups = [&](auto kq_const) {
        constexpr int kKq = decltype(kq_const)::value;
        const int kq = kKq > 0 ? kKq : KQ;
        for (int g2 = 0; g2 < G; g2 += 2) {
          const float* __restrict__ x0 = nccf_m + quad_base[g2 * 16 + mb];
          const float* __restrict__ x1 = nccf_m + quad_base[g2 * 16 + 16 + mb];
          const float4* __restrict__ w0 = quad_w + static_cast<size_t>(g2) * kq * 64 + lane;
          const float4* __restrict__ w1 = w0 + kq * 64;
          f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int k4 = 0; k4 < kq; ++k4) {
            const float4 a0 = w0[k4 * 64], a1 = w1[k4 * 64];
            const float b00 = x0[4 * k4], b01 = x0[4 * k4 + 1], b02 = x0[4 * k4 + 2], b03 = x0[4 * k4 + 3];
            const float b10 = x1[4 * k4], b11 = x1[4 * k4 + 1], b12 = x1[4 * k4 + 2], b13 = x1[4 * k4 + 3];
            acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.x, b00, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.x, b10, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.y, b01, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.y, b11, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.z, b02, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.z, b12, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.w, b03, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.w, b13, acc1, 0, 0, 0);
          }
          if (valid_m) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int s0 = 64 * (g2 + h) + 4 * mb;
              const f32x4 acc = h ? acc1 : acc0;
              if (s0 + 4 <= S) {
                *reinterpret_cast<f32x4_a4*>(row + s0) = f32x4_a4{acc[0], acc[1], acc[2], acc[3]};
              } else {
#pragma unroll
                for (int i = 0; i < 3; ++i)
                  if (s0 + i < S) row[s0 + i] = acc[i];
              }
            }
          }
        }
      };
      if (KQ == 3) groups(std::integral_constant<int, 3>{});
      else groups(std::integral_constant<int, 0>{});
    }
  }
}

int pitch_stage_done(int trace, const char* name, int index, hipStream_t stream) {
  if (!trace) return 0;
  SNF_HIP_CHECK(hipStreamSynchronize(stream));
  fprintf(stderr, "[snf pitch] %s done\n", name);
  return trace == index ? 1 : 0;
}

int launch_pitch_front(const PitchDevTables& t, const PitchBatch& b, const PitchScratch& w, int trace,
                       hipStream_t stream, bool* stop) {
  *stop = true;   // (until every stage is behind us)
  if (b.total_down > 0) {
    const int threads = 256;
    // grid.y is limited to 65535: utterances are launched in slices
    for (int64_t u0 = 0; u0 < b.n_utts; u0 += 65535) {
      PitchBatch bs = b;
      bs.sample_offsets = b.sample_offsets + u0;
      bs.down_offsets = b.down_offsets + u0;
      const int64_t nu = b.n_utts - u0 < 65535 ? b.n_utts - u0 : 65535;
      // LDS: the input span of 256 outputs (ceil(256 in_unit / out_unit) + a unit of slack + one filter)
      const size_t span_lds = sizeof(float) * (static_cast<size_t>(threads + t.rs_out_unit) * t.rs_in_unit /
                                                   t.rs_out_unit + t.rs_in_unit + t.rs_max_taps + 8);
      if (span_lds > 64 * 1024)
        return set_error(SNF_E_RUNTIME, "pitch resampler: the input span of a workgroup does not fit in LDS");
      hipLaunchKernelGGL(pitch_resample_kernel,
                         dim3(static_cast<unsigned>((b.max_down + threads * kRsChunks - 1) / (threads * kRsChunks)),
                              static_cast<unsigned>(nu)),
                         dim3(threads), span_lds, stream, t, bs, w.down);
      SNF_HIP_CHECK(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(pitch_stats_kernel, dim3(static_cast<unsigned>(b.n_utts)), dim3(256), 0, stream,
                     t, b, w.down, w.ub);
  SNF_HIP_CHECK(hipGetLastError());
  if (pitch_stage_done(trace, "resample + stats", 1, stream)) return SNF_OK;
  const int L = t.num_lags;
  if (t.full_len >= 65536) return set_error(SNF_E_RUNTIME, "pitch: a correlation window of more than 65535 samples");
  hipLaunchKernelGGL(pitch_frame_meta_kernel, dim3(static_cast<unsigned>((b.total_frames + 255) / 256)),
                     dim3(256), 0, stream, t, b, w.ub, w.frame_meta);
  SNF_HIP_CHECK(hipGetLastError());
  const int WL = (t.full_len + 16 + 3) & ~3, LN = (L + t.ar_quad_taps + 3) & ~3;
  const size_t lds = sizeof(float) * (static_cast<size_t>(t.ar_groups) * t.ar_quad_taps * 64 +
                                      t.ar_groups * 16 +
                                      static_cast<size_t>(kNccfWaves) * 4 * nccf_layout(WL, LN, L).pitch);
  if (lds > 160 * 1024) return set_error(SNF_E_RUNTIME, "pitch lag tables do not fit in LDS");
  if (lds > 64 * 1024)
    SNF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pitch_nccf_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  const int64_t n_sets = (b.total_frames + 3) / 4;
  int64_t blocks = (n_sets + kNccfWaves - 1) / kNccfWaves;
  if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride: the taps are staged once per workgroup
  hipLaunchKernelGGL(pitch_nccf_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kNccfWaves * 64), lds,
                     stream, t, b, w.down, w.frame_meta, w.nccf_res, w.pov_nccf, w.anp);
  SNF_HIP_CHECK(hipGetLastError());
  if (pitch_stage_done(trace, "nccf", 2, stream)) return SNF_OK;
  *stop = false;
  return SNF_OK;
}

}  // namespace snf
