// Pitch post-processing (reference processor/pitch_kaldi.py:535-537 -> [KALDI-UPSTREAM] pitch-functions.cc
// OnlineProcessPitch): the POV mappings and the log pitch, the per-frame kernel, the tiled kernel that evaluates
// them once per frame, and launch_pitch_post.  Which kernel runs, its halos and its LDS: pitch_post_route,
// post_route.h.
#include "post_route.h"
#include "snf_internal.h"
#include "utt_search.h"

namespace snf {

namespace {

// counter-based N(0,1) for the delta-pitch noise
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ float gauss(uint64_t seed, uint64_t idx) {
  const uint64_t h = mix64(seed ^ mix64(idx));
  const float u1 = (static_cast<float>((h >> 40) & 0xFFFFFF) + 1.0f) * (1.0f / 16777216.0f);
  const float u2 = static_cast<float>((h >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Pitch post-processing: one thread per frame.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float nccf_to_pov_feature(float n) {
  n = fminf(fmaxf(n, -1.0f), 1.0f);
  return static_cast<float>(pow(1.0001 - static_cast<double>(n), 0.15) - 1.0);
}
__device__ __forceinline__ float nccf_to_pov(float n) {
  float a = fabsf(n);
  if (a > 1.0f) a = 1.0f;
  const double ad = a;
  // Kaldi calls Exp() with double arguments here -> double overload
  const float r = static_cast<float>(-5.2 + 5.4 * exp(7.5 * (ad - 1.0)) + 4.8 * ad -
                                     2.0 * exp(-10.0 * ad) + 4.2 * exp(20.0 * (ad - 1.0)));
  return static_cast<float>(1.0 / (1.0 + exp(-1.0 * static_cast<double>(r))));
}

// Log pitch.  The reference takes Kaldi's Log(float), glibc's logf, which is correctly rounded in all but a handful
// of arguments; the device's logf (log2 in hardware, then the product by ln 2) errs by up to 2 ulp at 50 - 400 Hz,
// which the float64 statement tells apart (tests/test_post_routes_gpu.py).  The double logarithm rounded once gives
// the reference's value.  pitch_post_tiled_kernel evaluates it once per frame, next to the four double exponentials
// of nccf_to_pov (0.0284 -> 0.0295 ms on 300 000 frames); pitch_post_kernel, the route of windows too long for LDS,
// pays for it at every window position like it does for the exponentials (0.46 -> 0.71 ms on 1 000 utterances of 300
// frames with a left context of 6 000).
__device__ __forceinline__ float log_pitch_of(float hz) {
  return static_cast<float>(log(static_cast<double>(hz)));
}

__global__ void pitch_post_kernel(const PitchPostParams p, const float* __restrict__ in,
                                  const int64_t* __restrict__ frame_offsets, const int64_t n_utts,
                                  const int64_t total_frames, float* __restrict__ out) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= total_frames) return;
  const int64_t u = find_utt(frame_offsets, n_utts, g);
  const int64_t f0 = frame_offsets[u], f1 = frame_offsets[u + 1];
  const snf_pitch_post_options& o = p.o;
  float* __restrict__ row = out + g * p.ndims;
  int idx = 0;
  const float nccf = in[g * 2], log_pitch = log_pitch_of(in[g * 2 + 1]);
  if (o.add_pov_feature) row[idx++] = o.pov_scale * nccf_to_pov_feature(nccf) + o.pov_offset;
  if (o.add_normalized_log_pitch) {
    int64_t wb = g - o.normalization_left_context, we = g + o.normalization_right_context + 1;
    if (wb < f0) wb = f0;
    if (we > f1) we = f1;
    double sum_pov = 0.0, sum_lp = 0.0;
    for (int64_t t = wb; t < we; ++t) {
      const float pov = nccf_to_pov(in[t * 2]), lp = log_pitch_of(in[t * 2 + 1]);
      sum_pov += pov;
      sum_lp += pov * lp;
    }
    const float avg = static_cast<float>(sum_lp / sum_pov);
    row[idx++] = (log_pitch - avg) * o.pitch_scale;
  }
  if (o.add_delta_pitch) {
    // ComputeDeltas(order 1, window w) over the clamped +-w neighbourhood of log-pitch
    const int w = o.delta_window;
    float normalizer = 0.0f;
    for (int j = -w; j <= w; ++j) normalizer += static_cast<float>(j * j);
    const float inv = static_cast<float>(1.0 / normalizer);
    int64_t lo = g - w, hi = g + w;
    if (lo < f0) lo = f0;
    if (hi > f1 - 1) hi = f1 - 1;
    float acc = 0.0f;
    for (int j = -w; j <= w; ++j) {
      int64_t t = g + j;
      t = t < lo ? lo : (t > hi ? hi : t);
      const float s = static_cast<float>(j) * inv;
      if (s != 0.0f) acc += s * log_pitch_of(in[t * 2 + 1]);
    }
    float noise = 0.0f;
    if (o.delta_pitch_noise_stddev != 0.0f)
      noise = gauss(p.seed, frame_noise_id(g - f0, f1 - f0, __float_as_uint(in[f0 * 2 + 1]))) *
              o.delta_pitch_noise_stddev;  // (keyed per utterance, not per batch row: snf_internal.h)
    row[idx++] = (acc + noise) * o.delta_pitch_scale;
  }
  if (o.add_raw_log_pitch) row[idx++] = log_pitch;
}

// Tiled variant of the same arithmetic: the POV weight and the log-pitch of a frame are evaluated
// ONCE (by the workgroup that needs them, into LDS) instead of once per window position - the POV
// mapping costs four double-precision exponentials, and the +-75-frame normalisation window made the
// kernel above evaluate it 151 times per frame.
__global__ __launch_bounds__(kPostRows) void pitch_post_tiled_kernel(
    const PitchPostParams p, const float* __restrict__ in, const int halo_l, const int halo_r,
    const int64_t* __restrict__ frame_offsets, const int64_t n_utts, const int64_t total_frames,
    float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* s_pov = reinterpret_cast<float*>(smem);        // [kPostRows + halo_l + halo_r]
  float* s_lp = s_pov + pitch_post_tile_rows(halo_l, halo_r);  // log-pitch
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * kPostRows;
  const int64_t t0 = g0 - halo_l;
  const int tile = pitch_post_tile_rows(halo_l, halo_r);
  for (int i = threadIdx.x; i < tile; i += blockDim.x) {
    const int64_t t = t0 + i;
    float pov = 0.0f, lp = 0.0f;
    if (t >= 0 && t < total_frames) {
      pov = nccf_to_pov(in[t * 2]);
      lp = log_pitch_of(in[t * 2 + 1]);
    }
    s_pov[i] = pov;
    s_lp[i] = lp;
  }
  __syncthreads();
  const int64_t g = g0 + threadIdx.x;
  if (g >= total_frames) return;
  const int64_t u = find_utt(frame_offsets, n_utts, g);
  const int64_t f0 = frame_offsets[u], f1 = frame_offsets[u + 1];
  const snf_pitch_post_options& o = p.o;
  float* __restrict__ row = out + g * p.ndims;
  int idx = 0;
  const float nccf = in[g * 2];
  const float log_pitch = s_lp[g - t0];
  if (o.add_pov_feature) row[idx++] = o.pov_scale * nccf_to_pov_feature(nccf) + o.pov_offset;
  if (o.add_normalized_log_pitch) {
    int64_t wb = g - o.normalization_left_context, we = g + o.normalization_right_context + 1;
    if (wb < f0) wb = f0;
    if (we > f1) we = f1;
    double sum_pov = 0.0, sum_lp = 0.0;
    for (int64_t t = wb; t < we; ++t) {
      const float pov = s_pov[t - t0], lp = s_lp[t - t0];
      sum_pov += pov;
      sum_lp += pov * lp;
    }
    const float avg = static_cast<float>(sum_lp / sum_pov);
    row[idx++] = (log_pitch - avg) * o.pitch_scale;
  }
  if (o.add_delta_pitch) {
    const int w = o.delta_window;
    float normalizer = 0.0f;
    for (int j = -w; j <= w; ++j) normalizer += static_cast<float>(j * j);
    const float inv = static_cast<float>(1.0 / normalizer);
    int64_t lo = g - w, hi = g + w;
    if (lo < f0) lo = f0;
    if (hi > f1 - 1) hi = f1 - 1;
    float acc = 0.0f;
    for (int j = -w; j <= w; ++j) {
      int64_t t = g + j;
      t = t < lo ? lo : (t > hi ? hi : t);
      const float sc = static_cast<float>(j) * inv;
      if (sc != 0.0f) acc += sc * s_lp[t - t0];
    }
    float noise = 0.0f;
    if (o.delta_pitch_noise_stddev != 0.0f)
      noise = gauss(p.seed, frame_noise_id(g - f0, f1 - f0, __float_as_uint(in[f0 * 2 + 1]))) *
              o.delta_pitch_noise_stddev;  // (keyed per utterance, not per batch row: snf_internal.h)
    row[idx++] = (acc + noise) * o.delta_pitch_scale;
  }
  if (o.add_raw_log_pitch) row[idx++] = log_pitch;
}

int launch_pitch_post(const PitchPostParams& p, const float* in, const int64_t* frame_offsets,
                      int64_t n_utts, int64_t total_frames, float* out, hipStream_t stream,
                      const char** launched) {
  if (launched) *launched = nullptr;
  if (total_frames <= 0) return SNF_OK;
  const PostRoute r = pitch_post_route(p.o, post_knobs_from_env());
  const dim3 grid(static_cast<unsigned>((total_frames + r.rows - 1) / r.rows)), block(r.threads);
  if (r.kernel == kPitchPostTiled) {
    const PitchPostHalos h = pitch_post_halos(p.o);
    hipLaunchKernelGGL(pitch_post_tiled_kernel, grid, block, r.lds_bytes, stream, p, in, h.left, h.right,
                       frame_offsets, n_utts, total_frames, out);
  } else {
    hipLaunchKernelGGL(pitch_post_kernel, grid, block, 0, stream, p, in, frame_offsets, n_utts, total_frames, out);
  }
  SNF_HIP_CHECK(hipGetLastError());
  if (launched) *launched = r.name();
  return SNF_OK;
}

}  // namespace snf
