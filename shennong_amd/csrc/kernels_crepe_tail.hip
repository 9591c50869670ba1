// The tail of the CREPE pitch path between the decoder and the Kaldi post-processing (reference
// processor/pitch_crepe.py:473-489 and :572-606), float64 on the device.  Compiled with -ffp-contract=off: the
// voicing lattice must take the decisions of the host function, which fuses nothing.
//
// Row resampling (crepe_rows_kernel): scipy.signal.resample of the (confidence, Hertz) rows of an utterance
// from N to M rows, as the sum it is for real input,
//     y[m] = (1 / N) sum_n x[n] D(m, n),   D = sin((2K + 1) t) / sin(t) + c cos(L t),   t = pi (m N - n M) / (M N),
// L = min(N, M), K = (L - 1) / 2, c = 0 for odd L, 2 for even L going down, 1 for even L going up; D = 2K + 1 + c
// where sin(t) = 0.  One workgroup of one wave per (utterance, tile of kCrepeRowsTile output rows): a lane owns
// an output row and adds its N terms in ascending n, both columns from one D; the input rows pass through LDS
// kCrepeRowsStage at a time and every lane reads the same address (a broadcast: no bank conflict, float64 or
// not).  An output row depends on its utterance's rows and on (N, M, m) alone: the same bits in any batch.
//   * The angles are reduced in INTEGERS: s = (m N - n M) reduced to (-MN / 2, MN / 2], a = (2K + 1) s and
//     b = L s modulo 2 MN, all three stepped from n to n + 1 by a subtraction and a conditional wrap (adding MN to
//     s adds an odd multiple of pi to the numerator's angle and pi to the denominator's: the quotient stays).
//     The trigonometric functions see a / MN, s / MN and b / MN in [-1/2, 2): sinpi and cospi of those lose
//     nothing to the size of k or n.
//   * M == N copies the rows.  Then the reference's clamp of column 0: below 1e-2 to 0, above 1 to 1.
//
// Voicing, interpolation and NCCF (crepe_voicing_kernel): one workgroup of one wave per utterance.
//   * The two-state Viterbi of predict_voicing is serial over the frames: lane 0 walks it, the confidences (then
//     the lattice, on the way back) staged in LDS kCrepeVoicingChunk frames at a time by all lanes.  The lattice
//     lives in scratch; the way back recomputes argmax_i(lattice[t][i] + logA[i][state[t + 1]]) like the host
//     does (first index on ties, a NaN counts as the maximum, as numpy has it) and leaves, per frame, the index
//     of the nearest voiced frame at or after it.
//   * The nearest voiced frame at or before a frame is a maximum scan over the wave (shuffles, a carry between
//     rounds of 64 frames); the pitch of an unvoiced frame is numpy's interp between the two, or the value of
//     the only neighbour there is.
//   * NCCF from POV: 64 halvings of [0, 1] over the map of Ghahremani et al., a frame per lane.
//   * Status: 1 no voiced frame, 2 a pitch that is not positive, 3 a POV outside the map's open range; the
//     lowest that applies.  With 1 and 2 the utterance's output rows are zeroed, with 3 the NCCF of the
//     offending frames is 0.
#include <math.h>

#include "snf_internal.h"

namespace snf {

namespace {

__global__ __launch_bounds__(64) void crepe_rows_kernel(const double* __restrict__ in,
                                                        const int64_t* __restrict__ in_off,
                                                        const int64_t* __restrict__ out_off,
                                                        const int32_t* __restrict__ tile_utt,
                                                        const int64_t* __restrict__ tile_off,
                                                        double* __restrict__ out) {
  __shared__ double s_x[2][kCrepeRowsStage];
  const int lane = threadIdx.x;
  const int64_t u = tile_utt[blockIdx.x];
  const int64_t N = in_off[u + 1] - in_off[u], M = out_off[u + 1] - out_off[u];
  const int64_t row = (static_cast<int64_t>(blockIdx.x) - tile_off[u]) * kCrepeRowsTile + lane;
  const bool valid = row < M;
  const int64_t m = valid ? row : M - 1;   // (a lane past the last row computes that row again and stores nothing)
  const double* x = in + 2 * in_off[u];
  double* y = out + 2 * (out_off[u] + m);
  double y0, y1;
  if (M == N) {
    y0 = x[2 * m];
    y1 = x[2 * m + 1];
  } else {
    const int64_t L = N < M ? N : M, odd = 2 * ((L - 1) / 2) + 1, MN = M * N, MN2 = 2 * MN;
    const double c = (L & 1) ? 0.0 : (M < N ? 2.0 : 1.0);
    const double inv = 1.0 / static_cast<double>(MN), flat = static_cast<double>(odd) + c;
    int64_t s = m * N;
    if (2 * s > MN) s -= MN;
    int64_t a = (odd * s) % MN2, b = (L * s) % MN2;
    if (a < 0) a += MN2;
    if (b < 0) b += MN2;
    const int64_t step_a = (odd * M) % MN2, step_b = (L * M) % MN2;
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t base = 0; base < N; base += kCrepeRowsStage) {
      const int count = static_cast<int>(N - base < kCrepeRowsStage ? N - base : kCrepeRowsStage);
      for (int i = lane; i < count; i += 64) {
        s_x[0][i] = x[2 * (base + i)];
        s_x[1][i] = x[2 * (base + i) + 1];
      }
      __syncthreads();
      for (int i = 0; i < count; ++i) {
        double D = flat;
        if (s != 0) {
          D = sinpi(static_cast<double>(a) * inv) / sinpi(static_cast<double>(s) * inv);
          if (c != 0.0) D += c * cospi(static_cast<double>(b) * inv);
        }
        acc0 += s_x[0][i] * D;
        acc1 += s_x[1][i] * D;
        s -= M;
        a -= step_a;
        b -= step_b;
        if (a < 0) a += MN2;
        if (b < 0) b += MN2;
        if (2 * s <= -MN) {
          s += MN;
          a += MN;
          if (a >= MN2) a -= MN2;
        }
      }
      __syncthreads();
    }
    y0 = acc0 / static_cast<double>(N);
    y1 = acc1 / static_cast<double>(N);
  }
  if (y0 < 1e-2) y0 = 0.0;
  if (y0 > 1.0) y0 = 1.0;
  if (valid) {
    y[0] = y0;
    y[1] = y1;
  }
}

struct VoicingModel {
  double log_norm, mean[2], variance, log_start, lt[2][2], pov_lo, pov_hi;
};

// numpy's max and argmax of a pair: a NaN wins, the first index on ties
__device__ inline double max_pair(double a, double b) { return a != a ? a : b != b ? b : a > b ? a : b; }
__device__ inline int argmax_pair(double a, double b) { return a != a ? 0 : b != b ? 1 : b > a ? 1 : 0; }

__device__ inline double log_emission(const VoicingModel& md, double c, int state) {
  const double d = c - md.mean[state];
  return -0.5 * (md.log_norm + d * d / md.variance);
}

__device__ inline double nccf_to_pov(double x) {
  const double y = -5.2 + 5.4 * exp(7.5 * (x - 1.0)) + 4.8 * x - 2.0 * exp(-10.0 * x) + 4.2 * exp(20.0 * (x - 1.0));
  return 1.0 / (1.0 + exp(-y));
}

__global__ __launch_bounds__(64) void crepe_voicing_kernel(const double* __restrict__ rows,
                                                           const int64_t* __restrict__ off, VoicingModel md,
                                                           double* lattice, int32_t* next_voiced,
                                                           float* __restrict__ out, int32_t* __restrict__ status) {
  __shared__ double s_buf[2 * kCrepeVoicingChunk];
  __shared__ int s_voiced;
  const int lane = threadIdx.x;
  const int64_t u = blockIdx.x, first = off[u];
  const int N = static_cast<int>(off[u + 1] - first);
  if (N == 0) {
    if (lane == 0) status[u] = 0;
    return;
  }
  const double* x = rows + 2 * first;
  double* lat = lattice + 2 * first;
  int32_t* nxt = next_voiced + first;
  float* o = out + 2 * first;

  // forward: lattice[t][j] = max_i(lattice[t - 1][i] + logA[i][j]) + logB[t][j]
  double l0 = 0.0, l1 = 0.0;
  for (int base = 0; base < N; base += kCrepeVoicingChunk) {
    const int count = N - base < kCrepeVoicingChunk ? N - base : kCrepeVoicingChunk;
    for (int i = lane; i < count; i += 64) s_buf[i] = x[2 * (base + i)];
    __syncthreads();
    if (lane == 0)
      for (int i = 0; i < count; ++i) {
        const double e0 = log_emission(md, s_buf[i], 0), e1 = log_emission(md, s_buf[i], 1);
        if (base + i == 0) {
          l0 = md.log_start + e0;
          l1 = md.log_start + e1;
        } else {
          const double n0 = max_pair(l0 + md.lt[0][0], l1 + md.lt[1][0]) + e0;
          const double n1 = max_pair(l0 + md.lt[0][1], l1 + md.lt[1][1]) + e1;
          l0 = n0;
          l1 = n1;
        }
        lat[2 * (base + i)] = l0;
        lat[2 * (base + i) + 1] = l1;
      }
    __syncthreads();
  }

  // backward: the states, kept as the index of the nearest voiced frame at or after every frame (N: none)
  int state = 0, voiced = 0, next = N;
  for (int base = (N - 1) / kCrepeVoicingChunk * kCrepeVoicingChunk; base >= 0; base -= kCrepeVoicingChunk) {
    const int count = N - base < kCrepeVoicingChunk ? N - base : kCrepeVoicingChunk;
    for (int i = lane; i < 2 * count; i += 64) s_buf[i] = lat[2 * base + i];
    __syncthreads();
    if (lane == 0)
      for (int i = count - 1; i >= 0; --i) {
        const int t = base + i;
        state = t == N - 1 ? argmax_pair(s_buf[2 * i], s_buf[2 * i + 1])
                           : argmax_pair(s_buf[2 * i] + md.lt[0][state], s_buf[2 * i + 1] + md.lt[1][state]);
        if (state) {
          next = t;
          ++voiced;
        }
        nxt[t] = next;
      }
    __syncthreads();
  }
  if (lane == 0) s_voiced = voiced;
  __syncthreads();
  if (s_voiced == 0) {
    for (int i = lane; i < 2 * N; i += 64) o[i] = 0.f;
    if (lane == 0) status[u] = 1;
    return;
  }

  // pitch: the frame's own when voiced, numpy's interp between the voiced neighbours otherwise
  int carry = -1, bad = 0;
  for (int base = 0; base < N; base += 64) {
    const int t = base + lane;
    const bool in = t < N;
    const int after = in ? nxt[t] : N;
    int before = (in && after == t) ? t : -1;
    for (int d = 1; d < 64; d <<= 1) {
      const int other = __shfl_up(before, d);
      if (lane >= d && other > before) before = other;
    }
    if (carry > before) before = carry;
    carry = __shfl(before, 63);
    if (in) {
      double p;
      if (after == t) {
        p = x[2 * t + 1];
      } else if (before < 0) {
        p = x[2 * after + 1];
      } else if (after >= N) {
        p = x[2 * before + 1];
      } else {
        const double fa = x[2 * before + 1], fb = x[2 * after + 1];
        const double slope = (fb - fa) / (static_cast<double>(after) - static_cast<double>(before));
        p = slope * (static_cast<double>(t) - static_cast<double>(before)) + fa;
        if (p != p) {
          p = slope * (static_cast<double>(t) - static_cast<double>(after)) + fb;
          if (p != p && fa == fb) p = fa;
        }
      }
      if (!(p > 0.0)) bad = 1;
      o[2 * t + 1] = static_cast<float>(p);
    }
  }
  if (__any(bad)) {
    __syncthreads();
    for (int i = lane; i < 2 * N; i += 64) o[i] = 0.f;
    if (lane == 0) status[u] = 2;
    return;
  }

  // NCCF: 0 and 1 map to themselves, anything else by bisection of the increasing map
  for (int t = lane; t < N; t += 64) {
    const double pov = x[2 * t];
    double r;
    if (pov == 0.0 || pov == 1.0) {
      r = pov;
    } else if (pov <= md.pov_lo || pov >= md.pov_hi) {
      r = 0.0;
      bad = 1;
    } else {
      double lo = 0.0, hi = 1.0;
      for (int k = 0; k < 64; ++k) {
        const double mid = 0.5 * (lo + hi);
        if (nccf_to_pov(mid) < pov) lo = mid; else hi = mid;
      }
      r = 0.5 * (lo + hi);
    }
    o[2 * t] = static_cast<float>(r);
  }
  const int any_bad = __any(bad);
  if (lane == 0) status[u] = any_bad ? 3 : 0;
}

}  // namespace

int launch_crepe_rows(const double* in, const int64_t* in_off, const int64_t* out_off, const int32_t* tile_utt,
                      const int64_t* tile_off, int64_t n_tiles, double* out, hipStream_t stream) {
  if (n_tiles <= 0) return SNF_OK;
  hipLaunchKernelGGL(crepe_rows_kernel, dim3(static_cast<unsigned>(n_tiles)), dim3(64), 0, stream, in, in_off, out_off,
                     tile_utt, tile_off, out);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_crepe_voicing(const double* rows, const int64_t* off, int64_t n_utts, const double* h_model,
                         double* lattice, int32_t* next_voiced, float* out, int32_t* status, hipStream_t stream) {
  if (n_utts <= 0) return SNF_OK;
  VoicingModel md;
  md.log_norm = h_model[0];
  md.mean[0] = h_model[1];
  md.mean[1] = h_model[2];
  md.variance = h_model[3];
  md.log_start = h_model[4];
  md.lt[0][0] = h_model[5];
  md.lt[0][1] = h_model[6];
  md.lt[1][0] = h_model[7];
  md.lt[1][1] = h_model[8];
  md.pov_lo = h_model[9];
  md.pov_hi = h_model[10];
  hipLaunchKernelGGL(crepe_voicing_kernel, dim3(static_cast<unsigned>(n_utts)), dim3(64), 0, stream, rows, off, md,
                     lattice, next_voiced, out, status);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
