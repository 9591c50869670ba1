// General, batched LinearResample on gfx950: Kaldi's ResampleWaveform (resample.cc LinearResample with a cutoff
// of 0.99 x half the lower rate and 6 zero crossings), which is what torchaudio's kaldi.resample_waveform
// computes, for any pair of different rates, down or up, on int16 or float32 samples.  A sibling of
// pitch_resample_kernel (kernels_pitch_front.hip), which runs the one pair and sample type the pitch tracker needs.
//
// linear_resample_kernel: blockIdx.y = utterance, blockIdx.x = a run of kResampleChunks x kResampleChunk = 1024
// consecutive outputs of it.  Per chunk of 256 outputs the workgroup stages the input span they touch (at most
// `span` samples, known on the host) into LDS as floats with coalesced loads - zeros outside the utterance:
// fmaf(w, 0, s) = s exactly, the accumulator never being -0 - while the samples of the next chunk are in flight
// in registers; every thread then runs Kaldi's tap loop for its output from LDS.
//
// The phase table.  Output k uses the filter of phase k mod out_unit: out_unit rows of up to max_taps weights,
// each with its first input (first[]) and its tap count (ntaps[]), 5 440 floats for 44.1 -> 16 kHz.  Two readers:
//   - the chunk geometry needs first[] at a workgroup-uniform index: read from the blob in global memory, which
//     the compiler turns into scalar loads;
//   - the tap loop reads a different row per lane.  A per-lane address cannot use the scalar path, and through the
//     vector memory path every tap of every lane would be a global load, so the blob is copied into LDS once
//     per workgroup (1024 outputs share it) and the rows are read from there.  The rows are `stride` floats
//     apart, max_taps made odd: the lanes of a wave sit on consecutive phases, so tap i of a wave falls into
//     different banks.  A table of ONE phase (integer ratios down) is the exception: its weights are at uniform
//     addresses too and stay on the scalar path, as in pitch_resample_kernel.
//
// Arithmetic contract (oracle/kaldi_oracle.c linres_apply): s = fmaf(w[i], in[idx], s) over the taps ascending
// from s = 0.0f, on the weights of linres_init (host_tables.cpp make_linear_resample gives the same bits).  The
// int16 form rounds the sum with rintf (ties to even) and clamps it to [-32768, 32767].  This file is compiled
// with -ffp-contract=off and every fused multiply-add is written as one.  An output depends on its utterance's
// samples alone: the same bits alone and in any batch, whatever the destination.
#include <algorithm>
#include <cstring>

#include "snf_internal.h"

namespace snf {

namespace {

constexpr int kRegSamples = 6;   // staged samples per thread and chunk that travel through registers

__device__ __forceinline__ void put_sample(float* out, float s) { *out = s; }
__device__ __forceinline__ void put_sample(int16_t* out, float s) {
  s = fminf(fmaxf(rintf(s), -32768.0f), 32767.0f);
  *out = static_cast<int16_t>(static_cast<int>(s));
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(kResampleChunk) void linear_resample_kernel(const ResampleTable t,
                                                                         const T* __restrict__ src,
                                                                         const ResampleUtt* __restrict__ utts,
                                                                         T* __restrict__ dst) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* tab = reinterpret_cast<int32_t*>(smem);
  float* xs = reinterpret_cast<float*>(smem + ((static_cast<size_t>(t.table_words) * 4 + 15) & ~size_t(15)));
  const ResampleUtt u = utts[blockIdx.y];
  const int64_t nd = u.n_out, n = u.n_in;
  const int64_t k_begin = static_cast<int64_t>(blockIdx.x) * (kResampleChunk * kResampleChunks);
  if (k_begin >= nd) return;   // (the whole workgroup; n_out > 0 implies n_in > 0)
  const T* __restrict__ w = src + u.src;
  T* __restrict__ out = dst + u.dst;
  const int out_unit = t.out_unit, in_unit = t.in_unit, stride = t.stride;
  const int tid = static_cast<int>(threadIdx.x);
  // (32-bit index arithmetic: an utterance has fewer than 2^31 samples on either side, checked by the launcher)
  auto first_of = [&](int k) -> int64_t {   // uniform index: scalar loads
    const int unit = k / out_unit;
    return t.blob[k - unit * out_unit] + static_cast<int64_t>(unit) * in_unit;
  };
  // input span of the chunk that starts at output k0: [base, base + span), span <= t.span
  auto geometry = [&](int64_t k0, int64_t* base, int* span) {
    const int k_first = static_cast<int>(k0);
    const int k_last = k0 + (kResampleChunk - 1) < nd - 1 ? k_first + (kResampleChunk - 1) : static_cast<int>(nd) - 1;
    *base = first_of(k_first);                               // (first inputs are non-decreasing in k)
    *span = static_cast<int>(first_of(k_last) + t.max_taps - *base);
  };
  auto sample = [&](int64_t j) -> float { return (j >= 0 && j < n) ? static_cast<float>(w[j]) : 0.0f; };
  // samples in flight: raw values from clamped (always valid) addresses, converted when they are staged
  auto fetch = [&](int64_t j) -> T {
    const int64_t jc = j < 0 ? 0 : (j < n ? j : n - 1);
    return w[jc];
  };
  T pre[kRegSamples];
  int64_t base;
  int span;
  geometry(k_begin, &base, &span);
#pragma unroll
  for (int q = 0; q < kRegSamples; ++q)
    pre[q] = tid + kResampleChunk * q < span ? fetch(base + tid + kResampleChunk * q) : T(0);
  // the table, word for word (the first __syncthreads of the chunk loop publishes it); a single phase is read
  // from global memory at uniform addresses instead (see the tap loop)
  if (out_unit > 1)
    for (int i = tid; i < t.table_words; i += kResampleChunk) tab[i] = t.blob[i];
  const int32_t* __restrict__ tab_first = tab;
  const int32_t* __restrict__ tab_ntaps = tab + out_unit;
  const float* __restrict__ tab_w = reinterpret_cast<const float*>(tab + 2 * out_unit);
  for (int c = 0; c < kResampleChunks; ++c) {
    const int64_t k0 = k_begin + kResampleChunk * c;
    if (k0 >= nd) break;
#pragma unroll
    for (int q = 0; q < kRegSamples; ++q) {
      const int i = tid + kResampleChunk * q;
      const int64_t j = base + i;
      if (i < span) xs[i] = (j >= 0 && j < n) ? static_cast<float>(pre[q]) : 0.0f;
    }
    for (int i = tid + kResampleChunk * kRegSamples; i < span; i += kResampleChunk)
      xs[i] = sample(base + i);   // (rate ratios above 5)
    __syncthreads();
    const int64_t base_cur = base;
    if (c + 1 < kResampleChunks && k0 + kResampleChunk < nd) {
      geometry(k0 + kResampleChunk, &base, &span);
#pragma unroll
      for (int q = 0; q < kRegSamples; ++q)
        pre[q] = tid + kResampleChunk * q < span ? fetch(base + tid + kResampleChunk * q) : T(0);
    }
    const int k = static_cast<int>(k0) + tid;
    if (k < nd) {
      float s = 0.0f;
      if (out_unit == 1) {
        // one filter for every output (integer ratios down, 16 -> 8 kHz): the weights sit at uniform addresses,
        // so they come through the scalar path and the tap loop reads LDS once per tap, not twice
        const float* __restrict__ x = xs + (t.blob[0] + static_cast<int64_t>(k) * in_unit - base_cur);
        const float* __restrict__ wt = reinterpret_cast<const float*>(t.blob + 2);
        const int ntaps = t.blob[1];
        for (int i = 0; i < ntaps; ++i) s = __builtin_fmaf(wt[i], x[i], s);
      } else {
        const int unit = k / out_unit, wrapped = k - unit * out_unit;
        const float* __restrict__ x = xs + (tab_first[wrapped] + static_cast<int64_t>(unit) * in_unit - base_cur);
        const float* __restrict__ wt = tab_w + wrapped * stride;
        const int ntaps = tab_ntaps[wrapped];
        for (int i = 0; i < ntaps; ++i) s = __builtin_fmaf(wt[i], x[i], s);
      }
      put_sample(out + k, s);
    }
    __syncthreads();  // (the next chunk overwrites the staged span)
  }
}

void resample_layout(const LinearResampleHost& r, ResampleTable* t) {
  t->in_unit = r.in_unit;
  t->out_unit = r.out_unit;
  t->max_taps = r.max_taps;
  t->stride = r.max_taps | 1;
  const int64_t words = static_cast<int64_t>(r.out_unit) * (2 + t->stride);
  t->table_words = words > 0x7fffffff ? 0x7fffffff : static_cast<int>(words);
  // a chunk's span: from the first input of its first output to the last input its last output can touch
  int64_t span = 0;
  for (int p = 0; p < r.out_unit; ++p) {
    const int64_t k = static_cast<int64_t>(p) + kResampleChunk - 1;
    const int64_t last = r.first[k % r.out_unit] + (k / r.out_unit) * r.in_unit;
    span = std::max<int64_t>(span, last - r.first[p] + r.max_taps);
  }
  t->span = span > 0x7fffffff ? 0x7fffffff : static_cast<int>(span);
  t->blob = nullptr;
}

void resample_blob(const LinearResampleHost& r, const ResampleTable& t, std::vector<int32_t>* blob) {
  blob->assign(static_cast<size_t>(t.table_words), 0);
  for (int p = 0; p < r.out_unit; ++p) {
    (*blob)[p] = r.first[p];
    (*blob)[r.out_unit + p] = r.ntaps[p];
    memcpy(blob->data() + 2 * static_cast<size_t>(r.out_unit) + static_cast<size_t>(p) * t.stride,
           r.weights.data() + static_cast<size_t>(p) * r.max_taps, sizeof(float) * r.max_taps);
  }
}

int launch_linear_resample(const ResampleTable& t, int kind, const void* src, const ResampleUtt* d_utts,
                           int64_t n_utts, int64_t max_out, void* dst, hipStream_t stream) {
  if (n_utts <= 0 || max_out <= 0) return SNF_OK;
  if (max_out > 0x7fffff00) return set_error(SNF_E_INVALID, "resample: an utterance of more than 2^31 samples");
  const size_t lds = ((static_cast<size_t>(t.table_words) * 4 + 15) & ~size_t(15)) + sizeof(float) * t.span;
  if (lds > kResampleLdsBytes) return set_error(SNF_E_INVALID, "resample: the table and the span do not fit in LDS");
  const int run = kResampleChunk * kResampleChunks;
  const unsigned runs = static_cast<unsigned>((max_out + run - 1) / run);
  // grid.y is limited to 65535: utterances are launched in slices
  for (int64_t u0 = 0; u0 < n_utts; u0 += 65535) {
    const unsigned nu = static_cast<unsigned>(n_utts - u0 < 65535 ? n_utts - u0 : 65535);
    if (kind == 0)
      hipLaunchKernelGGL(linear_resample_kernel<int16_t>, dim3(runs, nu), dim3(kResampleChunk), lds, stream, t,
                         static_cast<const int16_t*>(src), d_utts + u0, static_cast<int16_t*>(dst));
    else
      hipLaunchKernelGGL(linear_resample_kernel<float>, dim3(runs, nu), dim3(kResampleChunk), lds, stream, t,
                         static_cast<const float*>(src), d_utts + u0, static_cast<float*>(dst));
    SNF_HIP_CHECK(hipGetLastError());
  }
  return SNF_OK;
}

}  // namespace snf
