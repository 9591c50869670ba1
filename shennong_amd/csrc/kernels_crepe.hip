// CREPE pitch tracker (Kim et al., ICASSP 2018; reference processor/pitch_crepe.py): frame ingest, the six
// convolution blocks and the classifier on the FP32 matrix cores, and the decoders.
//
// Convolution (crepe_conv_kernel): an implicit GEMM Y = epilogue(A W) on the FP32 tile of gemm_tiles.h (block
// 128 x 128 x 32 on v_mfma_f32_32x32x2_f32; the tiling, the LDS layout and the prefetch are described there).
//   * Activations are channels-last, [frame][position][channel].  Output row r = (frame f, position t) of a
//     layer with T positions reads ONE contiguous run of K = width * C_in floats of its frame's block of L
//     floats, from s = (t * stride - pad_left) * C_in on; what falls outside [0, L) is the zero padding.  The A
//     loader therefore takes a base (f L), an offset (s) and a bound (L) per row, computed once per thread for
//     its four rows; the im2col matrix is never written.  Layer 1 is the same with C_in = 1, stride 4, K = 512
//     (offsets are not multiples of 4 floats there: scalar loads); the classifier is T = 1, s = 0, K = L.
//   * W is the Keras kernel [width][1][C_in][C_out] read as a row-major [K x N] matrix: k = tap * C_in + channel,
//     the order of the run above.
//   * Epilogue per element: + bias, ReLU, * scale[c] + shift[c] (the inference form of the batch normalisation,
//     applied AFTER the ReLU as the network does, not folded anywhere: the next layer zero-pads this output, and
//     a negative scale does not commute with the pool), then the maximum over the position pair (2p, 2p + 1).
//     In the accumulator layout a lane holds rows (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) of one column, so
//     the pair is registers reg, reg + 1 of the same lane: the pool costs one v_max and the output is written
//     once, already pooled.  The classifier's epilogue is + bias and the logistic sigmoid.
//   * Summation order, fixed per element: chains of fused multiply-adds over kChain = 256 consecutive k
//     ascending from a zero accumulator (padding adds fma(0, w, acc) = acc), the chains' results added in
//     ascending order.  The value depends on the frame's own samples only, not on the batch or the tiling.
//     One chain over all k (as in bn_dense_kernel) was measured first: at the full model's K = 65 536 its
//     round-off (about sqrt(K) eps times the running sum) was 19.5 times that of float32 numpy on the host.
//
// bfloat16 convolution (crepe_conv_bf16_kernel, blocks 2 to 6 under precision 'bfloat16'): the same implicit
// GEMM on the bfloat16 tile of gemm_tiles.h (block 128 x 128 x 64 on v_mfma_f32_32x32x16_bf16, XCD-contiguous
// workgroup order).
//   * W is the packed image Wt[N][Kp] of bn_pack_bf16_kernel: a B fragment is 16 contiguous bytes.
//   * A is the gather above, 8 consecutive k per load.  C_in is a multiple of 8, so s, k, L and K are too and
//     a fragment lies inside the frame's block as a whole or not at all: one 16-byte load of bfloat16 or two of
//     float32 from a clamped address, then a select (no branch between the loads of a tile).  The source type is
//     a template parameter: float32 is rounded in the loader before the LDS write (to nearest, ties to even:
//     block 2 reading block 1), bfloat16 is copied (blocks 3 to 6, whose producers stored that rounding).
//   * Summation order, fixed per element: chains of kChainBf = 1024 consecutive k (16 k tiles, 64 MFMA steps
//     of 16 k each) from a zero accumulator, the chains' results added in ascending order.  At K = 65 536 that is 64 steps per chain and 64 chains, the
//     two levels in balance; the value depends on the frame's samples and K alone.
//   * Epilogue as above (bias, ReLU, scale and shift, the pool as one v_max over registers r, r + 1, or the
//     sigmoid), all float32; the store is float32 or bfloat16 (to nearest, ties to even) by an argument.
//
// Ingest (crepe_frames_kernel): one workgroup per frame, int16 samples straight from the resident audio (the
// 512 zeros on either side of a centred signal are an index test, no padded copy exists); mean and deviation
// from float64 sums in a fixed order (4 samples per thread ascending, then a binary tree in LDS).
//
// Decoders: row maximum and first argmax (one wave per frame), the 360-state Viterbi smoothing over the
// argmax observations in float64 log domain (one workgroup per utterance, a band of +-11 states, first index
// on ties, back pointers in scratch), the weighted average of cents around the chosen bin, cents to Hertz.
#include <math.h>

#include "snf_internal.h"
#include "device_fft.h"
#include "gemm_tiles.h"

namespace snf {

namespace {

constexpr int kChain = 256;      // k per multiply-add chain of the FP32 kernel (a multiple of kBK)
constexpr int kChainBf = 1024;   // ... of the bfloat16 kernel (a multiple of kQK)

constexpr int kFrame = 1024, kHalf = 512, kBinsOut = 360, kBand = 11, kBandW = 2 * kBand + 1;
// float64 offsets in the decoder's table blob
constexpr int kTabTrans = 0, kTabStart = kBinsOut * kBandW, kTabSame = kTabStart + 1, kTabOther = kTabStart + 2,
              kTabCents = kTabStart + 3;

struct ConvArgs {
  const float* x;
  const float* w;
  const float* b;
  const float* scale;
  const float* shift;
  float* y;
  int64_t M;       // rows: frames * T
  int K, N;
  int T;           // output positions per frame before the pool
  int step;        // floats between the runs of consecutive positions: stride * C_in
  int lead;        // floats of zero padding before position 0's run: pad_left * C_in
  int L;           // floats of one frame's input block
  int flags;       // kConvNorm | kConvPool | kConvSigmoid
  int vec_a, vec_b;
};

__device__ __forceinline__ float crepe_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// The run of a tile row: row r = (frame f, position t) reads from s = t * step - lead on inside the frame's block
template <class Args>
__device__ __forceinline__ void conv_run(const Args& g, int64_t r, int64_t* base, int* s) {
  const int64_t f = r / g.T;
  *base = f * g.L;
  *s = static_cast<int>(r - f * g.T) * g.step - g.lead;
}

// A of the FP32 convolution
struct ConvRuns {
  const ConvArgs& g;
  int64_t base[4];
  int s[4];
  bool ok[4];
  __device__ __forceinline__ ConvRuns(const ConvArgs& g_, const Tile& t) : g(g_) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = t.m0 + t.lr + 32 * i;
      ok[i] = r < g.M;
      base[i] = 0;
      s[i] = -g.lead;
      if (ok[i]) conv_run(g, r, &base[i], &s[i]);
    }
  }
  // 4 consecutive k of tile row i; zeros outside the block, M and K
  __device__ __forceinline__ float4 operator()(int i, int k) const {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!ok[i] || k >= g.K) return v;
    const int p = s[i] + k;
    if (g.vec_a) {   // s, k, L and K are multiples of 4: the four floats are inside together or not at all
      if (p < 0 || p >= g.L) return v;
      return *reinterpret_cast<const float4*>(g.x + base[i] + p);
    }
    float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k + j < g.K && p + j >= 0 && p + j < g.L) t[j] = g.x[base[i] + p + j];
    return make_float4(t[0], t[1], t[2], t[3]);
  }
};

// epilogue of both kernels: bias, ReLU and normalisation or sigmoid, the pool over the row pair, one
// store(index, value) per output
template <class Args, class Store>
__device__ __forceinline__ void conv_epilogue(const Args& g, const Tile& t, const f32x16 (&sum)[2][2], Store&& store) {
  const bool norm = g.flags & kConvNorm, pool = g.flags & kConvPool, sigm = g.flags & kConvSigmoid;
  for_each_owned_pair(t, sum, g.N, [&](int c) __attribute__((always_inline)) {
    const float bias = g.b[c];
    const float sc = norm ? g.scale[c] : 1.0f, sh = norm ? g.shift[c] : 0.0f;
    return [=, &g, &store](int64_t row, float v0, float v1) __attribute__((always_inline)) {
      v0 += bias;
      v1 += bias;
      if (norm) {
        v0 = fmaf(fmaxf(v0, 0.0f), sc, sh);
        v1 = fmaf(fmaxf(v1, 0.0f), sc, sh);
      }
      if (sigm) {
        v0 = crepe_sigmoid(v0);
        v1 = crepe_sigmoid(v1);
      }
      if (pool) {   // (M is even: the pair is inside together)
        if (row < g.M) store((row >> 1) * g.N + c, fmaxf(v0, v1));
      } else {
        if (row < g.M) store(row * g.N + c, v0);
        if (row + 1 < g.M) store((row + 1) * g.N + c, v1);
      }
    };
  });
}

__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) crepe_conv_kernel(const ConvArgs g, int n_tiles_n) {
  const Tile t = tile_of_workgroup<false>(n_tiles_n);
  f32x16 sum[2][2];
  gemm_f32<kChain>(t, ConvRuns(g, t), g.w, g.K, g.N, g.vec_b, sum);
  conv_epilogue(g, t, sum, [&](int64_t at, float v) __attribute__((always_inline)) { g.y[at] = v; });
}

// ---- bfloat16 convolution -------------------------------------------------------------------------------
struct ConvBf16Args {
  const void* x;        // float32 or bfloat16 (the template parameter)
  const uint16_t* wt;   // packed kernel Wt[N][Kp]
  const float* b;
  const float* scale;
  const float* shift;
  void* y;              // float32 or bfloat16 (y_bf16)
  int64_t M;
  int K, Kp, N, T, step, lead, L, flags, y_bf16;
};

// 8 consecutive k of a row, as the loader keeps them until the LDS write; `in`: the run lies inside [0, L) and
// below K, else the LDS write puts zeros
template <bool kSrcBf16>
struct Frag8 {
  float4 lo, hi;
  bool in;
  __device__ __forceinline__ u32x4 bits() const {
    return u32x4{bf16_pack2(lo.x, lo.y), bf16_pack2(lo.z, lo.w), bf16_pack2(hi.x, hi.y), bf16_pack2(hi.z, hi.w)};
  }
};
template <>
struct Frag8<true> {
  u32x4 q;
  bool in;
  __device__ __forceinline__ u32x4 bits() const { return q; }
};

// A of the bfloat16 convolution.  Tile rows beyond M repeat the last one.
template <bool kSrcBf16>
struct ConvRunsBf16 {
  typedef Frag8<kSrcBf16> Frag;
  const ConvBf16Args& g;
  int64_t base[4];
  int s[4];
  __device__ __forceinline__ ConvRunsBf16(const ConvBf16Args& g_, const Tile& t) : g(g_) {
#pragma unroll
    for (int i = 0; i < 4; ++i) conv_run(g, min(t.m0 + t.lr + 32 * i, g.M - 1), &base[i], &s[i]);
  }
  // k .. k + 7 of tile row i, read whole from an address clamped into the block (everything is a multiple of 8).
  // The select waits until the LDS write, so no branch comes between the loads of a tile.
  __device__ __forceinline__ Frag load(int i, int k) const {
    const int p = s[i] + k;
    const int64_t at = base[i] + min(max(p, 0), g.L - 8);
    Frag f;
    f.in = k < g.K && p >= 0 && p < g.L;
    if constexpr (kSrcBf16) {
      f.q = *reinterpret_cast<const u32x4*>(static_cast<const uint16_t*>(g.x) + at);
    } else {
      const float4* src = reinterpret_cast<const float4*>(static_cast<const float*>(g.x) + at);
      f.lo = src[0];
      f.hi = src[1];
    }
    return f;
  }
  __device__ __forceinline__ u32x4 bits(const Frag& f) const { return f.in ? f.bits() : u32x4{0u, 0u, 0u, 0u}; }
};

template <bool kSrcBf16>
__global__ void __launch_bounds__(kThreads, 2) crepe_conv_bf16_kernel(const ConvBf16Args g, int n_tiles_n) {
  const Tile t = tile_of_workgroup<true>(n_tiles_n);
  f32x16 sum[2][2];
  gemm_bf16<kChainBf>(t, ConvRunsBf16<kSrcBf16>(g, t), g.wt, g.K, g.Kp, g.N, sum);
  // the store is in the output's type
  conv_epilogue(g, t, sum, [&](int64_t at, float v) __attribute__((always_inline)) {
    if (g.y_bf16) static_cast<uint16_t*>(g.y)[at] = bf16_rne(v);
    else static_cast<float*>(g.y)[at] = v;
  });
}

// ---- ingest ---------------------------------------------------------------------------------------------
// frames [first, first + count) of the batch, normalised, to out[count x 1024]
__global__ void __launch_bounds__(kThreads) crepe_frames_kernel(const int16_t* __restrict__ wave,
                                                               const int64_t* __restrict__ soff,
                                                               const int64_t* __restrict__ foff, int64_t n_utts,
                                                               int64_t first, int hop, int center,
                                                               float* __restrict__ out) {
  __shared__ double red[kThreads];
  const int64_t g = first + blockIdx.x;
  const int64_t u = find_utt(foff, n_utts, g);
  const int64_t len = soff[u + 1] - soff[u];
  const int64_t start = (g - foff[u]) * hop - (center ? kHalf : 0);
  const int16_t* src = wave + soff[u];
  float x[4];
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t i = start + 4 * threadIdx.x + j;
    x[j] = (i >= 0 && i < len) ? static_cast<float>(src[i]) : 0.0f;
    s += static_cast<double>(x[j]);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const float mean = static_cast<float>(red[0] / kFrame);
  __syncthreads();
  s = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x[j] -= mean;
    s += static_cast<double>(x[j]) * static_cast<double>(x[j]);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const float dev = fmaxf(static_cast<float>(sqrt(red[0] / kFrame)), 1e-8f);
  float4 v = make_float4(x[0] / dev, x[1] / dev, x[2] / dev, x[3] / dev);
  reinterpret_cast<float4*>(out + static_cast<int64_t>(blockIdx.x) * kFrame)[threadIdx.x] = v;
}

// ---- decoders -------------------------------------------------------------------------------------------
// conf[t] = max of row t, obs[t] = its first index (one wave per frame)
__global__ void __launch_bounds__(kThreads) crepe_argmax_kernel(const float* __restrict__ act, int64_t total,
                                                               float* __restrict__ conf, int32_t* __restrict__ obs) {
  const int lane = threadIdx.x & 63;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  if (t >= total) return;   // (whole waves leave together; no barrier below)
  const float* row = act + t * kBinsOut;
  float best = row[lane];
  int arg = lane;
  for (int i = lane + 64; i < kBinsOut; i += 64) {
    const float v = row[i];
    if (v > best) { best = v; arg = i; }
  }
  for (int d = 32; d > 0; d >>= 1) {
    const float ob = __shfl_xor(best, d);
    const int oa = __shfl_xor(arg, d);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  }
  if (lane == 0) {
    conf[t] = best;
    obs[t] = arg;
  }
}

constexpr int kVitThreads = 384;

// path[t] over the frames of one utterance per workgroup; psi: back pointers [total x 360]
__global__ void __launch_bounds__(kVitThreads) crepe_viterbi_kernel(const int32_t* __restrict__ obs,
                                                                   const int64_t* __restrict__ foff,
                                                                   const double* __restrict__ tab,
                                                                   uint16_t* __restrict__ psi,
                                                                   int32_t* __restrict__ path) {
  __shared__ double delta[2][kBinsOut];
  const int64_t f0 = foff[blockIdx.x], F = foff[blockIdx.x + 1] - f0;
  if (F <= 0) return;
  const int j = threadIdx.x;
  const bool live = j < kBinsOut;
  const double e_same = tab[kTabSame], e_other = tab[kTabOther];
  double trans[kBandW];
  if (live) {
#pragma unroll
    for (int d = 0; d < kBandW; ++d) trans[d] = tab[kTabTrans + j * kBandW + d];   // log A[j - 11 + d][j]
    delta[0][j] = __dadd_rn(tab[kTabStart], obs[f0] == j ? e_same : e_other);
  }
  __syncthreads();
  for (int64_t t = 1; t < F; ++t) {
    const double* prev = delta[(t - 1) & 1];
    if (live) {
      double best = -INFINITY;
      int arg = 0;
      bool any = false;
#pragma unroll
      for (int d = 0; d < kBandW; ++d) {
        const int i = j - kBand + d;
        if (i < 0 || i >= kBinsOut) continue;
        const double v = __dadd_rn(prev[i], trans[d]);
        if (!any || v > best) { best = v; arg = i; any = true; }
      }
      delta[t & 1][j] = __dadd_rn(best, obs[f0 + t] == j ? e_same : e_other);
      psi[(f0 + t) * kBinsOut + j] = static_cast<uint16_t>(arg);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double* last = delta[(F - 1) & 1];
    int state = 0;
    for (int i = 1; i < kBinsOut; ++i)
      if (last[i] > last[state]) state = i;
    path[f0 + F - 1] = state;
    for (int64_t t = F - 1; t > 0; --t) {
      state = psi[(f0 + t) * kBinsOut + state];
      path[f0 + t - 1] = state;
    }
  }
}

// out[t] = (confidence, 10 * 2^(cents / 1200)) with cents the weighted average over bins [c - 4, c + 5)
__global__ void __launch_bounds__(kThreads) crepe_cents_kernel(const float* __restrict__ act,
                                                              const float* __restrict__ conf,
                                                              const int32_t* __restrict__ centre,
                                                              const double* __restrict__ tab, int64_t total,
                                                              double* __restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (t >= total) return;
  const int c = centre[t];
  const int a = max(0, c - 4), b = min(kBinsOut, c + 5);
  double ps = 0.0, ws = 0.0;
  for (int i = a; i < b; ++i) {
    const double v = static_cast<double>(act[t * kBinsOut + i]);
    ps = __dadd_rn(ps, __dmul_rn(v, tab[kTabCents + i]));
    ws = __dadd_rn(ws, v);
  }
  const double hz = 10.0 * exp2(ps / ws / 1200.0);
  out[2 * t] = static_cast<double>(conf[t]);
  out[2 * t + 1] = isnan(hz) ? 0.0 : hz;
}

unsigned blocks(int64_t n, int64_t per) { return static_cast<unsigned>((n + per - 1) / per); }

}  // namespace

int crepe_table_doubles() { return kTabCents + kBinsOut; }

int launch_crepe_conv(const float* x, int64_t frames, int T, int step, int lead, int L, int K, const float* w,
                      const float* b, const float* scale, const float* shift, int N, int flags, float* y,
                      hipStream_t stream) {
  if (frames <= 0) return SNF_OK;
  ConvArgs g;
  g.x = x; g.w = w; g.b = b; g.scale = scale; g.shift = shift; g.y = y;
  g.M = frames * T; g.K = K; g.N = N; g.T = T; g.step = step; g.lead = lead; g.L = L; g.flags = flags;
  g.vec_a = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && K % 4 == 0 && L % 4 == 0 && step % 4 == 0 && lead % 4 == 0;
  g.vec_b = (reinterpret_cast<uintptr_t>(w) & 15) == 0 && N % 4 == 0;
  unsigned grid;
  int tiles_n;
  if (int rc = gemm_tile_grid(g.M, N, "crepe: too many tiles for one launch", &grid, &tiles_n)) return rc;
  hipLaunchKernelGGL(crepe_conv_kernel, dim3(grid), dim3(kThreads), 0, stream, g, tiles_n);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_crepe_conv_bf16(const void* x, int x_bf16, int64_t frames, int T, int step, int lead, int L, int K,
                           const uint16_t* wt, const float* b, const float* scale, const float* shift, int N,
                           int flags, void* y, int y_bf16, hipStream_t stream) {
  if (frames <= 0) return SNF_OK;
  if (step % 8 || lead % 8 || L % 8 || K % 8 || L < 8 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wt)) & 15))
    return set_error(SNF_E_INVALID, "crepe: the bfloat16 convolution needs multiples of 8 channels and 16-byte aligned operands");
  ConvBf16Args g;
  g.x = x; g.wt = wt; g.b = b; g.scale = scale; g.shift = shift; g.y = y;
  g.M = frames * T; g.K = K; g.Kp = bn_bf16_padded_k(K); g.N = N; g.T = T; g.step = step; g.lead = lead; g.L = L;
  g.flags = flags; g.y_bf16 = y_bf16;
  unsigned grid;
  int tiles_n;
  if (int rc = gemm_tile_grid(g.M, N, "crepe: too many tiles for one launch", &grid, &tiles_n)) return rc;
  hipLaunchKernelGGL(x_bf16 ? crepe_conv_bf16_kernel<true> : crepe_conv_bf16_kernel<false>, dim3(grid), dim3(kThreads),
                     0, stream, g, tiles_n);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_crepe_frames(const int16_t* wave, const int64_t* soff, const int64_t* foff, int64_t n_utts, int64_t first,
                        int64_t count, int hop, int center, float* out, hipStream_t stream) {
  if (count <= 0) return SNF_OK;
  hipLaunchKernelGGL(crepe_frames_kernel, dim3(static_cast<unsigned>(count)), dim3(kThreads), 0, stream, wave, soff,
                     foff, n_utts, first, hop, center, out);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_crepe_decode(const float* act, const int64_t* foff, int64_t n_utts, int64_t total, int viterbi,
                        const double* tab, float* conf, uint16_t* psi, int32_t* bins, double* out,
                        hipStream_t stream) {
  if (total <= 0) return SNF_OK;
  int32_t* obs = bins;
  int32_t* path = bins + total;
  hipLaunchKernelGGL(crepe_argmax_kernel, dim3(blocks(total, kThreads / 64)), dim3(kThreads), 0, stream, act, total,
                     conf, obs);
  SNF_HIP_CHECK(hipGetLastError());
  if (viterbi) {
    hipLaunchKernelGGL(crepe_viterbi_kernel, dim3(static_cast<unsigned>(n_utts)), dim3(kVitThreads), 0, stream, obs,
                       foff, tab, psi, path);
    SNF_HIP_CHECK(hipGetLastError());
  } else {
    SNF_HIP_CHECK(hipMemcpyAsync(path, obs, sizeof(int32_t) * total, hipMemcpyDeviceToDevice, stream));
  }
  hipLaunchKernelGGL(crepe_cents_kernel, dim3(blocks(total, kThreads)), dim3(kThreads), 0, stream, act, conf, path,
                     tab, total, out);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
