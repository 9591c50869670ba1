// BUT/Phonexia bottleneck feature extractor (reference processor/bottleneck.py:403-764): voice activity
// detection, the HTK log-mel front end, the Hamming-DCT context projection and the two stacked networks.
//
// Dense layer (bn_dense_kernel): Y = act(A W + b), float32 row-major, on the FP32 tile of gemm_tiles.h (block
// 128 x 128 x 32 on v_mfma_f32_32x32x2_f32; the tiling, the LDS layout and the prefetch are described there).
//   * Every output element is ONE chain of fused multiply-adds over k ascending from a zero accumulator
//     (the MFMA is bit for bit that chain), bias added last, then the activation.  The chain of an element
//     reads its own A row and W column only: the value does not depend on M, on the row's place in the
//     batch or on the tiling.  Zero padding beyond K adds fma(0, 0, acc) = acc.
//   * Row gather: with `a_row` the A operand is a virtual matrix, A[r][k] = X[a_row[r] + gs (k / gw)][k % gw]
//     over rows of width gw: the five-frame stack of the second network (gw = 80, gs = 5) is read straight
//     from the first network's output and never written to memory.
//
// bfloat16 dense layer (bn_dense_bf16_kernel): Y = act(bf16(A) bf16(W) + b) on the bfloat16 tile of gemm_tiles.h
// (block 128 x 128 x 64 on v_mfma_f32_32x32x16_bf16, XCD-contiguous workgroup order), for the layers that read
// sigmoid outputs (W2, W3, W6, W7).  A and Y are float32 in memory, the sums float32, one chain over all k.
//   * Weight image (bn_pack_bf16_kernel, once per network): Wt[n][kp] bfloat16, k-contiguous per output column,
//     kp = K rounded up to the k tile of 64 and zero beyond K.
//   * Rounding: to nearest, ties to even, by v_cvt_pk_bf16_f32 (a NaN stays a NaN), for A in the loader before
//     the LDS write and for W in the pack kernel, so operands that were rounded beforehand give the same bits.
//     (The same rounding in integer arithmetic, about 7 instructions per element, was measured 10 % slower on the
//     square layer at 1500.)
//   * A is prefetched as 8 float4 per thread and k tile; tile rows beyond M repeat the last valid one.
//   * An element's value depends on its A row, its W column and K only (the MFMA's fixed summation order over
//     the 16 k of a step, steps ascending), not on M, the row's place or the tiling: batch invariance as above.
//
// Front end (bn_fbank_kernel): 16 lanes per frame, 16 frames per workgroup.  200 samples (+ uniform dither
// keyed by utterance and sample index), Hamming window, zero-extended to 256, complex 16 x 16 FFT (two
// register fft16 around one LDS transpose), power of bins 0..128, 24 filters from the host-built table,
// log(max(1, .)).
//
// VAD (bn_vad_kernel): one workgroup per utterance.  int16-wrapped squares summed per frame in int64,
// then float64 throughout: standardisation and five EM passes of the 1-D 3-component GMM, every sum a
// fixed-order reduction (strided partials ascending, then a binary tree in LDS).  No atomics.
//
// Status (bn_status_kernel, the last launch of snf_bottleneck_extract): one workgroup per utterance reads the
// voiced count and the utterance's output rows where the last layer put them and writes one word - bit 0 no voiced
// frame, bit 1 a value that is not finite - so that the one-call extractor needs no host round trip between its
// stages: the host reads the words after the call's only wait.
#include <math.h>

#include "snf_internal.h"
#include "device_fft.h"
#include "gemm_tiles.h"

namespace snf {

namespace {

struct DenseArgs {
  const float* x;
  const float* w;
  const float* b;
  float* y;
  int64_t M;
  int K, N, act;
  const int64_t* a_row;  // gather: first source row of every A row, or nullptr
  int gw, gs;            // gather: source row width and row step per block of gw columns
  int vec_a, vec_b;      // 16-byte loads allowed
};

__device__ __forceinline__ float bn_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// A of the FP32 layer: plain or gathered rows
struct DenseRows {
  const DenseArgs& g;
  int64_t src[4];   // source base row of this thread's four tile rows
  bool ok[4];
  __device__ __forceinline__ DenseRows(const DenseArgs& g_, const Tile& t) : g(g_) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = t.m0 + t.lr + 32 * i;
      ok[i] = r < g.M;
      src[i] = ok[i] ? (g.a_row ? g.a_row[r] : r) : 0;
    }
  }
  // 4 consecutive k of tile row i, zeros outside M and K
  __device__ __forceinline__ float4 operator()(int i, int k) const {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!ok[i] || k >= g.K) return v;
    if (g.a_row) {
      if (g.vec_a) {
        const int blk = k / g.gw, c = k - blk * g.gw;
        return *reinterpret_cast<const float4*>(g.x + (src[i] + static_cast<int64_t>(g.gs) * blk) * g.gw + c);
      }
      float t[4] = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < 4; ++j) {
        const int kk = k + j;
        if (kk < g.K) {
          const int blk = kk / g.gw, c = kk - blk * g.gw;
          t[j] = g.x[(src[i] + static_cast<int64_t>(g.gs) * blk) * g.gw + c];
        }
      }
      return make_float4(t[0], t[1], t[2], t[3]);
    }
    const float* p = g.x + src[i] * g.K + k;
    if (g.vec_a) return *reinterpret_cast<const float4*>(p);
    v.x = p[0];
    if (k + 1 < g.K) v.y = p[1];
    if (k + 2 < g.K) v.z = p[2];
    if (k + 3 < g.K) v.w = p[3];
    return v;
  }
};

// epilogue of both layers: bias, activation, one store per element
__device__ __forceinline__ void dense_epilogue(const Tile& t, const f32x16 (&acc)[2][2], const float* b, int act,
                                               float* y, int64_t M, int N) {
  for_each_owned_pair(t, acc, N, [&](int c) __attribute__((always_inline)) {
    const float bias = b[c];
    auto one = [=](int64_t row, float v) __attribute__((always_inline)) {
      if (row >= M) return;
      v += bias;
      if (act) v = bn_sigmoid(v);
      y[row * N + c] = v;
    };
    return [=](int64_t row, float v0, float v1) __attribute__((always_inline)) {
      one(row, v0);
      one(row + 1, v1);
    };
  });
}

__global__ void __launch_bounds__(kThreads) bn_dense_kernel(const DenseArgs g, int n_tiles_n) {
  const Tile t = tile_of_workgroup<false>(n_tiles_n);
  f32x16 acc[2][2];
  gemm_f32<0>(t, DenseRows(g, t), g.w, g.K, g.N, g.vec_b, acc);
  dense_epilogue(t, acc, g.b, g.act, g.y, g.M, g.N);
}

// ---- bfloat16 dense layer -------------------------------------------------------------------------------
struct DenseBf16Args {
  const float* x;
  const uint16_t* wt;   // packed weights Wt[N][Kp]
  const float* b;
  float* y;
  int64_t M;
  int K, Kp, N, act;
};

// A of the bfloat16 layer: float32 rows, rounded at the LDS write.  kVec (K a multiple of 4, x 16-byte aligned):
// unconditional 16-byte loads from a clamped address and a select, so that no branch separates the loads of a tile
template <bool kVec>
struct DenseRowsBf16 {
  struct Frag { float4 lo, hi; };
  const DenseBf16Args& g;
  int64_t row[4];   // tile rows beyond M repeat the last one
  __device__ __forceinline__ DenseRowsBf16(const DenseBf16Args& g_, const Tile& t) : g(g_) {
#pragma unroll
    for (int i = 0; i < 4; ++i) row[i] = min(t.m0 + t.lr + 32 * i, g.M - 1);
  }
  // 4 consecutive k of row r (< M) of x, zeros outside K
  __device__ __forceinline__ float4 load_q4(int64_t r, int k) const {
    if (kVec) {
      const float4 v = *reinterpret_cast<const float4*>(g.x + r * g.K + min(k, g.K - 4));
      return k < g.K ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k >= g.K) return v;
    const float* p = g.x + r * g.K + k;
    v.x = p[0];
    if (k + 1 < g.K) v.y = p[1];
    if (k + 2 < g.K) v.z = p[2];
    if (k + 3 < g.K) v.w = p[3];
    return v;
  }
  __device__ __forceinline__ Frag load(int i, int k) const {
    return Frag{load_q4(row[i], k), load_q4(row[i], k + 4)};
  }
  __device__ __forceinline__ u32x4 bits(const Frag& f) const {
    return u32x4{bf16_pack2(f.lo.x, f.lo.y), bf16_pack2(f.lo.z, f.lo.w), bf16_pack2(f.hi.x, f.hi.y),
                 bf16_pack2(f.hi.z, f.hi.w)};
  }
};

template <bool kVec>
__global__ void __launch_bounds__(kThreads, 3) bn_dense_bf16_kernel(const DenseBf16Args g, int n_tiles_n) {
  const Tile t = tile_of_workgroup<true>(n_tiles_n);
  f32x16 acc[2][2];
  gemm_bf16<0>(t, DenseRowsBf16<kVec>(g, t), g.wt, g.K, g.Kp, g.N, acc);
  dense_epilogue(t, acc, g.b, g.act, g.y, g.M, g.N);
}

// wt[n][k] = bfloat16(w[k][n]) for k < K, 0 for K <= k < Kp: 32 x 32 tiles transposed through LDS
__global__ void __launch_bounds__(kThreads) bn_pack_bf16_kernel(const float* __restrict__ w, int K, int N, int Kp,
                                                               uint16_t* __restrict__ wt) {
  __shared__ uint16_t tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int k0 = static_cast<int>(blockIdx.x) * 32, n0 = static_cast<int>(blockIdx.y) * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = k0 + ty + 8 * i, n = n0 + tx;
    tile[ty + 8 * i][tx] = (k < K && n < N) ? bf16_rne(w[static_cast<int64_t>(k) * N + n]) : uint16_t(0);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + ty + 8 * i, k = k0 + tx;
    if (n < N && k < Kp) wt[static_cast<int64_t>(n) * Kp + k] = tile[tx][ty + 8 * i];
  }
}

// a_row[r] = in_off[u] + (r - out_off[u]) for the utterance u of output row r
__global__ void __launch_bounds__(kThreads) bn_row_map_kernel(const int64_t* __restrict__ in_off,
                                                             const int64_t* __restrict__ out_off, int64_t n_utts,
                                                             int64_t rows, int64_t* __restrict__ a_row) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (r >= rows) return;
  const int64_t u = find_utt(out_off, n_utts, r);
  a_row[r] = in_off[u] + (r - out_off[u]);
}

// ---- front end ------------------------------------------------------------------------------------------
constexpr int kWin = 200, kShift = 80, kFft = 256, kBins = 129, kMel = 24, kBases = 6, kEdge = 15;
constexpr int kFramesPerBlock = 16;
constexpr int kTabWindow = 0, kTabTw = kWin, kTabMel = kWin + 2 * kFft;   // float offsets in the table blob

// uniform in [-1, 1) for sample `i` of the utterance with noise word `word`
__device__ __forceinline__ float bn_uniform(uint32_t word, uint64_t seed, int64_t i) {
  uint32_t h = fmix32(static_cast<uint32_t>(i) * 0x9E3779B1u + static_cast<uint32_t>(seed));
  h = fmix32(h ^ word ^ static_cast<uint32_t>(static_cast<uint64_t>(i) >> 32) ^ static_cast<uint32_t>(seed >> 32));
  return static_cast<float>(h >> 8) * (1.0f / 8388608.0f) - 1.0f;
}

__global__ void __launch_bounds__(kThreads) bn_fbank_kernel(const int16_t* __restrict__ wave,
                                                           const int64_t* __restrict__ soff,
                                                           const int64_t* __restrict__ foff, int64_t n_utts,
                                                           int64_t total_frames, const float* __restrict__ tables,
                                                           float dither, uint64_t seed,
                                                           const uint32_t* __restrict__ utt_noise,
                                                           float* __restrict__ out) {
  __shared__ float2 tile[kFramesPerBlock][16 * 17];
  __shared__ float power[kFramesPerBlock][kBins + 3];
  __shared__ float mel[kBins * kMel];
  for (int i = threadIdx.x; i < kBins * kMel; i += kThreads) mel[i] = tables[kTabMel + i];
  const int fl = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int64_t g_raw = static_cast<int64_t>(blockIdx.x) * kFramesPerBlock + fl;
  const bool live = g_raw < total_frames;
  const int64_t g = live ? g_raw : total_frames - 1;
  const int64_t u = find_utt(foff, n_utts, g);
  const int64_t first = 80 * (g - foff[u]);          // first sample of the frame inside the utterance
  const int16_t* src = wave + soff[u] + first;
  const uint32_t word = dither != 0.0f ? utt_noise[u] : 0u;
  float2 v[16];
#pragma unroll
  for (int n1 = 0; n1 < 16; ++n1) {
    const int n = 16 * n1 + l;
    float s = 0.0f;
    if (n < kWin) {
      s = static_cast<float>(src[n]);
      if (dither != 0.0f) s += dither * bn_uniform(word, seed, first + n);
      s *= tables[kTabWindow + n];
    }
    v[n1] = make_float2(s, 0.0f);
  }
  fft16(v);   // over n1 -> k1
  const float2* tw = reinterpret_cast<const float2*>(tables + kTabTw);
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) tile[fl][k1 * 17 + l] = cmul(v[k1], tw[l * k1]);
  __syncthreads();
#pragma unroll
  for (int n2 = 0; n2 < 16; ++n2) v[n2] = tile[fl][l * 17 + n2];
  fft16(v);   // over n2 -> k2: v[k2] = X[l + 16 k2]
#pragma unroll
  for (int k2 = 0; k2 <= 8; ++k2) {
    const int k = l + 16 * k2;
    if (k < kBins) power[fl][k] = v[k2].x * v[k2].x + v[k2].y * v[k2].y;
  }
  __syncthreads();
  for (int j = l; j < kMel; j += 16) {
    float acc = 0.0f;
    for (int k = 0; k < kBins; ++k) acc = fmaf(power[fl][k], mel[k * kMel + j], acc);
    if (live) out[g * kMel + j] = logf(fmaxf(1.0f, acc));
  }
}

// ---- VAD ------------------------------------------------------------------------------------------------
// sum of v[0 .. n) over the workgroup, n <= 9, result in v of every thread; fixed binary tree
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* red) {
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) red[i * kThreads + threadIdx.x] = v[i];
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
#pragma unroll
      for (int i = 0; i < N; ++i) red[i * kThreads + threadIdx.x] += red[i * kThreads + threadIdx.x + w];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = red[i * kThreads];
}

struct Gmm3 {
  double inv_c[3], inv_cm[3], gconst[3];
};

__device__ __forceinline__ bool gmm3_prep(const double (&w)[3], const double (&m)[3], const double (&c)[3], Gmm3* g) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ok = ok && w[i] > 0.0 && c[i] > 0.0 && isfinite(w[i]) && isfinite(m[i]) && isfinite(c[i]);
    g->inv_c[i] = 1.0 / c[i];
    g->inv_cm[i] = g->inv_c[i] * m[i];
    g->gconst[i] = log(w[i]) - 0.5 * (log(c[i]) + m[i] * m[i] * g->inv_c[i] + 1.8378770664093453);
  }
  return ok;
}

// posteriors of the three components for the value e
__device__ __forceinline__ void gmm3_post(const Gmm3& g, double e, double (&p)[3]) {
  double gm[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) gm[i] = -0.5 * e * e * g.inv_c[i] + e * g.inv_cm[i] + g.gconst[i];
  const double mx = fmax(gm[0], fmax(gm[1], gm[2]));
  const double llh = mx + log(exp(gm[0] - mx) + exp(gm[1] - mx) + exp(gm[2] - mx));
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = exp(gm[i] - llh);
}

__global__ void __launch_bounds__(kThreads) bn_vad_kernel(const int16_t* __restrict__ wave,
                                                         const int64_t* __restrict__ soff,
                                                         const int64_t* __restrict__ foff,
                                                         double* __restrict__ energy, uint8_t* __restrict__ mask,
                                                         int32_t* __restrict__ voiced) {
  __shared__ double red[9 * kThreads];
  const int64_t u = blockIdx.x;
  const int64_t f0 = foff[u], F = foff[u + 1] - f0;
  const int16_t* src = wave + soff[u];
  double* E = energy + f0;
  if (F <= 0) {
    if (threadIdx.x == 0) voiced[u] = 0;
    return;
  }
  double s1[1] = {0.0};
  for (int64_t f = threadIdx.x; f < F; f += kThreads) {
    long long e = 0;
    for (int n = 0; n < kWin; ++n) {
      const int s = src[kShift * f + n];
      e += static_cast<int16_t>(static_cast<uint32_t>(s * s) & 0xFFFFu);   // the square wraps to int16
    }
    E[f] = static_cast<double>(e);
    s1[0] += static_cast<double>(e);
  }
  block_sum(s1, red);
  const double mean = s1[0] / static_cast<double>(F);
  double s2[1] = {0.0};
  for (int64_t f = threadIdx.x; f < F; f += kThreads) {
    const double e = E[f] - mean;
    E[f] = e;
    s2[0] += e;
  }
  block_sum(s2, red);
  const double mean2 = s2[0] / static_cast<double>(F);   // (numpy's std() takes the mean again)
  double s3[1] = {0.0};
  for (int64_t f = threadIdx.x; f < F; f += kThreads) {
    const double d = E[f] - mean2;
    s3[0] += d * d;
  }
  block_sum(s3, red);
  const double sd = sqrt(s3[0] / static_cast<double>(F));
  bool ok = sd > 0.0 && isfinite(sd);
  double w[3] = {0.33, 0.33, 0.33}, m[3] = {-1.0, 0.0, 1.0}, c[3] = {1.0, 1.0, 1.0};
  Gmm3 g;
  if (ok) {
    for (int64_t f = threadIdx.x; f < F; f += kThreads) E[f] = E[f] / sd;
    ok = gmm3_prep(w, m, c, &g);
  }
  for (int it = 0; it < 5 && ok; ++it) {   // (ok is uniform over the workgroup)
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t f = threadIdx.x; f < F; f += kThreads) {
      const double e = E[f];
      double p[3];
      gmm3_post(g, e, p);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        acc[i] += p[i];
        acc[3 + i] += p[i] * e;
        acc[6 + i] += p[i] * e * e;
      }
    }
    block_sum(acc, red);
    const double total = acc[0] + acc[1] + acc[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ok = ok && acc[i] > 0.0;
      w[i] = acc[i] / total;
      m[i] = acc[3 + i] / acc[i];
      c[i] = acc[6 + i] / acc[i] - m[i] * m[i];
    }
    ok = ok && gmm3_prep(w, m, c, &g);
  }
  double cnt[1] = {0.0};
  for (int64_t f = threadIdx.x; f < F; f += kThreads) {
    bool v = false;
    if (ok) {
      double p[3];
      gmm3_post(g, E[f], p);
      v = p[0] < 0.3;
    }
    mask[f0 + f] = v ? 1 : 0;
    cnt[0] += v ? 1.0 : 0.0;
  }
  block_sum(cnt, red);
  if (threadIdx.x == 0) voiced[u] = static_cast<int32_t>(cnt[0]);
}

// ---- voiced mean and context projection -----------------------------------------------------------------
// mean[u][band] over the voiced frames of utterance u (float64 sums in a fixed order; 0 without voiced frames)
__global__ void __launch_bounds__(192) bn_voiced_mean_kernel(const float* __restrict__ logmel,
                                                            const uint8_t* __restrict__ mask,
                                                            const int32_t* __restrict__ voiced,
                                                            const int64_t* __restrict__ foff,
                                                            float* __restrict__ mean) {
  __shared__ double part[8][kMel];
  const int64_t u = blockIdx.x;
  const int64_t f0 = foff[u], F = foff[u + 1] - f0;
  const int p = threadIdx.x / kMel, b = threadIdx.x % kMel;
  double s = 0.0;
  for (int64_t f = p; f < F; f += 8)
    if (mask[f0 + f]) s += static_cast<double>(logmel[(f0 + f) * kMel + b]);
  part[p][b] = s;
  __syncthreads();
  if (p == 0) {
    double t = 0.0;
    for (int q = 0; q < 8; ++q) t += part[q][b];
    const int n = voiced[u];
    mean[u * kMel + b] = n > 0 ? static_cast<float>(t / static_cast<double>(n)) : 0.0f;
  }
}

constexpr int kMaxContext = 64;

// x[row][band * 6 + j] = sum_t hd[t][j] * (fea[clamp(row + t - 15)][band] - mean[band]), t <= 2 context
__global__ void __launch_bounds__(kThreads) bn_nn_input_kernel(const float* __restrict__ logmel,
                                                              const float* __restrict__ mean,
                                                              const int64_t* __restrict__ foff,
                                                              const int64_t* __restrict__ roff, int64_t n_utts,
                                                              int64_t total_rows, int context,
                                                              const float* __restrict__ hd, float* __restrict__ x) {
  __shared__ float hs[(2 * kMaxContext + 1) * kBases];
  const int taps = 2 * context + 1;
  for (int i = threadIdx.x; i < taps * kBases; i += kThreads) hs[i] = hd[i];
  __syncthreads();
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= total_rows * kMel) return;
  const int64_t row = e / kMel;
  const int band = static_cast<int>(e % kMel);
  const int64_t u = find_utt(roff, n_utts, row);
  const int64_t r = row - roff[u], f0 = foff[u], F = foff[u + 1] - f0;
  const float mu = mean[u * kMel + band];
  float acc[kBases] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < taps; ++t) {
    int64_t f = r + t - kEdge;
    f = f < 0 ? 0 : (f > F - 1 ? F - 1 : f);
    const float v = logmel[(f0 + f) * kMel + band] - mu;
#pragma unroll
    for (int j = 0; j < kBases; ++j) acc[j] = fmaf(v, hs[t * kBases + j], acc[j]);
  }
  float* dst = x + row * (kMel * kBases) + band * kBases;
#pragma unroll
  for (int j = 0; j < kBases; ++j) dst[j] = acc[j];
}

// ---- status word of the one-call extractor --------------------------------------------------------------
// status[u] = (voiced[u] == 0) | 2 (some value of the utterance's output rows is not finite).  One workgroup per
// utterance; rows out_start[u] .. + (ooff[u + 1] - ooff[u]) of `out`.  Each wave folds its lanes' flags with one
// ballot, the four waves meet in LDS and one lane stores the word: no atomics.
__global__ void __launch_bounds__(kThreads) bn_status_kernel(const int32_t* __restrict__ voiced,
                                                            const float* __restrict__ out,
                                                            const int64_t* __restrict__ out_start,
                                                            const int64_t* __restrict__ ooff,
                                                            int32_t* __restrict__ status) {
  __shared__ int wave_bad[kThreads / 64];
  const int64_t u = blockIdx.x;
  const int64_t n = (ooff[u + 1] - ooff[u]) * 80;
  const float* src = out + out_start[u] * 80;
  bool bad = false;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) bad = bad || !isfinite(src[i]);
  const bool any = __ballot(bad) != 0ull;
  if ((threadIdx.x & 63) == 0) wave_bad[threadIdx.x >> 6] = any ? 1 : 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    int b = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) b |= wave_bad[w];
    status[u] = (voiced[u] == 0 ? 1 : 0) | (b ? 2 : 0);
  }
}

unsigned blocks(int64_t n, int64_t per) { return static_cast<unsigned>((n + per - 1) / per); }

}  // namespace

int launch_bn_status(const int32_t* voiced, const float* out, const int64_t* out_start, const int64_t* ooff,
                     int64_t n_utts, int32_t* status, hipStream_t stream) {
  if (n_utts <= 0) return SNF_OK;
  hipLaunchKernelGGL(bn_status_kernel, dim3(static_cast<unsigned>(n_utts)), dim3(kThreads), 0, stream, voiced, out,
                     out_start, ooff, status);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int bn_table_floats() { return kWin + 2 * kFft + kBins * kMel; }
int bn_max_context() { return kMaxContext; }

int launch_bn_dense(const float* x, int64_t M, int K, const float* w, const float* b, int N, int act, float* y,
                    const int64_t* a_row, int gw, int gs, hipStream_t stream) {
  if (M <= 0) return SNF_OK;
  DenseArgs g;
  g.x = x; g.w = w; g.b = b; g.y = y; g.M = M; g.K = K; g.N = N; g.act = act;
  g.a_row = a_row; g.gw = gw; g.gs = gs;
  const bool x16 = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  g.vec_a = x16 && (a_row ? (gw % 4 == 0 && K % 4 == 0) : K % 4 == 0);
  g.vec_b = (reinterpret_cast<uintptr_t>(w) & 15) == 0 && N % 4 == 0;
  unsigned grid;
  int tiles_n;
  if (int rc = gemm_tile_grid(M, N, "dense layer: too many tiles for one launch", &grid, &tiles_n)) return rc;
  hipLaunchKernelGGL(bn_dense_kernel, dim3(grid), dim3(kThreads), 0, stream, g, tiles_n);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int bn_bf16_padded_k(int K) { return (K + kQK - 1) / kQK * kQK; }

int launch_bn_pack_bf16(const float* w, int K, int N, uint16_t* wt, hipStream_t stream) {
  const int Kp = bn_bf16_padded_k(K);
  hipLaunchKernelGGL(bn_pack_bf16_kernel, dim3(blocks(Kp, 32), blocks(N, 32)), dim3(kThreads), 0, stream, w, K, N, Kp,
                     wt);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_bn_dense_bf16(const float* x, int64_t M, int K, const uint16_t* wt, const float* b, int N, int act,
                         float* y, hipStream_t stream) {
  if (M <= 0) return SNF_OK;
  DenseBf16Args g;
  g.x = x; g.wt = wt; g.b = b; g.y = y; g.M = M; g.K = K; g.Kp = bn_bf16_padded_k(K); g.N = N; g.act = act;
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && K % 4 == 0;
  unsigned grid;
  int tiles_n;
  if (int rc = gemm_tile_grid(M, N, "dense layer: too many tiles for one launch", &grid, &tiles_n)) return rc;
  hipLaunchKernelGGL(vec ? bn_dense_bf16_kernel<true> : bn_dense_bf16_kernel<false>, dim3(grid), dim3(kThreads), 0,
                     stream, g, tiles_n);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_bn_row_map(const int64_t* in_off, const int64_t* out_off, int64_t n_utts, int64_t rows, int64_t* a_row,
                      hipStream_t stream) {
  if (rows <= 0) return SNF_OK;
  hipLaunchKernelGGL(bn_row_map_kernel, dim3(blocks(rows, kThreads)), dim3(kThreads), 0, stream, in_off, out_off,
                     n_utts, rows, a_row);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_bn_fbank(const int16_t* wave, const int64_t* soff, const int64_t* foff, int64_t n_utts,
                    int64_t total_frames, const float* tables, float dither, uint64_t seed, uint32_t* utt_noise,
                    float* out, hipStream_t stream) {
  if (total_frames <= 0) return SNF_OK;
  if (dither != 0.0f) {
    BatchArgs b{};
    b.wave = wave;
    b.sample_offsets = soff;
    b.n_utts = n_utts;
    int rc = launch_build_utt_noise(b, utt_noise, stream);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(bn_fbank_kernel, dim3(blocks(total_frames, kFramesPerBlock)), dim3(kThreads), 0, stream, wave,
                     soff, foff, n_utts, total_frames, tables, dither, seed, utt_noise, out);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_bn_vad(const int16_t* wave, const int64_t* soff, const int64_t* foff, int64_t n_utts, double* energy,
                  uint8_t* mask, int32_t* voiced, hipStream_t stream) {
  if (n_utts <= 0) return SNF_OK;
  hipLaunchKernelGGL(bn_vad_kernel, dim3(static_cast<unsigned>(n_utts)), dim3(kThreads), 0, stream, wave, soff, foff,
                     energy, mask, voiced);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_bn_nn_input(const float* logmel, const uint8_t* mask, const int32_t* voiced, const int64_t* foff,
                       const int64_t* roff, int64_t n_utts, int64_t total_rows, int context, const float* hd,
                       float* mean, float* x, hipStream_t stream) {
  if (n_utts <= 0 || total_rows <= 0) return SNF_OK;
  hipLaunchKernelGGL(bn_voiced_mean_kernel, dim3(static_cast<unsigned>(n_utts)), dim3(192), 0, stream, logmel, mask,
                     voiced, foff, mean);
  SNF_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(bn_nn_input_kernel, dim3(blocks(total_rows * kMel, kThreads)), dim3(kThreads), 0, stream, logmel,
                     mean, foff, roff, n_utts, total_rows, context, hd, x);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
