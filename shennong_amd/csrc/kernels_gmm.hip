// Diagonal-covariance GMM kernels (reference processor/ubm.py -> [KALDI-UPSTREAM] gmm/diag-gmm.cc
// DiagGmm::LogLikelihoods / GaussianSelection / GaussianSelectionPreselect / LogLikelihoodsPreselect,
// gmm/mle-diag-gmm.cc AccumDiagGmm::AccumulateFromDiag / AccumulateFromPosteriors).
//
// Model in Kaldi's natural form, float32 row-major: gconsts[C], means_invvars[C x D], inv_vars[C x D].
// Frames x[F x D] float32.  The log-likelihood of frame f under Gaussian c is one GEMM plus a broadcast:
//
//   L[f,c] = gconsts[c] + sum_k X[f,k] * W[c,k],   X = [x | x*x],  W = [means_invvars | -0.5*inv_vars]
//
// with K = 2D padded with zeros to Kp = round_up(2D, 4).  EVERY entry point computes L the same way:
// the operands are xop() / wop() below, the product is a chain of v_mfma_f32_16x16x4_f32 over k ascending
// from a zero accumulator (ll_step), and gconst is added last (ll_finish).  An output element of an MFMA
// depends on its own A row and B column only, so the dense kernels (frames x Gaussians tiles staged in LDS)
// and the gathered kernel (one frame against a list of Gaussians, operands straight from memory) produce
// the same bits for the same (f, c).  tests/test_ubm_gpu.py checks that through gselect (n = C) and the
// log-sum-exps of gselect / accumulate against the downloaded L.
//
// MFMA 16x16x4 f32 (exact f32, the FP32 vector rate, MI355X_MICROARCH "Matrix cores"): lane l supplies
// A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15]; the result D[row = 4*(l>>4) + r][col = l&15], r < 4.
// The 16x16x4 form was chosen over 32x32x2 for its 16-wide tails (C, D, F tails cost at most 15 lanes).
//
// E-step (accumulate): three launches on the caller's stream, no float atomics, deterministic.
//   1. gmm_dense_kernel<kLse>: per 64-frame tile (4 waves x 16 frames) L over all C in 64-Gaussian blocks,
//      online max / sum-exp per (frame, lane), then a fixed-order butterfly over the 16 lanes of a frame:
//      lse[f].  Per workgroup sum_f w_f * lse_f in fp64 -> one partial per tile.
//   2. gmm_stats_kernel: grid (Gaussian block of 64) x (column block of 128 of [1 | x | x^2]) x (frame
//      chunk).  Per 64-frame tile it RECOMPUTES L for its 64 Gaussians (same device path), forms
//      P = exp(L - lse_f) * w_f into LDS (Gaussian-major), stages Y = [1 | x | x^2] (column-major) and runs
//      S[c, j] += sum_f P[f, c] * Y[f, j] on the MFMA (K = the 64 frames of the tile).  fp32 over one tile,
//      folded into fp64 registers after every tile, fp64 partial per workgroup to HBM.
//   3. gmm_reduce_kernel: stats[i] = sum over chunks in chunk order; tot_like likewise (one workgroup,
//      fixed-order tree).  Same inputs, same bits, every run.
//   Why recompute L rather than keep it: one 64-frame tile of L at C = 2048 is 512 KiB (LDS is 160 KiB),
//   and staging L through HBM at F = 500 000, C = 2048 is 4.1 GB written + read (~1.6 ms at ~5 TB/s), while
//   recomputing it is 2*F*C*2D = 1.6e11 FLOP (~1.0 ms at the 155 TF matrix peak).  Total E-step work is
//   then 2*(2*F*C*2D) + 2*F*C*(2D+1) = 4.8e11 FLOP at C = 2048 (3.2e11 of it "useful", see DESIGN).
//
// gselect: L for a block of frames staged through HBM (scratch [rows x C], rows sized to ~128 MB), then one
// wave per frame picks the top n by n rounds of "best pair below the previous pick": the order is Kaldi's
// std::sort of (loglike, index) pairs with std::greater (diag-gmm.cc GaussianSelection), i.e. descending
// loglike, and among EQUAL loglikes the HIGHER Gaussian index first.  With preselection the index compared
// is the preselected Gaussian's own index, as in GaussianSelectionPreselect.
//
// Selection posteriors: gathered L of the selected Gaussians (gmm_sel_loglike_kernel), then one thread per
// frame: Kaldi's VectorBase::ApplySoftMax and the reference's sequential min_post loop (ubm.py:559-569).
//
// Dense posteriors (snf_gmm_posteriors, the posteriorgram): gmm_dense_kernel<kLse> as in the E-step (unit weights;
// lse is bit-equal to accumulate's), then gmm_posteriors_kernel recomputes L per 64-frame tile and 64-Gaussian block,
// as gmm_stats_kernel does, and writes exp(L - lse_f): the block of P goes through LDS so that a thread stores 4
// consecutive Gaussians of a frame (16 bytes when C % 4 == 0 and the output is aligned).  No [F x C] L in HBM.
//
// Resource usage (hipcc -O3 gfx950, -Rpass-analysis=kernel-resource-usage; scratch 0 B in every kernel):
//   gmm_posteriors_kernel       57 VGPRs + 16 AGPRs, LDS 52 224 B: 3 waves/SIMD (LDS-bound: 3 workgroups/CU)
//   gmm_dense_kernel<loglikes>  50 VGPRs + 16 AGPRs, LDS 34 816 B: 4 waves/SIMD (LDS-bound: 4 workgroups/CU)
//   gmm_dense_kernel<lse>       58 VGPRs + 16 AGPRs, LDS 34 944 B: 4 waves/SIMD
//   gmm_stats_kernel           230 VGPRs + 192 AGPRs, LDS 52 224 B: 1 wave/SIMD (the 8 x 4 fp64 partials and
//                              8 fp32 MFMA accumulators per lane; register-bound)
//   gmm_topn_kernel 29, gmm_sel_loglike_kernel 30 + 4 AGPRs, gmm_post_kernel 15, gmm_reduce_kernel 8,
//   gmm_reduce_one_kernel 12 VGPRs: 8 waves/SIMD.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "snf_internal.h"

namespace snf {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTileF = 64;      // frames per workgroup tile (4 waves x 16)
constexpr int kBlockC = 64;     // Gaussians per block (4 MFMA column tiles)
constexpr int kChunkK = 64;     // k per LDS stage
constexpr int kLd = kChunkK + 4;  // LDS row stride: 4*row + (l>>4) covers the 64 banks once (no conflict)
constexpr int kBlockJ = 128;    // columns of [1 | x | x^2] per stats workgroup
constexpr int kThreads = 256;

// ---- the one definition of L ------------------------------------------------------------------
__device__ __forceinline__ float xop(const float* __restrict__ xrow, int D, int k) {
  if (k < D) return xrow[k];
  if (k < 2 * D) { const float v = xrow[k - D]; return v * v; }
  return 0.0f;
}
__device__ __forceinline__ float wop(const float* __restrict__ mi, const float* __restrict__ iv,
                                     int64_t c, int D, int k) {
  if (k < D) return mi[c * D + k];
  if (k < 2 * D) return -0.5f * iv[c * D + (k - D)];
  return 0.0f;
}
__device__ __forceinline__ f32x4 ll_step(float a, float b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ float ll_finish(float gconst, float acc) { return gconst + acc; }

struct GmmArgs {
  const float* x;  // [F x D]
  int64_t F;
  int D, C, Kp;
  const float* gconst;
  const float* mi;
  const float* iv;
};

// Stages X[64 frames][k0 .. k0+64) and W[64 Gaussians][k0 .. k0+64) into LDS (zeros outside F / C / Kp).
__device__ __forceinline__ void stage_chunk(const GmmArgs& g, int64_t f0, int c0, int k0, float* xs, float* ws) {
  for (int i = threadIdx.x; i < kTileF * kChunkK; i += kThreads) {
    const int r = i / kChunkK, k = k0 + (i % kChunkK);
    const int64_t f = f0 + r;
    xs[r * kLd + (i % kChunkK)] = (f < g.F && k < g.Kp) ? xop(g.x + f * g.D, g.D, k) : 0.0f;
    const int c = c0 + r;
    ws[r * kLd + (i % kChunkK)] = (c < g.C && k < g.Kp) ? wop(g.mi, g.iv, c, g.D, k) : 0.0f;
  }
}

// acc[t] (t < 4): the 16 frames of this wave x Gaussians c0 + 16t + (l&15), k over the whole of Kp.
__device__ __forceinline__ void dense_block(const GmmArgs& g, int64_t f0, int c0, float* xs, float* ws,
                                            f32x4 acc[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, h = lane >> 4;
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < g.Kp; k0 += kChunkK) {
    __syncthreads();
    stage_chunk(g, f0, c0, k0, xs, ws);
    __syncthreads();
    const int steps = min(kChunkK, g.Kp - k0) >> 2;
    const float* xa = xs + (wave * 16 + i) * kLd + h;
    const float* wb = ws + i * kLd + h;
    for (int s = 0; s < steps; ++s) {
      const float a = xa[4 * s];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = ll_step(a, wb[16 * t * kLd + 4 * s], acc[t]);
    }
  }
}

__device__ __forceinline__ void lse_push(float v, float& m, float& s) {
  if (v == -INFINITY) return;
  if (m == -INFINITY) { m = v; s = 1.0f; return; }
  if (v > m) { s = s * expf(m - v) + 1.0f; m = v; }
  else s += expf(v - m);
}
__device__ __forceinline__ void lse_merge(float m2, float s2, float& m, float& s) {
  if (m2 == -INFINITY) return;
  if (m == -INFINITY) { m = m2; s = s2; return; }
  const float M = fmaxf(m, m2);
  s = s * expf(m - M) + s2 * expf(m2 - M);
  m = M;
}

enum { kModeLoglikes = 0, kModeLse = 1 };

// Dense L over all C for one 64-frame tile.  kModeLoglikes: writes L[f, c] (row stride C).
// kModeLse: lse[f] and the tile's fp64 sum_f w_f * lse_f.
template <int Mode>
__global__ void __launch_bounds__(kThreads) gmm_dense_kernel(const GmmArgs g, float* __restrict__ out,
                                                            const float* __restrict__ weights,
                                                            double* __restrict__ tl_part) {
  __shared__ float xs[kTileF * kLd];
  __shared__ float ws[kBlockC * kLd];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t f0 = static_cast<int64_t>(blockIdx.x) * kTileF;
  const int64_t fr = f0 + wave * 16 + 4 * (lane >> 4);  // this lane's 4 frames: fr + r
  float m[4], s[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; s[r] = 0.0f; }
  for (int c0 = 0; c0 < g.C; c0 += kBlockC) {
    f32x4 acc[4];
    dense_block(g, f0, c0, xs, ws, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int c = c0 + 16 * t + (lane & 15);
      if (c >= g.C) continue;
      const float gc = g.gconst[c];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float L = ll_finish(gc, acc[t][r]);
        if (Mode == kModeLoglikes) {
          if (fr + r < g.F) out[(fr + r) * g.C + c] = L;
        } else {
          lse_push(L, m[r], s[r]);
        }
      }
    }
  }
  if (Mode == kModeLse) {
    __shared__ double red[kThreads / 16];
    double mine = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mm = m[r], ss = s[r];
      // fixed-order butterfly over the 16 lanes that share these frames (merge is commutative bit for bit)
      for (int o = 1; o < 16; o <<= 1) {
        const float m2 = __shfl_xor(mm, o), s2 = __shfl_xor(ss, o);
        lse_merge(m2, s2, mm, ss);
      }
      const float lse = mm + logf(ss);
      const int64_t f = fr + r;
      if ((lane & 15) == 0 && f < g.F) {
        out[f] = lse;
        mine += static_cast<double>(weights ? weights[f] : 1.0f) * static_cast<double>(lse);
      }
    }
    if ((lane & 15) == 0) red[threadIdx.x >> 4] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int i = 0; i < kThreads / 16; ++i) t += red[i];
      tl_part[blockIdx.x] = t;
    }
  }
}

// Statistics for (Gaussian block blockIdx.x, column block blockIdx.y, frame chunk blockIdx.z).
// part[(chunk * C + c) * J + j], J = 2D + 1, columns [occupancy | sum P x | sum P x^2].
__global__ void __launch_bounds__(kThreads) gmm_stats_kernel(const GmmArgs g, const float* __restrict__ lse,
                                                            const float* __restrict__ weights,
                                                            int64_t tiles_per_chunk,
                                                            double* __restrict__ part) {
  // xs / ws (L stage) and yt (Y, column-major) are never live together
  __shared__ float stage[2 * kTileF * kLd];
  __shared__ float pt[kBlockC * kLd];   // P, Gaussian-major: pt[c * kLd + f]
  float* xs = stage;
  float* ws = stage + kTileF * kLd;
  float* yt = stage;                    // yt[j * kLd + f], j < kBlockJ (128 * 68 = 2 * 64 * 68 floats)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, h = lane >> 4;
  const int c0 = blockIdx.x * kBlockC, j0 = blockIdx.y * kBlockJ;
  const int J = 2 * g.D + 1;
  const int64_t ntiles = (g.F + kTileF - 1) / kTileF;
  const int64_t t0 = static_cast<int64_t>(blockIdx.z) * tiles_per_chunk;
  const int64_t t1 = min(ntiles, t0 + tiles_per_chunk);
  double sum[8][4];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[a][r] = 0.0;
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t f0 = tile * kTileF;
    f32x4 acc[4];
    dense_block(g, f0, c0, xs, ws, acc);
    // P into LDS
    const int64_t fr = f0 + wave * 16 + 4 * h;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cl = 16 * t + i, c = c0 + cl;
      const float gc = c < g.C ? g.gconst[c] : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t f = fr + r;
        float p = 0.0f;
        if (c < g.C && f < g.F) {
          const float w = weights ? weights[f] : 1.0f;
          p = expf(ll_finish(gc, acc[t][r]) - lse[f]) * w;
        }
        pt[cl * kLd + (wave * 16 + 4 * h + r)] = p;
      }
    }
    __syncthreads();   // xs / ws reads done (dense_block) and pt written
    for (int e = threadIdx.x; e < kBlockJ * kTileF; e += kThreads) {
      const int j = j0 + e / kTileF, fl = e % kTileF;
      const int64_t f = f0 + fl;
      float y = 0.0f;
      if (f < g.F && j < J) {
        const float* xr = g.x + f * g.D;
        if (j == 0) y = 1.0f;
        else if (j <= g.D) y = xr[j - 1];
        else { const float v = xr[j - 1 - g.D]; y = v * v; }
      }
      yt[(e / kTileF) * kLd + fl] = y;
    }
    __syncthreads();
    f32x4 s[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) s[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* pa = pt + (wave * 16 + i) * kLd + h;   // A[c][f] = P[f][c]
    const float* yb = yt + i * kLd + h;                  // B[f][j] = Y[f][j]
    const int jt_n = min(8, (J - j0 + 15) >> 4);
    for (int st = 0; st < kTileF / 4; ++st) {
      const float a = pa[4 * st];
#pragma unroll
      for (int a8 = 0; a8 < 8; ++a8)
        if (a8 < jt_n) s[a8] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, yb[16 * a8 * kLd + 4 * st], s[a8], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[a][r] += static_cast<double>(s[a][r]);
    // (the next dense_block starts with a barrier before it overwrites the stage)
  }
  // D[row = c][col = j]: c = c0 + 16*wave + 4h + r, j = j0 + 16a + i
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int j = j0 + 16 * a + i;
    if (j >= J) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + 16 * wave + 4 * h + r;
      if (c < g.C) part[(static_cast<int64_t>(blockIdx.z) * g.C + c) * J + j] = sum[a][r];
    }
  }
}

// Dense posteriors of one 64-frame tile: post[f, c] = exp(L[f, c] - lse[f]) over all C in 64-Gaussian blocks, L
// recomputed by the same device path as in gmm_stats_kernel.  The accumulators hold one Gaussian per lane; a block of
// P goes through LDS (frame-major) so that a thread stores 4 consecutive Gaussians of a frame: 16 bytes where the
// rows are aligned (`vec`: C % 4 == 0 and post 16-byte aligned), 16 threads = 256 contiguous bytes of a row.
__global__ void __launch_bounds__(kThreads) gmm_posteriors_kernel(const GmmArgs g, const float* __restrict__ lse,
                                                                 float* __restrict__ post, const int vec) {
  __shared__ float xs[kTileF * kLd];
  __shared__ float ws[kBlockC * kLd];
  __shared__ __attribute__((aligned(16))) float pt[kTileF * kLd];   // P: pt[frame * kLd + Gaussian of the block]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, h = lane >> 4;
  const int64_t f0 = static_cast<int64_t>(blockIdx.x) * kTileF;
  const int64_t fr = f0 + wave * 16 + 4 * h;   // this lane's 4 frames: fr + r
  float ls[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) ls[r] = fr + r < g.F ? lse[fr + r] : 0.0f;
  for (int c0 = 0; c0 < g.C; c0 += kBlockC) {
    f32x4 acc[4];
    dense_block(g, f0, c0, xs, ws, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cl = 16 * t + i, c = c0 + cl;
      const float gc = c < g.C ? g.gconst[c] : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = 0.0f;
        if (c < g.C && fr + r < g.F) p = expf(ll_finish(gc, acc[t][r]) - ls[r]);
        pt[(wave * 16 + 4 * h + r) * kLd + cl] = p;
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kTileF * (kBlockC / 4); e += kThreads) {
      const int fl = e / (kBlockC / 4), c4 = 4 * (e % (kBlockC / 4));
      const int64_t f = f0 + fl;
      const int c = c0 + c4;
      if (f >= g.F || c >= g.C) continue;
      const float* src = pt + fl * kLd + c4;
      float* dst = post + f * g.C + c;
      if (vec) {   // (C % 4 == 0: the four are inside the row)
        *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(src);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c + q < g.C) dst[q] = src[q];
      }
    }
    // (the next dense_block starts with a barrier before anything writes pt again)
  }
}

__global__ void __launch_bounds__(kThreads) gmm_reduce_kernel(const double* __restrict__ part, int64_t n,
                                                             int64_t chunks, double* __restrict__ out) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= n) return;
  double t = 0.0;
  for (int64_t ch = 0; ch < chunks; ++ch) t += part[ch * n + e];
  out[e] = t;
}

__global__ void __launch_bounds__(kThreads) gmm_reduce_one_kernel(const double* __restrict__ part, int64_t n,
                                                                 double* __restrict__ out) {
  __shared__ double red[kThreads];
  double t = 0.0;
  for (int64_t e = threadIdx.x; e < n; e += kThreads) t += part[e];
  red[threadIdx.x] = t;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
}

// (v1, i1) ranks above (v2, i2): descending loglike, ties to the higher index (std::greater on pairs)
__device__ __forceinline__ bool above(float v1, int i1, float v2, int i2) {
  return v1 > v2 || (v1 == v2 && i1 > i2);
}

// One wave per frame: top n of row L[f, 0 .. P) (index = map[f, p] when given, else p), best first, and the
// log-sum-exp of the picked loglikes.  Rows of frames f < rows.
__global__ void __launch_bounds__(kThreads) gmm_topn_kernel(const float* __restrict__ L, const int32_t* __restrict__ map,
                                                           int64_t rows, int P, int n, int32_t* __restrict__ out_idx,
                                                           float* __restrict__ out_lse) {
  const int lane = threadIdx.x & 63;
  const int64_t f = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  if (f >= rows) return;
  const float* row = L + f * P;
  const int32_t* mrow = map ? map + f * P : nullptr;
  float pv = INFINITY;
  int pi = 0x7FFFFFFF;
  float m0 = -INFINITY, sum = 0.0f;
  for (int q = 0; q < n; ++q) {
    float bv = -INFINITY;
    int bi = -1;
    for (int p = lane; p < P; p += 64) {
      const float v = row[p];
      const int id = mrow ? mrow[p] : p;
      if (above(pv, pi, v, id) && above(v, id, bv, bi)) { bv = v; bi = id; }
    }
    for (int o = 1; o < 64; o <<= 1) {
      const float v2 = __shfl_xor(bv, o);
      const int i2 = __shfl_xor(bi, o);
      if (above(v2, i2, bv, bi)) { bv = v2; bi = i2; }
    }
    pv = bv; pi = bi;
    if (q == 0) { m0 = bv; sum = 1.0f; }
    else if (bv != -INFINITY) sum += expf(bv - m0);
    if (lane == 0) out_idx[f * n + q] = bi;
  }
  if (lane == 0 && out_lse) out_lse[f] = m0 + logf(sum);
}

// One wave per frame: L[f, sel[f, p]] for p < P, written to out[f * P + p].  Rows of the A operand all hold
// the same frame; row 0 of the result (lanes 0-15, register 0) is kept.  An index outside [0, C) leaves NaN
// and raises *bad.
__global__ void __launch_bounds__(kThreads) gmm_sel_loglike_kernel(const GmmArgs g, const int32_t* __restrict__ sel,
                                                                  int P, float* __restrict__ out,
                                                                  int* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int64_t f = static_cast<int64_t>(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
  if (f >= g.F) return;
  const int i = lane & 15, h = lane >> 4;
  const float* xr = g.x + f * g.D;
  for (int p0 = 0; p0 < P; p0 += 16) {
    const int p = p0 + i;
    int c = p < P ? sel[f * P + p] : 0;
    const bool ok = c >= 0 && c < g.C;
    if (!ok) { if (p < P) *bad = 1; c = 0; }
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = h; k < g.Kp; k += 4) acc = ll_step(xop(xr, g.D, k), wop(g.mi, g.iv, c, g.D, k), acc);
    if (h == 0 && p < P) out[f * P + p] = ok ? ll_finish(g.gconst[c], acc[0]) : NAN;
  }
}

// One thread per frame, in place over post[f, 0 .. n): Kaldi VectorBase::ApplySoftMax, then (min_post > 0)
// the reference's sequential pruning loop, ubm.py:559-569.
__global__ void __launch_bounds__(kThreads) gmm_post_kernel(float* __restrict__ post, int64_t F, int n,
                                                           float min_post, int prune, float* __restrict__ loglike) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (f >= F) return;
  float* v = post + f * n;
  float mx = v[0];
  for (int j = 1; j < n; ++j) mx = fmaxf(mx, v[j]);
  float sum = 0.0f;
  for (int j = 0; j < n; ++j) { const float e = expf(v[j] - mx); v[j] = e; sum += e; }
  const float scale = static_cast<float>(1.0 / static_cast<double>(sum));
  for (int j = 0; j < n; ++j) v[j] *= scale;
  loglike[f] = mx + logf(sum);
  if (!prune) return;
  int imax = 0;
  for (int j = 1; j < n; ++j)
    if (v[j] > v[imax]) imax = j;
  for (int j = 0; j < n; ++j) {
    if (v[j] < min_post) v[j] = 0.0f;
    float total = 0.0f;
    for (int q = 0; q < n; ++q) total += v[q];
    if (total == 0.0f) {
      v[imax] = 1.0f;
    } else {
      const float sc = static_cast<float>(1.0 / static_cast<double>(total));
      for (int q = 0; q < n; ++q) v[q] *= sc;
    }
  }
}

GmmArgs make_args(const float* x, int64_t F, int D, const float* gconst, const float* mi, const float* iv, int C) {
  GmmArgs g;
  g.x = x; g.F = F; g.D = D; g.C = C; g.Kp = (2 * D + 3) & ~3;
  g.gconst = gconst; g.mi = mi; g.iv = iv;
  return g;
}

unsigned blocks(int64_t n, int64_t per) { return static_cast<unsigned>((n + per - 1) / per); }

}  // namespace

int64_t gmm_stats_chunks(int64_t F, int C, int D) {
  const int64_t ntiles = (F + kTileF - 1) / kTileF;
  const int64_t grid = static_cast<int64_t>((C + kBlockC - 1) / kBlockC) * ((2 * D + 1 + kBlockJ - 1) / kBlockJ);
  int64_t chunks = std::max<int64_t>(1, (2048 + grid - 1) / grid);
  chunks = std::min(chunks, std::max<int64_t>(ntiles, 1));
  const int64_t per = (ntiles + chunks - 1) / chunks;
  return std::max<int64_t>(1, (ntiles + per - 1) / per);
}

int64_t gmm_tiles(int64_t F) { return (F + kTileF - 1) / kTileF; }

int launch_gmm_loglikes(const float* x, int64_t F, int D, const float* gconst, const float* mi, const float* iv, int C,
                        float* out, hipStream_t stream) {
  if (F <= 0) return SNF_OK;
  const GmmArgs g = make_args(x, F, D, gconst, mi, iv, C);
  hipLaunchKernelGGL(gmm_dense_kernel<kModeLoglikes>, dim3(blocks(F, kTileF)), dim3(kThreads), 0, stream, g, out,
                     nullptr, nullptr);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_gmm_accumulate(const float* x, int64_t F, int D, const float* weights, const float* gconst,
                          const float* mi, const float* iv, int C, float* lse, double* tl_part, double* part,
                          double* stats, double* tot_like, hipStream_t stream) {
  const GmmArgs g = make_args(x, F, D, gconst, mi, iv, C);
  const int64_t ntiles = gmm_tiles(F);
  const int64_t chunks = gmm_stats_chunks(F, C, D);
  const int64_t per = (ntiles + chunks - 1) / chunks;
  const int J = 2 * D + 1;
  hipLaunchKernelGGL(gmm_dense_kernel<kModeLse>, dim3(static_cast<unsigned>(ntiles)), dim3(kThreads), 0, stream, g,
                     lse, weights, tl_part);
  SNF_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(gmm_stats_kernel,
                     dim3(blocks(C, kBlockC), blocks(J, kBlockJ), static_cast<unsigned>(chunks)), dim3(kThreads), 0,
                     stream, g, lse, weights, per, part);
  SNF_HIP_CHECK(hipGetLastError());
  const int64_t n = static_cast<int64_t>(C) * J;
  hipLaunchKernelGGL(gmm_reduce_kernel, dim3(blocks(n, kThreads)), dim3(kThreads), 0, stream, part, n, chunks, stats);
  SNF_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(gmm_reduce_one_kernel, dim3(1), dim3(kThreads), 0, stream, tl_part, ntiles, tot_like);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_gmm_posteriors(const float* x, int64_t F, int D, const float* gconst, const float* mi, const float* iv,
                          int C, float* lse, double* tl_part, float* post, hipStream_t stream) {
  if (F <= 0) return SNF_OK;
  const GmmArgs g = make_args(x, F, D, gconst, mi, iv, C);
  const int64_t ntiles = gmm_tiles(F);
  // the E-step's own reduction (unit weights): lse is bit-equal to snf_gmm_accumulate's
  hipLaunchKernelGGL(gmm_dense_kernel<kModeLse>, dim3(static_cast<unsigned>(ntiles)), dim3(kThreads), 0, stream, g,
                     lse, nullptr, tl_part);
  SNF_HIP_CHECK(hipGetLastError());
  const int vec = (C % 4 == 0) && (reinterpret_cast<uintptr_t>(post) & 15) == 0;
  hipLaunchKernelGGL(gmm_posteriors_kernel, dim3(static_cast<unsigned>(ntiles)), dim3(kThreads), 0, stream, g, lse,
                     post, vec);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_gmm_topn(const float* L, const int32_t* map, int64_t rows, int P, int n, int32_t* out_idx, float* out_lse,
                    hipStream_t stream) {
  if (rows <= 0) return SNF_OK;
  hipLaunchKernelGGL(gmm_topn_kernel, dim3(blocks(rows, kThreads / 64)), dim3(kThreads), 0, stream, L, map, rows, P,
                     n, out_idx, out_lse);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_gmm_sel_loglikes(const float* x, int64_t F, int D, const float* gconst, const float* mi, const float* iv,
                            int C, const int32_t* sel, int P, float* out, int* bad, hipStream_t stream) {
  if (F <= 0) return SNF_OK;
  const GmmArgs g = make_args(x, F, D, gconst, mi, iv, C);
  hipLaunchKernelGGL(gmm_sel_loglike_kernel, dim3(blocks(F, kThreads / 64)), dim3(kThreads), 0, stream, g, sel, P,
                     out, bad);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

int launch_gmm_post(float* post, int64_t F, int n, float min_post, int prune, float* loglike, hipStream_t stream) {
  if (F <= 0) return SNF_OK;
  hipLaunchKernelGGL(gmm_post_kernel, dim3(blocks(F, kThreads)), dim3(kThreads), 0, stream, post, F, n, min_post,
                     prune, loglike);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
