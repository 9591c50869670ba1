// Linear-VTLN training kernels (reference processor/vtln.py -> [KALDI-UPSTREAM] transform/fmllr-diag-gmm.cc
// FmllrDiagGmmAccs::AccumulateFromPosteriorsPreselect / CommitSingleFrameStats, FmllrAuxFuncDiagGmm,
// ComputeFmllrMatrixDiagGmmOffset / ComputeFmllrMatrixDiagGmmDiagonal, transform/transform-common.cc
// ApplyFeatureTransformToStats / ComposeTransforms, transform/lvtln.cc LinearVtln::ComputeTransform, and the
// sums of gmm-train-lvtln-special as restated in reference vtln.py:299-343).
//
// A SEGMENT is a contiguous run of frames [off[s], off[s+1]) (one speaker, or one utterance); the host orders
// the frames so that every segment is contiguous.  D <= 64.
//
// 1. fMLLR statistics (Kaldi's AffineXformStats) per segment, with x+ = [x | 1]:
//      a_f = sum_j p_fj means_invvars[g_fj],  b_f = sum_j p_fj inv_vars[g_fj],  count_f = sum_j p_fj
//      beta = sum_f count_f,  K = sum_f a_f x+^T  [D x D+1],  G[d] = sum_f b_f[d] x+ x+^T  [D+1 x D+1]
//    all ONE segmented product  S = sum_f u_f v_f^T  with  u_f = [b_f (x) x+ | a_f | count_f]  (U = D(D+1)+D+1
//    rows: row d(D+1)+k = b_f[d] x+_k, row D(D+1)+d = a_f[d], row U-1 = count_f) and v_f = x+ (V = D+1
//    columns).  Output per segment: S [U x V] float64 row-major, so G[d][k][l] = S[d(D+1)+k][l],
//    K[d][l] = S[D(D+1)+d][l], beta = S[U-1][D] (row U-1 also holds sum_f count_f x_f).  G is formed in full.
//    a_f, b_f, count_f are float64 sums (j ascending) of exact float products; Kaldi keeps them in BaseFloat
//    (a divergence of ~1e-7 relative).  Every frame is counted (Kaldi's lazy CommitSingleFrameStats merges
//    repeated identical frames, which changes nothing in exact arithmetic).
// 2. Weighted Gram for the mapping transforms: S = sum_f w_f z_f z_f^T, z = [x | 1 | y] (U = V = 2D+1), one
//    segment.  Its blocks are every sum of reference vtln.py:299-343 (Q, l, c, beta, sum_xplus, sumsq_x and,
//    from the diagonals, sumsq_diff).
//    The Gram's frames are either two compact [F x D] arrays or (snf_vtln_gram_rows) rows gathered from
//    [rows x D] blocks by a (block, row) list: the same records in the same order, so the same bits.
//    Both products run through vtln_product_kernel: a pre-pass writes per-frame float64 records (fMLLR:
//    [x+ | b | a | count], R = 3D+2; Gram: [x | 1 | y | w], R = 2D+2); a workgroup (4 waves) owns 128 rows x
//    64 columns of S for one ITEM (a run of at most vtln_item_frames() = 2 048 frames of one segment), stages kTileT-frame
//    tiles of records in LDS and runs v_mfma_f64_16x16x4_f64 (A[i = l&15][k = l>>4], B[k = l>>4][j = l&15],
//    D[row = (l>>4) + 4r][col = l&15], r < 4; K = 4 frames per instruction).  Each lane forms its A operand
//    as rec[ia] * rec[ib] (fp64, the product of two floats is exact) and its B operand as rec[j].  A segment
//    of one item writes its S directly; longer segments write float64 partials per item, summed in item order
//    by vtln_reduce_kernel.  No atomics: the same inputs give the same bits.
// 3. Class search (LinearVtln::ComputeTransform), one workgroup per segment.  For class c with A = A_c:
//    ApplyFeatureTransformToStats gives K' = K Ahat^T, G'_d = Ahat G_d Ahat^T (Ahat = [[A, 0], [0, 1]]); the
//    solves and the aux function need only, per row d,
//      kdd = A[d].K[d][:D] = K'[d][d],  kdD = K[d][D] = K'[d][D],  gdd = A[d] G_d[:D,:D] A[d]^T = G'_d[d][d],
//      gdD = A[d].G_d[:D][D] = G'_d[d][D],  gDD = G_d[D][D] = G'_d[D][D].
//    none: s = 1, o = 0.  offset: s = 1, o = (kdD - gdD) / gDD.  diag: o = (kdD - s gdD) / gDD with s the
//    positive root of  Aq s^2 - Bq s - beta = 0,  Aq = gdd - gdD^2/gDD,  Bq = kdd - kdD gdD/gDD.
//    The composed transform is W = [diag(s) A | o] (ComposeTransforms), and FmllrAuxFuncDiagGmm(W, stats) =
//      beta (sum_d log|s_d| + log|A|) + sum_d [s_d kdd + o_d kdD - 0.5 (s_d^2 gdd + 2 s_d o_d gdD + o_d^2 gDD)]
//    in float64 (Kaldi evaluates it on W rounded to float).  LinearVtln adds (logdet_scale - 1) beta logdets[c],
//    so the log-determinant term of A is logdet_scale * beta * logdets[c] (logdets from the host).  The class is
//    the FIRST maximum; objf_impr = best - aux(identity) with aux(I) = sum_d (K[d][d] - 0.5 G_d[d][d]).
//    beta = 0: the default class, W = [A_default | 0], impr = count = 0 and objectives 0.
// 4. Per-segment affine apply: y_f = W_s[:, :D] x_f + W_s[:, D] in float32 (fma chain, k ascending).
//
// Resource usage (hipcc -O3 gfx950, -Rpass-analysis=kernel-resource-usage; scratch 0 B in every kernel):
//   vtln_product_kernel<fmllr|gram>  86 VGPRs + 64 AGPRs (8 f64x4 accumulators per lane), LDS 49 664 B:
//                                    3 waves/SIMD
//   lvtln_select_kernel              82 VGPRs, LDS 50 728 B (G_d, K_d, a 32 x 64 fp64 (class, k) table): 3 waves/SIMD
//   vtln_fmllr_rec_kernel 22, vtln_gram_rec_kernel 13, vtln_gram_rows_rec_kernel 14, vtln_reduce_kernel 8,
//   vtln_apply_kernel 13 VGPRs: 8 waves/SIMD
#include <math.h>

#include <algorithm>

#include "snf_internal.h"

namespace snf {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kTileT = 32;          // frames per LDS stage
constexpr int kMaxD = 64;
constexpr int kMaxR = 3 * kMaxD + 2;
constexpr int kRowsWg = 128;        // 4 waves x 2 row tiles of 16
constexpr int kColsWg = 64;         // 4 column tiles of 16
constexpr int kSelClasses = 32;     // classes per pass of the class search

unsigned blocks(int64_t n, int64_t per) { return static_cast<unsigned>((n + per - 1) / per); }

// ---- per-frame records ---------------------------------------------------------------------------------
// fMLLR: rec[f] = [x (D) | 1 | b (D) | a (D) | count], one thread per (frame, d <= D).
__global__ void __launch_bounds__(kThreads) vtln_fmllr_rec_kernel(const float* __restrict__ x, int64_t F, int D,
                                                                 const int32_t* __restrict__ sel,
                                                                 const float* __restrict__ post, int n,
                                                                 const float* __restrict__ mi,
                                                                 const float* __restrict__ iv, int C,
                                                                 double* __restrict__ rec, int* __restrict__ bad) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t f = e / (D + 1);
  const int d = static_cast<int>(e % (D + 1));
  if (f >= F) return;
  const int R = 3 * D + 2;
  double* r = rec + f * R;
  const int32_t* sr = sel + f * n;
  const float* pr = post + f * n;
  if (d < D) {
    double a = 0.0, b = 0.0;
    for (int j = 0; j < n; ++j) {
      int g = sr[j];
      if (g < 0 || g >= C) { *bad = 1; g = 0; }
      const double p = static_cast<double>(pr[j]);
      a += p * static_cast<double>(mi[static_cast<int64_t>(g) * D + d]);
      b += p * static_cast<double>(iv[static_cast<int64_t>(g) * D + d]);
    }
    r[d] = static_cast<double>(x[f * D + d]);
    r[D + 1 + d] = b;
    r[2 * D + 1 + d] = a;
  } else {
    double c = 0.0;
    for (int j = 0; j < n; ++j) c += static_cast<double>(pr[j]);
    r[D] = 1.0;
    r[3 * D + 1] = c;
  }
}

// Gram: rec[f] = [x (D) | 1 | y (D) | w], one thread per (frame, d <= D).
__global__ void __launch_bounds__(kThreads) vtln_gram_rec_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ y,
                                                                const float* __restrict__ w, int64_t F, int D,
                                                                double* __restrict__ rec) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t f = e / (D + 1);
  const int d = static_cast<int>(e % (D + 1));
  if (f >= F) return;
  double* r = rec + f * (2 * D + 2);
  if (d < D) {
    r[d] = static_cast<double>(x[f * D + d]);
    r[D + 1 + d] = static_cast<double>(y[f * D + d]);
  } else {
    r[D] = 1.0;
    r[2 * D + 1] = w ? static_cast<double>(w[f]) : 1.0;
  }
}

// Gram over gathered rows: record f takes row row[f] of block blk[f] of both x and y (blocks row-major
// [rows x D]); the records, hence the product, equal those of the rows gathered into x / y beforehand.
__global__ void __launch_bounds__(kThreads) vtln_gram_rows_rec_kernel(const float* const* __restrict__ xb,
                                                                     const float* const* __restrict__ yb,
                                                                     const int32_t* __restrict__ blk,
                                                                     const int64_t* __restrict__ row,
                                                                     const float* __restrict__ w, int64_t F, int D,
                                                                     double* __restrict__ rec) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t f = e / (D + 1);
  const int d = static_cast<int>(e % (D + 1));
  if (f >= F) return;
  double* r = rec + f * (2 * D + 2);
  if (d < D) {
    const int b = blk[f];
    const int64_t src = row[f] * D + d;
    r[d] = static_cast<double>(xb[b][src]);
    r[D + 1 + d] = static_cast<double>(yb[b][src]);
  } else {
    r[D] = 1.0;
    r[2 * D + 1] = w ? static_cast<double>(w[f]) : 1.0;
  }
}

// ---- the segmented product -----------------------------------------------------------------------------
enum { kModeFmllr = 0, kModeGram = 1 };

struct ProductArgs {
  const double* rec;      // [F x R]
  int R, D, U, V;
  const int64_t* items;   // [n_items x 3]: first frame, end frame, destination slot
  int64_t n_slots_out;    // slots below this are rows of `out`, the others rows of `part`
  double* out;            // [segments x U x V]
  double* part;           // [partial slots x U x V]
  int col_groups;
};

// A operand of row r: rec[ia] * rec[ib] (ib < 0: rec[ia] alone; ia < 0: zero)
template <int Mode>
__device__ __forceinline__ void row_source(int r, int D, int U, int& ia, int& ib) {
  ia = -1; ib = -1;
  if (r >= U) return;
  if (Mode == kModeFmllr) {
    const int V = D + 1;
    if (r < D * V) { ia = V + r / V; ib = r % V; }
    else if (r < D * V + D) { ia = 2 * D + 1 + (r - D * V); }
    else { ia = 3 * D + 1; }
  } else {
    ia = r; ib = 2 * D + 1;
  }
}

template <int Mode>
__global__ void __launch_bounds__(kThreads) vtln_product_kernel(const ProductArgs a) {
  __shared__ double tile[kTileT * kMaxR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, h = lane >> 4;
  const int rg = blockIdx.x / a.col_groups, cg = blockIdx.x % a.col_groups;
  const int r0 = rg * kRowsWg + wave * 32, c0 = cg * kColsWg;
  const int64_t* it = a.items + 3 * static_cast<int64_t>(blockIdx.y);
  const int64_t f0 = it[0], f1 = it[1], slot = it[2];
  int ia[2], ib[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) row_source<Mode>(r0 + 16 * t + i, a.D, a.U, ia[t], ib[t]);
  int jb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) { const int j = c0 + 16 * t + i; jb[t] = j < a.V ? j : -1; }
  const int nct = min(4, (a.V - c0 + 15) >> 4);
  f64x4 acc[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = f64x4{0.0, 0.0, 0.0, 0.0};
  const bool rows_live = r0 < a.U;
  for (int64_t t0 = f0; t0 < f1; t0 += kTileT) {
    const int nt = static_cast<int>(min<int64_t>(kTileT, f1 - t0));
    __syncthreads();
    for (int e = threadIdx.x; e < kTileT * a.R; e += kThreads) {
      const int fl = e / a.R;
      tile[e] = fl < nt ? a.rec[(t0 + fl) * a.R + (e - fl * a.R)] : 0.0;
    }
    __syncthreads();
    if (!rows_live) continue;
    for (int s = 0; s < kTileT / 4; ++s) {
      const double* fr = tile + (4 * s + h) * a.R;   // lane's frame for this k step
      double av[2], bv[4];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const double p = ia[t] >= 0 ? fr[ia[t]] : 0.0;
        av[t] = ib[t] >= 0 ? p * fr[ib[t]] : p;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) bv[c] = jb[c] >= 0 ? fr[jb[c]] : 0.0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c >= nct) break;
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t], bv[c], acc[t][c], 0, 0, 0);
      }
    }
  }
  if (!rows_live) return;
  const int64_t uv = static_cast<int64_t>(a.U) * a.V;
  double* dst = slot < a.n_slots_out ? a.out + slot * uv : a.part + (slot - a.n_slots_out) * uv;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = c0 + 16 * c + i;
      if (col >= a.V) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = r0 + 16 * t + h + 4 * r;
        if (row < a.U) dst[static_cast<int64_t>(row) * a.V + col] = acc[t][c][r];
      }
    }
}

// out[seg] = sum of its partial slots, in slot order.  red[k] = (segment, first partial, count).
__global__ void __launch_bounds__(kThreads) vtln_reduce_kernel(const double* __restrict__ part,
                                                              const int64_t* __restrict__ red, int64_t uv,
                                                              double* __restrict__ out) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= uv) return;
  const int64_t* q = red + 3 * static_cast<int64_t>(blockIdx.y);
  double t = 0.0;
  for (int64_t k = 0; k < q[2]; ++k) t += part[(q[1] + k) * uv + e];
  out[q[0] * uv + e] = t;
}

// ---- class search ----------------------------------------------------------------------------------------
struct SelectArgs {
  const double* stats;    // [S x U x (D+1)]
  int D, C, norm_type, default_class;
  double logdet_scale;
  const double* A;        // [C x D x D]
  const double* logdets;  // [C]
  double* objf;           // [S x C]
  int32_t* cls;
  double* impr;
  double* count;
  float* transform;       // [S x D x (D+1)]
};

// Row terms for classes c0 .. c0+nc of row d.  Threads tid < nc receive (s, o, row aux) of class c0 + tid.
__device__ void select_row(const SelectArgs& a, double beta, int d, int c0, int nc, const double* g, const double* k,
                           double* part, bool active, double& s_out, double& o_out, double& aux_out) {
  const int D = a.D, V = D + 1;
  const int tid = threadIdx.x;
  for (int p = tid; p < nc * D; p += kThreads) {
    const int cl = p / D, kk = p % D;
    const double* Ar = a.A + (static_cast<int64_t>(c0 + cl) * D + d) * D;
    double t = 0.0;
    for (int l = 0; l < D; ++l) t += g[kk * V + l] * Ar[l];
    part[cl * kMaxD + kk] = Ar[kk] * t;
  }
  __syncthreads();
  if (active) {
    const double* Ar = a.A + (static_cast<int64_t>(c0 + tid) * D + d) * D;
    double gdd = 0.0, kdd = 0.0, gdD = 0.0;
    for (int kk = 0; kk < D; ++kk) {
      gdd += part[tid * kMaxD + kk];
      kdd += Ar[kk] * k[kk];
      gdD += Ar[kk] * g[kk * V + D];
    }
    const double kdD = k[D], gDD = g[D * V + D];
    double s = 1.0, o = 0.0;
    if (a.norm_type == 1) {
      o = (kdD - gdD) / gDD;
    } else if (a.norm_type == 2) {
      const double aq = gdd - gdD * gdD / gDD, bq = kdd - kdD * gdD / gDD;
      s = (bq + sqrt(bq * bq + 4.0 * aq * beta)) / (2.0 * aq);
      o = (kdD - s * gdD) / gDD;
    }
    s_out = s;
    o_out = o;
    aux_out = beta * log(fabs(s)) + s * kdd + o * kdD - 0.5 * (s * s * gdd + 2.0 * s * o * gdD + o * o * gDD);
  }
  __syncthreads();   // part is reused by the next row
}

__device__ void stage_row(const double* st, int D, int d, double* g, double* k) {
  const int V = D + 1;
  for (int e = threadIdx.x; e < V * V; e += kThreads) g[e] = st[static_cast<int64_t>(d) * V * V + e];
  for (int e = threadIdx.x; e < V; e += kThreads) k[e] = st[(static_cast<int64_t>(D) * V + d) * V + e];
  __syncthreads();
}

__global__ void __launch_bounds__(kThreads) lvtln_select_kernel(const SelectArgs a) {
  __shared__ double g[(kMaxD + 1) * (kMaxD + 1)];
  __shared__ double k[kMaxD + 1];
  __shared__ double part[kSelClasses * kMaxD];
  __shared__ double best_sh[2];
  __shared__ int best_c;
  const int D = a.D, V = D + 1, U = D * V + D + 1;
  const int64_t s = blockIdx.x;
  const double* st = a.stats + s * static_cast<int64_t>(U) * V;
  const int tid = threadIdx.x;
  const double beta = st[static_cast<int64_t>(U - 1) * V + D];
  float* W = a.transform + s * static_cast<int64_t>(D) * V;
  if (beta == 0.0) {
    for (int e = tid; e < D * V; e += kThreads) {
      const int r = e / V, c = e % V;
      W[e] = c < D ? static_cast<float>(a.A[(static_cast<int64_t>(a.default_class) * D + r) * D + c]) : 0.0f;
    }
    for (int c = tid; c < a.C; c += kThreads) a.objf[s * a.C + c] = 0.0;
    if (tid == 0) { a.cls[s] = a.default_class; a.impr[s] = 0.0; a.count[s] = 0.0; }
    return;
  }
  // aux of the identity transform: sum_d K[d][d] - 0.5 G_d[d][d], d ascending
  if (tid == 0) {
    double t = 0.0;
    for (int d = 0; d < D; ++d)
      t += st[(static_cast<int64_t>(D) * V + d) * V + d] - 0.5 * st[(static_cast<int64_t>(d) * V + d) * V + d];
    best_sh[1] = t;
    best_sh[0] = -1.0e100;
    best_c = -1;
  }
  double dummy_s, dummy_o;
  for (int c0 = 0; c0 < a.C; c0 += kSelClasses) {
    const int nc = min(kSelClasses, a.C - c0);
    const bool active = tid < nc;
    double obj = 0.0;
    for (int d = 0; d < D; ++d) {
      stage_row(st, D, d, g, k);
      double aux = 0.0;
      select_row(a, beta, d, c0, nc, g, k, part, active, dummy_s, dummy_o, aux);
      if (active) obj += aux;
    }
    if (active) {
      obj += a.logdet_scale * beta * a.logdets[c0 + tid];
      a.objf[s * a.C + c0 + tid] = obj;
      part[tid] = obj;
    }
    __syncthreads();
    if (tid == 0)
      for (int c = 0; c < nc; ++c)
        if (part[c] > best_sh[0]) { best_sh[0] = part[c]; best_c = c0 + c; }
    __syncthreads();
  }
  // the chosen class again, row by row, for its transform (no finite objective: the default class)
  const int bc = best_c >= 0 ? best_c : a.default_class;
  for (int d = 0; d < D; ++d) {
    stage_row(st, D, d, g, k);
    double sd = 1.0, od = 0.0, aux = 0.0;
    select_row(a, beta, d, bc, 1, g, k, part, tid == 0, sd, od, aux);
    if (tid == 0) {
      k[0] = sd;  // (k is restaged before it is read again)
      k[1] = od;
    }
    __syncthreads();
    sd = k[0];
    od = k[1];
    for (int c = tid; c < V; c += kThreads)
      W[static_cast<int64_t>(d) * V + c] =
          c < D ? static_cast<float>(sd * a.A[(static_cast<int64_t>(bc) * D + d) * D + c]) : static_cast<float>(od);
    __syncthreads();
  }
  if (tid == 0) {
    a.cls[s] = bc;
    a.impr[s] = best_sh[0] - best_sh[1];
    a.count[s] = beta;
  }
}

// ---- per-segment affine apply ----------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) vtln_apply_kernel(const float* __restrict__ x, int64_t F, int D,
                                                             const int64_t* __restrict__ off, int64_t S,
                                                             const float* __restrict__ W, float* __restrict__ y) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t f = e / D;
  const int r = static_cast<int>(e % D);
  if (f >= F) return;
  int64_t lo = 0, hi = S;   // the segment s with off[s] <= f < off[s + 1]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= f) lo = mid; else hi = mid;
  }
  const float* w = W + (lo * D + r) * (D + 1);
  const float* xr = x + f * D;
  float t = 0.0f;
  for (int c = 0; c < D; ++c) t = fmaf(w[c], xr[c], t);
  y[f * D + r] = t + w[D];
}

template <int Mode>
int launch_product(const double* rec, int R, int D, int U, int V, const int64_t* items, int64_t n_items,
                   int64_t n_slots_out, double* out, double* part, const int64_t* red, int64_t n_red,
                   hipStream_t stream) {
  ProductArgs a;
  a.rec = rec; a.R = R; a.D = D; a.U = U; a.V = V; a.items = items; a.n_slots_out = n_slots_out;
  a.out = out; a.part = part;
  a.col_groups = (V + kColsWg - 1) / kColsWg;
  const unsigned gx = static_cast<unsigned>(((U + kRowsWg - 1) / kRowsWg) * a.col_groups);
  for (int64_t i0 = 0; i0 < n_items; i0 += 65535) {
    a.items = items + 3 * i0;
    const unsigned gy = static_cast<unsigned>(std::min<int64_t>(65535, n_items - i0));
    hipLaunchKernelGGL(vtln_product_kernel<Mode>, dim3(gx, gy), dim3(kThreads), 0, stream, a);
    SNF_HIP_CHECK(hipGetLastError());
  }
  const int64_t uv = static_cast<int64_t>(U) * V;
  for (int64_t i0 = 0; i0 < n_red; i0 += 65535) {
    const unsigned gy = static_cast<unsigned>(std::min<int64_t>(65535, n_red - i0));
    hipLaunchKernelGGL(vtln_reduce_kernel, dim3(blocks(uv, kThreads), gy), dim3(kThreads), 0, stream, part,
                       red + 3 * i0, uv, out);
    SNF_HIP_CHECK(hipGetLastError());
  }
  return SNF_OK;
}

}  // namespace

int64_t vtln_item_frames() { return 2048; }

int launch_fmllr_accumulate(const float* x, int64_t F, int D, const int32_t* sel, const float* post, int n,
                            const float* mi, const float* iv, int C, double* rec, int* bad, const int64_t* items,
                            int64_t n_items, int64_t S, double* out, double* part, const int64_t* red, int64_t n_red,
                            hipStream_t stream) {
  const int V = D + 1, U = D * V + D + 1;
  if (F > 0) {
    hipLaunchKernelGGL(vtln_fmllr_rec_kernel, dim3(blocks(F * (D + 1), kThreads)), dim3(kThreads), 0, stream, x, F,
                       D, sel, post, n, mi, iv, C, rec, bad);
    SNF_HIP_CHECK(hipGetLastError());
  }
  return launch_product<kModeFmllr>(rec, 3 * D + 2, D, U, V, items, n_items, S, out, part, red, n_red, stream);
}

int launch_vtln_gram(const float* x, const float* y, const float* w, int64_t F, int D, double* rec,
                     const int64_t* items, int64_t n_items, double* out, double* part, const int64_t* red,
                     int64_t n_red, hipStream_t stream) {
  const int V = 2 * D + 1;
  if (F > 0) {
    hipLaunchKernelGGL(vtln_gram_rec_kernel, dim3(blocks(F * (D + 1), kThreads)), dim3(kThreads), 0, stream, x, y, w,
                       F, D, rec);
    SNF_HIP_CHECK(hipGetLastError());
  }
  return launch_product<kModeGram>(rec, 2 * D + 2, D, V, V, items, n_items, 1, out, part, red, n_red, stream);
}

int launch_vtln_gram_rows(const float* const* xb, const float* const* yb, const int32_t* blk, const int64_t* row,
                          const float* w, int64_t F, int D, double* rec, const int64_t* items, int64_t n_items,
                          double* out, double* part, const int64_t* red, int64_t n_red, hipStream_t stream) {
  const int V = 2 * D + 1;
  if (F > 0) {
    hipLaunchKernelGGL(vtln_gram_rows_rec_kernel, dim3(blocks(F * (D + 1), kThreads)), dim3(kThreads), 0, stream, xb,
                       yb, blk, row, w, F, D, rec);
    SNF_HIP_CHECK(hipGetLastError());
  }
  return launch_product<kModeGram>(rec, 2 * D + 2, D, V, V, items, n_items, 1, out, part, red, n_red, stream);
}

int launch_lvtln_select(const double* stats, int64_t S, int D, const double* A, const double* logdets, int C,
                        int norm_type, double logdet_scale, int default_class, double* objf, int32_t* cls,
                        double* impr, double* count, float* transform, hipStream_t stream) {
  SelectArgs a;
  a.stats = stats; a.D = D; a.C = C; a.norm_type = norm_type; a.default_class = default_class;
  a.logdet_scale = logdet_scale; a.A = A; a.logdets = logdets; a.objf = objf; a.cls = cls; a.impr = impr;
  a.count = count; a.transform = transform;
  for (int64_t s0 = 0; s0 < S; s0 += 65535) {
    SelectArgs b = a;
    const int64_t U = static_cast<int64_t>(D) * (D + 1) + D + 1;
    b.stats += s0 * U * (D + 1);
    b.objf += s0 * C; b.cls += s0; b.impr += s0; b.count += s0; b.transform += s0 * D * (D + 1);
    hipLaunchKernelGGL(lvtln_select_kernel, dim3(static_cast<unsigned>(std::min<int64_t>(65535, S - s0))),
                       dim3(kThreads), 0, stream, b);
    SNF_HIP_CHECK(hipGetLastError());
  }
  return SNF_OK;
}

int launch_affine_apply_segments(const float* x, int64_t F, int D, const int64_t* off, int64_t S, const float* W,
                                 float* y, hipStream_t stream) {
  if (F <= 0) return SNF_OK;
  hipLaunchKernelGGL(vtln_apply_kernel, dim3(blocks(F * D, kThreads)), dim3(kThreads), 0, stream, x, F, D, off, S, W,
                     y);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
