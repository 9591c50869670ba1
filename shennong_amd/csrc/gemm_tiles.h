// The two matrix-core tiles that the model kernels share (kernels_bottleneck.hip: bn_dense_kernel,
// bn_dense_bf16_kernel; kernels_crepe.hip: crepe_conv_kernel, crepe_conv_bf16_kernel), each piece once: constants,
// workgroup and lane coordinates, the B loaders, the two main loops, the walk over a lane's accumulators and the
// host's tile grid.  A kernel adds what is its own: how a row of A is addressed (a loader policy), the chain
// length of its sums (a template argument) and its epilogue (a callable over the walk).
//
// Both tiles: Y[M x N] = A[M x K] B[K x N] in block tiles of 128 x 128, 256 threads = 4 waves in 2 x 2, a wave
// owns 64 x 64 = 2 x 2 MFMA tiles of 32 x 32 (16 accumulator registers each); the result of a tile sits at
// D[row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)][col = l & 31] of lane l.  The next k tile's global loads are
// issued before the MFMAs of the current one (register prefetch, one LDS buffer, two barriers per tile).
//
// FP32 tile (gemm_f32), k tile 32, v_mfma_f32_32x32x2_f32: lane l supplies A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31].
//   * A tile in LDS row-major with stride 34 floats: the 32 rows x 2 k of one operand read fall on 64 different
//     banks (34 m mod 64 takes every even bank once for m < 32, the second k the odd ones).  B tile k-major with
//     stride 160: the two k rows of a read are 32 banks apart.  Reads are conflict-free ds_read_b32; a k step of 2
//     costs a wave 4 reads for 4 MFMAs of 64 cycles each.
//   * The MFMA is bit for bit a chain of fused multiply-adds over k ascending; zero padding beyond K adds
//     fma(0, 0, acc) = acc.  kChain = 0: ONE chain over all k from a zero accumulator.  kChain > 0 (a multiple of
//     the k tile): chains of kChain consecutive k, each from a zero accumulator, their results added in ascending
//     order.
//
// bfloat16 tile (gemm_bf16), k tile 64, v_mfma_f32_32x32x16_bf16, float32 sums: lane l holds
// A[l & 31][8 (l >> 5) + j] and B[8 (l >> 5) + j][l & 31], j = 0..7.
//   * B is the weight image Wt[n][kp] of bn_pack_bf16_kernel: bfloat16, k-contiguous per output column, kp = K
//     rounded up to the k tile and zero beyond K.  A B fragment is 8 consecutive k of one column, i.e. 16
//     contiguous bytes of the image, and an A fragment 8 consecutive k of one row.  No transpose anywhere.
//   * A k tile is 4 steps of 16 and costs a wave 16 ds_read_b128 for 16 MFMAs.  Both tiles sit in LDS as [row][k]
//     with a row stride of 144 bytes (9 slots of 16): the 16 lanes that a ds_read_b128 serves together read one k
//     chunk of 16 rows that differ modulo 16, and 9 r mod 16 is a bijection, so they fall on 16 different slots of
//     the 256-byte bank row; the 8 lanes that a ds_write_b128 serves together write 128 contiguous bytes of one row.
//   * Tile columns beyond N repeat the last valid one, and the A policies do the same for rows beyond M (no branch
//     between the loads; rows and columns of a product do not mix and the epilogues store neither); k beyond K is
//     zero in both operands, and a zero product leaves a float32 sum as it is.
//   * Summation order: the MFMA's own over the 16 k of a step, steps ascending; kChain as above, in k.
//   * Workgroups go to the 8 XCDs in turn, each with an L2 of its own: every XCD gets a contiguous run of tiles,
//     so that the tiles_n workgroups that share a block of A rows meet in one L2 (measured + 5 to 8 % on the
//     square dense layers at 500 and 1500 against the plain order, same bits).  The FP32 kernels keep the plain
//     order.
#pragma once
#include "snf_internal.h"

namespace snf {
namespace {

constexpr int kBM = 128, kBN = 128, kBK = 32;
constexpr int kLdA = 34;    // floats per A row in LDS
constexpr int kLdB = 160;   // floats per B k-row in LDS
constexpr int kThreads = 256;
constexpr int kQK = 64;     // bfloat16 k tile: the weight image pads K to a multiple of it
constexpr int kQLd = 72;    // bfloat16 per tile row in LDS (144 bytes = 9 slots of 16)
constexpr unsigned kXcds = 8;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // 8 bfloat16, 16 bytes

// Where a thread stands: its wave in the 2 x 2 grid (wm, wn), its lane in the MFMA (li = l & 31, lh = l >> 5), the
// origin of the workgroup's tile, and its place as a loader: tile rows lr + 32 i, i < 4, and from lc on 4 k (FP32,
// A) or 8 k (bfloat16, both operands).
struct Tile {
  int wm, wn, li, lh, lr, lc;
  int64_t m0;
  int n0;
};

// kXcdOrder: tile ids in XCD-contiguous runs, a bijection of the workgroup ids; else the plain order
template <bool kXcdOrder>
__device__ __forceinline__ Tile tile_of_workgroup(int n_tiles_n) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Tile t;
  t.wm = wave >> 1; t.wn = wave & 1; t.li = lane & 31; t.lh = lane >> 5;
  unsigned id = blockIdx.x;
  if (kXcdOrder) {
    const unsigned nwg = gridDim.x, xcd = blockIdx.x % kXcds, q = nwg / kXcds, r = nwg % kXcds;
    id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + blockIdx.x / kXcds;
  }
  t.m0 = static_cast<int64_t>(id / n_tiles_n) * kBM;
  t.n0 = static_cast<int>(id % n_tiles_n) * kBN;
  t.lc = tid & 7; t.lr = tid >> 3;
  return t;
}

// 4 consecutive n of row k of the row-major w[K x N], zeros outside; vec_b: 16-byte loads allowed
__device__ __forceinline__ float4 load_b4(const float* w, int K, int N, int vec_b, int k, int n) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k >= K || n >= N) return v;
  const float* p = w + static_cast<int64_t>(k) * N + n;
  if (vec_b) return *reinterpret_cast<const float4*>(p);
  v.x = p[0];
  if (n + 1 < N) v.y = p[1];
  if (n + 2 < N) v.z = p[2];
  if (n + 3 < N) v.w = p[3];
  return v;
}

// 8 consecutive k of column n (< N) of the packed weights (k < Kp always: the image is padded)
__device__ __forceinline__ u32x4 load_w8(const uint16_t* wt, int Kp, int n, int k) {
  return *reinterpret_cast<const u32x4*>(wt + static_cast<int64_t>(n) * Kp + k);
}

__device__ __forceinline__ void clear(f32x16 (&v)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) v[a][b][r] = 0.0f;
}

// The 2 x 2 step: acc[i][j] += a[i] b[j] over the k of one MFMA
__device__ __forceinline__ void mfma_2x2(float a0, float a1, float b0, float b1, f32x16 (&acc)[2][2]) {
  acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
  acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
  acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
  acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
}
__device__ __forceinline__ void mfma_2x2(bf16x8 a0, bf16x8 a1, bf16x8 b0, bf16x8 b1, f32x16 (&acc)[2][2]) {
  acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
  acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
  acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
  acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
}

// out = A w over the workgroup's tile, FP32.  a4(i, k): the 4 floats k .. k + 3 of tile row t.lr + 32 i, zeros
// beyond M and K.
template <int kChain, class ALoad>
__device__ __forceinline__ void gemm_f32(const Tile& t, const ALoad& a4, const float* w, int K, int N, int vec_b,
                                         f32x16 (&out)[2][2]) {
  static_assert(kChain % kBK == 0, "a chain is whole k tiles");
  __shared__ __attribute__((aligned(16))) float As[kBM * kLdA];
  __shared__ __attribute__((aligned(16))) float Bs[kBK * kLdB];
  const int b_nq = threadIdx.x & 31, b_k = threadIdx.x >> 5;    // B: k rows b_k + 8 i, columns 4 b_nq ..
  f32x16 chain_acc[2][2];
  f32x16 (&acc)[2][2] = kChain > 0 ? chain_acc : out;   // the running chain; `out`: the chains done so far
  clear(acc);
  if constexpr (kChain > 0) clear(out);
  float4 ra[4], rb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = a4(i, 4 * t.lc);
    rb[i] = load_b4(w, K, N, vec_b, b_k + 8 * i, t.n0 + 4 * b_nq);
  }
  for (int k0 = 0; k0 < K; k0 += kBK) {
    __syncthreads();   // the previous tile's operand reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float2* pa = reinterpret_cast<float2*>(As + (t.lr + 32 * i) * kLdA + 4 * t.lc);
      pa[0] = make_float2(ra[i].x, ra[i].y);
      pa[1] = make_float2(ra[i].z, ra[i].w);
      *reinterpret_cast<float4*>(Bs + (b_k + 8 * i) * kLdB + 4 * b_nq) = rb[i];
    }
    __syncthreads();
    if (k0 + kBK < K) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[i] = a4(i, k0 + kBK + 4 * t.lc);
        rb[i] = load_b4(w, K, N, vec_b, k0 + kBK + b_k + 8 * i, t.n0 + 4 * b_nq);
      }
    }
    const int kmax = min(kBK, (K - k0 + 1) & ~1);
    const float* pa = As + (t.wm * 64 + t.li) * kLdA + t.lh;
    const float* pb = Bs + t.lh * kLdB + t.wn * 64 + t.li;
    for (int kk = 0; kk < kmax; kk += 2)
      mfma_2x2(pa[kk], pa[32 * kLdA + kk], pb[kk * kLdB], pb[kk * kLdB + 32], acc);
    if constexpr (kChain > 0) {
      if ((k0 + kBK) % kChain == 0 || k0 + kBK >= K) {   // a chain of kChain k is complete (or K is)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              out[a][b][r] += acc[a][b][r];
              acc[a][b][r] = 0.0f;
            }
      }
    }
  }
}

// out = bf16(A) Wt over the workgroup's tile.  a8.load(i, k): the fragment k .. k + 7 of tile row t.lr + 32 i as
// the policy keeps it in registers (ALoad::Frag); a8.bits(frag): its 16 bytes of bfloat16 at the LDS write, zeros
// beyond K.
template <int kChain, class ALoad>
__device__ __forceinline__ void gemm_bf16(const Tile& t, const ALoad& a8, const uint16_t* wt, int K, int Kp, int N,
                                          f32x16 (&out)[2][2]) {
  static_assert(kChain % kQK == 0, "a chain is whole k tiles");
  __shared__ __attribute__((aligned(16))) uint16_t As[kBM * kQLd];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[kBN * kQLd];
  int b_col[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) b_col[i] = min(t.n0 + t.lr + 32 * i, N - 1);
  typename ALoad::Frag ra[4];
  u32x4 rb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = a8.load(i, 8 * t.lc);
    rb[i] = load_w8(wt, Kp, b_col[i], 8 * t.lc);
  }
  const uint16_t* pa = As + (t.wm * 64 + t.li) * kQLd + 8 * t.lh;
  const uint16_t* pb = Bs + (t.wn * 64 + t.li) * kQLd + 8 * t.lh;
  f32x16 chain_acc[2][2];
  f32x16 (&acc)[2][2] = kChain > 0 ? chain_acc : out;   // the running chain; `out`: the chains done so far
  if constexpr (kChain > 0) clear(out);
  int kc = 0;
  do {   // one chain: the k tiles of [kc, kend) into a zero accumulator
    const int kend = kChain > 0 ? min(kc + kChain, K) : K;
    clear(acc);
    for (int k0 = kc; k0 < kend; k0 += kQK) {
      __syncthreads();   // the previous tile's operand reads are done
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<u32x4*>(As + (t.lr + 32 * i) * kQLd + 8 * t.lc) = a8.bits(ra[i]);
        *reinterpret_cast<u32x4*>(Bs + (t.lr + 32 * i) * kQLd + 8 * t.lc) = rb[i];
      }
      __syncthreads();
      if (k0 + kQK < K) {   // (the image is padded to Kp: the whole tile is there)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          ra[i] = a8.load(i, k0 + kQK + 8 * t.lc);
          rb[i] = load_w8(wt, Kp, b_col[i], k0 + kQK + 8 * t.lc);
        }
      }
      // always the whole tile: beyond K both operands are zeros in LDS, and a zero product leaves a sum as it is
#pragma unroll
      for (int s = 0; s < kQK / 16; ++s)
        mfma_2x2(*reinterpret_cast<const bf16x8*>(pa + 16 * s), *reinterpret_cast<const bf16x8*>(pa + 32 * kQLd + 16 * s),
                 *reinterpret_cast<const bf16x8*>(pb + 16 * s), *reinterpret_cast<const bf16x8*>(pb + 32 * kQLd + 16 * s),
                 acc);
    }
    if constexpr (kChain > 0) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) out[a][b] += acc[a][b];
    }
    kc = kend;
  } while (kChain > 0 && kc < K);
}

// The walk over what a lane owns of the workgroup's tile.  For each of its columns c < N, column(c) gives the
// callable of that column, which then gets (row, v0, v1) for every pair of registers r, r + 1: v0 belongs to `row`
// (even) and v1 to row + 1, the position pair of a pool.  Rows may lie beyond M: the callable checks.
template <class Column>
__device__ __forceinline__ void for_each_owned_pair(const Tile& t, const f32x16 (&acc)[2][2], int N, Column&& column) {
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int c = t.n0 + t.wn * 64 + tn * 32 + t.li;
    if (c >= N) continue;
    auto pair = column(c);
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const int64_t row = t.m0 + t.wm * 64 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * t.lh;
        pair(row, acc[tm][tn][r], acc[tm][tn][r + 1]);
      }
    }
  }
}

// Host: one workgroup per tile of an M x N result.  `too_many`: the caller's wording when the grid does not fit.
inline int gemm_tile_grid(int64_t M, int N, const char* too_many, unsigned* grid, int* tiles_n) {
  const int64_t tiles_m = (M + kBM - 1) / kBM;
  *tiles_n = (N + kBN - 1) / kBN;
  if (tiles_m * *tiles_n > 0x7FFFFFFFll) return set_error(SNF_E_INVALID, too_many);
  *grid = static_cast<unsigned>(tiles_m * *tiles_n);
  return SNF_OK;
}

}  // namespace
}  // namespace snf
