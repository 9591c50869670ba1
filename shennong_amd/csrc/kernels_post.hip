// What is left of the post-processing path once its families have files of their own (kernels_plp_tail.hip,
// kernels_delta.hip, kernels_pitch_post.hip, kernels_cmvn.hip): the column-wise concatenation of two feature blocks
// (reference features.py:386-437) and the non-finite count of Features.validate (features.py:170-215), with their
// launchers.  Both have one route.
#include "snf_internal.h"
#include "utt_search.h"

namespace snf {

// Column-wise concatenation of two feature blocks per utterance (reference Features.concatenate,
// features.py:386-437: the longer side is trimmed to the shorter one within the caller's tolerance):
// out[u][t] = [a[u][t], b[u][t]] for t < rows_out(u).  A workgroup owns kConcatRows consecutive output rows: one
// lane per row finds the row's utterance (the only search; it used to be one per ELEMENT) and leaves where the row
// starts in `a` and `b` in LDS; then the 256 lanes walk the rows' elements in output order - coalesced stores, and
// loads that are contiguous wherever consecutive rows belong to one utterance.  HBM-bound by design:
// 4 (ca + cb) bytes read + as many written per row.
constexpr int kConcatRows = 32;
__global__ __launch_bounds__(256) void concat_columns_kernel(
    const float* __restrict__ a, const int ca, const int64_t* __restrict__ off_a, const float* __restrict__ bm,
    const int cb, const int64_t* __restrict__ off_b, const int64_t n_utts, float* __restrict__ out,
    const int64_t* __restrict__ off_o, const int64_t total_rows) {
  __shared__ int64_t row_a[kConcatRows], row_b[kConcatRows];
  const int co = ca + cb;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kConcatRows;
  const int rows = static_cast<int>(total_rows - row0 < kConcatRows ? total_rows - row0 : kConcatRows);
  if (static_cast<int>(threadIdx.x) < rows) {
    const int64_t g = row0 + threadIdx.x;
    const int64_t u = find_utt(off_o, n_utts, g);
    const int64_t t = g - off_o[u];
    row_a[threadIdx.x] = (off_a[u] + t) * ca;
    row_b[threadIdx.x] = (off_b[u] + t) * cb - ca;   // (indexed with the output column)
  }
  __syncthreads();
  float* __restrict__ dst = out + row0 * co;
  const int count = rows * co;
  for (int i = threadIdx.x; i < count; i += 256) {
    const int r = i / co, c = i - r * co;
    dst[i] = c < ca ? a[row_a[r] + c] : bm[row_b[r] + c];
  }
}

int launch_concat_columns(const float* a, int cols_a, const int64_t* d_off_a, const float* b, int cols_b,
                          const int64_t* d_off_b, int64_t n_utts, float* out, const int64_t* d_off_out,
                          int64_t total_rows, hipStream_t stream) {
  if (total_rows <= 0) return SNF_OK;
  hipLaunchKernelGGL(concat_columns_kernel, dim3(static_cast<unsigned>((total_rows + kConcatRows - 1) / kConcatRows)),
                     dim3(256), 0, stream, a, cols_a, d_off_a, b, cols_b, d_off_b, n_utts, out, d_off_out,
                     total_rows);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

// Features.validate's data check (reference features.py:170-215 `is_valid`: "data contains non-finite
// numbers") for a block that is still in HBM: the number of NaN / +-Inf among n floats.  An exponent
// field of all ones is the test; 16-byte loads over the aligned body, the 0 - 3 floats behind it by the first
// lanes of workgroup 0.  A wave none of whose lanes saw a bad value adds nothing; in any other wave EVERY lane
// executes the atomic add with its own count (zeros included): one atomic per lane of such a wave as written,
// not one per workgroup - there is no reduction across the waves of a workgroup - and none in the usual case.
__global__ void __launch_bounds__(256) count_nonfinite_kernel(const float* __restrict__ x, uint64_t n,
                                                              unsigned long long* __restrict__ count) {
  const uint64_t n4 = n >> 2;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const u32x4* x4 = reinterpret_cast<const u32x4*>(x);
  unsigned bad = 0;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const u32x4 v = __builtin_nontemporal_load(x4 + i);
    bad += ((v.x & 0x7F800000u) == 0x7F800000u) + ((v.y & 0x7F800000u) == 0x7F800000u) +
           ((v.z & 0x7F800000u) == 0x7F800000u) + ((v.w & 0x7F800000u) == 0x7F800000u);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const unsigned v = __float_as_uint(x[(n4 << 2) + threadIdx.x]);
    bad += (v & 0x7F800000u) == 0x7F800000u;
  }
  if (__builtin_amdgcn_ballot_w64(bad != 0) == 0) return;  // (the usual case: nothing to add)
  atomicAdd(count, static_cast<unsigned long long>(bad));
}

int launch_count_nonfinite(const float* x, uint64_t n, unsigned long long* d_count, hipStream_t stream) {
  if (n == 0) return SNF_OK;
  const uint64_t want = (n / 4 + 255) / 256;
  const unsigned blocks = static_cast<unsigned>(want < 1 ? 1 : (want > 256 * 16 ? 256 * 16 : want));
  hipLaunchKernelGGL(count_nonfinite_kernel, dim3(blocks), dim3(256), 0, stream, x, n, d_count);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
