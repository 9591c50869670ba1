// Collation of a ragged feature block into a padded batch (snf_collate_padded; an extension, the reference hands
// every utterance to its caller as a numpy array of its own and has no call behind this):
//
//   out[u][j][(k + left) dim + d] = cast(in[row0(u) + clamp(offset + j subsample + k, 0, T_u - 1)][d])   j <  n_u
//   out[u][j][:]                  = cast(pad_value)                                                         j >= n_u
//   lengths[u]                    = n_u
//
// for j < t_max, k in [-left, right]: Kaldi's splice-feats (edge frames repeated) over the frames that
// subsample-feats keeps (offset, offset + subsample, ...), cast to float32 (a copy), float16 or bfloat16 (both to
// nearest, ties to even; v_cvt_pk_bf16_f32 for the latter).
//
// One HBM-bound pass.  The output is ONE flat 16-byte-aligned array whatever `dim` is, so a lane owns one 16-byte
// chunk of it (4 floats or 8 halves): it maps the chunk's first element back to (u, j, k, d) once - four divisions by
// launch constants -, steps through the chunk's elements with carries, and stores the chunk with one 16-byte store.
// Only the last chunk of the array can be narrower; it is stored element by element.  The loads are 4-byte loads:
// neither the utterance starts nor the spliced rows are 16-byte aligned for dim = 13, 39, 257...; consecutive lanes
// read consecutive addresses wherever the output row continues an input row.  Every byte of `out` and `lengths` is
// written.  Indices are 32-bit: the launcher refuses an output of 2^31 elements or more.
#include "snf_internal.h"

namespace snf {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

template <int TYPE>
__device__ __forceinline__ unsigned cast_pair(float lo, float hi);
template <>
__device__ __forceinline__ unsigned cast_pair<SNF_COLLATE_F16>(float lo, float hi) {
  f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
}
template <>
__device__ __forceinline__ unsigned cast_pair<SNF_COLLATE_BF16>(float lo, float hi) { return bf16_pack2(lo, hi); }

template <int TYPE>
__global__ __launch_bounds__(256) void collate_padded_kernel(const float* __restrict__ in,
                                                             const CollateUtt* __restrict__ utts, const CollateShape s,
                                                             const float pad, void* __restrict__ out,
                                                             int32_t* __restrict__ lengths) {
  constexpr int E = TYPE == SNF_COLLATE_F32 ? 4 : 8;   // elements of a 16-byte chunk
  const unsigned chunk = blockIdx.x * 256u + threadIdx.x;
  if (chunk < s.n_utts) lengths[chunk] = utts[chunk].n_out;
  // (chunk * E < 2^31 + 8 * 256: the launcher bounds `total`, the grid is rounded up to whole workgroups)
  const unsigned e0 = chunk * E;
  if (e0 >= s.total) return;
  unsigned u = e0 / s.utt_elems, r = e0 - u * s.utt_elems;
  int j = static_cast<int>(r / s.row_elems);
  r -= j * s.row_elems;
  int k = static_cast<int>(r / s.dim), d = static_cast<int>(r - k * s.dim);
  CollateUtt utt = utts[u];
  const float* row = in;
  bool valid = false;
  auto locate = [&]() {
    valid = j < utt.n_out;
    if (!valid) return;   // (a pad row: nothing is read, and j * subsample need not fit)
    int t = s.offset + j * s.subsample + k - s.left;   // (offset + j subsample < frames: it is a kept frame)
    t = t < utt.frames - 1 ? t : utt.frames - 1;
    t = t > 0 ? t : 0;
    row = in + (utt.row0 + t) * s.dim;
  };
  locate();
  float v[E];
#pragma unroll
  for (int i = 0; i < E; ++i) {
    // (past the end of the array - the last chunk - `u` has run off the table: nothing is read there)
    v[i] = (e0 + i < s.total && valid) ? row[d] : pad;
    if (++d == s.dim) {
      d = 0;
      if (++k == s.width) {
        k = 0;
        if (++j == s.t_max) {
          j = 0;
          if (++u < s.n_utts) utt = utts[u];
          else utt.n_out = 0;
        }
      }
      locate();
    }
  }
  if constexpr (TYPE == SNF_COLLATE_F32) {
    float* o = static_cast<float*>(out) + e0;
    if (e0 + E <= s.total) {
      u32x4 w = {__builtin_bit_cast(unsigned, v[0]), __builtin_bit_cast(unsigned, v[1]),
                 __builtin_bit_cast(unsigned, v[2]), __builtin_bit_cast(unsigned, v[3])};
      *reinterpret_cast<u32x4*>(o) = w;
    } else {
      for (int i = 0; i < E; ++i)
        if (e0 + i < s.total) o[i] = v[i];
    }
  } else {
    const u32x4 w = {cast_pair<TYPE>(v[0], v[1]), cast_pair<TYPE>(v[2], v[3]), cast_pair<TYPE>(v[4], v[5]),
                     cast_pair<TYPE>(v[6], v[7])};
    uint16_t* o = static_cast<uint16_t*>(out) + e0;
    if (e0 + E <= s.total) {
      *reinterpret_cast<u32x4*>(o) = w;
    } else {
      for (int i = 0; i < E; ++i)
        if (e0 + i < s.total) o[i] = static_cast<uint16_t>(w[i >> 1] >> (16 * (i & 1)));
    }
  }
}

}  // namespace

int launch_collate_padded(const float* in, const CollateUtt* d_utts, const CollateShape& shape, int out_type,
                          float pad_value, void* out, int32_t* lengths, hipStream_t stream) {
  if (shape.n_utts == 0) return SNF_OK;
  const int per_chunk = out_type == SNF_COLLATE_F32 ? 4 : 8;
  const uint64_t chunks = (static_cast<uint64_t>(shape.total) + per_chunk - 1) / per_chunk;
  const uint64_t lanes = chunks > shape.n_utts ? chunks : shape.n_utts;
  const dim3 grid(static_cast<unsigned>((lanes + 255) / 256)), block(256);
  if (out_type == SNF_COLLATE_F32)
    hipLaunchKernelGGL(collate_padded_kernel<SNF_COLLATE_F32>, grid, block, 0, stream, in, d_utts, shape, pad_value,
                       out, lengths);
  else if (out_type == SNF_COLLATE_F16)
    hipLaunchKernelGGL(collate_padded_kernel<SNF_COLLATE_F16>, grid, block, 0, stream, in, d_utts, shape, pad_value,
                       out, lengths);
  else
    hipLaunchKernelGGL(collate_padded_kernel<SNF_COLLATE_BF16>, grid, block, 0, stream, in, d_utts, shape, pad_value,
                       out, lengths);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
