// Cross-lane and search helpers of the pitch tracker that more than one of its translation units uses
// (kernels_pitch_front.hip, kernels_pitch_viterbi.hip, kernels_pitch_flat.hip).  Every file that includes this is
// compiled with -ffp-contract=off: see the arithmetic contract at the head of kernels_pitch_front.hip.
// (kFwdPad and the other constants of the LDS layouts: pitch_route.h, which the launcher reads on the host.)
#ifndef SNF_PITCH_WAVE_H_
#define SNF_PITCH_WAVE_H_

#include <float.h>

#include "snf_internal.h"
#include "pitch_route.h"

namespace snf {

namespace {

// Ordering point between the phases of ONE wave over LDS that only this wave touches (every wave of the
// Viterbi / NCCF kernels owns its slice; the one shared table is written before the __syncthreads of the
// prologue): the LDS executes a wave's instructions in issue order, so only the compiler must keep the
// accesses in program order - wavefront-scope fences emit no instruction, where workgroup scope costs an
// s_waitcnt lgkmcnt(0) (the wave sits until every store is acknowledged) at each of the ~12 points per frame
// (round 4; tools/experiments/README.md has the workgroup-scope form)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Cross-lane steps on the VALU (DPP + v_readlane); __shfl_xor lowers to ds_bpermute_b32, an LDS round
// trip per step.  quad_perm [1,0,3,2] = 0xB1, [2,3,0,1] = 0x4E; row_ror:4 = 0x124, row_ror:8 = 0x128
// (rotations reach the other three quads of a 16-lane row).
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf,
                                                               0xf, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
// a value every lane of the wave holds, moved to scalar registers
__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(v))));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint64_t>(v) >> 32)));
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}
__device__ __forceinline__ float lane_f(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// sum over the wave: DPP all-reduce inside the 16-lane rows, then the four row values (read with
// v_readlane) are combined uniformly, so every lane gets the same bits
__device__ __forceinline__ float wave_sum_v(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x124>(v);
  v += dpp_f<0x128>(v);
  return (lane_f(v, 0) + lane_f(v, 16)) + (lane_f(v, 32) + lane_f(v, 48));
}
__device__ __forceinline__ float wave_min_f(float v) {
  v = fminf(v, dpp_f<0xB1>(v));
  v = fminf(v, dpp_f<0x4E>(v));
  v = fminf(v, dpp_f<0x124>(v));
  v = fminf(v, dpp_f<0x128>(v));
  return fminf(fminf(lane_f(v, 0), lane_f(v, 16)), fminf(lane_f(v, 32), lane_f(v, 48)));
}
// (cost, index) argmin step: lower cost wins, lower index on ties.  Costs are non-negative floats and indices
// non-negative ints, so that is the unsigned order of (cost bits << 32 | index): one 64-bit compare and two selects
// (the float / int form compiled to four compares and two exec-masked blocks per step)
__device__ __forceinline__ void argmin_take(float& c, int& j, float oc, int oj) {
  const unsigned long long mine = (static_cast<unsigned long long>(__builtin_bit_cast(unsigned, c)) << 32) | static_cast<unsigned>(j);
  const unsigned long long other = (static_cast<unsigned long long>(__builtin_bit_cast(unsigned, oc)) << 32) | static_cast<unsigned>(oj);
  const bool take = other < mine;
  c = take ? oc : c;
  j = take ? oj : j;
}
__device__ __forceinline__ void quad_argmin(float& c, int& j) {
  argmin_take(c, j, dpp_f<0xB1>(c), dpp_i<0xB1>(j));
  argmin_take(c, j, dpp_f<0x4E>(c), dpp_i<0x4E>(j));
}
__device__ __forceinline__ void wave_argmin(float& c, int& j) {
  quad_argmin(c, j);
  argmin_take(c, j, dpp_f<0x124>(c), dpp_i<0x124>(j));
  argmin_take(c, j, dpp_f<0x128>(c), dpp_i<0x128>(j));
  float bc = lane_f(c, 0);
  int bj = __builtin_amdgcn_readlane(j, 0);
  argmin_take(bc, bj, lane_f(c, 16), __builtin_amdgcn_readlane(j, 16));
  argmin_take(bc, bj, lane_f(c, 32), __builtin_amdgcn_readlane(j, 32));
  argmin_take(bc, bj, lane_f(c, 48), __builtin_amdgcn_readlane(j, 48));
  c = bc;
  j = bj;
}

// cost of reaching state i from state j: must round exactly like Kaldi's
// (j - i)^2 * inter_frame_factor + prev_forward_cost[j] (no FMA contraction)
__device__ __forceinline__ float trans_cost(int j, float fi, float factor, float fwd_j) {
  const float d = static_cast<float>(j) - fi;
  return __fadd_rn(__fmul_rn(d * d, factor), fwd_j);
}

// exact argmin over j in [lo, hi] (lowest index wins ties), 4 candidates in flight per step.  The
// last step may look at up to 3 states beyond `hi`: the argmin is monotone in i, so none of them can
// beat the optimum inside the range (an equal cost loses to the lower index), and the forward costs
// are padded with FLT_MAX beyond the last state.
__device__ __forceinline__ void scan_range(const float* __restrict__ fwd, int lo, int hi, float fi,
                                           float factor, float& best, int& best_j) {
  // The running value is d = j - i (small integers: exact in float, so d equals Kaldi's j - i whichever way
  // it is reached); per candidate: one add, two multiplies, one add, one compare, one select (the best d)
  // and one minimum (costs are >= 0 and never NaN: the minimum IS the select of the cost).
  float d = static_cast<float>(lo) - fi;
  float b = __fadd_rn(__fmul_rn(d * d, factor), fwd[lo]), bd = d;
  // the four forward costs of a step are read one step ahead (behind the window: the FLT_MAX padding): the
  // LDS round trip of step n + 1 runs under the 28 vector instructions of step n instead of in front of them
  float n0 = fwd[lo + 1], n1 = fwd[lo + 2], n2 = fwd[lo + 3], n3 = fwd[lo + 4];
  for (int j = lo + 1; j <= hi; j += 4) {
    const float f0 = n0, f1 = n1, f2 = n2, f3 = n3;
    n0 = fwd[j + 4];
    n1 = fwd[j + 5];
    n2 = fwd[j + 6];
    n3 = fwd[j + 7];
    const float d0 = d + 1.0f, d1 = d + 2.0f, d2 = d + 3.0f, d3 = d + 4.0f;
    const float c0 = __fadd_rn(__fmul_rn(d0 * d0, factor), f0);
    const float c1 = __fadd_rn(__fmul_rn(d1 * d1, factor), f1);
    const float c2 = __fadd_rn(__fmul_rn(d2 * d2, factor), f2);
    const float c3 = __fadd_rn(__fmul_rn(d3 * d3, factor), f3);
    bd = c0 < b ? d0 : bd;
    b = fminf(b, c0);
    bd = c1 < b ? d1 : bd;
    b = fminf(b, c1);
    bd = c2 < b ? d2 : bd;
    b = fminf(b, c2);
    bd = c3 < b ? d3 : bd;
    b = fminf(b, c3);
    d = d3;
  }
  best = b;
  best_j = static_cast<int>(fi + bd);
}


// sum of the 16 values of a DPP row as a balanced tree of neighbours; every lane gets the same bits
__device__ __forceinline__ float tree16(float v) {
  v += dpp_f<0xB1>(v);   // quad_perm [1,0,3,2]: lane ^ 1
  v += dpp_f<0x4E>(v);   // quad_perm [2,3,0,1]: lane ^ 2
  v += dpp_f<0x141>(v);  // row_half_mirror: quad 0 <-> 1, 2 <-> 3
  v += dpp_f<0x140>(v);  // row_mirror: half 0 <-> 1
  return v;
}

}  // namespace

}  // namespace snf

#endif  // SNF_PITCH_WAVE_H_
