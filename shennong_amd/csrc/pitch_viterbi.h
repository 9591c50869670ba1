// What the three Viterbi kernels of the pitch tracker share around their forward passes (kernels_pitch_viterbi.hip:
// a lane per state, one wave or a team of waves per utterance; kernels_pitch_flat.hip: a lane per candidate): the
// traceback and the output rows.  (Each kernel finds its utterance in its own first lines: a shared helper for
// them was built in four forms and every form changed the register allocation of all four kernels - the
// compiler's output follows where the early returns and the conditional loads of the ballasts stand.)
#ifndef SNF_PITCH_VITERBI_H_
#define SNF_PITCH_VITERBI_H_

#include "pitch_wave.h"

namespace snf {

namespace {

struct VitShared {
  float* fwd;    // [num_states + kFwdPad]
  float* nxt;    // [num_states]
  int* bpw;      // [num_states]   backpointers of the current frame
  int4* queue;   // [64]           (state, lo, hi) of the long windows of a pass
};

// traceback of one utterance by ONE wave: best final state (lowest index wins ties), then the chain of
// backpointers -> states[f0 ...]; `sh.fwd` holds the final forward costs, `sh.nxt` is scratch
__device__ __forceinline__ void viterbi_traceback(const int S, const int64_t T, const int64_t f0,
                                                  const int16_t* __restrict__ bp, int32_t* __restrict__ states,
                                                  const VitShared& sh, const int lane) {
  __threadfence_block();
  {
    float bv = FLT_MAX;
    int best = 0x7fffffff;
    for (int s = lane; s < S; s += 64) {
      const float c = sh.fwd[s];
      if (c < bv) { bv = c; best = s; }
    }
    wave_argmin(bv, best);
    // 64 frames at a time.  The chain of dependent 2-byte loads is the whole cost (a trip to HBM per
    // frame), so the wave first touches the rows of the chunk at the columns around the current state -
    // the path moves a few states per frame, the touched lines hold 64 - and lane 0 then walks through
    // lines that are already in the cache; the path goes to LDS and is written out 64 frames at once
    // (a store inside the chain would be waited for together with every load).
    int* trace = reinterpret_cast<int*>(sh.nxt);
    for (int64_t hi = T; hi > 0; hi -= 64) {
      const int n = hi < 64 ? static_cast<int>(hi) : 64;
      best = __builtin_amdgcn_readfirstlane(best);
      {
        int col_t = best + ((lane & 32) ? 24 : -24);
        col_t = col_t < 0 ? 0 : (col_t > S - 1 ? S - 1 : col_t);
        const int64_t fa = hi - 1 - (lane & 31), fb = fa - 32;
        const int16_t va = bp[(fa > 0 ? fa : 0) * S + col_t], vb = bp[(fb > 0 ? fb : 0) * S + col_t];
        asm volatile("" : : "v"(va), "v"(vb));
      }
      if (lane == 0) {
        for (int k = 0; k < n; ++k) {
          trace[k] = best;
          best = bp[(hi - 1 - k) * S + best];
        }
      }
      wave_sync();
      if (lane < n) states[f0 + hi - 1 - lane] = trace[lane];
      wave_sync();
    }
  }
}

// output rows of one utterance: (POV NCCF resampled at the chosen lag, 1 / lag); frames first, first + stride, ...
__device__ __forceinline__ void pitch_output_rows(const PitchDevTables& t, const int L, const int64_t T,
                                                  const int64_t f0, const int32_t* __restrict__ states,
                                                  const float* __restrict__ pov_nccf, float* __restrict__ out,
                                                  const int first, const int stride) {
  for (int64_t frame = first; frame < T; frame += stride) {
    const int s = states[f0 + frame];
    const float* __restrict__ wt = t.ar_w + s * t.ar_max_taps;
    const float* __restrict__ src = pov_nccf + frame * L + t.ar_first[s];
    const int n = t.ar_n[s];
    float pov = 0.0f;
    for (int j = 0; j < n; ++j) pov = __builtin_fmaf(src[j], wt[j], pov);
    out[(f0 + frame) * 2 + 0] = pov;
    out[(f0 + frame) * 2 + 1] = 1.0f / t.lags[s];
  }
}

}  // namespace

}  // namespace snf

#endif  // SNF_PITCH_VITERBI_H_
