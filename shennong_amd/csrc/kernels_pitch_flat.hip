// Stage 4 of the Kaldi pitch tracker, third form: pitch_viterbi_flat_kernel (kernels_pitch_front.hip has the
// arithmetic contract, pitch_route.h says when this form runs and the LDS it needs, pitch_viterbi.h holds the
// traceback and the output rows it shares with kernels_pitch_viterbi.hip).
#include "pitch_viterbi.h"

namespace snf {

namespace {

// ---- 4c. the same forward pass with a lane per CANDIDATE (round 5) ------------------------------------------
// The search of kernels_pitch_viterbi.hip gives a lane to every STATE and lets it scan its window, which is as long
// as the backpointer function is steep there: windows of 1 to 100+ candidates side by side in one wave, hence the scan loops, the
// queue of long windows, the 8-lane teams and five levels of set-up - 3 070 instructions per frame and wave
// of which the candidate arithmetic is a sixth (profiles/r05_pmc_pitch10k_before_summary.txt,
// tools/pitch_search_replay.py).  Here every lane owns seven consecutive CANDIDATES j = 7 lane + k.  Per level
// (the multiples of 128 exactly, then of 32, 8, 4, then every state - the same five levels):
//   * the backpointers of the known states are counted into marks[j]; a prefix sum over j (six adds per lane, one
//     scan over the lanes) tells every candidate between which two known states' backpointers it lies: its gap;
//   * a candidate strictly inside a gap offers its cost to the (one or three) new states of that gap with ONE LDS
//     instruction each: an atomic minimum on the 64-bit key (cost bits << 32 | j) - costs are non-negative
//     floats, so the unsigned order of the keys is "lower cost first, lower index on ties", Kaldi's rule;
//   * the two ends of a window (candidates that ARE a known backpointer belong to two windows) are offered by the
//     new state itself, which thereby also initialises its key.
// No loop depends on the data, there is no long-window case, and a jump of the backpointer function costs what
// its candidates cost, once per level.  Same candidates per state, same arithmetic (d = j - i exact in float,
// fl(fl(d d) f) + fwd[j] without contraction), same tie-break: bit-identical to viterbi_forward.
// MEASURED (10 000 x 3 s, same box, whole pitch call; lane-per-state kernel 14.1-14.3 ms, 3 070 instructions per
// frame and wave).  An LDS atomic costs ~0.6 clocks per active LANE: one per candidate: 35 ms; one per run of a
// lane's candidates that share a gap: 16.0; level 1 through DPP instead of four 64-lane atomics on one key: 15.2;
// the two coarse levels (13 states, windows hundreds of candidates wide, where every lane's last run hits one of
// 3 keys) in the lane-per-state form of viterbi_forward: 13.8; keys in four planes by state mod 4 (bank conflicts
// 490 -> 320 clocks per frame): 13.6; window ends by a lane per gap instead of per new state: 13.1; marks cumulative
// over the levels of a frame: 13.0; a run's restart as arithmetic: 12.6; (cost, index) keys reduced over the lanes with
// one 64-bit compare per step, level 1 as a scalar loop, level 2 on 60 lanes: **11.8-11.9 ms**, 2 050 instructions per
// frame and wave (tools/experiments/README.md has the table).  The default since then (SNF_PITCH_FLAT=0: the
// lane-per-state kernel).
constexpr int kFlatCand = 7;               // candidates per lane: 7 x 64 = 448 states at most

struct FlatShared {
  float* fwd;                   // [448 + kFwdPad]  normalised forward costs of the previous frame (FLT_MAX behind S)
  unsigned long long* slots;    // [kFlatSlots]     key of every state: cost bits << 32 | backpointer
  unsigned* marks;              // [448]            number of known states whose backpointer is j
};

// exclusive prefix sum over the 64 lanes (DPP inside the 16-lane rows, the three row totals through v_readlane)
__device__ __forceinline__ int wave_exclusive_sum(int v, int lane) {
  int t = v;
  t += __builtin_amdgcn_update_dpp(0, t, 0x111, 0xf, 0xf, true);   // row_shr:1
  t += __builtin_amdgcn_update_dpp(0, t, 0x112, 0xf, 0xf, true);   // row_shr:2
  t += __builtin_amdgcn_update_dpp(0, t, 0x114, 0xf, 0xf, true);   // row_shr:4
  t += __builtin_amdgcn_update_dpp(0, t, 0x118, 0xf, 0xf, true);   // row_shr:8
  const int r0 = __builtin_amdgcn_readlane(t, 15), r1 = __builtin_amdgcn_readlane(t, 31),
            r2 = __builtin_amdgcn_readlane(t, 47);
  int base = lane >= 16 ? r0 : 0;
  base += lane >= 32 ? r1 : 0;
  base += lane >= 48 ? r2 : 0;
  return t + base - v;
}

// Where the key of state u lives: four planes by u mod 4, each indexed by u / 4.  At the last level the known
// states (multiples of 4) and each of the three kinds of new states are then contiguous, at the level before the
// known states are two entries apart: with the keys in state order every access of a level was 32 / 64 / 256
// bytes apart - 4, 2 or 1 banks for the whole wave (SQ_LDS_BANK_CONFLICT 490 clocks per frame and wave).
constexpr int kFlatPlane = kFlatSlots / 4;
__device__ __forceinline__ int flat_slot(int u) { return (u & 3) * kFlatPlane + (u >> 2); }

// minimum of two floats that are never NaN: fminf() quiets its operands first (a v_max_f32 x, x per call)
__device__ __forceinline__ float min_nonan(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ __forceinline__ unsigned long long flat_key(float cost, int j) {
  return (static_cast<unsigned long long>(__builtin_bit_cast(unsigned, cost)) << 32) | static_cast<unsigned>(j);
}

// one step of an argmin over lanes ON THE KEYS: the unsigned order of (cost bits, index) is "lower cost, then lower
// index" for non-negative costs - two DPP moves, one 64-bit compare and two selects, where the same step on a
// (float, int) pair compiles to four compares and two exec-masked blocks
template <int CTRL>
__device__ __forceinline__ unsigned long long key_min_step(unsigned long long key) {
  const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<unsigned>(key)), CTRL, 0xf, 0xf, true));
  const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(static_cast<unsigned>(key >> 32)), CTRL, 0xf, 0xf, true));
  const unsigned long long other = (static_cast<unsigned long long>(hi) << 32) | lo;
  return other < key ? other : key;
}
// the same with the key of the lane `CTRL` names taken from `from` (row_shl:n: lane + n of the row; a lane whose
// source lies outside its row keeps its own halves of `from`)
template <int CTRL>
__device__ __forceinline__ unsigned long long key_min_shl(unsigned long long key, unsigned long long from) {
  const int flo = static_cast<int>(static_cast<unsigned>(from)), fhi = static_cast<int>(static_cast<unsigned>(from >> 32));
  const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_update_dpp(flo, flo, CTRL, 0xf, 0xf, false));
  const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_update_dpp(fhi, fhi, CTRL, 0xf, 0xf, false));
  const unsigned long long other = (static_cast<unsigned long long>(hi) << 32) | lo;
  return other < key ? other : key;
}

// one level: the states u = g KNOWN + (s + 1) NEW (s < KNOWN / NEW - 1) of every gap g between the known states
// g KNOWN and (g + 1) KNOWN
// FRESH: the stride of the states that became known since the marks were last brought up to date (the marks are
// cumulative over the levels of a frame: only the backpointers of those states are added)
template <int KNOWN, int NEW, int FRESH_FROM>
__device__ __forceinline__ void flat_level(const FlatShared& sh, const int S, const float factor, const int lane,
                                           const float (&fj)[kFlatCand], const float jf0) {
  constexpr int M = KNOWN / NEW - 1;
  static_assert(M == 1 || M == 3, "one or three new states per gap");
  const int n_gaps = S > NEW ? (S - NEW - 1) / KNOWN + 1 : 0;   // gaps that hold a new state below S
  const unsigned* __restrict__ bps = reinterpret_cast<const unsigned*>(sh.slots);   // plane 0, low words: backpointers
  unsigned* __restrict__ mk_lane = sh.marks + kFlatCand * lane;
  // The phases of a level are LDS round trips of one wave; what does not depend on each other is issued together:
  // (1) the backpointers the marks still lack and the two ends of every window, (2) the marks' atomic adds and the
  // forward costs at the window ends, (3) the lane's seven marks and the keys of the window ends.
  // ---- marks: the states t FRESH (FRESH_FROM == 0: all known states; else those that are not multiples of
  // FRESH_FROM) became known at the previous level
  constexpr int FRESH = KNOWN;
  const int n_fresh = (S + FRESH - 1) / FRESH;
  for (int t0 = 0; t0 < n_fresh; t0 += 64) {
    const int t = t0 + lane;
    const bool fresh = t < n_fresh && (FRESH_FROM == 0 || (t * FRESH) % FRESH_FROM != 0);
    if (fresh) atomicAdd(&sh.marks[bps[2 * (t * (FRESH / 4))]], 1u);
  }
  // ---- the ends of every window: a lane per GAP offers lo and hi to each of the gap's new states (the three
  // states of a gap share the window: one pair of reads, keys written one entry or one plane apart) -----------
  for (int g0 = 0; g0 < n_gaps; g0 += 64) {
    const int g = g0 + lane;
    if (g < n_gaps) {
      const int above = (g + 1) * KNOWN;
      const int lo = static_cast<int>(bps[2 * (g * (KNOWN / 4))]);
      const int hi = above < S ? static_cast<int>(bps[2 * (above / 4)]) : S - 1;
      const float f_lo = sh.fwd[lo], f_hi = sh.fwd[hi];
      const float e_lo = static_cast<float>(lo - g * KNOWN), e_hi = static_cast<float>(hi - g * KNOWN);
      unsigned long long* __restrict__ first = sh.slots + g * (KNOWN / 4);
#pragma unroll
      for (int sidx = 0; sidx < M; ++sidx) {
        // (a new state behind the last state of a partial gap gets a key nobody reads: the array has the room)
        const float d_lo = e_lo - static_cast<float>((sidx + 1) * NEW), d_hi = e_hi - static_cast<float>((sidx + 1) * NEW);
        const float c_lo = __fadd_rn(__fmul_rn(d_lo * d_lo, factor), f_lo);
        const float c_hi = __fadd_rn(__fmul_rn(d_hi * d_hi, factor), f_hi);
        first[NEW >= 4 ? (sidx + 1) * (NEW / 4) : (sidx + 1) * kFlatPlane] =
            c_hi < c_lo ? flat_key(c_hi, hi) : flat_key(c_lo, lo);   // (lo <= hi: the lower index on ties)
      }
    }
  }
  wave_sync();
  int mk[kFlatCand], gap[kFlatCand];
  int total = 0;
#pragma unroll
  for (int k = 0; k < kFlatCand; ++k) {
    mk[k] = static_cast<int>(mk_lane[k]);
    total += mk[k];
  }
  int count = wave_exclusive_sum(total, lane);   // known states with a backpointer below this lane's candidates
#pragma unroll
  for (int k = 0; k < kFlatCand; ++k) {
    count += mk[k];
    gap[k] = count - 1;                           // candidate j lies right of (or on) the backpointer of state gap
  }
  // ---- the candidates strictly inside a window ---------------------------------------------------------
  // An LDS atomic costs ~0.6 clocks per LANE whatever the addresses (measured: one atomic per candidate and
  // state, 4 400 lane operations per frame, was 2 500 LDS clocks per frame and wave - three times the whole
  // lane-per-state search).  The seven candidates of a lane are consecutive, so they fall into runs that share a
  // gap: the lane keeps the best of the run in registers (ascending j, strict <: the lower index on ties) and
  // offers it once, when the gap changes or its candidates end - 1 300 lane operations per frame.
  // A candidate that carries a mark (it IS a known backpointer) opens a new gap and is itself outside every
  // window: the lane's running best restarts there (and at its first candidate); it is offered at the last
  // candidate before the next mark (or at the lane's last one) if the run saw any candidate.
  float bc[M];
  int bj[M];
#pragma unroll
  for (int sidx = 0; sidx < M; ++sidx) {
    bc[sidx] = FLT_MAX;
    bj[sidx] = 0;
  }
#pragma unroll
  for (int k = 0; k < kFlatCand; ++k) {
    const int j = kFlatCand * lane + k;
    const bool restart = k == 0 || mk[k] != 0;
    // (one unsigned comparison for 0 <= gap < n_gaps; candidates behind the last state need no test: their
    // forward cost is the FLT_MAX padding)
    const bool inside = mk[k] == 0 && static_cast<unsigned>(gap[k]) < static_cast<unsigned>(n_gaps);
    // (a candidate that is not inside a window offers FLT_MAX: x + FLT_MAX = FLT_MAX for these x, never < best)
    const float fjm = inside ? fj[k] : FLT_MAX;
    const int ub = gap[k] * KNOWN;
    const float e = (jf0 + static_cast<float>(k)) - static_cast<float>(ub);   // j - g KNOWN: exact
    // (a restart as arithmetic: best + inf = inf, which every cost is below - an add in place of two selects on
    // a scalar mask per state; best + 0 = best exactly, the costs being >= +0)
    const float reset = restart ? __builtin_inff() : 0.0f;
#pragma unroll
    for (int sidx = 0; sidx < M; ++sidx) {
      const float d = e - static_cast<float>((sidx + 1) * NEW);
      const float c = __fadd_rn(__fmul_rn(d * d, factor), fjm);
      const float kept = __fadd_rn(bc[sidx], reset);
      bj[sidx] = c < kept ? j : bj[sidx];
      bc[sidx] = min_nonan(kept, c);
    }
    const bool last_of_run = k == kFlatCand - 1 || mk[k + (k < kFlatCand - 1 ? 1 : 0)] != 0;
    if (last_of_run && bc[0] < FLT_MAX) {   // (the states of a gap see the same candidates: one test for all)
      // (ub is a multiple of 4: plane 0 at ub / 4; the new states are whole entries or whole planes further)
      unsigned long long* __restrict__ first = sh.slots + (ub >> 2);
#pragma unroll
      for (int sidx = 0; sidx < M; ++sidx)
        atomicMin(first + (NEW >= 4 ? (sidx + 1) * (NEW / 4) : (sidx + 1) * kFlatPlane), flat_key(bc[sidx], bj[sidx]));
    }
  }
  wave_sync();
}

// one forward pass over all frames (S <= 448); returns with sh.fwd = final normalised forward cost
__device__ void viterbi_forward_flat(const PitchDevTables& t, const float* __restrict__ res,
                                     const float* __restrict__ anp, int64_t T, int64_t T1, bool rescale,
                                     float old_b1, float old_b2, float new_ballast, int16_t* __restrict__ bp,
                                     const FlatShared& sh, const float* __restrict__ st_lag, const int lane) {
  constexpr int NK = 7;
  const int S = t.num_states;
  for (int s = lane; s < S; s += 64) sh.fwd[s] = 0.0f;
  for (int s = S + lane; s < 448 + kFwdPad; s += 64) sh.fwd[s] = FLT_MAX;
  const float factor = t.inter_frame_factor;
  float ahead[NK], soft_lag[NK];
  int col[NK], bpv[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    col[k] = lane + 64 * k < S ? lane + 64 * k : S - 1;
    ahead[k] = T > 0 ? res[col[k]] : 0.0f;
    soft_lag[k] = t.soft_min_f0 * st_lag[col[k]];
    bpv[k] = 0;
  }
  const float jf0 = static_cast<float>(kFlatCand * lane);
  const float* __restrict__ fwd_lane = sh.fwd + kFlatCand * lane;
  for (int64_t frame = 0; frame < T; ++frame) {
    float scale = 1.0f;
    if (rescale) {
      const float old_ballast = frame < T1 ? old_b1 : old_b2, a = anp[frame];
      scale = sqrtf((old_ballast + a) / (new_ballast + a));
    }
    const float* __restrict__ row = res + frame * static_cast<int64_t>(S);
    // local costs (kept in registers until the end of the frame), the backpointers of the previous frame, the
    // row of the next one: as in viterbi_forward (see there for the order of the memory operations)
    float local[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      float v = ahead[k];
      if (rescale) v *= scale;
      local[k] = 1.0f - v;
      local[k] += soft_lag[k] * v;
    }
    if (frame > 0) {
      int16_t* __restrict__ bp_row = bp + (frame - 1) * S;
#pragma unroll
      for (int k = 0; k < NK; ++k) bp_row[col[k]] = static_cast<int16_t>(bpv[k]);
    }
    const float* __restrict__ nrow = frame + 1 < T ? row + S : row;
#pragma unroll
    for (int k = 0; k < NK; ++k) ahead[k] = nrow[col[k]];
    // ---- the lane's seven candidates ----------------------------------------------------------------------
    wave_sync();
    float fj[kFlatCand];
#pragma unroll
    for (int k = 0; k < kFlatCand; ++k) fj[k] = fwd_lane[k];
    {
      // (the marks of a frame are cumulative over its levels: zeroed once, here)
      unsigned* __restrict__ mk_lane = sh.marks + kFlatCand * lane;
#pragma unroll
      for (int k = 0; k < kFlatCand; ++k) mk_lane[k] = 0u;
    }
    // ---- levels 1 and 2 as in viterbi_forward (a 16-lane row per state of level 1 over all candidates, 4 lanes per
    // state of level 2 over its window: 13 states whose windows are hundreds of candidates wide - the lane-per-
    // candidate form pays for them with one DPP reduction per state or with 64 lanes on 3 keys), keys to `slots` --
    {
      const int n_super = (S + 127) >> 7, n_reps = (S + 31) >> 5;
      for (int base = 0; base < n_super; base += 4) {
        const int r = base + (lane >> 4), sub = lane & 15;
        const int i_rep = r << 7;
        float best = FLT_MAX;
        int best_j = 0x7fffffff;
        if (r < n_super) {
          const float fi = static_cast<float>(i_rep);
          float d = static_cast<float>(sub) - fi, bd = 1.0e9f;
          // (the same number of steps in every lane - a scalar loop, no exec mask: the reads behind S - 1 land in
          // the FLT_MAX padding, whose cost FLT_MAX is below nothing)
          // (three steps per trip, their reads first: at most 47 entries behind S - 1, inside the 448 + kFwdPad
          // entries that hold FLT_MAX from S on for every S <= 448)
          const int n_steps = (S + 15) >> 4;
          const float* __restrict__ fw = sh.fwd + sub;
          float f3[3], g3[3];
#pragma unroll
          for (int w = 0; w < 3; ++w) f3[w] = fw[16 * w];
          for (int t = 0; t < n_steps; t += 3) {
            if (t + 3 < n_steps) {   // (scalar branch: the next trip's reads run under this trip's arithmetic)
#pragma unroll
              for (int w = 0; w < 3; ++w) g3[w] = fw[16 * (t + 3 + w)];
            }
#pragma unroll
            for (int w = 0; w < 3; ++w) {
              const float c = __fadd_rn(__fmul_rn(d * d, factor), f3[w]);
              const bool better = c < best;   // (one compare, two selects on vcc: no minimum, no canonicalisation)
              bd = better ? d : bd;
              best = better ? c : best;
              d += 16.0f;
            }
#pragma unroll
            for (int w = 0; w < 3; ++w) f3[w] = g3[w];
          }
          best_j = static_cast<int>(fi + bd);
        }
        unsigned long long key = flat_key(best, best_j);
        key = key_min_step<0xB1>(key);    // quad_perm [1,0,3,2]
        key = key_min_step<0x4E>(key);    // quad_perm [2,3,0,1]
        key = key_min_step<0x124>(key);   // row_ror:4
        key = key_min_step<0x128>(key);   // row_ror:8
        if (sub == 0 && r < n_super) {
          if (static_cast<unsigned>(key) >= static_cast<unsigned>(S)) key &= 0xffffffff00000000ull;   // (index 0)
          sh.slots[flat_slot(i_rep)] = key;
        }
      }
      wave_sync();
      // (five lanes per state, three states per 16-lane row: up to twelve states per trip - the ten multiples
      // of 32 below 448 that are not multiples of 128 - on 60 lanes; four lanes per state used 40 and took a
      // third more trips of the candidate loop)
      for (int base = 0; base < n_reps; base += 12) {
        const int in_row = lane & 15, group = (in_row * 13) >> 6, sub = in_row - 5 * group;   // in_row / 5, % 5
        const int k = base + 3 * (lane >> 4) + group;
        const int m = k + k / 3 + 1;
        const int i_rep = group < 3 ? m << 5 : S;   // (lane 15 of a row: idle)
        float best = FLT_MAX;
        int best_j = 0x7fffffff, lo = 0;
        if (i_rep < S) {
          const int below = i_rep & ~127, above = below + 128;
          lo = static_cast<int>(static_cast<unsigned>(sh.slots[flat_slot(below)]));
          const int hi = above < S ? static_cast<int>(static_cast<unsigned>(sh.slots[flat_slot(above)])) : S - 1;
          const float fi = static_cast<float>(i_rep);
          float d = static_cast<float>(lo + sub) - fi, bd = d;
          // (reads up to 35 entries behind hi <= S - 1: inside the kFwdPad entries of FLT_MAX)
          for (int j = lo + sub; j <= hi; j += 40) {
            float ff[8];
#pragma unroll
            for (int w = 0; w < 8; ++w) ff[w] = sh.fwd[j + 5 * w];
#pragma unroll
            for (int w = 0; w < 8; ++w) {
              const float dw = d + static_cast<float>(5 * w);
              const float c = __fadd_rn(__fmul_rn(dw * dw, factor), ff[w]);
              bd = c < best ? dw : bd;
              best = fminf(best, c);
            }
            d += 40.0f;
          }
          best_j = static_cast<int>(fi + bd);
        }
        // the five keys of a state -> its lane sub == 0: neighbours (row_shl:1), pairs (row_shl:2), the fifth
        unsigned long long key = flat_key(best, best_j);
        const unsigned long long own = key;
        key = key_min_shl<0x101>(key, key);
        key = key_min_shl<0x102>(key, key);
        key = key_min_shl<0x104>(key, own);
        if (sub == 0 && i_rep < S) {
          // (only if every cost was NaN / inf: the lower end of the window, which lane sub == 0 still holds)
          if (static_cast<unsigned>(key) >= static_cast<unsigned>(S)) key = (key & 0xffffffff00000000ull) | static_cast<unsigned>(lo);
          sh.slots[flat_slot(i_rep)] = key;
        }
      }
      wave_sync();
    }
    flat_level<32, 8, 0>(sh, S, factor, lane, fj, jf0);
    flat_level<8, 4, 32>(sh, S, factor, lane, fj, jf0);
    flat_level<4, 1, 8>(sh, S, factor, lane, fj, jf0);
    // ---- new forward costs: best + local cost, minus their minimum ----------------------------------------
    float nx[NK], lane_min = FLT_MAX;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const unsigned long long key = sh.slots[flat_slot(col[k])];
      bpv[k] = static_cast<int>(static_cast<unsigned>(key));
      nx[k] = __builtin_bit_cast(float, static_cast<unsigned>(key >> 32)) + local[k];
      lane_min = fminf(lane_min, nx[k]);
    }
    const float mn = wave_min_f(lane_min);
    wave_sync();
#pragma unroll
    for (int k = 0; k < NK; ++k) sh.fwd[col[k]] = nx[k] + (-mn);
  }
  if (T > 0) {
    int16_t* __restrict__ bp_row = bp + (T - 1) * S;
#pragma unroll
    for (int k = 0; k < NK; ++k) bp_row[col[k]] = static_cast<int16_t>(bpv[k]);
  }
  wave_sync();
}

}  // namespace

// one wavefront per utterance with the lane-per-candidate search (viterbi_forward_flat): 129 .. 448 states
__global__ __launch_bounds__(kFlatWaves * 64, 4) void pitch_viterbi_flat_kernel(
    const PitchDevTables t, const PitchBatch b, const float* __restrict__ nccf_res,
    const float* __restrict__ anp, const float* __restrict__ ub, int16_t* __restrict__ backptr,
    int32_t* __restrict__ states, const float* __restrict__ pov_all, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int S = t.num_states, L = t.num_lags, S4 = (S + 3) & ~3;
  float* st_lag = reinterpret_cast<float*>(smem);
  for (int s = threadIdx.x; s < S; s += blockDim.x) st_lag[s] = t.lags[s];
  __syncthreads();
  // (the wave's index as a SCALAR: the utterance, its offsets and the row pointers derived from them then live in
  // scalar registers - 128 -> 124 vector registers and no spill left in the kernel)
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t slot = static_cast<int64_t>(blockIdx.x) * kFlatWaves + wid;
  if (slot >= b.n_utts) return;
  // (values loaded at a uniform address arrive in vector registers: back to scalars, see wid)
  const int64_t u = uniform_i64(b.order ? b.order[slot] : slot);
  const int64_t f0 = uniform_i64(b.frame_offsets[u]), T = uniform_i64(b.frame_offsets[u + 1]) - f0;
  if (T <= 0) return;
  const int64_t T1 = uniform_i64(b.frames_phase1[u]);
  // per wave: keys (8-byte aligned: first), forward costs, marks
  // (the lags' bytes are pitch_flat_lags_bytes(S4), written out: through the function the compiler folds the
  // rounding of S4 into it another way and the kernel's listing changes by one instruction)
  char* mine = smem + ((S4 * 4 + 15) & ~15) + wid * kFlatWaveBytes;  FlatShared fs;
  fs.slots = reinterpret_cast<unsigned long long*>(mine);
  fs.fwd = reinterpret_cast<float*>(mine + kFlatSlots * 8);
  fs.marks = reinterpret_cast<unsigned*>(mine + kFlatSlots * 8 + (448 + kFwdPad) * 4);
  int16_t* __restrict__ bp = backptr + f0 * S;
  const float* __restrict__ res = nccf_res + f0 * static_cast<int64_t>(S);
  const float* __restrict__ pov_nccf = pov_all + f0 * L;
  const float* __restrict__ o = ub + u * 6;
  const bool recompute = (T < t.recompute_frame || T1 < t.recompute_frame) && o[5] != 0.0f;   // (see pitch_viterbi_kernel)
  const float ob1 = recompute ? o[2] : 0.0f, ob2 = recompute ? o[3] : 0.0f, nb = recompute ? o[4] : 0.0f;
  viterbi_forward_flat(t, res, anp + f0, T, T1, recompute, ob1, ob2, nb, bp, fs, st_lag, lane);
  // traceback: its scratch (64 ints) goes where the marks were
  VitShared sh;
  sh.fwd = fs.fwd;
  sh.nxt = reinterpret_cast<float*>(fs.marks);
  sh.bpw = nullptr;
  sh.queue = nullptr;
  viterbi_traceback(S, T, f0, bp, states, sh, lane);
  wave_sync();
  __threadfence_block();
  pitch_output_rows(t, L, T, f0, states, pov_nccf, out, lane, 64);
}

int launch_pitch_viterbi_flat(const PitchDevTables& t, const PitchBatch& b, const PitchScratch& w, size_t lds,
                              float* out, hipStream_t stream) {
  if (lds > 64 * 1024)
    SNF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(pitch_viterbi_flat_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  const unsigned blocks = static_cast<unsigned>((b.n_utts + kFlatWaves - 1) / kFlatWaves);
  hipLaunchKernelGGL(pitch_viterbi_flat_kernel, dim3(blocks), dim3(kFlatWaves * 64), lds, stream, t, b,
                     w.nccf_res, w.anp, w.ub, w.backptr, w.states, w.pov_nccf, out);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

}  // namespace snf
