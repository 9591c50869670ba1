// Which of the three Viterbi forms of the pitch tracker a batch runs on, and the LDS each form needs: the
// ladder launch_pitch (kernels_pitch_viterbi.hip) follows and the sizes its kernels carve their workgroup's
// block up with, stated once.  Plain C++17 - no device, no library -, so that tests/tools/pitch_route_dump.cpp
// compiles it alone (tests/test_pitch_route.py states the ladder a second time, independently).
#ifndef SNF_PITCH_ROUTE_H_
#define SNF_PITCH_ROUTE_H_

#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace snf {

constexpr int kFwdPad = 36;    // FLT_MAX entries behind the forward costs (unclamped scan steps)
constexpr int kQueueEntries = 128;                // long-window queue of a wave: int4 (state, lo, hi, -)
constexpr int kQueueFloats = kQueueEntries * 4;
constexpr int kTeam4Utts = 768;    // batches up to this many utterances: four waves per utterance,
constexpr int kTeam2Utts = 1280;   // up to this many: two (tools/time_pitch.py: 250 / 500 / 1 000 / 1 500
                                   // utterances take 3.20 / 3.29 / 3.46 / 3.61 ms with one wave, 2.40 / 2.63 /
                                   // 3.06 / 3.69 with two, 2.23 / 2.43 / 3.20 / 4.14 with four)
constexpr int kVitWaves = 8;   // utterances (= wavefronts) per workgroup of the Viterbi kernel
constexpr int kFlatSlots = 448 + 32;       // keys: a last partial gap of the first candidate level names states up to S + 15
constexpr int kFlatWaves = 8;              // utterances (= wavefronts) per workgroup: two workgroups per CU = 4 waves per SIMD
// (10 waves per workgroup and 96 registers = 5 waves per SIMD: 36 spilled registers, 14 scratch accesses per frame,
// 15.9 against 12.6 ms per 10 000 utterances)
constexpr int kFlatWaveBytes = kFlatSlots * 8 + (448 + kFwdPad) * 4 + 448 * 4;   // keys, forward costs, marks of a wave

// ---- LDS layouts, S4 = the state count rounded up to a multiple of 4.  Every form starts with the lags of the
// states (S4 floats), shared by the workgroup. ---------------------------------------------------------------
// by state (pitch_viterbi_kernel): per wave the forward costs and their padding, the new costs, the
// backpointers, the long-window queue (S4 and kFwdPad are multiples of 4: the queue is 16-byte aligned)
constexpr int pitch_state_wave_floats(int S4) { return 3 * S4 + kFwdPad + kQueueFloats; }
constexpr size_t pitch_state_lds_bytes(int S4) {
  return sizeof(float) * (S4 + static_cast<size_t>(kVitWaves) * pitch_state_wave_floats(S4));
}
// team of W waves (pitch_viterbi_team_kernel<W>): ONE state space, then W queues and W floats of the minimum
constexpr size_t pitch_team_lds_bytes(int S4, int W) {
  return sizeof(float) * (4 * static_cast<size_t>(S4) + kFwdPad + W * (kQueueFloats + 1));
}
// by candidate (pitch_viterbi_flat_kernel): the lags rounded up to 16 bytes (the keys are 8 bytes wide), then
// kFlatWaveBytes per wave
constexpr int pitch_flat_lags_bytes(int S4) { return (S4 * 4 + 15) & ~15; }
constexpr size_t pitch_flat_lds_bytes(int S4) {
  return static_cast<size_t>(pitch_flat_lags_bytes(S4)) + static_cast<size_t>(kFlatWaves) * kFlatWaveBytes;
}
constexpr size_t kPitchLdsLimit = 160 * 1024;

// ---- developer knobs ------------------------------------------------------------------------------------
struct PitchKnobs {
  int team;    // SNF_PITCH_TEAM: 1, 2 or 4 forces that many waves per utterance; anything else: by batch size
  int flat;    // SNF_PITCH_FLAT: 0 = the by-state kernel where the by-candidate one would run (A/B runs)
  int trace;   // SNF_PITCH_TRACE: synchronise and report after every stage, stop behind stage `trace`
};
inline PitchKnobs pitch_knobs_parse(const char* team, const char* flat, const char* trace) {
  PitchKnobs k;
  k.team = team ? atoi(team) : 0;
  k.flat = flat && flat[0] == '0' ? 0 : 1;
  k.trace = trace ? atoi(trace) : 0;
  return k;
}
// The only reader of the environment in the tracker.  Team and flat are honoured per call (the tests run every
// form in one process), trace is read once (tools/time_resample.py sets it for the whole process).
inline PitchKnobs pitch_knobs_from_env() {
  static const int trace = pitch_knobs_parse(nullptr, nullptr, getenv("SNF_PITCH_TRACE")).trace;
  PitchKnobs k = pitch_knobs_parse(getenv("SNF_PITCH_TEAM"), getenv("SNF_PITCH_FLAT"), nullptr);
  k.trace = trace;
  return k;
}

// ---- the ladder -----------------------------------------------------------------------------------------
enum PitchForm { kPitchByState = 0, kPitchTeam = 1, kPitchFlat = 2 };
struct PitchRoute {
  PitchForm form;
  int waves;             // waves per workgroup: the team's size, or the utterances of a workgroup
  int nk;                // by state: 64-state slices a lane keeps in registers (7, 8; 0: rows read from HBM); else -1
  size_t lds_bytes;
  const char* refusal;   // nullptr, or why no form runs this state count
};
// Small batches: several waves per utterance (viterbi_forward_team) - one wave per utterance leaves most SIMDs
// with a single wave whose latency is the kernel's time.  Else the lane-per-candidate search (round 5): bit-
// identical to the lane-per-state kernel, 25 % fewer instructions, 11.8 against 14.2 ms per 10 000 utterances;
// SNF_PITCH_FLAT=0 keeps the old kernel (A/B runs, tests/test_parity_gpu.py::test_pitch_flat_search).
inline PitchRoute pitch_viterbi_route(int num_states, int64_t n_utts, const PitchKnobs& knobs) {
  const int S = num_states, S4 = (S + 3) & ~3;
  const bool forced = knobs.team == 1 || knobs.team == 2 || knobs.team == 4;
  int team = forced ? knobs.team : n_utts <= kTeam4Utts ? 4 : n_utts <= kTeam2Utts ? 2 : 1;
  if (S > 512 || S < 128) team = 1;
  if (team > 1) return {kPitchTeam, team, -1, pitch_team_lds_bytes(S4, team), nullptr};
  if (S > 128 && S <= 448 && knobs.flat != 0) return {kPitchFlat, kFlatWaves, -1, pitch_flat_lds_bytes(S4), nullptr};
  const size_t lds = pitch_state_lds_bytes(S4);
  return {kPitchByState, kVitWaves, S <= 448 ? 7 : S <= 512 ? 8 : 0, lds,
          lds > kPitchLdsLimit ? "pitch state space does not fit in LDS" : nullptr};
}

}  // namespace snf

#endif  // SNF_PITCH_ROUTE_H_
