// Prints what shennong_amd/csrc/pitch_route.h decides, for tests/test_pitch_route.py: host code only, the header
// alone - no device, no library.
//   route S=<states> n=<utterances> team=<knob|-> flat=<knob|-> form=<0 state|1 team|2 flat> waves= nk= lds= refusal=<0|1>
//   knobs in_team=<string> in_flat=<string> team=<int> flat=<int> trace=<int>
//   limit state=<first S4 the by-state form refuses>
#include <cstdio>
#include <cstring>

#include "pitch_route.h"

int main() {
  using namespace snf;
  const int states[] = {1, 127, 128, 129, 417, 448, 449, 461, 512, 513, 521, 1400, 1600};
  const long long utts[] = {1, 768, 769, 1280, 1281, 100000};
  const char* team_knobs[] = {nullptr, "1", "2", "3", "4"};
  const char* flat_knobs[] = {nullptr, "0", "1"};
  for (int S : states)
    for (long long n : utts)
      for (const char* team : team_knobs)
        for (const char* flat : flat_knobs) {
          const PitchRoute r = pitch_viterbi_route(S, n, pitch_knobs_parse(team, flat, nullptr));
          printf("route S=%d n=%lld team=%s flat=%s form=%d waves=%d nk=%d lds=%zu refusal=%d\n", S, n,
                 team ? team : "-", flat ? flat : "-", static_cast<int>(r.form), r.waves, r.nk, r.lds_bytes,
                 r.refusal ? 1 : 0);
          if (r.refusal && strcmp(r.refusal, "pitch state space does not fit in LDS") != 0) return 1;
        }
  const char* parse_cases[][2] = {{"3", "0x"}, {"", "1"}, {"0", ""}, {"4", "0"}, {"2", "00"}, {"1", "10"}};
  for (const auto& c : parse_cases) {
    const PitchKnobs k = pitch_knobs_parse(c[0], c[1], "2");
    printf("knobs in_team=%s in_flat=%s team=%d flat=%d trace=%d\n", c[0], c[1], k.team, k.flat, k.trace);
  }
  // both sides of the by-state form's refusal, found through the route itself (one wave per utterance forced)
  const PitchKnobs one_wave = pitch_knobs_parse("1", "0", nullptr);
  int S = 513;
  while (!pitch_viterbi_route(S, 1, one_wave).refusal) ++S;
  printf("limit state=%d last_lds=%zu first_lds=%zu\n", S, pitch_viterbi_route(S - 1, 1, one_wave).lds_bytes,
         pitch_viterbi_route(S, 1, one_wave).lds_bytes);
  return 0;
}
