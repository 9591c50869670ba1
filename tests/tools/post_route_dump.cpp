// Prints what shennong_amd/csrc/post_route.h decides, for tests/test_post_route.py: host code only, the header
// alone - no device, no library.  Every route line ends with
//   kernel=<PostKernel> name=<its name> variant= threads= rows= lds= build=<0|1> refusal=<0|1>
// behind its inputs:
//   plp bins= order= ceps= knobs=<-|small|generic|both> compress=<third|0.3>     (+ a line `refusal <text>` if it refuses)
//   delta order= window= cols= n_scales= buffer=<0|1> aligned=<0|1>
//   pitch left= right= window= knob=<0|1> halo_l= halo_r=
//   cmvn cols=
// and then
//   knobs which=<0 generic|1 small|2 per frame> in=<-|empty|0> generic= small= per_frame=
//   consts max_bins= max_lpc= delta_rows= post_rows= flat_tile_bytes= lds_limit= flat=<cols>:<rows>,...
#include <cstdio>
#include <vector>

#include "post_route.h"

using namespace snf;

static void tail(const PostRoute& r) {
  printf(" kernel=%d name=%s variant=%d threads=%d rows=%d lds=%zu build=%d refusal=%d\n", static_cast<int>(r.kernel),
         r.name(), r.variant, r.threads, r.rows, r.lds_bytes, r.build_records ? 1 : 0, r.refusal ? 1 : 0);
  if (r.refusal) printf("refusal %s\n", r.refusal);
}

int main() {
  const int shapes[][3] = {{23, 12, 13}, {23, 12, 12}, {22, 12, 13}, {32, 16, 13}, {33, 16, 13},
                           {32, 17, 13}, {126, 63, 13}, {127, 12, 13}, {23, 64, 13}};
  const char* knob_names[] = {"-", "small", "generic", "both"};
  for (const auto& s : shapes)
    for (int k = 0; k < 4; ++k)
      for (int third = 1; third >= 0; --third) {
        const PostKnobs knobs = post_knobs_parse(k & 2 ? "" : nullptr, k & 1 ? "" : nullptr, nullptr);
        printf("plp bins=%d order=%d ceps=%d knobs=%s compress=%s", s[0], s[1], s[2], knob_names[k],
               third ? "third" : "0.3");
        tail(plp_tail_route(s[0], s[1], s[2], third ? 0.33333334f : 0.3f, knobs));
      }
  for (int order = 1; order <= 3; ++order)
    for (int window = 1; window <= 3; ++window) {
      int n_scales = 0;
      for (int i = 0; i <= order; ++i) n_scales += 2 * i * window + 1;
      std::vector<int> cols = {1, 13, 23, 40, 43, 44, 256, 257};
      int first = 1;   // the first column count whose tile does not fit, and the last that does
      while (delta_tiled_lds_bytes(n_scales, order * window, first) <= kPostLdsLimit) ++first;
      cols.push_back(first - 1);
      cols.push_back(first);
      for (int c : cols)
        for (int buffer = 1; buffer >= 0; --buffer)
          for (int aligned = 1; aligned >= 0; --aligned) {
            printf("delta order=%d window=%d cols=%d n_scales=%d buffer=%d aligned=%d", order, window, c, n_scales,
                   buffer, aligned);
            tail(delta_route(order, window, n_scales, c, buffer != 0, aligned != 0));
          }
    }
  // halos of 5 888 frames in all (the last that fits) and of 5 889; 5 888 again, 2 of them from the delta window above
  // a left context of 0; a delta window above both contexts; a negative context
  // under a positive and under a negative window; the knob on a short window
  const int pitch[][4] = {{5000, 888, 2, 0}, {5000, 889, 2, 0}, {0, 5886, 2, 0}, {3, 1, 7, 0},
                          {-5, 10, 2, 0}, {-5, 10, -1, 0}, {75, 75, 2, 1}, {75, 75, 2, 0}};
  for (const auto& c : pitch) {
    snf_pitch_post_options o = {};
    o.normalization_left_context = c[0];
    o.normalization_right_context = c[1];
    o.delta_window = c[2];
    const PitchPostHalos h = pitch_post_halos(o);
    printf("pitch left=%d right=%d window=%d knob=%d halo_l=%d halo_r=%d", c[0], c[1], c[2], c[3], h.left, h.right);
    tail(pitch_post_route(o, post_knobs_parse(nullptr, nullptr, c[3] ? "1" : nullptr)));
  }
  for (int c : {1, 128, 129, 256, 257}) {
    printf("cmvn cols=%d", c);
    tail(cmvn_stats_route(c));
  }
  const char* strings[] = {nullptr, "", "0"};
  for (int which = 0; which < 3; ++which)
    for (const char* s : strings) {
      const PostKnobs k = post_knobs_parse(which == 0 ? s : nullptr, which == 1 ? s : nullptr, which == 2 ? s : nullptr);
      printf("knobs which=%d in=%s generic=%d small=%d per_frame=%d\n", which, !s ? "-" : s[0] ? s : "empty",
             k.plp_generic_tail ? 1 : 0, k.plp_small_tail ? 1 : 0, k.pitch_post_per_frame ? 1 : 0);
    }
  printf("consts max_bins=%d max_lpc=%d delta_rows=%d post_rows=%d flat_tile_bytes=%d lds_limit=%zu flat=", kMaxBins,
         kMaxLpc, kDeltaRows, kPostRows, kFlatTileBytes, kPostLdsLimit);
  for (int d : kFlatCols) printf("%d:%d,", d, flat_rows(d));
  printf("\n");
  return 0;
}
