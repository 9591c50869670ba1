// What the launchers of fbank512_kernel (kernels_fbank512.hip) and fbank256x2_kernel (kernels_fbank256x2.hip)
// share: the workgroup geometry and the ladder from a plan's run-time options to template arguments.
#ifndef SNF_FAST512_LAUNCH_H_
#define SNF_FAST512_LAUNCH_H_

#include <cstdlib>
#include <type_traits>

#include "snf_internal.h"

namespace snf {

namespace {

// floats a workgroup stages into LDS: the blob of its utterance's warp factor on the per-utterance schedule
// (`table_stride` apart; one blob, warp 1.0, when the caller set none), else the plan's only blob
inline int fast512_staged_floats(const Fast512Params& p, bool per_utt) {
  if (!per_utt) return p.table_floats;
  return p.table_stride != 0 ? p.table_stride : (p.table_floats + 3) & ~3;
}

// Waves per workgroup and its dynamic LDS: two workgroups of 8 waves per CU where they fit, else one of 16; the
// fused-delta form has its own geometry.
inline int fast512_workgroup(const Fast512Params& p, bool per_utt, int* n_waves, size_t* lds) {
  const int table_floats = fast512_staged_floats(p, per_utt);
  *n_waves = kFast512MinWaves;
  *lds = fast512_lds_bytes(table_floats, *n_waves, false);
  if (2 * (*lds + 512) > kFast512LdsBytes) {  // two 8-wave workgroups do not fit: one of 16 waves
    *n_waves = kFast512MaxWaves;
    *lds = fast512_lds_bytes(table_floats, *n_waves, false);
  }
  if (p.fused_delta != 0) {  // (MFCC + deltas: always scheduled per utterance)
    if (!per_utt || p.kind != SNF_KIND_MFCC || p.num_ceps > kFast512FusedCols)
      return set_error(SNF_E_RUNTIME, "fast512: fused deltas need the per-utterance MFCC schedule");
    *n_waves = kFast512FusedWaves;
    *lds = fast512_lds_bytes(table_floats, *n_waves, true);
  }
  if (const char* forced = getenv("SNF_FAST512_WAVES")) {  // developer knob: occupancy experiments
    *n_waves = atoi(forced);
    *lds = fast512_lds_bytes(table_floats, *n_waves, false);
  }
  if (*lds > kFast512LdsBytes) return set_error(SNF_E_RUNTIME, "fast512: tables do not fit in LDS");
  return SNF_OK;
}

// The launch ladder: (nj, p.kind, the energy column, p.dither != 0, p.snip_edges) as compile-time constants.
// Calls f(nj, kind, energy, dither, snip) with std::integral_constant arguments (a generic lambda instantiates
// its kernel from their ::value, and leaves out with `if constexpr` what has no kernel) and returns what it
// returns.  energy: 0 = no log-energy column, 1 = raw, 2 = after the window.
template <typename F>
int with_nj_kind_energy_dither_snip(int nj, const Fast512Params& p, F&& f) {
  auto snip = [&](auto nj_c, auto kind, auto energy, auto dither) {
    return p.snip_edges ? f(nj_c, kind, energy, dither, std::true_type{})
                        : f(nj_c, kind, energy, dither, std::false_type{});
  };
  auto dither = [&](auto nj_c, auto kind, auto energy) {
    return p.dither != 0.0f ? snip(nj_c, kind, energy, std::true_type{})
                            : snip(nj_c, kind, energy, std::false_type{});
  };
  auto energy = [&](auto nj_c, auto kind) {
    if (p.need_raw) return dither(nj_c, kind, std::integral_constant<int, 1>{});
    if (p.need_post) return dither(nj_c, kind, std::integral_constant<int, 2>{});
    return dither(nj_c, kind, std::integral_constant<int, 0>{});
  };
  auto kind = [&](auto nj_c) {
    if (p.kind == SNF_KIND_FBANK) return energy(nj_c, std::integral_constant<int, SNF_KIND_FBANK>{});
    if (p.kind == SNF_KIND_MFCC) return energy(nj_c, std::integral_constant<int, SNF_KIND_MFCC>{});
    if (p.kind == SNF_KIND_SPECTROGRAM) return energy(nj_c, std::integral_constant<int, SNF_KIND_SPECTROGRAM>{});
    if (p.kind == SNF_KIND_ENERGY) return energy(nj_c, std::integral_constant<int, SNF_KIND_ENERGY>{});
    return energy(nj_c, std::integral_constant<int, SNF_KIND_PLP>{});
  };
  return nj == 13 ? kind(std::integral_constant<int, 13>{}) : kind(std::integral_constant<int, 16>{});
}

}  // namespace

}  // namespace snf

#endif  // SNF_FAST512_LAUNCH_H_
