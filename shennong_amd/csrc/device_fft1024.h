// What the two long-frame kernels share (kernels_fbank2048.hip: one 2048-sample frame per wave;
// kernels_fbank1024x2.hip: two 1024-sample frames per wave): the 1024-point complex transform of a wave64
// (16 x 4 x 16: three register passes around two transposes through the wave's LDS buffer), the partner
// exchange behind it, the frame-energy and MFCC conventions of the epilogue, the host side of the
// transform's twiddle tables and the launch ladder.  The index maps were checked lane by lane against
// numpy.fft, and every LDS access against the bank model, in tools/model_fbank2048.py
// (tests/test_fbank2048_model.py).
// Everything is static to the including translation unit, as in device_fft.h.
#ifndef SNF_DEVICE_FFT1024_H_
#define SNF_DEVICE_FFT1024_H_

#include <cmath>
#include <type_traits>

#include "snf_internal.h"
#include "device_fft.h"

namespace snf {

namespace {

constexpr int kLongWaves = 16;                 // one workgroup per CU: 16 transforms in flight
constexpr int kLongBufBytes = 1088 * 8;        // wave-private LDS: 16 rows x (64 + 4) complex = 64 rows x 17

__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
// sum over the 64 lanes, the same value in every lane
__device__ __forceinline__ float wave_sum64(float v) {
  v = row_sum16(v);
  return (readlane_f(v, 0) + readlane_f(v, 16)) + (readlane_f(v, 32) + readlane_f(v, 48));
}
// a wave-uniform 64-bit value as a scalar (keeps the base of the sample loads in SGPRs)
__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<int>(v));
  const unsigned hi = __builtin_amdgcn_readfirstlane(static_cast<int>(v >> 32));
  return static_cast<int64_t>((static_cast<unsigned long long>(hi) << 32) | lo);
}
// value of `v` in lane (lane - 1) mod 64: a DPP move with wave_ror:1 (gfx9 keeps the whole-wave rotations;
// checked on the device with tools/ubench_wave_ror.hip), not a trip through the LDS crossbar (ds_bpermute)
__device__ __forceinline__ float from_left_lane(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x13C, 0xf, 0xf, false));
}

// Lane-constant LDS bases of the transform (float2 pointers into the wave's buffer; every access adds a
// compile-time offset: four address registers serve all its LDS accesses).  The kernels fill this per trip of
// their frame loop from an opaque copy of the lane index, NOT once in front of it: see the comment there.
struct Fft1024Maps {
  int kq, bq;                  // lane = 4 kq + bq.  Pass C: (k1, quarter of b); pass D: (k1, c)
  int kappa;                   // the lane holds Z[kappa + 64 d], d < 16, after pass D
  const float2* base_lane;     // transpose 1 write, exchange write
  float2* base_quad;           // transpose 1 read, transpose 2 write
  const float2* base_row;      // transpose 2 read
  const float2* base_part;     // exchange read: the partner lane
};
__device__ __forceinline__ Fft1024Maps fft1024_maps(float2* buf, int lane_v) {
  Fft1024Maps m;
  m.kq = lane_v >> 2;
  m.bq = lane_v & 3;
  m.base_lane = buf + lane_v;
  m.base_quad = buf + 68 * m.kq + m.bq;
  m.base_row = buf + 17 * lane_v;
  m.base_part = buf + (m.kq == 0 ? ((4 - m.bq) & 3) : 4 * (16 - m.kq) + (3 - m.bq)) + (lane_v == 0 ? 64 : 0);
  m.kappa = m.kq + 16 * m.bq;
  return m;
}

// a * w as cmul computes it, with the one choice spelled out that a plain cmul was seen to leave open: which of
// the two products of the imaginary part the fused multiply-add absorbs - a.x w.y (IM_FUSES_AX: fma(a.x, w.y,
// a.y w.x)) or a.y w.x (fma(a.y, w.x, a.x w.y)).  The compiler's choice moved for four multiplies of pass C when
// the passes below left the two kernels, and another choice is another last bit of the spectrum.  The forms are
// those of every instantiation before the move: pass B the first, pass C the second (the scan of the listings
// is described in profiles/long_frames_refactor_isa.txt).  The real part is left as the expression it was: a
// subtraction has compiled to fma(a.x, w.x, -(a.y w.y)) throughout.
template <bool IM_FUSES_AX>
__device__ __forceinline__ float2 cmul_rounded(float2 a, float2 w) {
  return make_float2(a.x * w.x - a.y * w.y,
                     IM_FUSES_AX ? __builtin_fmaf(a.x, w.y, a.y * w.x) : __builtin_fmaf(a.y, w.x, a.x * w.y));
}

// Passes B - D: lane L holds z[j] = the signal's element L + 64 j (zero for j >= NJ) on entry and
// z[d] = Z[kappa + 64 d] on return.  `t_tw1`: the lane's row of W1024^(L k1), `t_tw2`: row bq of W64^(b c)
// (fft1024_twiddle_tables).  Row pitches 68 and 17 complex make every LDS access bank-conflict free.
template <int NJ>
__device__ __forceinline__ void cfft1024_passes(float2 (&z)[16], const float2* t_tw1, const float2* t_tw2,
                                                const Fft1024Maps& maps) {
  const float2* base_lane = maps.base_lane;
  float2* base_quad = maps.base_quad;
  const float2* base_row = maps.base_row;
  // ---- B: pass 1 (FFT over j), twiddle W1024^(L k1), transpose ---------------------------------------
  // (rows j >= NJ are the zero padding: the first layer skips them; butterflies with folded twiddles)
  fft16_lf_head<NJ>(z);
  float4 tw4[8];
  read_quads_whole<8>(t_tw1, tw4);
  lds_wait();
#pragma unroll
  for (int k1 = 1; k1 < 16; ++k1)
    z[k1] = cmul_rounded<true>(z[k1], (k1 & 1) ? make_float2(tw4[k1 >> 1].z, tw4[k1 >> 1].w)
                                               : make_float2(tw4[k1 >> 1].x, tw4[k1 >> 1].y));
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) const_cast<float2*>(base_lane)[k1 * 68] = z[k1];
  wave_lds_sync();
  // ---- C: lane (kq, bq): 4-point DFTs over the rows a for b = bq + 4 i, twiddle W64^(b c) --------------
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int a = 0; a < 4; ++a) z[4 * i + a] = base_quad[16 * a + 4 * i];
  float4 tw2q[8];
  read_quads_whole<8>(t_tw2, tw2q);
  lds_wait();
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float2 o0, o1, o2, o3;
    dft4(z[4 * i], z[4 * i + 1], z[4 * i + 2], z[4 * i + 3], o0, o1, o2, o3);
    z[4 * i] = o0;
    z[4 * i + 1] = cmul_rounded<false>(o1, make_float2(tw2q[2 * i].z, tw2q[2 * i].w));
    z[4 * i + 2] = cmul_rounded<false>(o2, make_float2(tw2q[2 * i + 1].x, tw2q[2 * i + 1].y));
    z[4 * i + 3] = cmul_rounded<false>(o3, make_float2(tw2q[2 * i + 1].z, tw2q[2 * i + 1].w));
  }
  // transpose: row r = 4 kq + c (pitch 17) holds b = 0..15
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) base_quad[17 * c + 4 * i] = z[4 * i + c];
  wave_lds_sync();
  read16_b64(base_row, z);
  lds_wait();
  wave_lds_sync();
  // ---- D: pass 3 (FFT over b): z[d] = Z[kappa + 64 d] ---------------------------------------------------
  fft16_lf(z);
  __builtin_amdgcn_sched_barrier(0);
}

// Phase E, first half: zpart[d] = Z[1024 - (kappa + 64 d)], d < 8, requested from the partner lane (register
// 15 - d of the lane with kappa' = 64 - kappa; own register 16 - d for kappa = 0).  The reads are only ISSUED:
// the caller adds the LDS reads it wants inside the same wait, then lds_wait() and wave_lds_sync().
__device__ __forceinline__ void cfft1024_partner_reads(const float2 (&z)[16], const Fft1024Maps& maps,
                                                       float2 (&zpart)[8]) {
#pragma unroll
  for (int d = 8; d < 16; ++d) const_cast<float2*>(maps.base_lane)[(d - 8) * 64] = z[d];
  wave_lds_sync();
#pragma unroll
  for (int d = 0; d < 8; ++d) zpart[d] = maps.base_part[(7 - d) * 64];
}

// Frame energy of the epilogue, conventions of mel_features_generic_kernel: PLP hands the linear energy of frame
// `g` to plp_tail_kernel as a double (shennong's PLP floors with float64 eps and takes a double log: reference
// plp.py:191-193), the other kinds take the floored log.  Returns the log energy (0 where the options name
// none, and for PLP)
template <int KIND>
__device__ __forceinline__ float frame_log_energy(const MelParams& p, int lane, float e_lin, int64_t g,
                                                  double* energy_out) {
  float log_energy = 0.0f;
  if (KIND == SNF_KIND_PLP) {
    if ((p.need_raw || p.need_post) && lane == 0)
      energy_out[g] = static_cast<double>(e_lin);  // (plp_tail_kernel takes the double log)
  } else if (p.need_raw || p.need_post) {
    log_energy = fast_log(floor_eps(e_lin));
    if (p.has_floor && log_energy < p.log_energy_floor) log_energy = p.log_energy_floor;
  }
  return log_energy;
}

// MFCC tail for the NF frames of a wave: DCT-II of the log-mel energies mel[f][0 .. num_bins) (in LDS) by teams
// of 4 lanes per cepstral coefficient, 16 coefficients per round; lifter, c0 := energy, HTK order.  Row 1 is
// written only if `two`.
template <int NF>
__device__ __forceinline__ void mfcc_dct_tail(const MelParams& p, int lane, bool two, const float* const (&mel)[NF],
                                              const float* log_energy, float* const (&row)[NF]) {
  const int nb = p.num_bins;
  const int ct = lane >> 2, cl = lane & 3;
  for (int c0 = 0; c0 < p.num_ceps; c0 += 16) {
    const int c = c0 + ct;
    const bool ca = c < p.num_ceps;
    const float* __restrict__ dm = p.dct + (ca ? c : 0) * nb;
    float v[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) v[f] = 0.0f;
    for (int m0 = 0; m0 < nb; m0 += 32) {  // 8 coefficients per lane in flight
      float dv[8], mv[NF][8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int m = m0 + cl + 4 * e;
        dv[e] = dm[m < nb ? m : 0];
#pragma unroll
        for (int f = 0; f < NF; ++f) mv[f][e] = mel[f][m < nb ? m : 0];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int f = 0; f < NF; ++f) v[f] += (m0 + cl + 4 * e < nb) ? dv[e] * mv[f][e] : 0.0f;
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) v[f] += dpp_row_ror<0xB1>(v[f]);
#pragma unroll
    for (int f = 0; f < NF; ++f) v[f] += dpp_row_ror<0x4E>(v[f]);
    if (ca && cl == 0) {
      if (p.lifter) {
#pragma unroll
        for (int f = 0; f < NF; ++f) v[f] *= p.lifter[c];
      }
      if (c == 0 && p.use_energy) {
#pragma unroll
        for (int f = 0; f < NF; ++f) v[f] = log_energy[f];
      }
      int oc = c;
      if (p.htk_compat) {
        oc = c == 0 ? p.num_ceps - 1 : c - 1;
        if (c == 0 && !p.use_energy) {
#pragma unroll
          for (int f = 0; f < NF; ++f)
            v[f] = static_cast<float>(static_cast<double>(v[f]) * 1.4142135623730950488016887);
        }
      }
      row[0][oc] = v[0];
      if (NF == 2 && two) row[NF - 1][oc] = v[NF - 1];
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
// The transform's twiddles in a kernel's table blob `t` (float2 units): W1024^(lane k1) as [64][18] at
// `off_tw1`, W64^(b c) as [4][16 + 2] at `off_tw2`; rows padded so that ds_read_b128 is conflict-free (the four
// rows of the second table are broadcast to 16 lanes each: 128-byte rows would put all four on the same banks)
inline void fft1024_twiddle_tables(float* t, int off_tw1, int off_tw2) {
  constexpr double kTwoPi = 6.283185307179586476925286766559005;
  auto put = [&](int index, double re, double im) {
    t[2 * index] = static_cast<float>(re);
    t[2 * index + 1] = static_cast<float>(im);
  };
  for (int lane = 0; lane < 64; ++lane)
    for (int j = 0; j < 16; ++j) {
      const double a1 = -kTwoPi * ((lane * j) % 1024) / 1024.0;  // W1024^(lane k1), k1 = j
      put(off_tw1 + lane * 18 + j, std::cos(a1), std::sin(a1));
    }
  for (int bq = 0; bq < 4; ++bq)
    for (int i = 0; i < 4; ++i)
      for (int c = 0; c < 4; ++c) {
        const double a = -kTwoPi * (((bq + 4 * i) * c) % 64) / 64.0;
        put(off_tw2 + bq * 18 + i * 4 + c, std::cos(a), std::sin(a));
      }
}

// The launch ladder: (p.kind, p.dither != 0, p.snip_edges) as compile-time constants.  Calls
// f(kind, dither, snip) with std::integral_constant arguments (a generic lambda instantiates its kernel from
// their ::value) and returns what it returns.
template <typename F>
int with_kind_dither_snip(const MelParams& p, F&& f) {
  auto snip = [&](auto kind, auto dither) {
    return p.snip_edges ? f(kind, dither, std::true_type{}) : f(kind, dither, std::false_type{});
  };
  auto dither = [&](auto kind) {
    return p.dither != 0.0f ? snip(kind, std::true_type{}) : snip(kind, std::false_type{});
  };
  if (p.kind == SNF_KIND_FBANK) return dither(std::integral_constant<int, SNF_KIND_FBANK>{});
  if (p.kind == SNF_KIND_MFCC) return dither(std::integral_constant<int, SNF_KIND_MFCC>{});
  if (p.kind == SNF_KIND_PLP) return dither(std::integral_constant<int, SNF_KIND_PLP>{});
  return dither(std::integral_constant<int, SNF_KIND_SPECTROGRAM>{});
}

}  // namespace

}  // namespace snf

#endif  // SNF_DEVICE_FFT1024_H_
