// Host tables of the register-resident 512-point fast path (fbank512_kernel, fbank512b_kernel,
// fbank256x2_kernel): which configurations it serves, and the packed blob its workgroups stage into LDS
// (layout: Fast512Params in snf_internal.h).  No device code and no HIP call: tools/fast512_tables_digest.cpp
// builds it on the CPU.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "snf_internal.h"

namespace snf {

bool fast512_eligible(const MelParams& mp, bool any_warp) {
  if (getenv("SNF_DISABLE_FAST512")) return false;
  if (any_warp) return false;
  // Frames that pad to 256 or 128 samples (8 kHz audio, short windows) run as the same 512-point
  // transform of the zero-extended frame: X512[s k] = X_N[k] with s = 512 / N, so the mel taps sit
  // on every s-th bin (spread_taps interleaves zero weights).  Twice the FFT arithmetic the frame
  // needs, still several times faster than the LDS radix-2 kernel.
  if ((mp.padded != 512 && mp.padded != 256 && mp.padded != 128) || !mp.pow2) return false;
  if (mp.win_len & 1) return false;
  if (mp.kind != SNF_KIND_FBANK && mp.kind != SNF_KIND_MFCC && mp.kind != SNF_KIND_PLP &&
      mp.kind != SNF_KIND_SPECTROGRAM && mp.kind != SNF_KIND_ENERGY)
    return false;
  // (the spectrogram needs the N / 2 + 1 bins themselves: 512-sample frames, or 256-sample frames on the
  // two-frames-per-transform kernel, whose conditions are those of fast512_dual_eligible)
  if (mp.kind == SNF_KIND_SPECTROGRAM && mp.padded != 512 &&
      !(mp.padded == 256 && mp.win_len + mp.win_shift <= 512 && !getenv("SNF_DISABLE_DUAL256")))
    return false;
  if (mp.kind == SNF_KIND_FBANK && !mp.use_power) return false;
  if (mp.num_bins > kFast512MaxBins) return false;
  if (mp.kind == SNF_KIND_MFCC && mp.num_ceps > 16) return false;
  return true;
}

bool fast512_dual_eligible(const MelParams& mp) {
  if (getenv("SNF_DISABLE_DUAL256")) return false;
  // (a pair is fetched as one span of the utterance: at most 512 samples, kernels_fbank256x2.hip load_span)
  return fast512_eligible(mp, false) && mp.padded == 256 && mp.win_len + mp.win_shift <= 512 &&
         (mp.kind == SNF_KIND_FBANK || mp.kind == SNF_KIND_MFCC || mp.kind == SNF_KIND_PLP ||
          mp.kind == SNF_KIND_SPECTROGRAM);
}

namespace {

constexpr double kTwoPi = 6.283185307179586476925286766559005;

// ---- the mel filterbank as MFMA blocks: what the steps of fast512_build share ----------------------
// Group g = mel bins 4 g .. 4 g + 3 spans the FFT bins [glo, ghi); it is cut into parts[g] runs of at
// most 4 mm_quads bins, one MFMA block each.  More parts for the widest groups shorten the chain;
// the parts of a group must sit in ONE row of 4 blocks (their sums are added through row DPP).
struct Block { int group, part, lo, hi, start; };  // FFT bins [lo, hi) of `group`; operands from `start`
struct BlockPlan {
  int n_groups = 0;
  std::vector<int> glo, ghi, parts;
  int chain = 16;             // instructions of the chain = bins of the longest part, in whole quads
  std::vector<Block> blocks;  // the 16 blocks of a wave (group -1: idle)
  int per_part(int g, int np) const { return ((ghi[g] - glo[g] + np - 1) / np + 3) & ~3; }
};

// frames shorter than 512 samples: spread the taps of every bin over the bins of the 512-point
// spectrum of the zero-extended frame (see fast512_eligible)
MelBanksHost spread_taps(const MelBanksHost& mb_in, int bin_stride) {
  MelBanksHost spread;
  spread.num_bins = mb_in.num_bins;
  spread.num_fft_bins = mb_in.num_fft_bins * bin_stride;
  spread.center_freqs = mb_in.center_freqs;
  for (int m = 0; m < mb_in.num_bins; ++m) {
    spread.first.push_back(mb_in.first[m] * bin_stride);
    spread.size.push_back(mb_in.size[m] > 0 ? (mb_in.size[m] - 1) * bin_stride + 1 : 0);
    spread.offset.push_back(static_cast<int>(spread.w.size()));
    for (int k = 0; k < mb_in.size[m]; ++k) {
      spread.w.push_back(mb_in.w[mb_in.offset[m] + k]);
      if (k + 1 < mb_in.size[m]) spread.w.insert(spread.w.end(), bin_stride - 1, 0.0f);
    }
  }
  return spread;
}

// the plan's options the kernels read from their arguments
Fast512Params scalar_params(const MelParams& mp, bool dual) {
  Fast512Params p{};
  p.win_len = mp.win_len;
  p.win_shift = mp.win_shift;
  p.remove_dc = mp.remove_dc;
  p.snip_edges = mp.snip_edges;
  p.preemph = mp.preemph;
  p.dither = mp.dither;
  p.seed = mp.seed;
  p.kind = mp.kind;
  p.compression = mp.compression;
  p.use_energy = mp.use_energy;
  p.need_raw = mp.need_raw;
  p.need_post = mp.need_post;
  p.htk_compat = mp.htk_compat;
  p.use_log = mp.use_log;
  p.has_floor = mp.has_floor;
  p.log_energy_floor = mp.log_energy_floor;
  p.num_bins = mp.num_bins;
  p.num_ceps = mp.num_ceps;
  p.dual = dual ? 1 : 0;
  return p;
}

// window pairs, lane-major: row l = elements l + 16 j (j < 16), 2 complex of padding
void push_window_rows(const MelParams& mp, const std::vector<float>& window, bool dual, std::vector<float>* blob) {
  for (int l = 0; l < 16; ++l)
    for (int j = 0; j < 18; ++j) {
      const int n = l + 16 * j;
      if (dual) {  // element n of the row = sample n of BOTH sub-frames
        const float w = j < 16 && n < mp.win_len ? window[n] : 0.0f;
        blob->push_back(w);
        blob->push_back(w);
        continue;
      }
      blob->push_back(j < 16 && 2 * n < mp.win_len ? window[2 * n] : 0.0f);
      blob->push_back(j < 16 && 2 * n + 1 < mp.win_len ? window[2 * n + 1] : 0.0f);
    }
}

// Twiddles as (cos, tan) pairs: W = cos (1 + i tan) (device_fft.h, Linzer-Feig butterflies).  An exact
// -i (zero cosine) is (2^-40, -2^40): every product with it is an exact power-of-two scaling.
void push_cos_tan(int num, int den, std::vector<float>* blob) {
  const int r = ((num % den) + den) % den;  // exp(-2 pi i r / den)
  if (4 * r == den) {                        // -i
    blob->push_back(9.094947017729282e-13f);
    blob->push_back(-1099511627776.0f);
    return;
  }
  if (4 * r == 3 * den) {                    // +i
    blob->push_back(9.094947017729282e-13f);
    blob->push_back(1099511627776.0f);
    return;
  }
  const double a = -kTwoPi * r / den;
  blob->push_back(static_cast<float>(std::cos(a)));
  blob->push_back(static_cast<float>(std::tan(a)));
}

void push_twiddle_rows(std::vector<float>* blob) {
  // inter-pass twiddles, lane-major: row n1 = exp(-2 pi i n1 k2 / 256), k2 < 16
  for (int n1 = 0; n1 < 16; ++n1)
    for (int k2 = 0; k2 < 18; ++k2) push_cos_tan(n1 * (k2 < 16 ? k2 : 0), 256, blob);
  // unpack twiddles, lane-major: row l = exp(-2 pi i (l + 16 k1) / 512), k1 < 8 (angles in (-pi/2, 0])
  for (int l = 0; l < 16; ++l)
    for (int k1 = 0; k1 < 10; ++k1) push_cos_tan(l + 16 * (k1 < 8 ? k1 : 0), 512, blob);
}

// first-fit-decreasing of the part counts into 4 rows of 4 blocks; returns false when they do not fit
bool pack_rows(const std::vector<int>& np, std::vector<int>* first_block) {
  std::vector<int> order(np.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = static_cast<int>(i);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return np[x] > np[y]; });
  int used[4] = {0, 0, 0, 0};
  if (first_block) first_block->assign(np.size(), -1);
  for (int g : order) {
    int r = 0;
    while (r < 4 && used[r] + np[g] > 4) ++r;
    if (r == 4) return false;
    if (first_block) (*first_block)[g] = 4 * r + used[r];
    used[r] += np[g];
  }
  return true;
}

// The block plan: the groups' spans, their parts, the rows the parts are packed into and the chain length.
// false: more than 16 groups (not eligible).
bool plan_blocks(const MelBanksHost& mb, bool dual, BlockPlan* bp) {
  const int n_groups = bp->n_groups = (mb.num_bins + 3) / 4;
  std::vector<int>&glo = bp->glo, &ghi = bp->ghi, &parts = bp->parts;
  glo.assign(n_groups, 0);
  ghi.assign(n_groups, 0);
  parts.assign(n_groups, 1);
  for (int g = 0; g < n_groups; ++g) {
    int lo = 1 << 30, hi = 0;
    for (int m = 4 * g; m < 4 * g + 4 && m < mb.num_bins; ++m) {
      if (mb.size[m] <= 0) continue;
      lo = std::min(lo, mb.first[m]);
      hi = std::max(hi, mb.first[m] + mb.size[m]);
    }
    if (hi == 0) lo = 0;
    glo[g] = lo & ~3;
    ghi[g] = std::max(hi, glo[g]);
  }
  if (n_groups > 0 && !pack_rows(parts, nullptr)) return false;
  for (;;) {
    int worst = -1, worst_len = 0;
    for (int g = 0; g < n_groups; ++g)
      if (bp->per_part(g, parts[g]) > worst_len) {
        worst_len = bp->per_part(g, parts[g]);
        worst = g;
      }
    if (worst < 0 || parts[worst] >= 4 || bp->per_part(worst, parts[worst] + 1) >= worst_len) break;
    std::vector<int> trial = parts;
    ++trial[worst];
    if (!pack_rows(trial, nullptr)) break;
    parts = trial;
  }
  // The chain is as long as the longest part (a multiple of 4 bins = whole quads): 28 for 40 bins and 24
  // for 23 bins at 16 kHz (round 3; it used to be padded to 32).  fbank512b_kernel issues an odd quad on its
  // own; fbank512_kernel issues quads in pairs and runs the row of zeros behind the table as the eighth
  // (same sums, four idle instructions on the per-utterance / dithered paths); the two-frames-per-row
  // kernel keeps an even count.
  int chain = 16;
  for (int g = 0; g < n_groups; ++g) chain = std::max(chain, bp->per_part(g, parts[g]));
  bp->chain = chain = dual ? ((chain + 7) & ~7) : ((chain + 3) & ~3);
  std::vector<int> first_block;
  pack_rows(parts, &first_block);
  bp->blocks.assign(16, Block{-1, 0, 0, 0, 0});
  const int max_start = (260 - chain) & ~3;  // the B operands stay inside the written part of the tile
  for (int g = 0; g < n_groups; ++g) {
    const int per = bp->per_part(g, parts[g]);
    for (int q = 0; q < parts[g]; ++q) {
      Block& bk = bp->blocks[first_block[g] + q];
      bk.group = g;
      bk.part = q;
      bk.lo = std::min(glo[g] + q * per, ghi[g]);
      bk.hi = std::min(glo[g] + (q + 1) * per, ghi[g]);
      bk.start = std::max(0, std::min(bk.lo, max_start)) & ~3;
    }
  }
  return true;
}

// LDS banks of the B reads: a ds_read_b128 is served in groups of 16 lanes - the blocks
// {0,3,5,6}, {1,2,4,7}, {8,11,13,14}, {9,10,12,15} - and the four frames of a block already sit
// on the four 16-byte slots s, s+4, s+8, s+12 (mod 16) of its start: a group is conflict-free when
// the starts / 4 of its 4 blocks differ modulo 4.  A block shorter than the chain may start up to its
// slack earlier (leading taps carry zero weights): choose the shifts greedily, least slack first.
void shift_block_starts(BlockPlan* bp) {
  std::vector<Block>& blocks = bp->blocks;
  const int chain = bp->chain;
  static const int kGroups[4][4] = {{0, 3, 5, 6}, {1, 2, 4, 7}, {8, 11, 13, 14}, {9, 10, 12, 15}};
  for (const auto& grp : kGroups) {
    bool taken[4] = {false, false, false, false};
    int order[4] = {grp[0], grp[1], grp[2], grp[3]};
    auto slack = [&](int bi) {
      const Block& bk = blocks[bi];
      if (bk.group < 0) return 1 << 20;
      return std::min(bk.start / 4, (bk.start + chain - std::max(bk.hi, bk.start)) / 4);
    };
    std::stable_sort(order, order + 4, [&](int x, int y) { return slack(x) < slack(y); });
    for (int bi : order) {
      Block& bk = blocks[bi];
      if (bk.group < 0) {  // idle block: any free residue
        int r = 0;
        while (r < 3 && taken[r]) ++r;
        bk.start = 4 * r;
        taken[r] = true;
        continue;
      }
      const int sl = slack(bi);
      int best = 0;
      for (int k = 0; k <= sl && k < 4; ++k)
        if (!taken[((bk.start / 4) - k) & 3]) {
          best = k;
          break;
        }
      bk.start -= 4 * best;
      taken[(bk.start / 4) & 3] = true;
    }
  }
}

void push_int(int v, std::vector<float>* blob) {
  float as_float;
  std::memcpy(&as_float, &v, 4);
  blob->push_back(as_float);
}

// the A operands of the mel chain, float4 mm_a[mm_quads + 2][64], and the lanes' constants, mm_lane[5][64]
void push_mel_chain(const MelBanksHost& mb, const BlockPlan& bp, std::vector<float>* blob, Fast512Params* p) {
  const std::vector<Block>& blocks = bp.blocks;
  while (blob->size() % 4) blob->push_back(0.0f);  // 16-byte alignment of the float4 tables
  p->off_mm_a = static_cast<int>(blob->size());
  for (int t = 0; t < p->mm_quads + 2; ++t)  // (+ two rows of zeros: the look-ahead reads of the pair loops)
    for (int lane = 0; lane < 64; ++lane)
      for (int c = 0; c < 4; ++c) {
        const Block& bk = blocks[lane >> 2];
        const int m = bk.group < 0 ? -1 : 4 * bk.group + (lane & 3);
        const int k = bk.start + 4 * t + c;  // FFT bin of this tap
        float w = 0.0f;
        if (t < p->mm_quads && m >= 0 && m < mb.num_bins && k >= bk.lo && k < bk.hi && k >= mb.first[m] &&
            k < mb.first[m] + mb.size[m])
          w = 0.25f * mb.w[mb.offset[m] + k - mb.first[m]];  // exact power-of-two scaling
        blob->push_back(w);
      }
  p->off_mm_lane = static_cast<int>(blob->size());
  for (int lane = 0; lane < 64; ++lane) push_int(blocks[lane >> 2].start, blob);
  for (int lane = 0; lane < 64; ++lane) {
    const Block& bk = blocks[lane >> 2];
    push_int(bk.group >= 0 && bk.part == 0 ? 4 * bk.group : -1, blob);
  }
  for (int level = 1; level <= 3; ++level)
    for (int lane = 0; lane < 64; ++lane) {
      const Block& bk = blocks[lane >> 2];
      blob->push_back(bk.group >= 0 && bk.part == 0 && bp.parts[bk.group] > level ? 1.0f : 0.0f);
    }
}

// The DCT-II of MFCC plans ships on the vector pipe (measured: a tie with the MFMA chain on the
// 512-point kernel - 1.17-1.21 against 1.19-1.22 ms -, 19 % faster on the two-frames-per-row kernel,
// which only has that form); SNF_DCT_MFMA=1 selects the chain.  Only the table of the selected form
// goes into the blob (both would not fit in LDS beside the fused-delta buffer); the lifter sits between
// the two.
void push_dct_and_lifter(const MelParams& mp, const std::vector<float>& dct, const std::vector<float>& lifter,
                         bool dual, std::vector<float>* blob, Fast512Params* p) {
  {
    const char* knob = getenv("SNF_DCT_MFMA");
    p->dct_mfma = (!dual && knob && knob[0] == '1') ? 1 : 0;
  }
  // DCT-II as MFMA blocks: block 4 cg + kp = cepstra 4 cg .. 4 cg + 3 x mel bins of partition kp
  p->dd_quads = 0;
  p->off_dd_a = static_cast<int>(blob->size());
  if (mp.kind == SNF_KIND_MFCC && p->dct_mfma) {
    p->dd_quads = ((mp.num_bins + 3) / 4 + 3) / 4;
    const int per = 4 * p->dd_quads;
    for (int t = 0; t < p->dd_quads; ++t)
      for (int lane = 0; lane < 64; ++lane)
        for (int c = 0; c < 4; ++c) {
          const int blk = lane >> 2, cep = 4 * (blk >> 2) + (lane & 3), m = (blk & 3) * per + 4 * t + c;
          blob->push_back(cep < mp.num_ceps && m < mp.num_bins
                              ? dct[static_cast<size_t>(cep) * mp.num_bins + m] : 0.0f);
        }
  }
  p->off_lifter = static_cast<int>(blob->size());
  for (int c = 0; c < 16; ++c)
    blob->push_back(c < static_cast<int>(lifter.size()) ? lifter[c] : 1.0f);
  // DCT-II for the vector pipe, lane-major: group g4 (mel bins 4 g4 .. 4 g4 + 3) x cepstrum l < 16
  while (blob->size() % 4) blob->push_back(0.0f);
  p->off_dd_v = static_cast<int>(blob->size());
  p->dd_groups = 0;
  if (mp.kind == SNF_KIND_MFCC && !p->dct_mfma) {
    p->dd_groups = (mp.num_bins + 3) / 4;
    for (int g4 = 0; g4 < p->dd_groups; ++g4)
      for (int l = 0; l < 16; ++l)
        for (int c = 0; c < 4; ++c) {
          const int m = 4 * g4 + c;
          blob->push_back(l < mp.num_ceps && m < mp.num_bins ? dct[static_cast<size_t>(l) * mp.num_bins + m]
                                                             : 0.0f);
        }
  }
}

// header: what the PERUTT kernel needs to know about THIS warp factor's tables
void write_header(const Fast512Params& p, std::vector<float>* blob) {
  int hdr[kFast512HeaderFloats] = {};
  hdr[0] = p.mm_quads;
  hdr[1] = p.mm_levels;
  hdr[2] = p.dd_quads;
  hdr[3] = p.off_mm_a;
  hdr[4] = p.off_mm_lane;
  hdr[5] = p.off_dd_a;
  hdr[6] = p.off_lifter;
  hdr[7] = p.table_floats;
  hdr[8] = p.off_dd_v;
  hdr[9] = p.dd_groups;
  std::memcpy(blob->data(), hdr, sizeof(hdr));
}

}  // namespace

// Builds the packed LDS table blob from the plan's host tables (warp 1.0 mel banks).  `dual`: tables of
// fbank256x2_kernel (window value per sample instead of per pair, mel taps on the 129 bins themselves).
// -> 0: built, 1: the fast path does not cover this shape
int fast512_build(const MelParams& mp, const std::vector<float>& window, const MelBanksHost& mb_in,
                  const std::vector<float>& dct, const std::vector<float>& lifter, bool dual,
                  std::vector<float>* blob, Fast512Params* out) {
  const int bin_stride = dual ? 1 : 512 / mp.padded;
  const bool spread = bin_stride > 1 && mb_in.num_bins > 0;
  const MelBanksHost spread_banks = spread ? spread_taps(mb_in, bin_stride) : MelBanksHost();
  const MelBanksHost& mb = spread ? spread_banks : mb_in;
  Fast512Params p = scalar_params(mp, dual);
  blob->clear();
  blob->resize(kFast512HeaderFloats, 0.0f);  // header, filled in at the end
  push_window_rows(mp, window, dual, blob);
  push_twiddle_rows(blob);
  BlockPlan bp;
  if (!plan_blocks(mb, dual, &bp)) return 1;
  p.mm_quads = bp.chain / 4;
  p.mm_levels = 1;
  for (int g = 0; g < bp.n_groups; ++g) p.mm_levels = std::max(p.mm_levels, bp.parts[g]);
  shift_block_starts(&bp);
  push_mel_chain(mb, bp, blob, &p);
  push_dct_and_lifter(mp, dct, lifter, dual, blob, &p);
  p.table_floats = static_cast<int>(blob->size());
  write_header(p, blob);
  // One 16-wave workgroup needs 16 x 4 frame tiles (139 264 bytes) beside the tables in the 160 KB of a
  // CU: wide banks (many bins on zero-extended frames, long DCT tables) that leave no room run on the
  // generic kernel instead of failing at launch (found by tests/tools/fuzz_parity.py).
  if (fast512_lds_bytes(p.table_floats, kFast512MaxWaves, false) > kFast512LdsBytes) return 1;
  *out = p;
  return SNF_OK;
}

}  // namespace snf
