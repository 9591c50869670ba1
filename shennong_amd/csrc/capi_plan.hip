// C ABI of libshennong_hip.so (include/shennong_amd.h): building and querying plans - the tables of every
// plan kind, the choice of the front-end kernel family, the per-warp-factor mel tables.
#include "plan.h"

using namespace snf;

namespace snf {

namespace {
int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}


// ---- mel-family plan -----------------------------------------------------------------------------

// Part 1: the options, checked in the order in which Kaldi's constructors report them (callers match on the
// messages), the scalar fields of MelParams / PlpParams, and the two host tables whose builders validate as
// they go: the window (plan->h_window) and the unwarped mel banks (plan->banks[0]).  No device work.
int mel_options(snf_plan* plan) {
  const snf_options& o = plan->o;
  snf_frame_options fo = o.frame;
  if (plan->kind == SNF_KIND_ENERGY && o.raw_energy) {
    // reference processor/energy.py:150-154: raw energy = no pre-emphasis, rectangular window
    fo.preemph_coeff = 0.0f;
    fo.window_type = SNF_WINDOW_RECTANGULAR;
  }
  MelParams& p = plan->mp;
  p.win_len = window_size(fo);
  p.win_shift = window_shift(fo);
  p.padded = padded_window_size(fo);
  if (p.win_shift <= 0) return set_error(SNF_E_RUNTIME, "frame shift is shorter than one sample");
  if (p.win_len < 2) return set_error(SNF_E_RUNTIME, "frame length must be at least 2 samples");
  // (the frame energy has no spectrum: an odd window - e.g. 25 ms at 22.05 kHz without rounding to a
  // power of two - is fine for it; Kaldi's RealFft asserts an even size for everything else)
  if (p.padded % 2 != 0 && plan->kind != SNF_KIND_ENERGY)
    return set_error(SNF_E_RUNTIME, "padded window size must be even (real FFT)");
  p.half = p.padded / 2;
  p.pow2 = (p.padded & (p.padded - 1)) == 0;
  p.log2_half = p.pow2 ? ilog2(p.half) : 0;
  p.snip_edges = fo.snip_edges;
  p.remove_dc = fo.remove_dc_offset;
  p.preemph = fo.preemph_coeff;
  p.dither = fo.dither;
  p.seed = o.seed;
  p.kind = plan->kind;
  int rc = make_window(fo, &plan->h_window);
  if (rc) return rc;

  p.use_energy = o.use_energy;
  p.raw_energy = o.raw_energy;
  p.htk_compat = o.htk_compat;
  p.use_log = o.use_log_fbank;
  p.use_power = o.use_power;
  p.num_bins = o.mel.num_bins;
  p.num_ceps = o.num_ceps;
  p.compression = o.compression;
  p.has_floor = o.energy_floor > 0.0f;
  p.log_energy_floor = p.has_floor ? logf(o.energy_floor) : 0.0f;
  p.dct = nullptr;
  p.lifter = nullptr;

  switch (plan->kind) {
    case SNF_KIND_SPECTROGRAM:
      plan->ndims = p.half + 1;
      p.need_raw = o.raw_energy ? 1 : 0;
      p.need_post = o.raw_energy ? 0 : 1;
      p.num_bins = 0;
      break;
    case SNF_KIND_FBANK:
      plan->ndims = o.mel.num_bins + (o.use_energy ? 1 : 0);
      break;
    case SNF_KIND_MFCC:
      plan->ndims = o.append_deltas ? 3 * o.num_ceps : o.num_ceps;
      if (o.append_deltas && (o.delta_order != 2 || o.delta_window != 2))
        return set_error(SNF_E_INVALID, "append_deltas supports delta_order 2 / delta_window 2 only");
      break;
    case SNF_KIND_PLP:
      plan->ndims = o.num_ceps;
      break;
    case SNF_KIND_ENERGY:
      if (o.compression != SNF_COMPRESS_OFF && o.compression != SNF_COMPRESS_LOG &&
          o.compression != SNF_COMPRESS_SQRT)
        return set_error(SNF_E_INVALID, "compression must be in off, log, sqrt");
      plan->ndims = 1;
      p.need_raw = 0;
      p.need_post = 0;
      p.num_bins = 0;
      break;
    default:
      return set_error(SNF_E_INVALID, "not a mel-family kind");
  }
  p.ndims = plan->ndims;
  if (plan->kind != SNF_KIND_SPECTROGRAM && plan->kind != SNF_KIND_ENERGY) {
    p.need_raw = (o.use_energy && o.raw_energy) ? 1 : 0;
    p.need_post = (o.use_energy && !o.raw_energy) ? 1 : 0;
    // Kaldi builds the warp-1.0 banks in the computer's constructor: option errors surface here.  Not for
    // PLP: the reference's own recipe builds the banks of a warp factor when the first frame asks for them
    // (shennong/processor/plp.py:482-494, :559) - an utterance without frames, or a batch in which every
    // utterance carries another warp factor, never sees the errors of the unwarped banks.  The plan then
    // holds zero-weight placeholders as bank 0 and reports the error when an utterance with frames needs it.
    MelBanksHost mb;
    if ((rc = make_mel_banks(o.mel, fo, 1.0f, &mb))) {
      if (plan->kind != SNF_KIND_PLP || rc != SNF_E_RUNTIME || o.mel.num_bins < 3 ||
          padded_window_size(fo) % 2 != 0)
        return rc;
      plan->base_banks_error = last_error();
      make_placeholder_banks(o.mel, fo, &mb);
    }
    plan->warps.assign(1, 1.0f);
    plan->banks.assign(1, mb);
    plan->warps_dirty = true;
  }
  if (plan->kind == SNF_KIND_MFCC) {
    if (o.num_ceps > o.mel.num_bins)
      return set_error(SNF_E_RUNTIME, "num-ceps cannot be larger than num-mel-bins. It should be "
                                      "smaller or equal. You provided num-ceps: " +
                                          std::to_string(o.num_ceps) + "  and num-mel-bins: " +
                                          std::to_string(o.mel.num_bins));
    if (o.num_ceps <= 0) return set_error(SNF_E_RUNTIME, "num-ceps must be strictly positive");
  }
  if (plan->kind == SNF_KIND_PLP) {
    if (o.num_ceps <= 0 || o.num_ceps > o.lpc_order + 1)
      return set_error(SNF_E_INVALID, "We must have 0 < num_ceps <= lpc_order+1");
    PlpParams& q = plan->pp;
    q.num_bins = o.mel.num_bins;
    q.lpc_order = o.lpc_order;
    q.num_ceps = o.num_ceps;
    q.use_energy = o.use_energy;
    q.htk_compat = o.htk_compat;
    q.has_floor = o.energy_floor > 0.0f;
    q.log_energy_floor = q.has_floor ? std::log(static_cast<double>(o.energy_floor)) : 0.0;
    q.rasta = o.rasta;
    q.compress_factor = o.compress_factor;
    q.exact_pow = getenv("SNF_PLP_EXACT_POW") != nullptr ? 1 : 0;
    q.cepstral_scale = o.cepstral_scale;
  }
  return SNF_OK;
}

int upload_delta_scales(snf_plan* plan, int order, int window) {
  std::vector<float> scales;
  std::vector<int> dims;
  make_delta_scales(order, window, &scales, &dims);
  int rc;
  if ((rc = plan->d_scales.upload(scales, plan->stream, &plan->dp.scales))) return rc;
  if ((rc = plan->d_dims.upload(dims, plan->stream, &plan->dp.dims))) return rc;
  plan->dp.order = order;
  plan->dp.window = window;
  plan->dp.n_scales = static_cast<int>(scales.size());
  return SNF_OK;
}

// Part 2: the kind's device tables.  The host tables the fast kernels' blobs are packed from stay in the plan
// (h_window; MFCC: h_dct, h_lifter), each built once.
int mel_tables(snf_plan* plan) {
  const snf_options& o = plan->o;
  MelParams& p = plan->mp;
  int rc;
  if ((rc = plan->mel_t.window.upload(plan->h_window, plan->stream, &p.window))) return rc;

  constexpr double kTwoPi = 6.283185307179586476925286766559005;
  // exp(-2 pi i k / period), k < n
  auto twiddles = [&](DevBuf* dst, int n, int period, const float2** dev) -> int {
    std::vector<float2> tw(n);
    for (int k = 0; k < n; ++k) {
      const double a = -kTwoPi * k / period;
      tw[k] = make_float2(static_cast<float>(std::cos(a)), static_cast<float>(std::sin(a)));
    }
    return dst->upload(tw, plan->stream, dev);
  };
  p.tw_fft = p.tw_unpack = p.tw_dft = nullptr;
  if (p.pow2) {
    if ((rc = twiddles(&plan->mel_t.tw_fft, p.half / 2 > 0 ? p.half / 2 : 1, p.half, &p.tw_fft))) return rc;
    if ((rc = twiddles(&plan->mel_t.tw_unpack, p.half / 2 + 1, p.padded, &p.tw_unpack))) return rc;
  } else {
    if ((rc = twiddles(&plan->mel_t.tw_dft, p.padded, p.padded, &p.tw_dft))) return rc;
  }

  std::vector<float> plp_lifter;
  std::vector<float>& lifter = plan->kind == SNF_KIND_MFCC ? plan->h_lifter : plp_lifter;
  const float* d_lifter = nullptr;
  if ((plan->kind == SNF_KIND_MFCC || plan->kind == SNF_KIND_PLP) && o.cepstral_lifter != 0.0f) {
    make_lifter(o.cepstral_lifter, o.num_ceps, &lifter);
    if ((rc = plan->mel_t.lifter.upload(lifter, plan->stream, &d_lifter))) return rc;
  }
  if (plan->kind == SNF_KIND_MFCC) {
    make_dct_matrix(o.num_ceps, o.mel.num_bins, &plan->h_dct);
    if ((rc = plan->mel_t.dct.upload(plan->h_dct, plan->stream, &p.dct))) return rc;
    p.lifter = d_lifter;
  }
  if (plan->kind == SNF_KIND_PLP) {
    std::vector<float> idft;
    make_idft_bases(o.lpc_order + 1, o.mel.num_bins + 2, &idft);
    if ((rc = plan->mel_t.idft.upload(idft, plan->stream, &plan->pp.idft))) return rc;
    plan->pp.lifter = d_lifter;
  }
  if (plan->kind == SNF_KIND_MFCC && o.append_deltas) {
    const char* knob = getenv("SNF_FUSED_DELTA");
    plan->chain_deltas = !(knob && knob[0] == '1');
    if ((rc = upload_delta_scales(plan, 2, 2))) return rc;
  }
  return SNF_OK;
}

// Filterbank plans the 64-bin kernel covers in two launches, and MFCC plans it covers up to the log-mel energies
// (round 6; the generic wave-per-frame kernel until then, 7 x slower per frame):
//  * a filterbank of 65 ... 128 bins (fbank-80 at 16 kHz is a common front end): the kernel's matrix-pipe mel
//    chain holds 16 blocks of 4 bins; a wider bank runs it TWICE, over the lower and the upper half of the bins
//    (twice the transform arithmetic, still 3.5 x faster than the generic kernel): two parameter sets, the
//    second one writing behind the columns of the first.  The energy column goes with the half it is adjacent to;
//  * MFCC with more than 16 cepstra (Kaldi's "hires" MFCC: 40 bins, 40 cepstra) or more than 64 bins: the
//    filterbank kernel writes [log energy |] log-mel rows to a scratch, mfcc_dct_kernel forms the cepstra.
// -> 0: plan->fp (and fp_hi) are built, 1: not covered, < 0: error
int build_fbank_fast(snf_plan* plan, const MelParams& pf) {
  if (plan->banks.empty() || pf.padded != 512) return 1;
  const std::vector<float>& window = plan->h_window;
  const MelBanksHost& mb = plan->banks[0];
  std::vector<float> none;
  if (pf.num_bins <= kFast512MaxBins) {
    if (!fast512_eligible(pf, false)) return 1;
    std::vector<float> blob;
    const int rc2 = fast512_build(pf, window, mb, none, none, false, &blob, &plan->fp);
    if (rc2 != 0) return rc2;
    if (int rc3 = plan->mel_t.fast.upload(blob, plan->stream, &plan->fp.tables)) return rc3;
    return 0;
  }
  if (pf.num_bins > 2 * kFast512MaxBins || getenv("SNF_DISABLE_WIDE512")) return 1;
  const int nb = pf.num_bins, lo_n = ((nb + 1) / 2 + 3) & ~3, hi_n = nb - lo_n;
  auto half_of = [&](int first_bin, int count, MelBanksHost* out) {
    out->num_bins = count;
    out->num_fft_bins = mb.num_fft_bins;
    for (int m = first_bin; m < first_bin + count; ++m) {
      out->first.push_back(mb.first[m]);
      out->size.push_back(mb.size[m]);
      out->offset.push_back(static_cast<int>(out->w.size()));
      out->w.insert(out->w.end(), mb.w.begin() + mb.offset[m], mb.w.begin() + mb.offset[m] + mb.size[m]);
      out->center_freqs.push_back(mb.center_freqs[m]);
    }
  };
  MelBanksHost mb_lo, mb_hi;
  half_of(0, lo_n, &mb_lo);
  half_of(lo_n, hi_n, &mb_hi);
  MelParams p_lo = pf, p_hi = pf;
  p_lo.num_bins = lo_n;
  p_hi.num_bins = hi_n;
  const bool energy_first = pf.use_energy && !pf.htk_compat;   // column 0; otherwise (htk) the last column
  MelParams& bare = energy_first ? p_hi : p_lo;                // the half that does not write the energy
  if (pf.use_energy) bare.use_energy = bare.need_raw = bare.need_post = 0;
  std::vector<float> blob_lo, blob_hi;
  if (hi_n < 3 || !fast512_eligible(p_lo, false) || !fast512_eligible(p_hi, false)) return 1;
  int rc2 = fast512_build(p_lo, window, mb_lo, none, none, false, &blob_lo, &plan->fp);
  if (rc2 == 0) rc2 = fast512_build(p_hi, window, mb_hi, none, none, false, &blob_hi, &plan->fp_hi);
  if (rc2 != 0) return rc2;
  if (int rc3 = plan->mel_t.fast.upload(blob_lo, plan->stream, &plan->fp.tables)) return rc3;
  if (int rc3 = plan->mel_t.fast_hi.upload(blob_hi, plan->stream, &plan->fp_hi.tables)) return rc3;
  plan->wide_offset = lo_n + (energy_first ? 1 : 0);
  plan->wide = true;
  return 0;
}

// Part 3: which register-resident kernel family serves the plan, if any.  The first that covers the
// configuration wins - fast512 (one launch; `fp.dual`: two 256-sample frames per row), fast512 + wide (two
// launches over the halves of the bank), fast512 + mfcc_via_fbank, pair1024, fast2048 - and is named by the
// plan's flags; none set: the generic kernel.
int choose_fast_path(snf_plan* plan) {
  const snf_options& o = plan->o;
  const MelParams& p = plan->mp;
  const std::vector<float>& window = plan->h_window;
  int rc;
  const bool want_fused = plan->kind == SNF_KIND_MFCC && o.append_deltas && !plan->chain_deltas;
  if (want_fused && (!fast512_eligible(p, false) || o.num_ceps > 16))
    return set_error(SNF_E_INVALID, "append_deltas needs frames that pad to 512 samples (the register-"
                                    "resident path); chain a delta plan for this configuration");
  if (fast512_eligible(p, false)) {
    std::vector<float> blob;
    const MelBanksHost no_banks;
    const bool dual = !want_fused && fast512_dual_eligible(p);
    rc = fast512_build(p, window, plan->banks.empty() ? no_banks : plan->banks[0], plan->h_dct, plan->h_lifter,
                       dual, &blob, &plan->fp);
    if (rc < 0) return rc;
    if (rc == 0) {  // rc > 0: shape not covered by the fast kernel, keep the generic one
      if ((rc = plan->mel_t.fast.upload(blob, plan->stream, &plan->fp.tables))) return rc;
      plan->fast512 = true;
      if (want_fused) {
        // (the fused form keeps 14 waves' tiles + the cepstra of 336 frames in LDS beside the tables)
        if (fast512_lds_bytes(plan->fp.table_floats, kFast512FusedWaves, true) > kFast512LdsBytes)
          return set_error(SNF_E_INVALID, "append_deltas: the mel / DCT tables of this configuration leave no "
                                          "room for the fused form in LDS; chain a delta plan");
        plan->fp.fused_delta = 1;
        plan->fp.delta_scales = plan->d_scales.as<float>();
      }
    }
  }
  if (!plan->fast512 && plan->kind == SNF_KIND_FBANK && p.num_bins > kFast512MaxBins) {
    const int rc2 = build_fbank_fast(plan, p);
    if (rc2 < 0) return rc2;
    plan->fast512 = rc2 == 0;
  }
  if (!plan->fast512 && plan->kind == SNF_KIND_MFCC && !want_fused && !getenv("SNF_DISABLE_MFCC_VIA_FBANK")) {
    MelParams pf = p;
    pf.kind = SNF_KIND_FBANK;
    pf.use_log = 1;
    pf.use_power = 1;
    pf.htk_compat = 0;     // (the energy in column 0 of the scratch rows, whatever the cepstra's layout)
    pf.num_ceps = 0;
    pf.dct = nullptr;
    pf.lifter = nullptr;
    const int rc2 = build_fbank_fast(plan, pf);
    if (rc2 < 0) return rc2;
    if (rc2 == 0) {
      // the DCT matrix transposed, rows of num_ceps rounded up to 16 (mfcc_dct_kernel reads sixteen cepstra at a time)
      const int nc8 = (o.num_ceps + 15) & ~15;
      std::vector<float> dct_t(static_cast<size_t>(o.mel.num_bins) * nc8, 0.0f);
      for (int c = 0; c < o.num_ceps; ++c)
        for (int m = 0; m < o.mel.num_bins; ++m)
          dct_t[static_cast<size_t>(m) * nc8 + c] = plan->h_dct[c * o.mel.num_bins + m];
      if ((rc = plan->mel_t.dct_t.upload(dct_t, plan->stream))) return rc;
      plan->fast512 = plan->mfcc_via_fbank = true;
    }
  }
  if (want_fused && !plan->fast512)
    return set_error(SNF_E_INVALID, "append_deltas: this configuration is not covered by the register-resident "
                                    "512-point kernel (its tables do not fit); chain a delta plan");
  if (plan->fast512) return SNF_OK;
  std::vector<float> blob;
  if (fbank1024x2_eligible(p)) {
    fbank1024x2_tables(p, window, &blob);
    plan->pair1024 = true;
  } else if (fbank2048_eligible(p)) {
    fbank2048_tables(p, window, &blob);
    plan->fast2048 = true;
  } else {
    return SNF_OK;
  }
  return plan->mel_t.long_tables.upload(blob, plan->stream);
}

}  // namespace

int build_mel_plan(snf_plan* plan) {
  int rc = mel_options(plan);
  if (!rc) rc = mel_tables(plan);
  if (!rc) rc = choose_fast_path(plan);
  return rc;
}

// (re)upload the per-warp mel tables after a new warp factor appeared
int sync_warp_tables(snf_plan* plan) {
  if (!plan->warps_dirty || plan->kind == SNF_KIND_SPECTROGRAM) return SNF_OK;
  const int nb = plan->o.mel.num_bins;
  std::vector<int> first, size, off;
  std::vector<float> w, eql;
  for (const MelBanksHost& mb : plan->banks) {
    const int base = static_cast<int>(w.size());
    for (int b = 0; b < nb; ++b) {
      first.push_back(mb.first[b]);
      size.push_back(mb.size[b]);
      off.push_back(base + mb.offset[b]);
    }
    w.insert(w.end(), mb.w.begin(), mb.w.end());
    if (plan->kind == SNF_KIND_PLP) {
      std::vector<float> e;
      make_equal_loudness(mb, &e);
      eql.insert(eql.end(), e.begin(), e.end());
    }
  }
  int rc;
  if ((rc = plan->mel_t.mel_first.upload(first, plan->stream, &plan->mp.mel_first))) return rc;
  if ((rc = plan->mel_t.mel_size.upload(size, plan->stream, &plan->mp.mel_size))) return rc;
  if ((rc = plan->mel_t.mel_off.upload(off, plan->stream, &plan->mp.mel_offset))) return rc;
  if ((rc = plan->mel_t.mel_w.upload(w, plan->stream, &plan->mp.mel_w))) return rc;
  if (plan->fast2048 || plan->pair1024) {
    // the long-frame kernels read a filter in 32-tap slices of 16-byte vectors: a copy of the weights in
    // which every filter is zero-padded to whole slices, behind one all-zero slice (for the lanes whose
    // filter has fewer slices than the widest one of their round)
    std::vector<float> w32(32, 0.0f);
    std::vector<int> off32;
    // ... every filter starts at a multiple of 4 bins (leading zeros) and each group of 4 taps is rotated
    // by the bin index modulo 4 (= the team of 8 lanes that reads it: kernels_fbank2048.hip)
    for (const MelBanksHost& mb : plan->banks)
      for (int b = 0; b < nb; ++b) {
        off32.push_back(static_cast<int>(w32.size()));
        const int lead = mb.first[b] & 3, taps = lead + mb.size[b], rot = b & 3;
        const size_t base32 = w32.size();
        w32.resize(base32 + ((taps + 31) & ~31), 0.0f);
        for (int t = 0; t < ((taps + 3) & ~3); ++t) {
          const int src = (t & ~3) + (((t & 3) + rot) & 3);  // tap stored at position t of its group
          if (src >= lead && src < taps) w32[base32 + t] = mb.w[mb.offset[b] + src - lead];
        }
      }
    if ((rc = plan->mel_t.mel_w32.upload(w32, plan->stream, &plan->mp.mel_w32))) return rc;
    if ((rc = plan->mel_t.mel_off32.upload(off32, plan->stream, &plan->mp.mel_off32))) return rc;
  }
  if (plan->kind == SNF_KIND_PLP) {
    if ((rc = plan->mel_t.eql.upload(eql, plan->stream, &plan->pp.eql))) return rc;
  }
  // the uploads read from host vectors that die at scope exit
  SNF_HIP_CHECK(hipStreamSynchronize(plan->stream));
  plan->warps_dirty = false;
  return SNF_OK;
}

// fast-kernel tables of every warp factor seen so far (rebuilt when a new one appeared)
int sync_fast_warp_tables(snf_plan* plan) {
  if (!plan->fast512 || !plan->fast_warps_ok) return SNF_OK;
  if (plan->fast_warps_built == plan->banks.size()) return SNF_OK;
  std::vector<std::vector<float>> blobs(plan->banks.size());
  size_t stride = 0;
  Fast512Params fp0{};
  for (size_t w = 0; w < plan->banks.size(); ++w) {
    Fast512Params fp{};
    // (per-utterance tables: always the 512-point form, also for plans whose flat batches run dual)
    const int rc = fast512_build(plan->mp, plan->h_window, plan->banks[w], plan->h_dct, plan->h_lifter,
                                 false, &blobs[w], &fp);
    if (rc < 0) return rc;
    if (rc > 0) {  // this warp's banks need more taps per slot than the kernel unrolls
      plan->fast_warps_ok = false;
      return SNF_OK;
    }
    if (w == 0) fp0 = fp;
    stride = std::max(stride, blobs[w].size());
  }
  stride = (stride + 3) & ~static_cast<size_t>(3);
  std::vector<float> all(stride * blobs.size(), 0.0f);
  for (size_t w = 0; w < blobs.size(); ++w)
    std::copy(blobs[w].begin(), blobs[w].end(), all.begin() + w * stride);
  int rc;
  if ((rc = plan->mel_t.fast_warp.upload(all, plan->stream))) return rc;
  plan->fp_warp = fp0;
  plan->fp_warp.fused_delta = plan->fp.fused_delta;
  plan->fp_warp.delta_scales = plan->fp.delta_scales;
  plan->fp_warp.tables = plan->mel_t.fast_warp.as<float>();
  plan->fp_warp.table_stride = static_cast<int>(stride);
  plan->fast_warps_built = plan->banks.size();
  return SNF_OK;
}

// map per-utterance warp factors to table ids, creating tables on demand
int resolve_warps(snf_plan* plan, const float* vtln_warp, const int64_t* frame_offsets, int64_t n_utts,
                  std::vector<int32_t>* ids, bool* any) {
  *any = false;
  if (!vtln_warp || plan->kind == SNF_KIND_SPECTROGRAM) return SNF_OK;
  ids->assign(n_utts, 0);
  for (int64_t u = 0; u < n_utts; ++u) {
    // Kaldi builds the banks of a warp factor when the first frame asks for them
    // ([KALDI-UPSTREAM] MfccComputer::GetMelBanks): an utterance without frames never does, and
    // never sees the option errors of its warp factor
    if (frame_offsets[u + 1] == frame_offsets[u]) continue;
    const float wf = vtln_warp[u];
    int id = -1;
    for (size_t k = 0; k < plan->warps.size(); ++k)
      if (plan->warps[k] == wf) {
        id = static_cast<int>(k);
        break;
      }
    if (id < 0) {
      MelBanksHost mb;
      int rc = make_mel_banks(plan->o.mel, plan->o.frame, wf, &mb);
      if (rc) return rc;
      plan->warps.push_back(wf);
      plan->banks.push_back(mb);
      plan->warps_dirty = true;
      id = static_cast<int>(plan->warps.size()) - 1;
    }
    (*ids)[u] = id;
    if (id != 0) *any = true;
  }
  return SNF_OK;
}

int build_delta_plan(snf_plan* plan) {
  const snf_options& o = plan->o;
  if (o.delta_order < 0 || o.delta_order >= 1000)
    return set_error(SNF_E_RUNTIME, "delta order must be in [0, 999]");
  if (o.delta_window <= 0 || o.delta_window >= 1000)
    return set_error(SNF_E_INVALID, "window must be in [1, 999]");
  plan->ndims = -1;
  return upload_delta_scales(plan, o.delta_order, o.delta_window);
}

int build_pitch_plan(snf_plan* plan) {
  const snf_pitch_options& o = plan->o.pitch;
  int rc = make_pitch_tables(o, &plan->pt);
  if (rc) return rc;
  const PitchTablesHost& t = plan->pt;
  PitchDevTables& d = plan->pd;
  if ((rc = plan->pitch_t.lags.upload(t.lags, plan->stream, &d.lags))) return rc;
  if ((rc = plan->pitch_t.ar_first.upload(t.ar_first, plan->stream, &d.ar_first))) return rc;
  if ((rc = plan->pitch_t.ar_n.upload(t.ar_n, plan->stream, &d.ar_n))) return rc;
  if ((rc = plan->pitch_t.ar_w.upload(t.ar_w, plan->stream, &d.ar_w))) return rc;
  if ((rc = plan->pitch_t.rs_first.upload(t.resample.first, plan->stream, &d.rs_first))) return rc;
  if ((rc = plan->pitch_t.rs_ntaps.upload(t.resample.ntaps, plan->stream, &d.rs_ntaps))) return rc;
  if ((rc = plan->pitch_t.rs_w.upload(t.resample.weights, plan->stream, &d.rs_w))) return rc;
  {
    // ArbitraryResample as 4 x 4 outer-product steps (see PitchDevTables): quad windows and weights
    const int S = t.num_states, groups = ((S + 63) / 64 + 1) & ~1;
    std::vector<int> qbase(static_cast<size_t>(groups) * 16, 0);
    int kmax = 1;
    for (int qd = 0; qd < groups * 16; ++qd) {
      const int s0 = qd * 4;
      if (s0 >= S) continue;
      int lo = t.ar_first[s0], hi = lo;
      for (int s = s0; s < s0 + 4 && s < S; ++s) {
        lo = std::min(lo, t.ar_first[s]);
        hi = std::max(hi, t.ar_first[s] + std::max(t.ar_n[s], 0));
      }
      qbase[qd] = lo;
      kmax = std::max(kmax, hi - lo);
    }
    const int taps = (kmax + 3) & ~3;
    std::vector<float> qw(static_cast<size_t>(groups) * taps * 64, 0.0f);
    for (int g = 0; g < groups; ++g)
      for (int k = 0; k < taps; ++k)
        for (int ln = 0; ln < 64; ++ln) {
          const int s = 64 * g + ln;
          if (s >= S) continue;
          const int j = qbase[g * 16 + ln / 4] + k - t.ar_first[s];
          if (j >= 0 && j < t.ar_n[s])
            qw[((static_cast<size_t>(g) * (taps / 4) + k / 4) * 64 + ln) * 4 + (k & 3)] =
                t.ar_w[static_cast<size_t>(s) * t.max_taps + j];
        }
    if ((rc = plan->pitch_t.ar_quad_w.upload(qw, plan->stream, &d.ar_quad_w))) return rc;
    if ((rc = plan->pitch_t.ar_quad_base.upload(qbase, plan->stream, &d.ar_quad_base))) return rc;
    d.ar_groups = groups;
    d.ar_quad_taps = taps;
  }
  d.first_lag = t.first_lag;
  d.last_lag = t.last_lag;
  d.num_lags = t.num_lags;
  d.num_states = t.num_states;
  d.win_size = t.win_size;
  d.win_shift = t.win_shift;
  d.full_len = t.full_len;
  d.ar_max_taps = t.max_taps;
  d.rs_in_unit = t.resample.in_unit;
  d.rs_out_unit = t.resample.out_unit;
  d.rs_max_taps = t.resample.max_taps;
  d.snip_edges = o.snip_edges;
  d.recompute_frame = o.recompute_frame;
  d.soft_min_f0 = o.soft_min_f0;
  const float delta_pitch_sq =
      static_cast<float>(std::pow(static_cast<double>(logf(static_cast<float>(1.0 + o.delta_pitch))), 2.0));
  d.inter_frame_factor = delta_pitch_sq * o.penalty_factor;
  d.nccf_ballast = o.nccf_ballast;
  plan->ndims = 2;
  return SNF_OK;
}

int64_t pitch_frames_for(const snf_plan* plan, int64_t n, int64_t* n_down, int64_t* n_down_p1,
                         int64_t* frames_p1) {
  const PitchTablesHost& t = plan->pt;
  const int64_t nd = t.resample.num_output(n, true), nd1 = t.resample.num_output(n, false);
  const bool snip = plan->o.pitch.snip_edges != 0;
  const int64_t T = t.frames_available(nd, true, snip);
  int64_t T1 = t.frames_available(nd1, false, snip);
  if (T1 > T) T1 = T;
  if (n_down) *n_down = nd;
  if (n_down_p1) *n_down_p1 = nd1;
  if (frames_p1) *frames_p1 = T1;
  return T;
}

}  // namespace snf

extern "C" {

int snf_plan_create(const snf_options* opts, int device_id, snf_plan** out) {
  if (!opts || !out) return set_error(SNF_E_INVALID, "null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_error(SNF_E_NODEVICE, "no HIP device visible: libshennong_hip needs an MI355X (gfx950)");
  if (device_id < 0 || device_id >= ndev) return set_error(SNF_E_INVALID, "bad device id");
  SNF_HIP_CHECK(hipSetDevice(device_id));
  std::unique_ptr<snf_plan> plan(new snf_plan);
  plan->o = *opts;
  plan->device = device_id;
  plan->kind = opts->kind;
  SNF_HIP_CHECK(hipStreamCreateWithFlags(&plan->stream, hipStreamNonBlocking));
  for (auto& e : plan->ev) SNF_HIP_CHECK(hipEventCreate(&e));
  int rc;
  switch (opts->kind) {
    case SNF_KIND_SPECTROGRAM:
    case SNF_KIND_FBANK:
    case SNF_KIND_MFCC:
    case SNF_KIND_PLP:
    case SNF_KIND_ENERGY:
      rc = build_mel_plan(plan.get());
      break;
    case SNF_KIND_VAD: {
      const snf_vad_options& v = opts->vad;
      plan->ndims = 1;
      rc = SNF_OK;
      if (v.frames_context < 0)
        rc = set_error(SNF_E_RUNTIME, "vad-frames-context must be >= 0");
      else if (!(v.proportion_threshold > 0.0f && v.proportion_threshold < 1.0f))
        rc = set_error(SNF_E_RUNTIME, "vad-proportion-threshold must be in (0, 1)");
      break;
    }
    case SNF_KIND_SLIDING_CMVN: {
      const snf_sliding_cmvn_options& c = opts->sliding_cmvn;
      rc = SNF_OK;
      if (c.cmn_window <= 0) rc = set_error(SNF_E_RUNTIME, "cmn_window must be positive");
      else if (c.min_window <= 0) rc = set_error(SNF_E_RUNTIME, "min_window must be positive");
      break;
    }
    case SNF_KIND_CMVN:
      rc = SNF_OK;
      break;
    case SNF_KIND_DELTA:
      rc = build_delta_plan(plan.get());
      break;
    case SNF_KIND_PITCH:
      rc = build_pitch_plan(plan.get());
      break;
    case SNF_KIND_PITCH_POST: {
      const snf_pitch_post_options& q = opts->pitch_post;
      plan->ppost.o = q;
      plan->ppost.seed = opts->seed;
      plan->ppost.ndims = (q.add_pov_feature ? 1 : 0) + (q.add_normalized_log_pitch ? 1 : 0) +
                          (q.add_delta_pitch ? 1 : 0) + (q.add_raw_log_pitch ? 1 : 0);
      plan->ndims = plan->ppost.ndims;
      rc = SNF_OK;
      if (plan->ndims <= 0)
        rc = set_error(SNF_E_INVALID, "at least one of the pitch post-processing features must be selected");
      else if (q.delay != 0)
        rc = set_error(SNF_E_RUNTIME, "pitch post-processing delay != 0 is not supported");
      else if (q.delta_window <= 0 || q.delta_window >= 1000)
        rc = set_error(SNF_E_RUNTIME, "delta_window must be in [1, 999]");
      break;
    }
    default:
      rc = set_error(SNF_E_INVALID, "unknown or unsupported plan kind");
  }
  if (rc) return rc;
  SNF_HIP_CHECK(hipStreamSynchronize(plan->stream));
  *out = plan.release();
  return SNF_OK;
}

void snf_plan_destroy(snf_plan* plan) {
  if (!plan) return;
  (void)hipSetDevice(plan->device);
  (void)hipStreamSynchronize(plan->stream);
  delete plan;
}

int32_t snf_plan_ndims(const snf_plan* plan) { return plan ? plan->ndims : -1; }
int32_t snf_plan_fast_path(const snf_plan* plan) {
  if (!plan) return -1;
  if (!is_mel_kind(plan->kind)) return 1;  // (no slower alternative exists for this kind)
  return (plan->fast512 || plan->fast2048 || plan->pair1024) ? 1 : 0;
}

int64_t snf_plan_num_frames(const snf_plan* plan, int64_t n) {
  if (!plan) return -1;
  if (is_mel_kind(plan->kind)) return num_frames(plan->o.frame, n);
  if (plan->kind == SNF_KIND_PITCH) return pitch_frames_for(plan, n, nullptr, nullptr, nullptr);
  return -1;
}

}  // extern "C"
