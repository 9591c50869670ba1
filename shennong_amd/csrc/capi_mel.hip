// C ABI of libshennong_hip.so (include/shennong_amd.h): running a batch of waveforms through a mel-family or
// pitch plan.  snf_plan_run_batch_device is three steps with a plain value between them: route (which
// front-end kernel family, which utterances are masked out, which derived tables), prepare (those tables,
// through the plan's OffsetsCache), launch (the front end, then the family's tail).
#include "plan.h"

using namespace snf;

namespace {

constexpr float kPairSplitRatio = 8.0f;   // fbank256x2_kernel: windowed-energy ratio beyond which a pair is redone
                                          // one frame at a time (kernels_fbank1024x2.hip holds the same number)

int check_offsets(const snf_plan* plan, const int64_t* sample_offsets, const int64_t* frame_offsets,
                  int64_t n_utts) {
  // (rows below offsets[0] would resolve to utterance 0 with a negative local frame)
  if (sample_offsets[0] != 0 || frame_offsets[0] != 0)
    return set_error(SNF_E_INVALID, "offsets tables must start at 0");
  for (int64_t u = 0; u < n_utts; ++u) {
    const int64_t n = sample_offsets[u + 1] - sample_offsets[u];
    const int64_t f = frame_offsets[u + 1] - frame_offsets[u];
    if (n < 0 || f < 0) return set_error(SNF_E_INVALID, "offsets tables must be non-decreasing");
    if (f != snf_plan_num_frames(plan, n))
      return set_error(SNF_E_INVALID, "frame_offsets do not match snf_plan_num_frames for utterance " +
                                          std::to_string(u));
  }
  return SNF_OK;
}

int run_pitch_device(snf_plan* plan, const int16_t* d_wave, const int64_t* sample_offsets,
                     int64_t n_utts, float* d_out, const int64_t* frame_offsets, hipStream_t s) {
  const int64_t total_frames = frame_offsets[n_utts];
  if (total_frames == 0) return SNF_OK;
  std::vector<int64_t> doff(n_utts + 1, 0), dp1(n_utts, 0), fp1(n_utts, 0);
  for (int64_t u = 0; u < n_utts; ++u) {
    int64_t nd, nd1, t1;
    pitch_frames_for(plan, sample_offsets[u + 1] - sample_offsets[u], &nd, &nd1, &t1);
    doff[u + 1] = doff[u] + nd;
    dp1[u] = nd1;
    fp1[u] = t1;
  }
  const int64_t total_down = doff[n_utts];
  int64_t max_down = 0;
  for (int64_t u = 0; u < n_utts; ++u) max_down = std::max(max_down, doff[u + 1] - doff[u]);
  int rc;
  PitchWork& ps = plan->pitch_s;
  PitchBatch b{};
  PitchScratch w{};
  std::vector<int64_t> soff(sample_offsets, sample_offsets + n_utts + 1);
  std::vector<int64_t> foff(frame_offsets, frame_offsets + n_utts + 1);
  if ((rc = plan->oc.soff.upload(soff, s, &b.sample_offsets))) return rc;
  if ((rc = plan->oc.foff.upload(foff, s, &b.frame_offsets))) return rc;
  if ((rc = ps.doff.upload(doff, s, &b.down_offsets))) return rc;
  if ((rc = ps.dp1.upload(dp1, s, &b.down_phase1))) return rc;
  if ((rc = ps.fp1.upload(fp1, s, &b.frames_phase1))) return rc;
  // ragged batches: the tracker walks one utterance per wavefront, so a workgroup lasts as long as
  // its longest utterance - hand the utterances out longest first (ties keep the batch order)
  std::vector<int32_t> order;
  bool ragged = false;
  for (int64_t u = 1; u < n_utts && !ragged; ++u)
    ragged = (foff[u + 1] - foff[u]) != (foff[1] - foff[0]);
  if (ragged && n_utts < (int64_t{1} << 31)) {
    order.resize(static_cast<size_t>(n_utts));
    for (int64_t u = 0; u < n_utts; ++u) order[u] = static_cast<int32_t>(u);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
      return foff[x + 1] - foff[x] > foff[y + 1] - foff[y];
    });
    if ((rc = ps.order.upload(order, s, &b.order))) return rc;
  }
  const size_t nf = static_cast<size_t>(total_frames);
  if ((rc = ps.down.ensure(static_cast<size_t>(total_down > 0 ? total_down : 1), &w.down))) return rc;
  if ((rc = ps.stats.ensure(6 * static_cast<size_t>(n_utts), &w.ub))) return rc;
  if ((rc = ps.bp.ensure(nf * plan->pd.num_states, &w.backptr))) return rc;
  if ((rc = ps.states.ensure(nf, &w.states))) return rc;
  if ((rc = ps.pov_nccf.ensure(nf * plan->pd.num_lags, &w.pov_nccf))) return rc;
  if ((rc = ps.nccf_res.ensure(nf * plan->pd.num_states, &w.nccf_res))) return rc;
  if ((rc = ps.anp.ensure(nf, &w.anp))) return rc;
  if ((rc = ps.frame_meta.ensure(nf, &w.frame_meta))) return rc;
  SNF_HIP_CHECK(hipStreamSynchronize(s));  // host vectors above go out of scope after launch setup
  b.wave = d_wave;
  b.n_utts = n_utts;
  b.total_frames = total_frames;
  b.total_down = total_down;
  b.max_down = max_down;
  return launch_pitch(plan->pd, b, w, d_out, s);
}

// ---- routing ---------------------------------------------------------------------------------------
// Which front-end kernel family a batch runs on.  Decided once per call by route_mel_batch, from the plan's
// static facts and the batch's offsets and warp ids; everything after it reads the route.
enum class FrontEnd {
  generic,        // mel_features_generic_kernel
  fast512,        // fbank512b_kernel / fbank512_kernel (launch_fbank512 picks; twice for a wide bank)
  dual256,        // fbank256x2_kernel: two 256-sample frames per row
  dual256_split,  // ... for the unwarped utterances, the 512-point form with per-warp tables for the warped ones
  pair1024,       // fbank1024x2_kernel
  long2048,       // fbank2048_kernel
};
struct MelRoute {
  FrontEnd fe = FrontEnd::generic;
  bool any_warp = false, any_short = false;
  bool fused = false;               // fbank512_kernel's fused deltas (needs fast512 and no short utterance)
  std::vector<uint8_t> short_mask;  // utterances that run on the generic kernel behind the front end
  // derived tables the family reads
  bool blocks = false;       // workgroup -> (utterance, first frame set) list
  bool pairs = false;        // frame pair table (cached with the offsets unless the batch masks utterances out)
  bool frame_start = false;  // frame -> first sample / edge mark / utterance (cached with the offsets)
  bool noise_keys = false;   // dither: per-frame noise keys of fbank512b_kernel
  bool rel32 = false;        // fbank512b_kernel: frame starts close enough for set-relative 32-bit sample offsets
  bool is_fast() const { return fe == FrontEnd::fast512 || fe == FrontEnd::dual256 || fe == FrontEnd::dual256_split; }
  bool is_dual() const { return fe == FrontEnd::dual256 || fe == FrontEnd::dual256_split; }
};

// VTLN batches of a wide bank / of a filterbank-first MFCC plan run on the generic kernel; every other
// 512-point plan has per-warp tables (sync_fast_warp_tables, before the route reads fast_warps_ok)
bool fast512_takes_warps(const snf_plan& plan) { return plan.fast512 && !(plan.wide || plan.mfcc_via_fbank); }

MelRoute route_mel_batch(const snf_plan& plan, const int64_t* sample_offsets, const int64_t* frame_offsets,
                         int64_t n_utts, bool any_warp) {
  MelRoute r;
  r.any_warp = any_warp;
  r.fused = plan.fp.fused_delta != 0;
  bool use_fast = plan.fast512;
  bool use_long = plan.fast2048 || plan.pair1024;  // (per-utterance VTLN warps included: they read the plan's bank tables)
  if (use_fast && any_warp) use_fast = fast512_takes_warps(plan) && plan.fast_warps_ok;
  // snip_edges = false: the clamped bulk loads of the centred frames need an utterance that holds one full
  // window.  A shorter utterance ALWAYS runs on the generic kernel, whatever else is in the batch (the
  // register-resident kernels leave it out, or compute its frames from some window inside the batch and
  // have them overwritten by the masked generic launch below); a batch shorter than one window holds
  // nothing but such utterances.
  if ((use_fast || use_long) && !plan.mp.snip_edges) {
    if (sample_offsets[n_utts] < plan.mp.win_len) {
      use_fast = use_long = false;
    } else {
      r.short_mask.assign(static_cast<size_t>(n_utts), 0);
      for (int64_t u = 0; u < n_utts; ++u) {
        const int64_t n = sample_offsets[u + 1] - sample_offsets[u];
        if (n > 0 && n < plan.mp.win_len && frame_offsets[u + 1] > frame_offsets[u]) {
          r.short_mask[u] = 1;
          r.any_short = true;
        }
      }
    }
  }
  // Two-frames-per-row plans (fbank256x2_kernel) in a batch with VTLN warps: the kernel an utterance runs
  // on must not depend on its neighbours (the two forms round differently in the last bits), so the
  // unwarped utterances keep the two-frame kernel and only the warped ones take the zero-extended
  // 512-point form with their per-warp tables - two launches over disjoint sets of utterances.
  // (a dual plan is never fused: build_mel_plan)
  if (use_fast) r.fe = !plan.fp.dual ? FrontEnd::fast512 : any_warp ? FrontEnd::dual256_split : FrontEnd::dual256;
  else if (use_long) r.fe = plan.pair1024 ? FrontEnd::pair1024 : FrontEnd::long2048;  // (every utterance, warped or not)
  // workgroup list: every workgroup stages the tables of one warp
  // (fused deltas: a workgroup owns a run of frames of one utterance + their delta halo)
  r.blocks = use_fast && (any_warp || r.fused);
  r.pairs = r.is_dual() || r.fe == FrontEnd::pair1024;
  r.frame_start = !r.pairs && !r.blocks;
  // fbank512b_kernel reads the noise key of a frame from a table: made exactly when launch_fbank512 will
  // choose that kernel for one of the plan's parameter sets
  r.noise_keys = plan.mp.dither != 0.0f && r.fe == FrontEnd::fast512 &&
                 (fbank512b_shape_ok(plan.fp, r.blocks) || (plan.wide && fbank512b_shape_ok(plan.fp_hi, r.blocks)));
  // ... and addresses the samples relative to the first frame of a set where the batch's offsets allow it; a batch
  // with three consecutive utterances that span 2^30 samples keeps the 64-bit form
  // (the answer for the tables is kept with the host's copy of them: a pass over both for every call otherwise)
  r.rel32 = r.fe == FrontEnd::fast512 && !r.blocks && !fbank512b_addr64_knob() &&
            (plan.oc.rel32 >= 0 ? plan.oc.rel32 == 1 : fbank512b_rel32_spans_ok(sample_offsets, frame_offsets, n_utts));
  return r;
}

// ---- prepare: the derived tables the route names ------------------------------------------------------
struct MelCall {
  snf_plan* plan;
  const MelRoute& r;
  hipStream_t s;
  bool own_stream;
  BatchArgs b;       // the batch as every kernel but the two-frame ones sees it
  BatchArgs b_dual;  // the arguments of the two-frame kernels (all utterances, or the unwarped ones)
  void mark(const char* name) const { if (own_stream) mark_kernel(plan, name); }
};

int prepare_mel_tables(MelCall* c, const int64_t* sample_offsets, const int64_t* frame_offsets,
                       const std::vector<int32_t>& warp_ids) {
  snf_plan* plan = c->plan;
  const MelRoute& r = c->r;
  MelScratch& ms = plan->mel_s;
  OffsetsCache& oc = plan->oc;
  BatchArgs& b = c->b;
  hipStream_t s = c->s;
  const int64_t n_utts = b.n_utts, total_frames = b.total_frames;
  int rc;
  if (r.blocks) {
    const int kSetsPerBlock = r.fused ? kFast512FusedSets : kFast512Sets;  // (fbank512_kernel: sets_per_block)
    std::vector<int32_t> blk_utt, blk_set0;
    for (int64_t u = 0; u < n_utts; ++u) {
      if (r.fe == FrontEnd::dual256_split && warp_ids[u] == 0) continue;  // (runs on fbank256x2_kernel)
      if (r.any_short && r.short_mask[u]) continue;                         // (runs on the generic kernel)
      const int64_t sets = (frame_offsets[u + 1] - frame_offsets[u] + 3) / 4;
      for (int64_t s0 = 0; s0 < sets; s0 += kSetsPerBlock) {
        blk_utt.push_back(static_cast<int32_t>(u));
        blk_set0.push_back(static_cast<int32_t>(s0));
      }
    }
    if ((rc = ms.blk_utt.upload(blk_utt, s, &b.blk_utt))) return rc;
    if ((rc = ms.blk_set0.upload(blk_set0, s, &b.blk_set0))) return rc;
    b.n_blocks = static_cast<int64_t>(blk_utt.size());
  }
  c->b_dual = b;
  if (r.pairs) {
    // frame pairs formed inside every utterance (PairRec), built once per offsets table
    // (a batch that leaves utterances to another launch: pairs of the others only, rebuilt on every call)
    const bool partial = r.fe == FrontEnd::dual256_split || r.any_short;
    if (partial) oc.pairs_valid = false;   // (what sits in ms.pairs is about to stop describing the whole table)
    if (!oc.pairs_valid) {
      std::vector<int64_t> poff(static_cast<size_t>(n_utts) + 1, 0);
      for (int64_t u = 0; u < n_utts; ++u) {
        // (an utterance that the two-frame kernels leave to another launch has no pairs)
        const bool off = (r.fe == FrontEnd::dual256_split && warp_ids[u] != 0) || (r.any_short && r.short_mask[u]);
        poff[u + 1] = poff[u] + (off ? 0 : (frame_offsets[u + 1] - frame_offsets[u] + 1) / 2);
      }
      oc.n_pairs = poff[n_utts];
      if ((rc = ms.poff.upload(poff, s))) return rc;
      if ((rc = ms.pairs.ensure(sizeof(PairRec) * static_cast<size_t>(oc.n_pairs)))) return rc;
      if ((rc = launch_build_pair_table(oc.foff.as<int64_t>(), oc.soff.as<int64_t>(), ms.poff.as<int64_t>(), n_utts,
                                        oc.n_pairs, plan->mp.win_shift, plan->mp.win_len, plan->mp.snip_edges,
                                        ms.pairs.as<PairRec>(), s)))
        return rc;
      if (!c->own_stream) SNF_HIP_CHECK(hipStreamSynchronize(s));  // (cached: see below)
      oc.pairs_valid = !partial;
    }
    BatchArgs& bd = c->b_dual;
    bd.pair_tab = ms.pairs.as<PairRec>();
    bd.n_pairs = oc.n_pairs;
    if (r.is_dual() && oc.n_pairs > 0 && !getenv("SNF_DUAL_NO_FIXUP")) {
      // fbank256x2_kernel: pairs of very different energies are redone one frame at a time by a second launch
      // (BatchArgs::fix_tab): room for every pair, the count zeroed in stream order
      if ((rc = ms.fix.ensure(2 * static_cast<size_t>(oc.n_pairs), &bd.fix_tab))) return rc;
      if ((rc = ms.fixcount.ensure(1, &bd.fix_count))) return rc;
      SNF_HIP_CHECK(hipMemsetAsync(ms.fixcount.p, 0, sizeof(unsigned int), s));
      static const float ratio = [] {
        const char* e = getenv("SNF_PAIR_SPLIT_RATIO");   // (experiments: 0 redoes every pair)
        return e ? static_cast<float>(atof(e)) : kPairSplitRatio;
      }();
      bd.split_ratio = ratio;
    }
    bd.blk_utt = nullptr;
    bd.blk_set0 = nullptr;
    bd.n_blocks = 0;
    if (r.is_dual()) bd.utt_warp = nullptr;
  } else if (r.frame_start && !oc.setidx_valid) {
    // frame -> first-sample index, edge marks and utterance index: built once per offsets table,
    // reused by later calls (fast kernel: bulk loads; generic kernel: no per-frame binary search)
    if ((rc = ms.setidx.ensure(sizeof(int64_t) * static_cast<size_t>(total_frames)))) return rc;
    if ((rc = ms.edge.ensure(sizeof(int32_t) * static_cast<size_t>(total_frames)))) return rc;
    if ((rc = ms.futt.ensure(sizeof(int32_t) * static_cast<size_t>(total_frames)))) return rc;
    if ((rc = launch_build_frame_start(oc.foff.as<int64_t>(), oc.soff.as<int64_t>(), n_utts, total_frames,
                                       sample_offsets[n_utts], plan->mp.win_shift, plan->mp.win_len,
                                       plan->mp.snip_edges, ms.setidx.as<int64_t>(), ms.edge.as<int32_t>(),
                                       ms.futt.as<int32_t>(), s)))
      return rc;
    // (the tables are cached: a later call may come in on another stream, so they must be complete)
    if (!c->own_stream) SNF_HIP_CHECK(hipStreamSynchronize(s));
    oc.setidx_valid = true;
  }
  b.frame_start = ms.setidx.as<int64_t>();
  b.frame_edge = ms.edge.as<int32_t>();
  b.frame_utt = oc.setidx_valid ? ms.futt.as<int32_t>() : nullptr;
  return SNF_OK;
}

// ---- launch ------------------------------------------------------------------------------------------
// the register-resident 512-point family: one launch, or two over disjoint utterances (dual256_split)
int run_fast(const MelCall& c, float* out, int cols, double* energy) {
  const snf_plan* plan = c.plan;
  const char* launched = nullptr;
  int rc;
  if (c.r.is_dual()) {
    if (c.b_dual.n_pairs > 0) {
      if ((rc = launch_fbank512(plan->fp, c.b_dual, out, cols, energy, c.s, &launched))) return rc;
      c.mark(launched);
    }
    if (c.r.fe == FrontEnd::dual256) return SNF_OK;
  }
  if (c.b.blk_utt != nullptr && c.b.n_blocks == 0) return SNF_OK;  // (no utterance left for this form)
  if ((rc = launch_fbank512(c.r.any_warp ? plan->fp_warp : plan->fp, c.b, out, cols, energy, c.s, &launched))) return rc;
  c.mark(launched);
  if (plan->wide) {   // the upper half of a wide bank, behind the columns of the lower one
    if ((rc = launch_fbank512(plan->fp_hi, c.b, out + plan->wide_offset, cols, energy, c.s, &launched))) return rc;
    c.mark(launched);
  }
  return SNF_OK;
}

// The front end of every mel-family kind: `out` receives [total_frames, cols] rows (PLP: linear mel energies,
// `energy` the frame energies).
int run_front_end(const MelCall& c, float* out, int cols, double* energy) {
  snf_plan* plan = c.plan;
  int rc;
  if (c.r.is_fast()) return run_fast(c, out, cols, energy);
  switch (c.r.fe) {
    case FrontEnd::pair1024: {  // a pair of 1024-sample frames per transform
      BatchArgs bp = c.b_dual;
      bp.utt_noise = c.b.utt_noise;
      if ((rc = launch_fbank1024x2(plan->mp, bp, plan->mel_t.long_tables.as<float>(), out, cols, energy, c.s))) return rc;
      c.mark("fbank1024x2_kernel");
      break;
    }
    case FrontEnd::long2048:  // one 2048-sample frame per wave
      if ((rc = launch_fbank2048(plan->mp, c.b, plan->mel_t.long_tables.as<float>(), out, cols, energy, c.s))) return rc;
      c.mark("fbank2048_kernel");
      break;
    default:  // FrontEnd::generic
      if ((rc = launch_mel_features(plan->mp, c.b, out, cols, energy, c.s))) return rc;
      c.mark("mel_features_generic_kernel");
      break;
  }
  return SNF_OK;
}

// utterances shorter than a window (snip_edges = false), after the register-resident kernels: the plan's own
// rows from the generic kernel
int run_short(const MelCall& c, float* out, int cols, double* energy) {
  snf_plan* plan = c.plan;
  if (!c.r.any_short || c.r.fe == FrontEnd::generic) return SNF_OK;
  int rc;
  if ((rc = plan->mel_s.umask.upload(c.r.short_mask, c.s))) return rc;
  BatchArgs bm = c.b;
  bm.utt_mask = plan->mel_s.umask.as<uint8_t>();
  if ((rc = launch_mel_features(plan->mp, bm, out, cols, energy, c.s))) return rc;
  c.mark("mel_features_generic_kernel");
  return SNF_OK;
}

}  // namespace

// =================================================================================================
extern "C" {

int snf_plan_run_batch_device(snf_plan* plan, const int16_t* d_wave, const int64_t* sample_offsets,
                              int64_t n_utts, const float* vtln_warp, float* d_out,
                              const int64_t* frame_offsets, void* stream) {
  const uint64_t named_call = take_noise_call();
  if (!plan) return set_error(SNF_E_INVALID, "null plan");
  std::lock_guard<std::mutex> lock(plan->mu);
  int rc = guard_device(plan);
  if (rc) return rc;
  if (n_utts < 0) return set_error(SNF_E_INVALID, "n_utts < 0");
  if (n_utts == 0) return SNF_OK;
  if (!sample_offsets || !frame_offsets) return set_error(SNF_E_INVALID, "null offsets table");
  OffsetsCache& oc = plan->oc;
  MelScratch& ms = plan->mel_s;
  const bool same_tables = oc.same(sample_offsets, frame_offsets, n_utts);
  if (!same_tables) {
    oc.invalidate();
    if ((rc = check_offsets(plan, sample_offsets, frame_offsets, n_utts))) return rc;
  }
  const int64_t total_frames = frame_offsets[n_utts];
  if (total_frames == 0) return SNF_OK;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : plan->stream;
  const bool own_stream = (stream == nullptr);

  if (plan->kind == SNF_KIND_PITCH) {
    // (the tracker uploads its tables with every call: nothing of it is cached)
    oc.invalidate();
    if (own_stream) begin_timing(plan);
    if ((rc = run_pitch_device(plan, d_wave, sample_offsets, n_utts, d_out, frame_offsets, s))) return rc;
    if (own_stream) {
      mark_kernel(plan, "pitch");
      SNF_HIP_CHECK(hipStreamSynchronize(s));
    }
    return SNF_OK;
  }
  if (!is_mel_kind(plan->kind)) return set_error(SNF_E_INVALID, "plan kind does not take audio input");

  std::vector<int32_t> warp_ids;
  bool any_warp = false;
  if ((rc = resolve_warps(plan, vtln_warp, frame_offsets, n_utts, &warp_ids, &any_warp))) return rc;
  if (!plan->base_banks_error.empty()) {
    // (PLP, see snf_plan_create) an utterance with frames that needs the unwarped banks
    for (int64_t u = 0; u < n_utts; ++u)
      if (frame_offsets[u + 1] > frame_offsets[u] && (warp_ids.empty() || warp_ids[u] == 0))
        return set_error(SNF_E_RUNTIME, plan->base_banks_error);
  }
  if ((rc = sync_warp_tables(plan))) return rc;

  if (!same_tables && (rc = oc.store(sample_offsets, frame_offsets, n_utts, s))) return rc;
  if (any_warp && (rc = ms.uwarp.upload(warp_ids, s))) return rc;
  BatchArgs b{};
  b.wave = d_wave;
  b.sample_offsets = oc.soff.as<int64_t>();
  b.frame_offsets = oc.foff.as<int64_t>();
  b.utt_warp = any_warp ? ms.uwarp.as<int32_t>() : nullptr;
  b.n_utts = n_utts;
  b.total_frames = total_frames;
  if (plan->mp.dither != 0.0f) {
    // what the dither streams know about an utterance: a hash of 64 of its samples (wave_noise_id)
    if ((rc = ms.unoise.ensure(static_cast<size_t>(n_utts > 0 ? n_utts : 1), &b.utt_noise))) return rc;
    if ((rc = launch_build_utt_noise(b, ms.unoise.as<uint32_t>(), s))) return rc;
  }
  const int nb = plan->o.mel.num_bins;
  if (plan->kind == SNF_KIND_PLP) {
    if ((rc = ms.mel.ensure(sizeof(float) * static_cast<size_t>(total_frames) * nb))) return rc;
    if ((rc = ms.energy.ensure(sizeof(double) * static_cast<size_t>(total_frames)))) return rc;
  }

  if (any_warp && fast512_takes_warps(*plan) && (rc = sync_fast_warp_tables(plan))) return rc;
  const MelRoute r = route_mel_batch(*plan, sample_offsets, frame_offsets, n_utts, any_warp);
  if (r.fused && (!r.is_fast() || r.any_short))
    return set_error(SNF_E_RUNTIME, "append_deltas: this batch cannot run on the 512-point path");
  if (r.rel32) b.rel32_samples = sample_offsets[n_utts];
  if (r.fe == FrontEnd::fast512 && !r.blocks && !fbank512b_addr64_knob() && !oc.h_foff.empty())
    oc.rel32 = r.rel32 ? 1 : 0;  // (the tables are the cached ones: kept for the calls that bring them again)
  MelCall c{plan, r, s, own_stream, b, b};
  if ((rc = prepare_mel_tables(&c, sample_offsets, frame_offsets, warp_ids))) return rc;

  if (own_stream) begin_timing(plan);
  if (plan->mp.dither != 0.0f) {
    const unsigned long long stream_key = plan->o.seed + 0x9E3779B97F4A7C15ull * (named_call ? named_call : ++plan->noise_calls);
    plan->mp.seed = plan->fp.seed = plan->fp_hi.seed = plan->fp_warp.seed = stream_key;
    // (the keys hold the utterance's noise word: made with every batch; 8 bytes per frame)
    if (r.noise_keys) {
      if ((rc = ms.noise.ensure(static_cast<size_t>(total_frames), &c.b.frame_noise))) return rc;
      if ((rc = launch_build_frame_noise(c.b, ms.noise.as<uint64_t>(), s))) return rc;
    }
  }
  if (plan->kind == SNF_KIND_PLP) {
    if ((rc = run_front_end(c, ms.mel.as<float>(), nb, ms.energy.as<double>()))) return rc;
    if ((rc = run_short(c, ms.mel.as<float>(), nb, ms.energy.as<double>()))) return rc;
    if (plan->o.rasta) {
      if ((rc = launch_rasta(ms.mel.as<float>(), c.b, nb, s))) return rc;
      c.mark("rasta_kernel");
    }
    const char* tail_launched = nullptr;
    if ((rc = launch_plp_tail(plan->pp, c.b, ms.mel.as<float>(), ms.energy.as<double>(), d_out, s, &tail_launched)))
      return rc;
    if (tail_launched) c.mark(tail_launched);
  } else {
    // append_deltas as two launches: the cepstra go to a scratch, the delta kernel forms the rows
    float* feat_out = d_out;
    int feat_cols = plan->ndims;
    if (plan->chain_deltas) {
      feat_cols = plan->o.num_ceps;
      if ((rc = ms.cep.ensure(static_cast<size_t>(total_frames) * feat_cols, &feat_out))) return rc;
    }
    if (r.is_fast() && plan->mfcc_via_fbank) {
      // [log energy |] log-mel rows from the filterbank kernel, then DCT / lifter / energy / htk conventions
      const int in_cols = nb + (plan->o.use_energy ? 1 : 0);
      if ((rc = ms.mel.ensure(sizeof(float) * static_cast<size_t>(total_frames) * in_cols))) return rc;
      if ((rc = run_front_end(c, ms.mel.as<float>(), in_cols, nullptr))) return rc;
      if ((rc = launch_mfcc_dct(ms.mel.as<float>(), in_cols, nb, plan->o.num_ceps, plan->mel_t.dct_t.as<float>(),
                                plan->mp.lifter, plan->o.use_energy ? 1 : 0, plan->o.htk_compat ? 1 : 0,
                                total_frames, feat_out, feat_cols, s)))
        return rc;
      c.mark("mfcc_dct_kernel");
    } else {
      if ((rc = run_front_end(c, feat_out, feat_cols, nullptr))) return rc;
    }
    if ((rc = run_short(c, feat_out, feat_cols, nullptr))) return rc;
    if (plan->chain_deltas) {
      const bool build_tiles = oc.tile_cols != feat_cols;
      if ((rc = ms.tile.ensure(4 * sizeof(int64_t) * static_cast<size_t>(total_frames / 32 + 2)))) return rc;
      const char* delta_launched = nullptr;
      if ((rc = launch_deltas(plan->dp, feat_out, feat_cols, oc.foff.as<int64_t>(), n_utts, total_frames,
                              d_out, ms.tile.as<int64_t>(), build_tiles, s, &delta_launched)))
        return rc;
      // (the tile records are cached: complete before a later call on another stream may use them)
      if (build_tiles && !own_stream) SNF_HIP_CHECK(hipStreamSynchronize(s));
      oc.tile_cols = feat_cols;
      if (delta_launched) c.mark(delta_launched);
    }
  }
  if (own_stream) SNF_HIP_CHECK(hipStreamSynchronize(s));
  return SNF_OK;
}

int snf_plan_run_batch(snf_plan* plan, const int16_t* wave, const int64_t* sample_offsets,
                       int64_t n_utts, const float* vtln_warp, float* out,
                       const int64_t* frame_offsets) {
  if (!plan) return set_error(SNF_E_INVALID, "null plan");
  std::lock_guard<std::mutex> host_lock(plan->host_mu);
  if (n_utts <= 0) return n_utts == 0 ? SNF_OK : set_error(SNF_E_INVALID, "n_utts < 0");
  if (!sample_offsets || !frame_offsets) return set_error(SNF_E_INVALID, "null offsets table");
  const int64_t total_samples = sample_offsets[n_utts] - sample_offsets[0];
  const int64_t total_frames = frame_offsets[n_utts];
  if (sample_offsets[0] != 0 || frame_offsets[0] != 0)
    return set_error(SNF_E_INVALID, "offsets tables must start at 0");
  int16_t* d_wave;
  float* d_out;
  {
    std::lock_guard<std::mutex> lock(plan->mu);
    int rc = guard_device(plan);
    if (rc) return rc;
    if ((rc = plan->stage.wave.ensure(static_cast<size_t>(total_samples > 0 ? total_samples : 1), &d_wave))) return rc;
    if ((rc = plan->stage.out.ensure(static_cast<size_t>(total_frames > 0 ? total_frames : 1) *
                                         (plan->ndims > 0 ? plan->ndims : 1), &d_out)))
      return rc;
    if (total_samples > 0)
      SNF_HIP_CHECK(hipMemcpyAsync(d_wave, wave, sizeof(int16_t) * total_samples, hipMemcpyHostToDevice,
                                   plan->stream));
  }
  int rc = snf_plan_run_batch_device(plan, d_wave, sample_offsets, n_utts, vtln_warp, d_out,
                                     frame_offsets, nullptr);
  if (rc || total_frames == 0) return rc;
  return download(plan, out, d_out, sizeof(float) * total_frames * plan->ndims);
}

// Test aid (include/shennong_amd.h): what snf_plan_run_batch_device runs behind the mel front end of a PLP plan -
// launch_rasta if the options ask for it, launch_plp_tail with the plan's PlpParams - on rows the caller chose.
// The buffers are the call's own (RASTA filters in place; the plan's scratch and offsets cache stay as they are).
int snf_debug_plp_tail(snf_plan* plan, const float* mel, const double* energy, const int64_t* frame_offsets,
                       int64_t n_utts, float* out, float* mel_out) {
  if (!plan || plan->kind != SNF_KIND_PLP) return set_error(SNF_E_INVALID, "not a PLP plan");
  if (n_utts < 0) return set_error(SNF_E_INVALID, "n_utts < 0");
  if (n_utts == 0) return SNF_OK;
  if (!frame_offsets) return set_error(SNF_E_INVALID, "null offsets table");
  if (frame_offsets[0] != 0) return set_error(SNF_E_INVALID, "offsets tables must start at 0");
  for (int64_t u = 0; u < n_utts; ++u)
    if (frame_offsets[u + 1] < frame_offsets[u])
      return set_error(SNF_E_INVALID, "offsets tables must be non-decreasing");
  const int64_t total_frames = frame_offsets[n_utts];
  if (total_frames == 0) return SNF_OK;
  if (!mel || !energy || !out) return set_error(SNF_E_INVALID, "null pointer");
  std::lock_guard<std::mutex> host_lock(plan->host_mu);
  std::lock_guard<std::mutex> lock(plan->mu);
  int rc = guard_device(plan);
  if (rc) return rc;
  if (!plan->base_banks_error.empty()) return set_error(SNF_E_RUNTIME, plan->base_banks_error);
  if ((rc = sync_warp_tables(plan))) return rc;
  hipStream_t s = plan->stream;
  const size_t nf = static_cast<size_t>(total_frames);
  const size_t nb = static_cast<size_t>(plan->o.mel.num_bins), nc = static_cast<size_t>(plan->ndims);
  DevBuf d_mel, d_energy, d_foff, d_out;
  if ((rc = d_mel.ensure(sizeof(float) * nf * nb))) return rc;
  if ((rc = d_energy.ensure(sizeof(double) * nf))) return rc;
  if ((rc = d_out.ensure(sizeof(float) * nf * nc))) return rc;
  if ((rc = d_foff.upload(std::vector<int64_t>(frame_offsets, frame_offsets + n_utts + 1), s))) return rc;
  SNF_HIP_CHECK(hipMemcpyAsync(d_mel.p, mel, sizeof(float) * nf * nb, hipMemcpyHostToDevice, s));
  SNF_HIP_CHECK(hipMemcpyAsync(d_energy.p, energy, sizeof(double) * nf, hipMemcpyHostToDevice, s));
  BatchArgs b{};
  b.frame_offsets = d_foff.as<int64_t>();
  b.n_utts = n_utts;
  b.total_frames = total_frames;
  begin_timing(plan);
  if (plan->o.rasta) {
    if ((rc = launch_rasta(d_mel.as<float>(), b, static_cast<int>(nb), s))) return rc;
    mark_kernel(plan, "rasta_kernel");
  }
  const char* launched = nullptr;
  rc = launch_plp_tail(plan->pp, b, d_mel.as<float>(), d_energy.as<double>(), d_out.as<float>(), s, &launched);
  if (!rc && launched) mark_kernel(plan, launched);
  if (!rc) {
    SNF_HIP_CHECK(hipMemcpyAsync(out, d_out.p, sizeof(float) * nf * nc, hipMemcpyDeviceToHost, s));
    if (mel_out) SNF_HIP_CHECK(hipMemcpyAsync(mel_out, d_mel.p, sizeof(float) * nf * nb, hipMemcpyDeviceToHost, s));
  }
  // (also after a refusal: the uploads read the caller's arrays, and the buffers are freed on return)
  SNF_HIP_CHECK(hipStreamSynchronize(s));
  return rc;
}

// Test aid (include/shennong_amd.h): the route's decision between the two sample addressings of fbank512b_kernel,
// from host offset tables alone (no plan, no device).
int snf_debug_fbank512b_rel32(const int64_t* sample_offsets, const int64_t* frame_offsets, int64_t n_utts) {
  if (!sample_offsets || !frame_offsets || n_utts < 0) return set_error(SNF_E_INVALID, "null offsets table");
  return fbank512b_rel32_ok(sample_offsets, frame_offsets, n_utts) ? 1 : 0;
}

// Test aid (include/shennong_amd.h): the share of frame sets that workgroup `block` of fbank512b_kernel deals to its
// waves, a host function of the three numbers (no plan, no device).
int snf_debug_fbank512b_share(int64_t n_sets, int64_t blocks, int64_t block, int64_t* lo, int64_t* hi) {
  if (!lo || !hi) return set_error(SNF_E_INVALID, "null output");
  if (n_sets < 0 || blocks < 0 || block < 0 || block > blocks) return set_error(SNF_E_INVALID, "no such workgroup");
  fbank512b_share(n_sets, blocks, block, lo, hi);
  return static_cast<int>(fbank512b_blocks(n_sets));  // (the workgroups the launcher starts for n_sets: at most 256)
}

}  // extern "C"
