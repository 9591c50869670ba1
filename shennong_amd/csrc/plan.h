// The plan behind the C ABI of libshennong_hip.so (include/shennong_amd.h), shared by the capi_*.hip sources.
//
// A plan owns (a) the immutable tables Kaldi would rebuild per utterance (window, FFT twiddles, mel
// banks per VTLN warp, DCT, lifter, IDFT bases, resampler taps), resident in HBM, (b) grow-only
// device scratch for the host-pointer entry points, (c) one HIP stream and the events that time the
// kernels on that stream.  Device buffers are grouped by the plan kind that uses them: a buffer has
// one meaning within a plan kind, and the groups of two kinds are never live in the same plan.
#ifndef SNF_PLAN_H_
#define SNF_PLAN_H_

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "snf_internal.h"

namespace snf {

// hipMalloc that asks the out-of-memory hook (snf_set_oom_hook) for room and tries once more (capi_runtime.hip)
hipError_t malloc_with_hook(void** p, size_t bytes);

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return SNF_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    SNF_HIP_CHECK(malloc_with_hook(&p, want));
    cap = want;
    return SNF_OK;
  }
  template <typename T>
  int upload(const std::vector<T>& v, hipStream_t s) {
    const size_t bytes = sizeof(T) * v.size();
    int rc = ensure(bytes > 0 ? bytes : 16);
    if (rc) return rc;
    if (bytes) {
      // the source is a short-lived pageable host vector: finish the copy before returning
      SNF_HIP_CHECK(hipMemcpyAsync(p, v.data(), bytes, hipMemcpyHostToDevice, s));
      SNF_HIP_CHECK(hipStreamSynchronize(s));
    }
    return SNF_OK;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
  // ... the same, and `*dev` = the buffer: a table's upload and the pointer the kernels get, in one line
  template <typename T, typename P>
  int upload(const std::vector<T>& v, hipStream_t s, P* dev) {
    const int rc = upload(v, s);
    *dev = as<T>();
    return rc;
  }
  template <typename T>
  int ensure(size_t count, T** dev) {
    const int rc = ensure(sizeof(T) * count);
    *dev = as<T>();
    return rc;
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

constexpr int kMaxSlots = 6;

// Scratch and a stream of its own for the plan-less entry points, per calling thread and device: no hipMalloc /
// hipFree per call (both wait for the whole device) and no device-wide wait at the end - the batches a pipeline
// keeps in flight on other threads, and the pitch tracker beside this thread, go on undisturbed.  Lives as long as
// the thread.
struct ThreadScratch {
  hipStream_t stream = nullptr;
  DevBuf buf;
};
ThreadScratch* thread_scratch(int device_id);

// A plan-less call: one block of the thread's scratch carved into 256-byte-aligned pieces, and the stream to run
// on (the caller's, or the thread's own).  `auto p = take<T>(count)` notes a piece; begin() grows the scratch to the
// total (no allocation once it has grown), after which `p` reads as the piece's address - a piece's size and its
// address come from the same line.  finish() waits for the stream, so the scratch is free again for the thread's
// next call.
struct Planless {
  static constexpr int kMaxPieces = 16;
  size_t total = 0, offset[kMaxPieces];
  char* base = nullptr;
  hipStream_t s = nullptr;
  int n_pieces = 0;
  template <typename T>
  struct Piece {
    const Planless* of;
    int index;
    operator T*() const { return reinterpret_cast<T*>(of->base + of->offset[index]); }
  };
  template <typename T>
  Piece<T> take(size_t count) {
    if (n_pieces == kMaxPieces) abort();
    offset[n_pieces] = total;
    total += (sizeof(T) * count + 255) & ~size_t(255);
    return {this, n_pieces++};
  }
  int begin(int device_id, void* stream) {
    SNF_HIP_CHECK(hipSetDevice(device_id));
    ThreadScratch* t = thread_scratch(device_id);
    if (!t) return SNF_E_HIP;
    int rc = t->buf.ensure(total > 0 ? total : 16);
    if (rc) return rc;
    base = t->buf.as<char>();
    s = stream ? static_cast<hipStream_t>(stream) : t->stream;
    return SNF_OK;
  }
  int finish(int rc, const char* what_failed) const {
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = set_error(SNF_E_HIP, what_failed);
    return rc;
  }
  // ... of kernels that raise a flag on the device (`d_bad`, zeroed by the caller in stream order) for an index
  // out of range: the flag comes back with the wait
  int finish(int rc, const char* what_failed, const int* d_bad, const char* copy_failed, const char* bad_index) const {
    int bad = 0;
    if (!rc && hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess)
      rc = set_error(SNF_E_HIP, copy_failed);
    rc = finish(rc, what_failed);
    if (!rc && bad) rc = set_error(SNF_E_INVALID, bad_index);
    return rc;
  }
};

// The offsets tables of the last batch, on the host and on the device: a pipeline runs the same batch layout
// call after call, so tables that did not change are neither validated nor uploaded again, and the tables the
// kernels derived from them (frame starts, frame pairs, delta tiles) stay.  The validity marks of everything
// derived are reset in invalidate() alone.  (Pitch and CMVN plans cache nothing: they upload into soff / foff
// with every call and leave the host copies empty.)
struct OffsetsCache {
  std::vector<int64_t> h_soff, h_foff;
  DevBuf soff, foff;
  bool setidx_valid = false;  // frame start / edge / utterance tables describe the cached tables
  bool pairs_valid = false;   // ... the frame pair table (n_pairs records)
  int64_t n_pairs = 0;
  int tile_cols = -1;         // ... the delta kernel's tile records, built for rows of this width (-1: none)
  int rel32 = -1;             // fbank512b_rel32_spans_ok of the cached tables (-1: not asked yet)

  // (post-processor plans have no sample offsets: null)
  bool same(const int64_t* sample_offsets, const int64_t* frame_offsets, int64_t n_utts) const {
    const size_t bytes = sizeof(int64_t) * static_cast<size_t>(n_utts + 1);
    return h_foff.size() == static_cast<size_t>(n_utts + 1) &&
           h_soff.size() == (sample_offsets ? h_foff.size() : 0) &&
           (!sample_offsets || std::memcmp(h_soff.data(), sample_offsets, bytes) == 0) &&
           std::memcmp(h_foff.data(), frame_offsets, bytes) == 0;
  }
  void invalidate() {
    h_soff.clear();
    h_foff.clear();
    setidx_valid = pairs_valid = false;
    tile_cols = -1;
    rel32 = -1;
  }
  int store(const int64_t* sample_offsets, const int64_t* frame_offsets, int64_t n_utts, hipStream_t s) {
    invalidate();
    std::vector<int64_t> so, fo(frame_offsets, frame_offsets + n_utts + 1);
    if (sample_offsets) so.assign(sample_offsets, sample_offsets + n_utts + 1);
    int rc;
    if (sample_offsets && (rc = soff.upload(so, s))) return rc;
    if ((rc = foff.upload(fo, s))) return rc;
    h_soff.swap(so);
    h_foff.swap(fo);
    return SNF_OK;
  }
};

// ---- device buffers by plan kind ------------------------------------------------------------------
struct MelTables {
  DevBuf window, tw_fft, tw_unpack, tw_dft, dct, lifter, idft;
  DevBuf mel_first, mel_size, mel_off, mel_w, eql, mel_w32, mel_off32;  // per VTLN warp (sync_warp_tables)
  DevBuf fast, fast_hi, fast_warp;  // packed blobs of the 512-point kernels: plan->fp, fp_hi, fp_warp
  DevBuf dct_t;                     // MFCC through the filterbank kernel: the DCT transposed
  DevBuf long_tables;               // fbank2048_kernel / fbank1024x2_kernel
};
struct MelScratch {
  DevBuf uwarp, unoise, noise;         // per utterance: warp id, noise word; per frame: noise key
  DevBuf blk_utt, blk_set0;            // workgroup list of the per-utterance 512-point schedule
  DevBuf setidx, edge, futt;           // per frame: first sample, edge mark, utterance
  DevBuf poff, pairs, fix, fixcount;   // frame pairs and the fix-up list of fbank256x2_kernel
  DevBuf umask;                        // utterances shorter than a window
  DevBuf mel, energy;                  // mel rows (PLP, MFCC through the filterbank kernel), frame energy (PLP)
  DevBuf cep, tile;                    // append_deltas as a chain: cepstra, the delta kernel's tile records
};
struct PitchTables {
  DevBuf lags, ar_first, ar_n, ar_w, ar_quad_w, ar_quad_base, rs_first, rs_ntaps, rs_w;
};
struct PitchWork {  // (the launcher's view of it, raw pointers: PitchScratch)
  DevBuf doff, dp1, fp1, order;  // per utterance: downsampled offsets, phase-1 counts, tracker order
  DevBuf down, stats, bp, states, pov_nccf, nccf_res, anp, frame_meta;  // see PitchScratch
};
struct PostScratch {
  DevBuf tile;                  // delta: tile records of the cached offsets table
  DevBuf stats;                 // VAD thresholds / CMVN sums, per utterance
  DevBuf norm, group, weights;  // CMVN: (offset, scale) per group, group of every utterance, frame weights
};
struct Staging {  // host-pointer entry points: owned by the call that holds host_mu
  DevBuf wave, in, out;
};

}  // namespace snf

struct snf_plan {
  snf_options o{};
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  std::mutex host_mu;  // a host-pointer call owns the plan's staging scratch (`stage`)
                       // from its upload to its download: whole-call lock, taken before `mu`
  int kind = 0, ndims = 0;

  // mel family
  snf::MelParams mp{};
  snf::MelTables mel_t;
  snf::MelScratch mel_s;
  std::vector<float> warps;  // distinct VTLN warp factors seen so far (index = warp id)
  std::string base_banks_error;  // PLP: why the unwarped banks (id 0) cannot be built; empty = they can
  std::vector<snf::MelBanksHost> banks;
  bool warps_dirty = true;
  snf::PlpParams pp{};
  // register-resident fast path for the 512-point configuration
  bool fast512 = false;
  snf::Fast512Params fp{};
  // filterbanks of 65 ... 128 bins (fbank-80): the 64-bin kernel twice, over the two halves of the bank - the
  // second launch with `fp_hi`, writing `wide_offset` floats into every row
  bool wide = false;
  snf::Fast512Params fp_hi{};
  int wide_offset = 0;
  // MFCC through the filterbank kernel + mfcc_dct_kernel (more than 16 cepstra, or more than 64 bins)
  bool mfcc_via_fbank = false;
  // ... and its per-warp-factor tables (VTLN): one blob per warp id, `fp_warp.table_stride` apart
  std::vector<float> h_window, h_dct, h_lifter;
  snf::Fast512Params fp_warp{};
  size_t fast_warps_built = 0;   // number of warp ids covered by mel_t.fast_warp
  bool fast_warps_ok = true;     // false: some warp's banks do not fit the fast kernel
  // register-resident 2048-point path (frames that pad to 2048 or 1024 samples)
  bool fast2048 = false;
  bool pair1024 = false;      // frames that pad to 1024 samples: two per transform (kernels_fbank1024x2.hip)

  // delta (post-processor plans, and MFCC plans with append_deltas)
  snf::DeltaParams dp{};
  snf::DevBuf d_scales, d_dims;
  // append_deltas: true = the MFCC kernel writes [T, num_ceps] to a scratch and the delta kernel forms the
  // rows (two launches: 1.17 + 0.11 ms per 2.98 M frames); false = fbank512_kernel's fused mode (one
  // launch, 1.46 ms: it loses to the chain, profiles/NOTEBOOK.md 4.4; SNF_FUSED_DELTA=1 selects it)
  bool chain_deltas = false;

  // pitch
  snf::PitchTablesHost pt;
  snf::PitchDevTables pd{};
  snf::PitchTables pitch_t;
  snf::PitchWork pitch_s;
  snf::PitchPostParams ppost{};

  snf::PostScratch post_s;
  snf::Staging stage;
  snf::OffsetsCache oc;
  // calls that draw random numbers (dither, delta-pitch noise) so far: every call gets its own noise
  // stream (the reference draws from one global rand(): two calls never repeat the same samples)
  uint64_t noise_calls = 0;

  // timing
  hipEvent_t ev[snf::kMaxSlots + 1] = {};
  const char* slot_name[snf::kMaxSlots + 1] = {};
  int n_slots = 0;
  bool events_valid = false;

  ~snf_plan() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace snf {

inline bool is_mel_kind(int kind) {
  return kind == SNF_KIND_SPECTROGRAM || kind == SNF_KIND_FBANK || kind == SNF_KIND_MFCC || kind == SNF_KIND_PLP ||
         kind == SNF_KIND_ENERGY;
}
inline int guard_device(const snf_plan* plan) {
  SNF_HIP_CHECK(hipSetDevice(plan->device));
  return SNF_OK;
}

// the last step of a host-pointer entry point: results back to the host, and the wait for them
inline int download(snf_plan* plan, void* host, const void* dev, size_t bytes) {
  std::lock_guard<std::mutex> lock(plan->mu);
  SNF_HIP_CHECK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, plan->stream));
  SNF_HIP_CHECK(hipStreamSynchronize(plan->stream));
  return SNF_OK;
}

inline void begin_timing(snf_plan* plan) {
  plan->n_slots = 0;
  plan->events_valid = false;
  (void)hipEventRecord(plan->ev[0], plan->stream);
}
inline void mark_kernel(snf_plan* plan, const char* name) {
  if (plan->n_slots >= kMaxSlots) return;
  ++plan->n_slots;
  plan->slot_name[plan->n_slots] = name;
  (void)hipEventRecord(plan->ev[plan->n_slots], plan->stream);
  plan->events_valid = true;
}

// The noise stream named for the next call of this thread (snf_set_noise_call), 0: none.  Every run entry point
// takes it first thing: a name given to a call that draws nothing is not left behind for the thread's next call.
uint64_t take_noise_call();

// capi_plan.hip
int build_mel_plan(snf_plan* plan);
int build_delta_plan(snf_plan* plan);
int build_pitch_plan(snf_plan* plan);
int sync_warp_tables(snf_plan* plan);
int sync_fast_warp_tables(snf_plan* plan);
int resolve_warps(snf_plan* plan, const float* vtln_warp, const int64_t* frame_offsets, int64_t n_utts,
                  std::vector<int32_t>* ids, bool* any);
int64_t pitch_frames_for(const snf_plan* plan, int64_t n, int64_t* n_down, int64_t* n_down_p1, int64_t* frames_p1);

}  // namespace snf

#endif  // SNF_PLAN_H_
