/*
 * shennong_amd.h — C ABI of libshennong_hip.so, the MI355X (gfx950) speech-features backend.
 *
 * This is the drop-in boundary for the hot path of bootphon/shennong: the seam where the
 * reference's Python processors hand one utterance to pykaldi/Kaldi
 *   - MelFeaturesProcessor._process:  cls(options).compute(SubVector(int16 wave), vtln_warp)
 *         (reference shennong/processor/base.py:408-436; filterbank.py:84; mfcc.py:86)
 *   - SpectrogramProcessor.process:   Spectrogram(options).compute(wave, 1.0)
 *         (reference shennong/processor/spectrogram.py:134-140)
 *   - PlpProcessor._compute:          per-frame Python loop over pykaldi primitives
 *         (reference shennong/processor/plp.py:510-626)
 *   - KaldiPitchProcessor.process:    compute_kaldi_pitch(options, wave)
 *         (reference shennong/processor/pitch_kaldi.py:296-299)
 *   - KaldiPitchPostProcessor.process: process_pitch(options, matrix)
 *         (reference shennong/processor/pitch_kaldi.py:535-537)
 *   - DeltaPostProcessor.process:     compute_deltas(options, matrix)
 *         (reference shennong/postprocessor/delta.py:129-131)
 *   - EnergyProcessor.process:        per-frame extract_window + sum of squares
 *         (reference shennong/processor/energy.py:148-186)
 *   - Frames.nframes / window():      num_frames / FeatureWindowFunction
 *         (reference shennong/frames.py:137; shennong/window.py:107-114)
 *   - VadPostProcessor.process:       kaldi.ivector.compute_vad_energy
 *         (reference shennong/postprocessor/vad.py:182-185)
 *   - CmvnPostProcessor.accumulate / process: kaldi.transform.cmvn.Cmvn.accumulate / apply
 *         (reference shennong/postprocessor/cmvn.py:216-219, :277-278)
 *   - SlidingWindowCmvnPostProcessor.process: kaldi.feat.functions.sliding_window_cmn
 *         (reference shennong/postprocessor/cmvn.py:493-495)
 *
 * The ABI is batch-first: one call covers N utterances given as one concatenated int16 buffer
 * plus an offsets table (the reference's process_all / joblib loop, base.py:56-107, becomes a
 * single launch).  Plain pointers and sizes only; no torch/numpy types.
 *
 * Threading: a plan is immutable after creation; run calls on the same plan serialise on an
 * internal mutex, calls on different plans may run concurrently.  The library never keeps a
 * caller pointer after a call returns.  Errors: every entry point returns 0 on success and a
 * negative SNF_E_* code otherwise; snf_last_error() returns a thread-local message.
 *
 * Option-struct field meanings and defaults are exactly Kaldi's FrameExtractionOptions /
 * MelBanksOptions / FbankOptions / MfccOptions / PlpOptions / SpectrogramOptions /
 * PitchExtractionOptions / ProcessPitchOptions / DeltaFeaturesOptions, which the reference
 * wraps one-to-one (reference shennong/processor/base.py:122-374, filterbank.py:48-55,
 * mfcc.py:48-56, plp.py:265-273, pitch_kaldi.py:86-91,321-327, delta.py:54).
 */
#ifndef SHENNONG_AMD_H_
#define SHENNONG_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ------------------------------------------------------------------------- */
#define SNF_OK 0
#define SNF_E_INVALID (-1)  /* bad argument (Python raises ValueError before reaching here)   */
#define SNF_E_RUNTIME (-2)  /* Kaldi-class option error (KALDI_ERR) -> Python RuntimeError     */
#define SNF_E_HIP (-3)      /* HIP runtime failure                                             */
#define SNF_E_NODEVICE (-4) /* no usable gfx950 device                                         */

/* ---- plan kinds --------------------------------------------------------------------------- */
#define SNF_KIND_SPECTROGRAM 0
#define SNF_KIND_FBANK 1
#define SNF_KIND_MFCC 2
#define SNF_KIND_PLP 3
#define SNF_KIND_PITCH 4
#define SNF_KIND_PITCH_POST 5
#define SNF_KIND_DELTA 6
#define SNF_KIND_ENERGY 7
#define SNF_KIND_VAD 8
#define SNF_KIND_CMVN 9
#define SNF_KIND_SLIDING_CMVN 10

/* ---- window types (reference shennong/processor/base.py:215-221) --------------------------- */
#define SNF_WINDOW_HAMMING 0
#define SNF_WINDOW_HANNING 1
#define SNF_WINDOW_POVEY 2
#define SNF_WINDOW_RECTANGULAR 3
#define SNF_WINDOW_BLACKMAN 4

/* energy compression of EnergyProcessor (reference shennong/processor/energy.py:81-84) */
#define SNF_COMPRESS_OFF 0
#define SNF_COMPRESS_LOG 1
#define SNF_COMPRESS_SQRT 2

/* Kaldi FrameExtractionOptions (reference shennong/processor/base.py:122-262). */
typedef struct snf_frame_options {
  float samp_freq;               /* 16000 */
  float frame_shift_ms;          /* 10    */
  float frame_length_ms;         /* 25    */
  float dither;                  /* 1.0 (0 = off; != 0 uses a counter-based GPU RNG)           */
  float preemph_coeff;           /* 0.97  */
  int32_t remove_dc_offset;      /* 1     */
  int32_t window_type;           /* SNF_WINDOW_POVEY */
  int32_t round_to_power_of_two; /* 1     */
  float blackman_coeff;          /* 0.42  */
  int32_t snip_edges;            /* 1     */
} snf_frame_options;

/* Kaldi MelBanksOptions (reference shennong/processor/base.py:288-374). */
typedef struct snf_mel_options {
  int32_t num_bins; /* 23 */
  float low_freq;   /* 20 */
  float high_freq;  /* 0 => Nyquist, <0 => offset from Nyquist */
  float vtln_low;   /* 100 */
  float vtln_high;  /* -500 */
} snf_mel_options;

/* Kaldi PitchExtractionOptions (reference shennong/processor/pitch_kaldi.py:86-91). */
typedef struct snf_pitch_options {
  float samp_freq;               /* 16000 */
  float frame_shift_ms;          /* 10 */
  float frame_length_ms;         /* 25 */
  float preemph_coeff;           /* 0 */
  float min_f0;                  /* 50 */
  float max_f0;                  /* 400 */
  float soft_min_f0;             /* 10 */
  float penalty_factor;          /* 0.1 */
  float lowpass_cutoff;          /* 1000 */
  float resample_freq;           /* 4000 */
  float delta_pitch;             /* 0.005 */
  float nccf_ballast;            /* 7000 */
  int32_t lowpass_filter_width;  /* 1 */
  int32_t upsample_filter_width; /* 5 */
  int32_t recompute_frame;       /* 500 (not exposed by the reference; Kaldi default)           */
  int32_t snip_edges;            /* 1   (not exposed by the reference; Kaldi default)           */
} snf_pitch_options;

/* Kaldi ProcessPitchOptions (reference shennong/processor/pitch_kaldi.py:321-327). */
typedef struct snf_pitch_post_options {
  float pitch_scale;                   /* 2.0 */
  float pov_scale;                     /* 2.0 */
  float pov_offset;                    /* 0.0 */
  float delta_pitch_scale;             /* 10.0 */
  float delta_pitch_noise_stddev;      /* 0.005 (0 = deterministic)                             */
  int32_t normalization_left_context;  /* 75 */
  int32_t normalization_right_context; /* 75 */
  int32_t delta_window;                /* 2 */
  int32_t delay;                       /* 0 */
  int32_t add_pov_feature;             /* 1 */
  int32_t add_normalized_log_pitch;    /* 1 */
  int32_t add_delta_pitch;             /* 1 */
  int32_t add_raw_log_pitch;           /* 0 */
} snf_pitch_post_options;

/* Kaldi VadEnergyOptions (reference shennong/postprocessor/vad.py:77-78). */
typedef struct snf_vad_options {
  float energy_threshold;     /* 5.0 */
  float energy_mean_scale;    /* 0.5 */
  int32_t frames_context;     /* 0 */
  float proportion_threshold; /* 0.6 */
} snf_vad_options;

/* Kaldi SlidingWindowCmnOptions (reference shennong/postprocessor/cmvn.py:407-408). */
typedef struct snf_sliding_cmvn_options {
  int32_t center;             /* 1 */
  int32_t cmn_window;         /* 600 */
  int32_t min_window;         /* 100 */
  int32_t normalize_variance; /* 0 */
} snf_sliding_cmvn_options;

/* One flat options record; `kind` selects which fields are read. */
typedef struct snf_options {
  int32_t kind; /* SNF_KIND_* */
  snf_frame_options frame;
  snf_mel_options mel;
  /* FbankOptions / MfccOptions / PlpOptions / SpectrogramOptions / EnergyProcessor */
  int32_t use_energy;
  float energy_floor;
  int32_t raw_energy;
  int32_t htk_compat;
  int32_t use_log_fbank; /* fbank only */
  int32_t use_power;     /* fbank only */
  int32_t num_ceps;      /* mfcc, plp */
  float cepstral_lifter; /* mfcc, plp */
  int32_t lpc_order;     /* plp */
  float compress_factor; /* plp */
  float cepstral_scale;  /* plp */
  int32_t rasta;         /* plp (shennong extension, reference plp.py:64-146) */
  int32_t compression;   /* energy: SNF_COMPRESS_* */
  /* DeltaFeaturesOptions */
  int32_t delta_order;  /* 2 */
  int32_t delta_window; /* 2 */
  /* mfcc only: non-zero appends the deltas of order 2 / window 2 to every row in the same call,
     [cepstra | delta | delta-delta] = what DeltaPostProcessor().process(MfccProcessor().process(audio))
     returns (reference postprocessor/delta.py:129-131 chained after processor/mfcc.py:86): the plan runs
     the MFCC kernel into a scratch in HBM and the delta kernel on it (any MFCC configuration).  The
     one-launch form of round 2 (512-point path only, slower) is selected by SNF_FUSED_DELTA=1 in the
     environment of snf_plan_create.  Other orders / windows are refused at plan creation. */
  int32_t append_deltas;
  snf_pitch_options pitch;
  snf_pitch_post_options pitch_post;
  snf_vad_options vad;
  snf_sliding_cmvn_options sliding_cmvn;
  uint64_t seed; /* RNG seed for dither / delta-pitch noise */
} snf_options;

typedef struct snf_plan snf_plan; /* opaque */

/* ---- library / device --------------------------------------------------------------------- */
const char* snf_version(void);
const char* snf_last_error(void);
int snf_device_count(void);
int snf_set_device(int device_id);
int snf_device_name(int device_id, char* buf, int buflen);
int snf_device_synchronize(void);

/* ---- host-side helpers that replace pykaldi free functions -------------------------------- */
/* kaldi.feat.window.num_frames(nsamples, opts, flush=True)   (reference frames.py:137) */
int64_t snf_num_frames(const snf_frame_options* o, int64_t num_samples);
/* kaldi.feat.window.first_sample_of_frame(frame, opts)        (reference plp.py:218) */
int64_t snf_first_sample_of_frame(const snf_frame_options* o, int64_t frame);
int32_t snf_window_size(const snf_frame_options* o);
int32_t snf_window_shift(const snf_frame_options* o);
int32_t snf_padded_window_size(const snf_frame_options* o);
/* FeatureWindowFunction.from_options(opts).window             (reference window.py:107-114);
   writes snf_window_size() floats. */
int snf_window_function(const snf_frame_options* o, float* out);
/* Number of frames Kaldi's pitch extractor emits for `num_samples` input samples. */
int64_t snf_pitch_num_frames(const snf_pitch_options* o, int64_t num_samples);

/* ---- plans ---------------------------------------------------------------------------------- */
/* Precomputes window, mel banks (per distinct vtln warp, on demand), DCT, lifter, IDFT bases,
   resampler taps... and uploads them to `device_id`.  Immutable afterwards. */
int snf_plan_create(const snf_options* opts, int device_id, snf_plan** out);
void snf_plan_destroy(snf_plan* plan);
/* output dimension (columns); for DELTA/PITCH_POST/ENERGY see the dedicated entry points */
int32_t snf_plan_ndims(const snf_plan* plan);
/* 1 when the plan runs on a register-resident kernel (even frames that pad to 512, 256 or 128 samples
   with up to 64 mel bins, 16 cepstra and a power spectrum: 8 and 16 kHz audio; or to 2048 / 1024 samples
   with up to 128 mel bins: 32, 44.1 and 48 kHz audio), 0 when its option combination falls back to the
   generic wave-per-frame kernel (5 to 8x slower per frame; e.g. 4096-sample frames, odd window lengths,
   magnitude filterbanks on short frames): hosts should say so instead of being silently slow. */
int32_t snf_plan_fast_path(const snf_plan* plan);
/* rows produced for an utterance of `num_samples` samples (bit-exact Kaldi NumFrames) */
int64_t snf_plan_num_frames(const snf_plan* plan, int64_t num_samples);

/*
 * Audio -> Features for a batch of utterances (kinds SPECTROGRAM, FBANK, MFCC, PLP, PITCH, ENERGY).
 *   wave            concatenated int16 PCM of all utterances            [sample_offsets[n_utts]]
 *   sample_offsets  n_utts+1 offsets into `wave`
 *   vtln_warp       n_utts warp factors or NULL (=1.0; ignored by SPECTROGRAM/PITCH/ENERGY)
 *   out             concatenated row-major float32 [frame_offsets[n_utts], ndims]
 *   frame_offsets   n_utts+1 row offsets; frame_offsets[u+1]-frame_offsets[u] must equal
 *                   snf_plan_num_frames(plan, samples of u)
 * The rows of an utterance are the same bits whatever else is in the batch (the reference processes one
 * utterance at a time: shennong/processor/base.py:150-180): the kernel an utterance runs on depends on the
 * plan, on its own warp factor and on its own length only - a batch may therefore take more than one
 * launch (unwarped / warped utterances of a two-frames-per-row plan; utterances shorter than one window
 * with snip_edges = 0 go to the generic kernel).  Exception: dither != 0 (a random stream keyed by the
 * frame's position in the batch).
 * Host-pointer variant: stages through device memory owned by the plan (H2D, kernels, D2H).
 */
int snf_plan_run_batch(snf_plan* plan, const int16_t* wave, const int64_t* sample_offsets,
                       int64_t n_utts, const float* vtln_warp, float* out,
                       const int64_t* frame_offsets);

/* Device-pointer variant: `d_wave`/`d_out` are device buffers on the plan's device; the offsets
   tables and vtln_warp stay host pointers (they are small and are uploaded by the call).
   `stream` is a hipStream_t (NULL = the plan's own stream).  Asynchronous w.r.t. the host when
   `stream` != NULL; with NULL the call returns after the plan's stream has been synchronised.
   A plan owns scratch in HBM - its offsets and frame tables, the lists of the two-frames-per-transform kernels,
   the mel / log-mel rows of PLP and of MFCC with more than 16 cepstra, the tracker's buffers: asynchronous
   calls of ONE plan on DIFFERENT streams must not overlap on the device unless they pass the same offsets
   tables and the plan writes no intermediate (the 512-sample filterbank / MFCC-13 / spectrogram kernels).  One
   plan per stream otherwise (what the Python host does for the pieces of a large batch: `Plan._clones`). */
int snf_plan_run_batch_device(snf_plan* plan, const int16_t* d_wave, const int64_t* sample_offsets,
                              int64_t n_utts, const float* vtln_warp, float* d_out,
                              const int64_t* frame_offsets, void* stream);

/*
 * Features -> Features post-processors (kinds DELTA, PITCH_POST, VAD, SLIDING_CMVN).
 * VAD writes one column of 0.0 / 1.0 (the reference casts it to uint8).
 *   in   concatenated row-major float32 [frame_offsets[n_utts], in_cols]
 *   out  concatenated row-major float32 [frame_offsets[n_utts], snf_post_ndims(plan, in_cols)]
 */
int32_t snf_post_ndims(const snf_plan* plan, int32_t in_cols);
int snf_post_run_batch(snf_plan* plan, const float* in, int32_t in_cols,
                       const int64_t* frame_offsets, int64_t n_utts, float* out);
int snf_post_run_batch_device(snf_plan* plan, const float* d_in, int32_t in_cols,
                              const int64_t* frame_offsets, int64_t n_utts, float* d_out,
                              void* stream);

/*
 * CMVN (plan kind SNF_KIND_CMVN).  Statistics are Kaldi's double [2, cols+1] blocks
 * (row 0: sums and, last, the weighted frame count; row 1: sums of squares).
 *   accumulate: stats[group[u]] += stats of utterance u (weights: per-frame, NULL = 1.0;
 *               group: per-utterance speaker index, NULL = one group 0).  `stats` is
 *               [n_groups, 2, cols+1] on the host and is accumulated INTO.
 *   apply:      out = Kaldi ApplyCmvn / ApplyCmvnReverse of each utterance with stats[group[u]];
 *               fails with SNF_E_INVALID when a used group has count < 1.
 */
int snf_cmvn_accumulate(snf_plan* plan, const float* in, int32_t cols, const int64_t* frame_offsets,
                        int64_t n_utts, const float* weights, const int32_t* group,
                        int32_t n_groups, double* stats);
int snf_cmvn_apply(snf_plan* plan, const float* in, int32_t cols, const int64_t* frame_offsets,
                   int64_t n_utts, const double* stats, const int32_t* group, int32_t n_groups,
                   int32_t norm_vars, int32_t reverse, float* out);
/* the same with the feature blocks (and the optional per-frame weights) resident in HBM; offsets,
 * group ids and statistics stay on the host */
int snf_cmvn_accumulate_device(snf_plan* plan, const float* d_in, int32_t cols,
                               const int64_t* frame_offsets, int64_t n_utts, const float* d_weights,
                               const int32_t* group, int32_t n_groups, double* stats);
int snf_cmvn_apply_device(snf_plan* plan, const float* d_in, int32_t cols,
                          const int64_t* frame_offsets, int64_t n_utts, const double* stats,
                          const int32_t* group, int32_t n_groups, int32_t norm_vars, int32_t reverse,
                          float* d_out);

/*
 * Column-wise concatenation of two device-resident feature blocks, utterance by utterance (reference
 * shennong/features.py:386-437 `Features.concatenate`, used by pipeline.py:636-641 to append the pitch
 * columns): out[u] = [a[u][:rows], b[u][:rows]] with rows = offsets_out[u+1] - offsets_out[u] (the
 * caller trims the longer side within its tolerance).  All offsets tables are host arrays [n_utts+1].
 */
int snf_concat_columns_device(int device_id, const float* d_a, int32_t cols_a,
                              const int64_t* offsets_a, const float* d_b, int32_t cols_b,
                              const int64_t* offsets_b, int64_t n_utts, float* d_out,
                              const int64_t* offsets_out);

/*
 * Random terms (dither, reference processor/base.py:122; delta-pitch noise, pitch_kaldi.py:321-327).  A
 * draw is keyed by (options seed, noise call, the frame's index inside its utterance, the utterance's
 * length and a hash of 64 samples spread over it): never by the frame's position in the batch.  The noise call is the plan's own
 * count of calls that draw - every call a new stream, like the reference's global rand() - unless the
 * calling thread names it for its NEXT such call with snf_set_noise_call(call != 0): a caller that must see
 * the same noise for the same utterance in two passes over a corpus (streamed CMVN by speaker: statistics
 * pass, then apply pass) names the same call in both.
 */
int snf_set_noise_call(uint64_t call);

/*
 * Number of NaN / +-Inf among n floats of a device-resident block (16-byte aligned): the data part of
 * reference shennong/features.py:170-215 `Features.is_valid` ("data contains non-finite numbers"), run on
 * the whole batch before its only device -> host copy.
 */
int snf_count_nonfinite_device(int device_id, const float* d_data, uint64_t n, uint64_t* count);

/* ---- diagonal GMM (reference processor/ubm.py, DiagUbmProcessor) -------------------------------
 * Model in Kaldi's DiagGmm natural form, float32 device buffers: gconsts[num_gauss],
 * means_invvars[num_gauss x dim], inv_vars[num_gauss x dim] (row-major); frames d_x[n_frames x dim].
 * L[f, c] = gconsts[c] + x_f . means_invvars[c] - 0.5 x_f^2 . inv_vars[c] ([KALDI-UPSTREAM] diag-gmm.cc
 * DiagGmm::LogLikelihoods), computed by one device path for every entry point below (kernels_gmm.hip), so
 * the same (frame, Gaussian) gives the same bits in all of them.  `stream` NULL: the calling thread's own
 * stream.  Every call waits for its stream before returning; scratch is the calling thread's (no
 * allocation once grown).  Invalid arguments return SNF_E_INVALID before any device work.
 */
/* L for every frame and Gaussian: d_loglikes[n_frames x num_gauss] (DiagGmm::LogLikelihoods). */
int snf_gmm_loglikes(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const float* d_gconsts,
                     const float* d_means_invvars, const float* d_inv_vars, int32_t num_gauss, float* d_loglikes,
                     void* stream);
/* E-step statistics (reference ubm.py:342-343, :625-626 accumulate_from_diag_multi_threaded ->
 * [KALDI-UPSTREAM] mle-diag-gmm.cc AccumDiagGmm::AccumulateFromDiag): posteriors P = softmax_c(L) * w_f
 * (d_frame_weights[n_frames], NULL = all ones); d_stats[num_gauss x (2 dim + 1)] float64 device rows
 * [sum_f P | sum_f P x | sum_f P x^2] (occupancy, mean and variance accumulators), *d_tot_like =
 * sum_f w_f lse_f (float64, device); d_lse[n_frames] (may be NULL) receives the per-frame log-sum-exp.
 * Deterministic: no atomics, fixed reduction order. */
int snf_gmm_accumulate(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const float* d_frame_weights,
                       const float* d_gconsts, const float* d_means_invvars, const float* d_inv_vars,
                       int32_t num_gauss, double* d_stats, double* d_tot_like, float* d_lse, void* stream);
/* Top num_gselect Gaussians per frame, best first (reference ubm.py:481-482 gaussian_selection_matrix ->
 * [KALDI-UPSTREAM] diag-gmm.cc DiagGmm::GaussianSelection): d_gselect[n_frames x num_gselect] int32 and
 * d_loglike[n_frames] (may be NULL) = log-sum-exp of the selected L.  Order: descending L, equal L to the
 * higher Gaussian index first (Kaldi's std::sort of (loglike, index) pairs with std::greater). */
int snf_gmm_gselect(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const float* d_gconsts,
                    const float* d_means_invvars, const float* d_inv_vars, int32_t num_gauss, int32_t num_gselect,
                    int32_t* d_gselect, float* d_loglike, void* stream);
/* The same among num_preselect preselected Gaussians per frame, d_preselect[n_frames x num_preselect]
 * (reference ubm.py:467-478 gaussian_selection_preselect -> [KALDI-UPSTREAM] DiagGmm::
 * GaussianSelectionPreselect); ties compare the Gaussians' own indices.  num_gselect <= num_preselect;
 * an index outside [0, num_gauss) fails with SNF_E_INVALID. */
int snf_gmm_gselect_preselect(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const float* d_gconsts,
                              const float* d_means_invvars, const float* d_inv_vars, int32_t num_gauss,
                              const int32_t* d_preselect, int32_t num_preselect, int32_t num_gselect,
                              int32_t* d_gselect, float* d_loglike, void* stream);
/* Posteriors of a selection (reference ubm.py:549-572 gaussian_selection_to_post, log_likelihoods_preselect +
 * apply_softmax_): d_post[n_frames x num_gselect] aligned with d_gselect, d_loglike[n_frames] the
 * log-sum-exp of the selected L.  min_post >= 0: the reference's sequential pruning loop (each entry in
 * turn: zeroed when below min_post, then the whole row renormalised; a row summing to 0 gets 1 at its
 * first maximum); min_post < 0: no pruning. */
int snf_gmm_selection_posteriors(int device_id, const float* d_x, int64_t n_frames, int32_t dim,
                                 const float* d_gconsts, const float* d_means_invvars, const float* d_inv_vars,
                                 int32_t num_gauss, const int32_t* d_gselect, int32_t num_gselect, float min_post,
                                 float* d_post, float* d_loglike, void* stream);
/* Dense posteriors, the posteriorgram of the model (an extension: the reference hands out the pruned posteriors of a
 * selection only): d_post[n_frames x num_gauss] float32 row-major, d_post[f, c] = expf(L[f, c] - lse_f) with
 * lse_f the per-frame log-sum-exp over all Gaussians, the one snf_gmm_accumulate computes (bit-equal; written to
 * d_lse[n_frames] unless that is NULL).  L is recomputed per 64-frame tile as in the E-step: no
 * [n_frames x num_gauss] block of L goes through memory.  Every element of d_post is written.  The rows are what
 * snf_dtw_pairs' SNF_DTW_SYMKL compares. */
int snf_gmm_posteriors(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const float* d_gconsts,
                       const float* d_means_invvars, const float* d_inv_vars, int32_t num_gauss, float* d_post,
                       float* d_lse, void* stream);

/* ---- linear VTLN (reference processor/vtln.py, VtlnProcessor) ----------------------------------
 * Segments: contiguous runs of frames, h_seg_offsets[n_segments + 1] (HOST int64, non-decreasing, first 0,
 * last n_frames); a segment may be empty.  dim <= 64.  Model buffers as in the snf_gmm_* block.  Outputs are
 * float64 sums over fixed-order partials (no atomics): the same inputs give the same bits.  `stream` NULL:
 * the calling thread's own stream; every call waits for its stream before returning.  Invalid arguments
 * return SNF_E_INVALID before any device work.
 */
/* fMLLR statistics per segment ([KALDI-UPSTREAM] fmllr-diag-gmm.cc FmllrDiagGmmAccs::
 * AccumulateFromPosteriorsPreselect, reference vtln.py:434-441): d_gselect / d_post [n_frames x num_gselect]
 * (int32 / float32, pruned posteriors 0), 1 <= num_gselect <= 64.  d_stats[n_segments x U x (dim + 1)]
 * float64 with U = dim (dim + 1) + dim + 1 and x+ = [x | 1]: rows d (dim + 1) + k hold G[d][k][:] =
 * sum_f b_f[d] x+_k x+, rows dim (dim + 1) + d hold K[d][:] = sum_f a_f[d] x+, the last row sum_f count_f x+
 * (its last entry is beta); a_f / b_f / count_f = sum_j p_fj means_invvars / inv_vars / 1 of g_fj. */
int snf_fmllr_accumulate(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const int32_t* d_gselect,
                         const float* d_post, int32_t num_gselect, const float* d_means_invvars,
                         const float* d_inv_vars, int32_t num_gauss, const int64_t* h_seg_offsets,
                         int64_t n_segments, double* d_stats, void* stream);
/* d_gram[(2 dim + 1) x (2 dim + 1)] float64 = sum_f w_f z_f z_f^T, z = [x | 1 | y] (the sums of reference
 * vtln.py:299-343, gmm-train-lvtln-special); d_weights[n_frames] NULL = all ones. */
int snf_vtln_gram(int device_id, const float* d_x, const float* d_y, const float* d_weights, int64_t n_frames,
                  int32_t dim, double* d_gram, void* stream);
/* snf_vtln_gram over rows gathered from blocks: record f takes row d_row[f] of block d_block[f] of both
 * d_x_blocks and d_y_blocks (DEVICE arrays of DEVICE pointers, each block row-major [rows x dim] float32);
 * d_weights[n_frames] NULL = all ones.  The caller keeps every (block, row) in range.  The result equals,
 * bit for bit, snf_vtln_gram on the same rows gathered in the same order. */
int snf_vtln_gram_rows(int device_id, const float* const* d_x_blocks, const float* const* d_y_blocks,
                       const int32_t* d_block, const int64_t* d_row, const float* d_weights,
                       int64_t n_frames, int32_t dim, double* d_gram, void* stream);
/* Class search per segment over the statistics of snf_fmllr_accumulate ([KALDI-UPSTREAM] lvtln.cc
 * LinearVtln::ComputeTransform): d_A[num_classes x dim x dim] and d_logdets[num_classes] float64;
 * norm_type 0 none, 1 offset, 2 diag; outputs d_objf[n_segments x num_classes] float64 (every class's
 * objective), d_class[n_segments] int32 (first maximum), d_impr / d_count[n_segments] float64 and
 * d_transform[n_segments x dim x (dim + 1)] float32.  beta = 0: default_class, [A_default | 0], 0, 0. */
int snf_lvtln_select(int device_id, const double* d_stats, int64_t n_segments, int32_t dim, const double* d_A,
                     const double* d_logdets, int32_t num_classes, int32_t norm_type, double logdet_scale,
                     int32_t default_class, double* d_objf, int32_t* d_class, double* d_impr, double* d_count,
                     float* d_transform, void* stream);
/* d_y[f] = W_s[:, :dim] x_f + W_s[:, dim] for the segment s of frame f, d_transforms[n_segments x dim x
 * (dim + 1)] float32 (reference vtln.py:659-665). */
int snf_affine_apply_segments(int device_id, const float* d_x, int64_t n_frames, int32_t dim,
                              const int64_t* h_seg_offsets, int64_t n_segments, const float* d_transforms,
                              float* d_y, void* stream);

/* ---- bottleneck features (reference processor/bottleneck.py, BottleneckProcessor) ----------------
 * The BUT/Phonexia extractor on 8 kHz int16 audio: frames of 200 samples every 80, n < 200 ? 0 :
 * (n - 200) / 80 + 1 of them per utterance.  Batch first: h_*_offsets[n_utts + 1] are HOST int64 tables
 * (non-decreasing, first 0) of samples, frames or rows per utterance; every other buffer is on the device.
 * float32 arithmetic except the VAD statistics (float64) and the voiced mean (float64 sums), every sum in
 * a fixed order (no atomics): an utterance gives the same bits alone and in any batch.  `stream` NULL: the
 * calling thread's own stream; every call waits for its stream before returning.  Invalid arguments return
 * SNF_E_INVALID before any device work.
 */
/* d_y[m x n] = act(d_x[m x k] d_w[k x n] + d_b[n]), row-major float32, act 0 = identity, 1 = logistic sigmoid
 * (reference bottleneck.py:461-462 _sigmoid_fun and the `f(Y.dot(W) + b)` of :485-500), on the FP32 matrix
 * cores: every element is one fused multiply-add chain over k ascending, independent of m. */
int snf_dense_layer(int device_id, const float* d_x, int64_t m, int32_t k, const float* d_w, const float* d_b,
                    int32_t n, int32_t act, float* d_y, void* stream);
/* Voice activity detection (reference bottleneck.py:403-453 _compute_vad with bugfix = False: int16-wrapped
 * squares, per-frame integer sums, standardisation and 5 EM passes of a 1-D 3-component GMM in float64):
 * d_mask[total_frames] uint8 (1 = voiced: posterior of component 0 below 0.3), d_voiced[n_utts] int32 the
 * voiced count.  Where the reference catches a RuntimeWarning (constant signal, an emptied or collapsed
 * component) the mask is all 0. */
int snf_bottleneck_vad(int device_id, const int16_t* d_wave, const int64_t* h_sample_offsets, int64_t n_utts,
                       uint8_t* d_mask, int32_t* d_voiced, void* stream);
/* HTK log-mel filterbank (reference bottleneck.py:117-118 _add_dither, :182-217 _fbank_htk): uniform dither
 * `dither` * U(-1, 1) per sample (keyed by the utterance's content, the sample index and `seed`; 0 = none,
 * exact), window, 256-point transform, power, 24 filters, log(max(1, .)): d_logmel[total_frames x 24].
 * d_tables (8-byte aligned float32, built by the host): window[200] | exp(-2 pi i j / 256) as (re, im),
 * j < 256 | filterbank[129 x 24] row-major (the matrix of bottleneck.py:135-179 _mel_fbank_mx). */
int snf_bottleneck_fbank(int device_id, const int16_t* d_wave, const int64_t* h_sample_offsets, int64_t n_utts,
                         const float* d_tables, float dither, uint64_t seed, float* d_logmel, void* stream);
/* Network input (reference bottleneck.py:743-754 and :465-474 _preprocess_nn_input): the mean over the voiced
 * frames is subtracted (0 for an utterance without voiced frames), the first and the last frame repeated 15
 * times, and every window of 2 context + 1 frames projected per band on the 6 columns of d_basis
 * [(2 context + 1) x 6]: d_x[rows x 144] band-major, frames + 30 - 2 context rows per utterance
 * (context <= 64; every utterance needs at least one frame and one row). */
int snf_bottleneck_nn_input(int device_id, const float* d_logmel, const uint8_t* d_mask, const int32_t* d_voiced,
                            const int64_t* h_frame_offsets, int64_t n_utts, int32_t context, const float* d_basis,
                            float* d_x, void* stream);
/* The two stacked networks (reference bottleneck.py:477-501 _create_nn_extract_st_BN, bn_position 2) with
 * the input and bottleneck normalisations folded into the first layer of each: h_params[12] HOST array of
 * DEVICE pointers W1 b1 W2 b2 W3 b3 W5 b5 W6 b6 W7 b7 with W1[144 x w0], W2[w0 x w1], W3[w1 x 80],
 * W5[400 x w2], W6[w2 x w3], W7[w3 x 80], h_widths = {w0, w1, w2, w3}.  d_bn[rows x 80] receives the first
 * stage; rows t, t + 5, ..., t + 20 of one utterance are read from it as the 400 inputs of W5 (never written
 * out as a matrix); d_out[(rows - 20 n_utts) x 80].  Every utterance needs more than 20 rows. */
int snf_bottleneck_forward(int device_id, const float* d_x, const int64_t* h_row_offsets, int64_t n_utts,
                           const int32_t* h_widths, const float* const* h_params, float* d_bn, float* d_out,
                           void* stream);
/* bfloat16 matrix-core path for the layers that read sigmoid outputs in (0, 1).  The numerics contract: at
 * the input of such a layer every activation and every weight is rounded to bfloat16 (round to nearest, ties
 * to even; a NaN stays a NaN), the products are accumulated in float32 on the matrix cores
 * (v_mfma_f32_32x32x16_bf16), bias and activation are float32, the output is float32.  An element depends on
 * its own input row, its weight column and k only: not on m, nor on the row's place in the batch.
 *
 * Packed weights: the image of d_w[k x n] is Wt[n][kp] uint16 (bfloat16 bits), k-contiguous per output column,
 * kp = k rounded up to a multiple of 64 and zero beyond k; it must be 16-byte aligned.
 * snf_packed_weights_bf16_size returns its number of uint16 elements, n * kp (host only; 0 unless
 * 1 <= k, n <= 2^20). */
int64_t snf_packed_weights_bf16_size(int32_t k, int32_t n);
/* d_packed = the packed bfloat16 image of d_w[k x n] row-major float32 (prepared once per network: replaces the
 * reference's float64 `W` operands of bottleneck.py:485-500 for these layers). */
int snf_pack_weights_bf16(int device_id, const float* d_w, int32_t k, int32_t n, uint16_t* d_packed, void* stream);
/* d_y[m x n] = act(bf16(d_x[m x k]) bf16(W) + d_b[n]) with W given as its packed image; float32 d_x, d_b, d_y;
 * act as snf_dense_layer (reference bottleneck.py:461-462 and the `f(Y.dot(W) + b)` of :485-500). */
int snf_dense_layer_bf16(int device_id, const float* d_x, int64_t m, int32_t k, const uint16_t* d_packed,
                         const float* d_b, int32_t n, int32_t act, float* d_y, void* stream);
/* snf_bottleneck_forward (reference bottleneck.py:477-501) with W2, W3, W6 and W7 (h_params[2], [4], [8], [10])
 * given as packed bfloat16 images and evaluated as snf_dense_layer_bf16; W1 and W5 (unbounded inputs, folded
 * normalisations, the row gather) and every bias are float32 as there, and so are d_bn and d_out. */
int snf_bottleneck_forward_bf16(int device_id, const float* d_x, const int64_t* h_row_offsets, int64_t n_utts,
                                const int32_t* h_widths, const void* const* h_params, float* d_bn, float* d_out,
                                void* stream);
/* The whole extractor in one call (reference bottleneck.py:670-764 BottleneckProcessor.process from the VAD on:
 * _compute_vad, _add_dither, _fbank_htk, the voiced mean, _preprocess_nn_input, _create_nn_extract_st_BN): from
 * the resident 8 kHz int16 block d_wave to the float32 feature rows, what snf_bottleneck_vad, _fbank, _nn_input
 * and _forward (bf16 != 0: _forward_bf16, h_params[2], [4], [8], [10] packed images) give when called one after
 * the other on the same input - bit for bit, for any scratch_bytes, dither included (keyed per utterance and
 * sample as there).  Everything is enqueued on one stream and waited for once, at the end; nothing comes back to
 * the host in between (an utterance without voiced frames has a zero mean and gives defined rows).
 *
 * Utterance u gives frames + 10 - 2 context rows, written to d_out[. x 80] from row h_out_offsets[u] on;
 * h_out_offsets[n_utts + 1] (HOST, first >= 0) must leave every utterance at least its rows, and rows of d_out
 * that belong to no utterance are not touched.  h_status[n_utts] (HOST int32) receives one word per utterance
 * (bn_status_kernel, after the last layer): bit 0 = no voiced frame, bit 1 = some output value is not finite.
 *
 * Bounded scratch: the mask, the voiced counts, the VAD energies, the log-mel energies, the 144-column input, the
 * first stage and the two hidden buffers live in the calling thread's scratch, none is the caller's.  The batch
 * is walked in runs of whole consecutive utterances whose intermediates fit scratch_bytes (0 = the default,
 * 1 GiB): the two hidden buffers take a quarter of the bound each (never less than one tile of 128 rows), the
 * rest holds the runs' utterances at 105 bytes per frame, 896 per first-stage row, 8 per output row and 104 per
 * utterance; an utterance that is larger than that runs alone.  Every element depends on its own utterance or
 * row only, so the cuts do not show in the result.  d_tables, d_basis, h_widths, h_params as in the staged calls. */
int snf_bottleneck_extract(int device_id, const int16_t* d_wave, const int64_t* h_sample_offsets, int64_t n_utts,
                           const float* d_tables, float dither, uint64_t seed, int32_t context, const float* d_basis,
                           const int32_t* h_widths, const void* const* h_params, int32_t bf16, float* d_out,
                           const int64_t* h_out_offsets, int32_t* h_status, int64_t scratch_bytes, void* stream);
/* The runs snf_bottleneck_extract walks for this batch (host only; the loop over the utterances of reference
 * bottleneck.py:670 process, which takes one signal at a time): returns their number and, when h_run_starts
 * [n_utts + 1] is given, writes the first utterance of every run followed by n_utts; a negative error code for
 * arguments the extractor refuses. */
int64_t snf_bottleneck_extract_runs(const int64_t* h_sample_offsets, int64_t n_utts, int32_t context,
                                    const int32_t* h_widths, int64_t scratch_bytes, int64_t* h_run_starts);

/* ---- CREPE pitch (reference processor/pitch_crepe.py, CrepePitchProcessor) -------------------------
 * The CREPE network on 16 kHz int16 audio: frames of 1024 samples every `hop`, a signal of n samples gives
 * 1 + (n + (center ? 1024 : 0) - 1024) / hop of them (it must hold at least one).  Six blocks of convolution,
 * ReLU, batch normalisation (inference form, given as scale and shift per channel) and max-pool 2, then a
 * dense layer of 360 sigmoids; float32 on the FP32 matrix cores, every element summed in one fixed order
 * (fused multiply-add chains over 256 consecutive k ascending, their results added in ascending order), so an
 * utterance gives the same bits alone and in any batch.  Offsets tables are HOST int64
 * (non-decreasing, first 0), every other buffer is on the device.  `stream` NULL: the calling thread's own
 * stream; every call waits for its stream before returning.  Invalid arguments return SNF_E_INVALID before any
 * device work.
 */
/* One convolution block on channels-last activations d_x[frames x in_len x c_in]: `width` taps at `stride`
 * with `pad_left` zeros before position 0 (and zeros after the last), positions = output positions before the
 * pool (even when pooled): ceil(in_len / stride) for "same" padding, fewer are allowed, more are invalid; d_w[width * c_in x c_out] row-major (the Keras kernel), flags: 1 = ReLU then
 * * d_scale + d_shift, 2 = maximum over position pairs, 4 = logistic sigmoid.  d_y[frames x positions (/ 2)
 * x c_out]. */
int snf_crepe_conv(int device_id, const float* d_x, int64_t frames, int32_t in_len, int32_t c_in, int32_t width,
                   int32_t stride, int32_t pad_left, int32_t positions, const float* d_w, const float* d_b,
                   const float* d_scale, const float* d_shift, int32_t c_out, int32_t flags, float* d_y,
                   void* stream);
/* Ingest (zero padding of 512 samples on either side when `center`, per-frame mean and deviation from
 * float64 sums in a fixed order, deviation floored at 1e-8) and the whole network, one block of frames at a
 * time: h_filters[6] the channels of the six blocks, h_params[26] HOST array of DEVICE pointers, per block
 * kernel [K x C], bias, scale, shift, then the classifier's kernel [4 C6 x 360] and bias.
 * d_activation[total_frames x 360]. */
int snf_crepe_forward(int device_id, const int16_t* d_wave, const int64_t* h_sample_offsets, int64_t n_utts,
                      int32_t hop, int32_t center, const int32_t* h_filters, const float* const* h_params,
                      float* d_activation, void* stream);
/* bfloat16 matrix-core path for convolution blocks 2 to 6, which hold nine tenths of the arithmetic and read ReLU
 * and batch-normalisation outputs of order 1.  The numerics contract: at the input of such a block every
 * activation and every kernel weight is rounded to bfloat16 (to nearest, ties to even; a NaN stays a NaN), the
 * products are accumulated in float32 on the matrix cores (v_mfma_f32_32x32x16_bf16) in one fixed order (chains
 * of 1024 consecutive k ascending from zero, their results added in ascending order); bias, ReLU, scale and
 * shift, pool and sigmoid are float32 as in snf_crepe_conv.  Rounding is deterministic, so a producer that
 * stores bfloat16 and a consumer that rounds float32 in its loader see the same bits.  An element depends on
 * its frame's samples and on K only.  Element types of activations in memory: */
#define SNF_TYPE_F32 0
#define SNF_TYPE_BF16 1
/* snf_crepe_conv with the kernel given as its packed image (snf_pack_weights_bf16 of d_w[width * c_in x c_out],
 * 16-byte aligned), d_x of type x_type (16-byte aligned; float32 is rounded on the way in) and d_y of type y_type
 * (bfloat16: rounded on the way out).  The checks of snf_crepe_conv, and: c_in a multiple of 8, width * c_in at
 * most 2^20, both types known. */
int snf_crepe_conv_bf16(int device_id, const void* d_x, int32_t x_type, int64_t frames, int32_t in_len, int32_t c_in,
                        int32_t width, int32_t stride, int32_t pad_left, int32_t positions, const uint16_t* d_packed,
                        const float* d_b, const float* d_scale, const float* d_shift, int32_t c_out, int32_t flags,
                        void* d_y, int32_t y_type, void* stream);
/* snf_crepe_forward with the kernels of blocks 2 to 6 (h_params[4], [8], [12], [16], [20]) given as packed
 * bfloat16 images and evaluated as snf_crepe_conv_bf16; the outputs of blocks 2 to 5 are kept as bfloat16.  The
 * ingest, block 1 (unbounded normalised audio, C_in = 1), the classifier (which decides the argmax), every bias,
 * scale and shift and d_activation are float32 as there.  h_filters[0..4] must be multiples of 8. */
int snf_crepe_forward_bf16(int device_id, const int16_t* d_wave, const int64_t* h_sample_offsets, int64_t n_utts,
                           int32_t hop, int32_t center, const int32_t* h_filters, const void* const* h_params,
                           float* d_activation, void* stream);
/* Decoders over d_activation[total_frames x 360]: per frame the maximum (the confidence) and its first
 * index; `viterbi` != 0: the most likely path of the reference's 360-state model over those indices (float64
 * log domain, first index on ties); the weighted average of cents over bins [c - 4, c + 5) around the chosen
 * bin c, then 10 * 2^(cents / 1200) (0 where that is NaN).  d_tables float64, built by the host: log
 * transition band [360 x 23] (entry (j, d) = log A[j - 11 + d][j]) | log start | log emission of the state's own
 * symbol | of another symbol | cents of the 360 bins.  d_out[total_frames x 2] float64 (confidence, Hertz),
 * d_bins[2 x total_frames] int32 (first argmax, chosen bin). */
int snf_crepe_decode(int device_id, const float* d_activation, const int64_t* h_frame_offsets, int64_t n_utts,
                     int32_t viterbi, const double* d_tables, double* d_out, int32_t* d_bins, void* stream);
/* The tail between the decoder and the Kaldi post-processing (reference pitch_crepe.py:473-489, :572-606), float64
 * on the device; the host layer runs snf_crepe_rows before snf_crepe_voicing_convert.
 *
 * Row resampling by the Fourier method plus the reference's clamp: utterance u, the N rows
 * [h_in_offsets[u], h_in_offsets[u + 1]) of d_in[total_in x 2] (confidence, Hertz: the layout of snf_crepe_decode's
 * d_out), becomes the M rows [h_out_offsets[u], h_out_offsets[u + 1]) of d_out[total_out x 2].  N >= 1 and M >= 1
 * (anything else is SNF_E_INVALID), both at most 2^20.  Each column is scipy.signal.resample(x, M) of real input:
 * the input bits when M == N, otherwise with L = min(N, M), K = (L - 1) / 2 and theta(m, n) = 2 pi (m / M - n / N)
 *     y[m] = (1 / N) sum_n x[n] D(m, n),   D = 1 + 2 sum_{k = 1..K} cos(k theta) + c cos((L / 2) theta),
 * c = 0 for odd L, 2 for even L when M < N, 1 for even L when M > N.  D is evaluated in its closed form
 * sin((2K + 1) theta / 2) / sin(theta / 2) + c cos((L / 2) theta) (2K + 1 + c where theta is a multiple of 2 pi),
 * every angle a fraction of pi reduced in integers modulo 2 M N before sinpi / cospi see it; the N terms of a row
 * are added in ascending n, so an utterance gives the same bits alone and in any batch.  Then column 0 is
 * clamped: values below 1e-2 become 0, values above 1 become 1.  Buffers 8-byte aligned. */
int snf_crepe_rows(int device_id, const double* d_in, const int64_t* h_in_offsets, const int64_t* h_out_offsets,
                   int64_t n_utts, double* d_out, void* stream);
/* CrepePitchPostProcessor's conversion of d_rows[total x 2] float64 (POV, Hertz; the output of snf_crepe_rows) into
 * d_out[total x 2] float32 (NCCF, pitch), the input of the Kaldi post-processing; utterance u is the rows
 * [h_offsets[u], h_offsets[u + 1]).  Per utterance:
 *  1. the most likely voiced / unvoiced state per frame under a two-state model, float64 log domain, no fused
 *     multiply-add, first index on ties: log emission of state s = -0.5 * (h_model[0] + (pov - mean_s)^2 /
 *     variance), lattice[0] = log_start + emission, lattice[t][j] = max_i(lattice[t - 1][i] + logA[i][j]) +
 *     emission[t][j], states read back from the lattice.  h_model[11] (HOST float64): log(2 pi variance), mean_0,
 *     mean_1, variance, log_start, logA[0][0], logA[0][1], logA[1][0], logA[1][1], then f(0) and f(1) of step 3;
 *  2. the pitch of the unvoiced frames by linear interpolation between the nearest voiced neighbours
 *     (slope * (t - t_before) + pitch_before), the value of the first / last voiced frame outside them;
 *  3. NCCF from POV: 0 and 1 map to themselves, everything else by 64 halvings of [0, 1] over
 *     f(x) = 1 / (1 + exp(-(-5.2 + 5.4 exp(7.5 (x - 1)) + 4.8 x - 2 exp(-10 x) + 4.2 exp(20 (x - 1)))));
 *  4. d_status[u] int32: 0 fine, 1 no voiced frame, 2 a pitch value that is not > 0 after the interpolation,
 *     3 a POV other than 0 and 1 outside (f(0), f(1)); the lowest that applies.  A non-zero status leaves the
 *     utterance's output rows finite or zero (1 and 2: zero) and touches no other utterance.
 * An utterance with one row is valid; one without rows gets status 0 and writes nothing.  At most 2^30 rows per
 * utterance.  d_rows 8-byte, d_out and d_status 4-byte aligned. */
int snf_crepe_voicing_convert(int device_id, const double* d_rows, const int64_t* h_offsets, int64_t n_utts,
                              const double* h_model, float* d_out, int32_t* d_status, void* stream);

/* ---- framed one-hot labels (reference processor/onehot.py, FramedOneHotProcessor) -------------------
 * Per-frame labels of a batch of time alignments, one call for the whole batch.  Alignment a holds segments
 * [h_segment_offsets[a], h_segment_offsets[a + 1]) of h_offsets (float64 seconds, not decreasing) and
 * h_token_ids (in [0, h_num_tokens[a])); sample i of it sits at i / sample_rate + h_first_onsets[a] (float64,
 * one division then one addition) and carries the first token whose offset is greater than that time - the
 * last token when rounding leaves none (the reference's walk, alignment.py:321-337, ends in an IndexError
 * there).  Frame f covers samples [f * frame_shift, f * frame_shift + frame_length); h_num_frames[a] of them
 * must fit in the h_num_samples[a] samples.  A frame takes the token all its samples carry, or else the token
 * with the largest window weight: the float32 sum of the window coefficients of its samples, added in sample
 * order from zero, one sum per token; an exact tie goes to the token that appears first in the frame
 * (processor/onehot.py:235-254).  The window is snf_window_function's table of frame_length coefficients
 * (ones for a length of 1, and of 2 when the window has zeros at both ends, reference window.py:97-105).
 * d_winners[total_frames] int32: the token id of every frame; d_onehot: the dense rows, alignment a's
 * [h_num_frames[a] x h_num_tokens[a]] uint8 (0 / 1) from byte h_row_offsets[a] on - h_row_offsets[n + 1], every
 * entry a multiple of 16, entry a + 1 at least frames x tokens bytes after entry a; the bytes between the last
 * row and the next entry are zeroed.  d_onehot holds h_row_offsets[n] bytes and is 16-byte aligned.  kernel_ms
 * (may be NULL): device time of the kernels, from events.  Three launches whatever the batch. */
int snf_framed_onehot(int device_id, double sample_rate, int32_t frame_length, int32_t frame_shift,
                      int32_t window_type, float blackman_coeff, int64_t n_alignments,
                      const int64_t* h_segment_offsets, const double* h_first_onsets, const double* h_offsets,
                      const int32_t* h_token_ids, const int64_t* h_num_samples, const int64_t* h_num_frames,
                      const int32_t* h_num_tokens, const int64_t* h_row_offsets, int32_t* d_winners,
                      uint8_t* d_onehot, float* kernel_ms, void* stream);

/* ---- waveform resampling (Kaldi ResampleWaveform, resample.cc; torchaudio kaldi.resample_waveform) ----
 * An extension: the reference resamples on the host (audio.py:358-424, sox or scipy's Fourier method), one
 * utterance at a time.  This is Kaldi's LinearResample as ResampleWaveform configures it - a Hann-windowed sinc
 * with a cutoff of (float)(0.99 * 0.5 * min(rate_in, rate_out)) Hz and 6 zero crossings, the whole signal in one
 * call (flush) - for a batch that stays on the device.  Rates in [1, 2^22] Hz.
 */
/* Output samples of n_in input samples (LinearResample::GetNumOutputSamples with flush = true): the number of
 * multiples of 1 / rate_out in [0, n_in / rate_in).  Host only.  < 0: SNF_E_INVALID (rates or n_in out of
 * range). */
int64_t snf_resample_num_out(int32_t rate_in, int32_t rate_out, int64_t n_in);
/* Resamples utterance u, the samples [h_src_offsets[u], h_src_offsets[u + 1]) of d_src, into the
 * snf_resample_num_out samples of d_dst that start at h_dst_starts[u] (any order; the ranges must not overlap,
 * which is the caller's to ensure).  `kind` 0: int16 in and out, the float32 sum rounded to nearest (ties to even)
 * and clamped to [-32768, 32767]; 1: float32 in and out.  Every output is one fused multiply-add chain over its
 * taps ascending from zero (ResampleWaveform hands that sum to BLAS; see the arithmetic contract of the pitch
 * tracker), so an utterance gives the same bits alone and in any batch.  Offsets tables are HOST int64, buffers
 * are on the device.  Equal rates, and a rate pair whose phase table (rate_out / gcd rows) and staged input span
 * do not fit in the 64 KiB of LDS of a workgroup - 44 100 -> 16 001 Hz has 16 001 phases - are SNF_E_INVALID,
 * found before any device work; n_utts == 0 and empty utterances are fine.  The phase table is built once per
 * rate pair and kept on the device.  `stream` NULL: the calling thread's own stream; the call waits for its
 * stream before returning. */
int snf_linear_resample(int device_id, int32_t rate_in, int32_t rate_out, int32_t kind, const void* d_src,
                        const int64_t* h_src_offsets, int64_t n_utts, void* d_dst, const int64_t* h_dst_starts,
                        void* stream);

/* ---- padded batches from a ragged block (Kaldi splice-feats + subsample-feats, then padding) ----
 * An extension with no reference call behind it: the reference returns one numpy array per utterance and leaves
 * batching to its caller.  For a consumer on the same GPU, the float32 block [rows, dim] that a run call left in
 * HBM becomes the tensor [n_utts, t_max, dim (left + 1 + right)] that a model reads, in one pass.
 */
#define SNF_COLLATE_F32 0  /* a copy                                                         */
#define SNF_COLLATE_F16 1  /* IEEE binary16, to nearest (ties to even), overflow to infinity */
#define SNF_COLLATE_BF16 2 /* bfloat16, to nearest (ties to even); a NaN stays a NaN         */
/* Frames that subsample-feats keeps of `frames`: offset, offset + subsample, ...: 0 when frames <= offset, else
 * (frames - offset + subsample - 1) / subsample.  Host only.  < 0: SNF_E_INVALID (frames < 0, subsample < 1, or
 * offset outside [0, subsample)). */
int64_t snf_collate_num_out(int64_t frames, int32_t subsample, int32_t offset);
/* With T_u = h_frame_offsets[u + 1] - h_frame_offsets[u], n_u = snf_collate_num_out(T_u, subsample, offset),
 * j < t_max and k in [-left, right]:
 *   d_out[u][j][(k + left) dim + d] = cast(d_in[h_frame_offsets[u] + clamp(offset + j subsample + k, 0, T_u - 1)][d])
 *                                                                                                   if j <  n_u
 *   d_out[u][j][:]                  = cast(pad_value)                                               if j >= n_u
 *   d_lengths[u]                    = n_u   (int32)
 * The edge rule is the one of Kaldi's splice-feats (the first and last frame are repeated), the frame selection
 * the one of subsample-feats.  `out_type`: SNF_COLLATE_*.  d_in is float32 [h_frame_offsets[n_utts], dim]; d_out
 * holds n_utts * t_max * dim * (left + 1 + right) elements and is 16-byte aligned; every byte of d_out and of
 * d_lengths is written.  SNF_E_INVALID, before any device work: t_max < max n_u, subsample < 1, offset outside
 * [0, subsample), a negative context, dim < 1, an unknown out_type, offsets that decrease or start below 0, a
 * misaligned d_out, or an output of 2^31 elements or more (the kernel indexes it with 32 bits).  The offsets
 * table is a HOST array that the call uploads.  Everything is enqueued on `stream` and the call returns without
 * waiting for it (the table is kept in a slot of its own until the kernel has read it); `stream` NULL: the
 * calling thread's own stream, which the call waits for before returning. */
int snf_collate_padded(int device_id, const float* d_in, int32_t dim, const int64_t* h_frame_offsets,
                       int64_t n_utts, int32_t left, int32_t right, int32_t subsample, int32_t offset,
                       int32_t out_type, float pad_value, int64_t t_max, void* d_out, int32_t* d_lengths,
                       void* stream);

/* ---- DTW distances between feature items (the step after extraction in the reference's worked examples) ----
 * An extension with no reference call behind it: both examples of the reference extract features and then run
 * `abx-distance -n 1` of an external toolkit on the CPU (reference examples/features_abx/scripts/abx_score.sh:21),
 * one pair at a time.  Here the pairs of one call are computed on the device from rows that lie in HBM.  The
 * definition is this project's own (tests/dtw_f64.py); agreement with that toolkit is unpinned.
 */
#define SNF_DTW_COSINE 0       /* acos(clamp(cos(x_i, y_j), -1, 1)) / pi; 1 if one row is zero, 0 if both */
#define SNF_DTW_SQEUCLIDEAN 1  /* sum_k (x_ik - y_jk)^2, as max(|x_i|^2 + |y_j|^2 - 2 x_i . y_j, 0)      */
/* Symmetric KL divergence of rows of probabilities (posteriorgrams: snf_gmm_posteriors), natural logarithm:
 * 0.5 sum_k (x~_ik - y~_jk) (ln x~_ik - ln y~_jk) with x~ = max(x, SNF_DTW_SYMKL_FLOOR) element-wise (zero and
 * negative entries count as the floor; rows need not sum to 1), computed as
 * max(0.5 (h(x_i) + h(y_j) - x~_i . ln y~_j - ln x~_i . y~_j), 0), h(r) = sum_k r~_k ln r~_k (DESIGN 4.16,
 * tests/symkl_f64.py).  This project's own definition too: agreement with the ABX toolkit's KL is unpinned. */
#define SNF_DTW_SYMKL 2
#define SNF_DTW_SYMKL_FLOOR 0x1p-40f /* 2^-40, exact in float32 */
#define SNF_DTW_MAX_FRAMES 4096 /* rows of one item */
#define SNF_DTW_MAX_DIM 4096
/* Item t is the rows [h_item_first[t], h_item_first[t] + h_item_count[t]) of the float32 block d_rows [., dim];
 * pair p = (h_pairs[2 p], h_pairs[2 p + 1]) = (x, y) indexes the items.  With d[i][j] the frame distance of row i
 * of x and row j of y (`metric`: SNF_DTW_*):
 *   C[0][0] = d[0][0], L[0][0] = 1;  C[i][j] = d[i][j] + C[q], L[i][j] = L[q] + 1, q the predecessor of smallest
 *   C among (i-1, j-1), (i-1, j), (i, j-1) where they exist, ties to the first of that order;
 *   d_cost[p] = C[N-1][M-1] (float32 sums), d_len[p] = L[N-1][M-1]: the normalised distance is their quotient.
 * Results are in the caller's pair order and every element of d_cost and d_len is written; a pair's result does
 * not depend on the other pairs of the call.  Non-finite features give undefined values, nothing worse.
 * SNF_E_INVALID, before any device work: dim outside [1, SNF_DTW_MAX_DIM], n_items < 1, n_pairs < 0, an item
 * that starts below row 0 or has fewer than 1 or more than SNF_DTW_MAX_FRAMES rows, a pair index outside
 * [0, n_items), an unknown metric, a null or misaligned pointer.  n_pairs = 0 does nothing.  The tables are HOST
 * arrays that the call uploads.  Everything is enqueued on `stream` and the call returns without waiting for it
 * (the tables and the row norms are kept in a slot of their own until the kernels have run); `stream` NULL: the
 * calling thread's own stream, which the call waits for before returning.  SNF_DTW_SYMKL keeps, in that slot, the
 * logarithms of every row between the first and the last row of the items too: (dim + 1) floats per row; when
 * that cannot be allocated the call fails with SNF_E_HIP before any kernel is launched. */
int snf_dtw_pairs(int device_id, const float* d_rows, int32_t dim, const int64_t* h_item_first,
                  const int32_t* h_item_count, int64_t n_items, const int32_t* h_pairs, int64_t n_pairs,
                  int32_t metric, float* d_cost, int32_t* d_len, void* stream);

/* ---- Query-by-example search: subsequence DTW of queries in targets -------------------------------------------
 * An extension with no reference call behind it.  It replaces the host double loop that a user of the features
 * (MFCCs, or the posteriorgrams of snf_gmm_posteriors, which were introduced for this task) runs to find where a
 * short query - a word, a segment of an alignment - occurs inside whole utterances: the pairs of one call are
 * searched on the device from rows that lie in HBM.  The definition is this project's own (DESIGN 4.17,
 * tests/dtw_search_f64.py); agreement with any outside toolkit is unpinned.
 *
 * Items, pairs, `metric` and the frame distance d are those of snf_dtw_pairs; of pair p = (query, target) the query
 * x [N, dim] gives the rows of the lattice and the target y [M, dim] its columns:
 *   C[0][j] = d[0][j], L[0][j] = 1, B[0][j] = j for every j                                      (free start)
 *   i >= 1: C[i][j] = d[i][j] + C[q], L[i][j] = L[q] + 1, B[i][j] = B[q], q the predecessor of smallest C among
 *   (i-1, j-1), (i-1, j), (i, j-1) that exist, ties to the first of that order;
 *   score[j] = C[N-1][j] / (float)L[N-1][j] (the correctly rounded float32 division) if `normalized`, else
 *   C[N-1][j]; end = the smallest j of minimal score (a strict < over ascending j)                   (free end)
 *   d_end[p] = end, d_start[p] = B[N-1][end], d_cost[p] = C[N-1][end] (float32 sums), d_len[p] = L[N-1][end].
 * The dynamic programme minimises C; `normalized` (0 or 1) only ranks the ends, which is why it is an argument here
 * and not a division left to the caller.  Frames are counted from the target's first row.
 * Curves: h_curve_first NULL (then the three d_curve_* are NULL too), or a HOST array of n_pairs element offsets:
 * (C, L, B)[N-1][j] of pair p go to element h_curve_first[p] + j, j < M, of d_curve_cost, d_curve_len and
 * d_curve_start; no other element of them is touched.  Limits: SNF_DTW_MAX_FRAMES rows per item (query or target),
 * SNF_DTW_MAX_DIM.  Results are in the caller's pair order, every element of the four result arrays is written, and
 * a pair's result does not depend on the other pairs of the call.  Non-finite features give undefined values,
 * nothing worse.
 * SNF_E_INVALID, before any device work: what snf_dtw_pairs refuses, `normalized` not 0 or 1, curve pointers
 * partly set, a curve stretch below element 0, ending beyond element 2^31 or overlapping another pair's.
 * n_pairs = 0 does nothing.  Streams, the slot of the tables and the symkl log block: as snf_dtw_pairs. */
int snf_dtw_search(int device_id, const float* d_rows, int32_t dim, const int64_t* h_item_first,
                   const int32_t* h_item_count, int64_t n_items, const int32_t* h_pairs /* (query, target) */,
                   int64_t n_pairs, int32_t metric, int32_t normalized, float* d_cost, int32_t* d_len,
                   int32_t* d_start, int32_t* d_end, const int64_t* h_curve_first, float* d_curve_cost,
                   int32_t* d_curve_len, int32_t* d_curve_start, void* stream);

/* ---- Search: several non-overlapping detections per pair, and the best few per query ---------------------------
 * Extensions with no reference call behind them, on top of snf_dtw_search: every place a query occurs in a target,
 * not only the best one, picked on the device from the ends of the same lattice, so that a search over a corpus
 * downloads detections and not 12 bytes per target frame.  The definition is this project's own (DESIGN 4.18,
 * tests/dtw_detect_f64.py); agreement with any outside toolkit is unpinned.
 *
 * snf_dtw_detect: the arguments, the lattice, score[j] and the curves of snf_dtw_search.  Of pair p every end j is
 * alive at first, and up to K = `max_detections` rounds follow:
 *   e = the smallest alive j of minimal score (a strict < over ascending j); stop if not score[e] <= max_score
 *   (a float32 comparison; +inf: no threshold); detection r = d_count[p] so far is d_end[p K + r] = e,
 *   d_start[p K + r] = B[N-1][e], d_cost[p K + r] = C[N-1][e], d_len[p K + r] = L[N-1][e];
 *   every end j' whose path interval [B[N-1][j'], j'] shares a frame with [B[N-1][e], e] dies (e among them).
 * It stops after K detections or when no end is alive.  d_count[p] detections come in ascending score, their
 * intervals are pairwise disjoint, and rank 0 is what snf_dtw_search returns.  Every element of d_count [P] and of
 * the four arrays [P K] is written: a slot at or beyond d_count[p] holds cost = +inf, len = 0, start = end = -1.
 * Results are in the caller's pair order and a pair's result does not depend on the other pairs of the call.
 * Non-finite features give undefined values, nothing worse.
 * SNF_E_INVALID, before any device work: what snf_dtw_search refuses, max_detections outside
 * [1, SNF_DTW_MAX_DETECTIONS], a NaN max_score.  n_pairs = 0 does nothing.  Streams and slots: as snf_dtw_pairs. */
#define SNF_DTW_MAX_DETECTIONS 64
int snf_dtw_detect(int device_id, const float* d_rows, int32_t dim, const int64_t* h_item_first,
                   const int32_t* h_item_count, int64_t n_items, const int32_t* h_pairs /* (query, target) */,
                   int64_t n_pairs, int32_t metric, int32_t normalized, int32_t max_detections, float max_score,
                   int32_t* d_count, float* d_cost, int32_t* d_len, int32_t* d_start, int32_t* d_end,
                   const int64_t* h_curve_first, float* d_curve_cost, int32_t* d_curve_len, int32_t* d_curve_start,
                   void* stream);
/* snf_dtw_topk: per query the T = `top_k` best detections of what snf_dtw_detect left on the device (d_count [P],
 * d_cost, d_len, d_start, d_end [P K], K = `max_detections` of that call; they are read where they lie).  The HOST
 * tables say which pairs belong to which query: query q owns h_group_pairs[h_group_first[q] ..
 * h_group_first[q + 1]), pair indices in [0, n_pairs) (a stable grouping of the caller's pair order;
 * h_group_first [Q + 1] starts at 0 and does not descend).  The candidates of a query are the first d_count[p]
 * slots of its pairs, never a sentinel slot.  They are ordered by the key (score, pair index, rank), the score being
 * d_cost / (float)d_len (the correctly rounded float32 division) if `normalized`, else d_cost; place i < d_top_count[q]
 * of query q is at q T + i of d_top_pair, d_top_rank, d_top_cost, d_top_len, d_top_start, d_top_end.  Every element
 * of d_top_count [Q] and of the six arrays [Q T] is written: a place at or beyond the count holds pair = rank = -1,
 * cost = +inf, len = 0, start = end = -1.  A pair listed twice is a candidate once (keys are compared, not slots).
 * SNF_E_INVALID, before any device work: max_detections outside [1, SNF_DTW_MAX_DETECTIONS], top_k outside
 * [1, SNF_DTW_MAX_TOPK], `normalized` not 0 or 1, negative sizes, group boundaries that do not start at 0 or descend,
 * a grouped pair outside [0, n_pairs), a null or misaligned pointer.  n_queries = 0 does nothing.  One wavefront
 * works per query, T passes over its candidates: meant for T up to the limit and pairs per query in the tens of
 * thousands.  Streams and slots: as snf_dtw_pairs. */
#define SNF_DTW_MAX_TOPK 1024
int snf_dtw_topk(int device_id, const int32_t* d_count, const float* d_cost, const int32_t* d_len,
                 const int32_t* d_start, const int32_t* d_end, int64_t n_pairs, int32_t max_detections,
                 int32_t normalized, const int32_t* h_group_pairs, const int64_t* h_group_first, int64_t n_queries,
                 int32_t top_k, int32_t* d_top_count, int32_t* d_top_pair, int32_t* d_top_rank, float* d_top_cost,
                 int32_t* d_top_len, int32_t* d_top_start, int32_t* d_top_end, void* stream);

/* ---- Warping paths: the alignment itself, of DTW pairs and of search hits ----------------------------------------
 * An extension with no reference call behind it, on top of snf_dtw_pairs and snf_dtw_detect: the frame-to-frame map
 * that their cost, length, start and end summarise.  The definition is this project's own (DESIGN 4.19,
 * tests/dtw_align_f64.py); agreement with any outside toolkit is unpinned.
 *
 * Items, pairs, `metric`, streams and slots are those of snf_dtw_pairs.  Every cell of the lattice keeps its decision
 * K: 0 for (i-1, j-1), 1 for (i-1, j), 2 for (i, j-1) - the predecessor that the lattice takes anyway, smallest C,
 * ties to the first of that order - and 3 for an origin.  The path of an end (N-1, e) follows K back to an origin and
 * is listed forward as frames (i, j), counted from the first row of each item; it has exactly L[N-1][e] cells.
 * `mode`:
 *   SNF_DTW_ALIGN_GLOBAL: the lattice of snf_dtw_pairs, d_cost [P] and d_len [P] as it writes them; one path per
 *   pair, from (0, 0) to (N-1, M-1).  K = 1 slot per pair; normalized, max_detections, max_score, d_count, d_start
 *   and d_end are not looked at.
 *   SNF_DTW_ALIGN_SUBSEQUENCE: the lattice and the detections of snf_dtw_detect with K = `max_detections` slots per
 *   pair, d_count [P] and d_cost, d_len, d_start, d_end [P K] as it writes them (no curves; K = 1 with max_score
 *   +inf is the match of snf_dtw_search); one path per detection, from (0, d_start) to (N-1, d_end).
 * Cost, length, start and end are bit for bit what the sibling calls return for the same tables.
 * Paths: h_path_first is a HOST array of P K element offsets.  Slot p K + r owns the N + M - 1 elements from
 * h_path_first[p K + r] of d_path_x and d_path_y (the longest path there can be); cell c < L of its path goes to
 * element h_path_first[p K + r] + c: the query's (x's) frame to d_path_x, the target's (y's) to d_path_y.  Exactly
 * the first L elements of a slot with a detection are written, nothing else in the two arrays is touched.
 * Scratch: the lattice leaves 16 bytes per step of every strip of 64 rows, 16 (N + ceil(N / 64) (M - 1)) bytes a pair
 * (29 KB for 298 x 298, 4.3 MB for 4096 x 4096), in a buffer of at most `scratch_bytes` (0: 1 GiB) that the slot
 * keeps; the pairs are worked in as many runs (a lattice launch per class and a traceback launch each, on the
 * stream) as that takes.  Non-finite features give undefined values and paths, nothing worse.
 * SNF_E_INVALID, before any device work: what snf_dtw_pairs (subsequence: snf_dtw_detect) refuses, an unknown mode,
 * a null path table or misaligned path array, a path stretch below element 0, ending beyond element 2^31 or
 * overlapping another's, a negative scratch_bytes or one below the records of the largest pair of the call.
 * n_pairs = 0 does nothing. */
#define SNF_DTW_ALIGN_GLOBAL 0
#define SNF_DTW_ALIGN_SUBSEQUENCE 1
int snf_dtw_align(int device_id, const float* d_rows, int32_t dim, const int64_t* h_item_first,
                  const int32_t* h_item_count, int64_t n_items, const int32_t* h_pairs, int64_t n_pairs,
                  int32_t metric, int32_t mode, int32_t normalized, int32_t max_detections, float max_score,
                  int32_t* d_count, float* d_cost, int32_t* d_len, int32_t* d_start, int32_t* d_end,
                  const int64_t* h_path_first, int32_t* d_path_x, int32_t* d_path_y, int64_t scratch_bytes,
                  void* stream);

/* ---- ABX triplet counts over a table of distances (the two steps after the distances in the reference's examples) --
 * An extension with no reference call behind it: the reference's examples run `abx-score` and `abx-analyze` of an
 * external toolkit on the CPU (reference examples/features_abx/scripts/abx_score.sh:22-23), one triplet at a time,
 * and average the scores of the cells (examples/features_abx/scripts/collapse_abx.py:35-42).  Here the triplets of
 * all the cells of a call are counted on the device from distances that lie in HBM, as snf_dtw_pairs leaves them;
 * the scores and their collapse are host arithmetic on the counts (shennong_amd/abx.py).  The definitions are this
 * project's own (tests/abx_np.py); agreement with that toolkit is unpinned.
 *
 * Cell c is the record h_cells[8 c ..] = {offA, offB, stride, nA, nB, nX, same, 0}.  With v[i] = d_cost[i] /
 * (float)d_len[i] (the correctly rounded float32 division: the value of dtw_distances(normalized=True) bit for
 * bit), or v[i] = d_cost[i] when d_len is NULL, its triplets are (a, b, x) in [0, nA) x [0, nB) x [0, nX), without
 * those with a == x when same != 0 (the A-list and the X-list are then the same items), and
 *   dAX = v[offA + x stride + a], dBX = v[offB + x stride + b]
 *   d_counts[3 c]     = less  = #{dAX < dBX}
 *   d_counts[3 c + 1] = equal = #{dAX == dBX}
 *   d_counts[3 c + 2] = bad   = #{dAX or dBX not finite}; a bad triplet is in neither of the other two counts.
 * The counts are exact integers and do not depend on how the device splits the work; every element of d_counts is
 * written; non-finite distances change counts and nothing else.  SNF_E_INVALID, before any device work: a null or
 * misaligned pointer, a negative size, nA, nB or nX below 1 (or 2^31 and above), a negative offset or stride, a
 * cell whose last element reaches outside [0, n_dist), same != 0 with nA != nX, a nonzero last word, a cell of
 * more than 2^62 triplets.  n_cells = 0 does nothing.  The cell table is a HOST array that the call uploads.
 * Everything is enqueued on `stream` and the call returns without waiting for it (the tables are kept in a slot of
 * their own until the kernels have run); `stream` NULL: the calling thread's own stream, which the call waits for
 * before returning. */
int snf_abx_cells(int device_id, const float* d_cost, const int32_t* d_len, int64_t n_dist, const int64_t* h_cells,
                  int64_t n_cells, uint64_t* d_counts, void* stream);

/* ---- device memory + timing (so hosts without torch can keep data resident in HBM) ---------- */
int snf_malloc(void** dptr, uint64_t bytes);
int snf_free(void* dptr);
/* Free and total bytes of HBM on the calling thread's current device (hipMemGetInfo): the streamed pipeline
 * sizes its batches from it (shennong_amd/pipeline.py extract_features_streamed) and bench.py reports the peak
 * use of BASELINE config 5.  No counterpart in the reference (CPU only). */
int snf_mem_info(uint64_t* free_bytes, uint64_t* total_bytes);
/* A host that pools freed device buffers (shennong_amd/_backend.py DEVICE_POOL) registers a callback that
 * releases them: an allocation of the library's own scratch that fails with out-of-memory calls it and tries
 * once more (NULL removes the hook).  No counterpart in the reference (CPU only). */
typedef void (*snf_oom_hook)(void);
int snf_set_oom_hook(snf_oom_hook hook);
int snf_memcpy_h2d(void* dst, const void* src, uint64_t bytes);
int snf_memcpy_d2h(void* dst, const void* src, uint64_t bytes);
int snf_memset(void* dst, int value, uint64_t bytes);  /* complete when it returns (the plans use their own streams) */
/* Streams and stream-ordered copies for callers that overlap the transfers of one batch with the
   kernels of another (the *_device entry points take the stream; page-locked host memory from
   snf_host_malloc is required for the copies to be asynchronous). */
int snf_stream_create(void** stream);
int snf_stream_destroy(void* stream);
int snf_stream_synchronize(void* stream);
/* 0 = everything enqueued on `stream` has completed, 1 = not yet (hipStreamQuery; never waits), < 0 = error.
   A host that must not wait for ever on work that depends on OTHER processes - the exchange steps below: a
   peer that died or stalled never completes them - polls this against a deadline instead of synchronising
   (bench.py's watchdog).  No counterpart in the reference (its pool is one process). */
int snf_stream_query(void* stream);
int snf_memcpy_h2d_async(void* dst, const void* src, uint64_t bytes, void* stream);
int snf_memcpy_d2h_async(void* dst, const void* src, uint64_t bytes, void* stream);
/* Timing marks on a caller's stream (hipEvent_t behind a plain pointer): a caller that enqueues several
   *_device calls on its own stream without waiting for each - the way a pipeline uses the path, and what
   bench.py times - brackets every call with two marks and reads the elapsed device time of each pair after
   ONE synchronisation (snf_plan_last_kernel_ms is for calls on the plan's own stream and waits for the call).
   snf_event_elapsed_ms waits for `stop`.  Marks belong to the calling thread's current device (the one of the
   stream they are recorded on). */
int snf_event_create(void** event);
int snf_event_destroy(void* event);
int snf_event_record(void* event, void* stream);
/* The host waits until `event` has happened (hipEventSynchronize): ONE copy of a stream that already carries the
   next one - the streamed pipeline sends the audio of batch k + 1 ahead on the stream that carried batch k's
   (shennong_amd/pipeline.py _Prefetch). */
int snf_event_synchronize(void* event);
/* Work enqueued on `stream` after this call starts only when `event` (recorded on another stream) has happened:
   the upload stream of a large batch runs ahead of the stream that launches the kernels and downloads the rows
   (shennong_amd/_backend.py Plan._run_large).  hipStreamWaitEvent; the host does not wait. */
int snf_stream_wait_event(void* stream, void* event);
int snf_event_elapsed_ms(void* start, void* stop, float* ms);
/* Page-locked host staging memory for the host-pointer entry points (snf_plan_run_batch, ...): a
   batch assembled in it (the reference hands over one numpy array per utterance, processor/base.py:428)
   crosses the link at full rate and its pages are faulted in once, not once per call.  Plain host
   memory as far as the caller is concerned. */
int snf_host_malloc(void** hptr, uint64_t bytes);
int snf_host_free(void* hptr);
/* ---- WAV ingest (host only) ---------------------------------------------------------
   The reference decodes one file per job in Python (shennong/audio.py:243-286: scipy, sox for other containers)
   and forces the signal to int16 before Kaldi sees it (processor/base.py:428).  These read RIFF / WAVE files
   natively: snf_wav_scan is `Audio.scan` (channels, sample rate, samples per channel, bits, format tag: 1 = PCM,
   3 = IEEE float); snf_wav_read_pcm16 copies samples [first_sample[i], first_sample[i] + n_samples[i]) of file i
   to dst + dst_offsets[i] for n_files files on `threads` threads - straight into the (page-locked) block a batch
   is uploaded from.  status[i]: 0 = read; 1 = not 16-bit mono PCM (the caller's general reader takes that file);
   2 = I/O error; 3 = the file holds fewer samples than asked for.  The call itself fails only for bad arguments. */
int snf_wav_scan(const char* path, int32_t* channels, int32_t* sample_rate, int64_t* nsamples, int32_t* bits,
                 int32_t* format_tag);
int snf_wav_read_pcm16(const char* const* paths, int64_t n_files, const int64_t* first_sample,
                       const int64_t* n_samples, int16_t* dst, const int64_t* dst_offsets, int32_t threads,
                       int32_t* status);

/* ---- multi-GPU exchange steps (RCCL over xGMI; one process per GPU) --------------------------------
   The features path shards by utterance and needs no data-path collective; what crosses GPUs is (a)
   the final gather of the per-rank feature blocks to a root - the counterpart of the reference's
   thread pool returning every utterance's matrix to one dict (processor/base.py:104-107) - and (b) the
   sum of the by-speaker CMVN statistics (postprocessor/cmvn.py:145-164).  RCCL is loaded on the first
   call.  Bootstrap: rank 0 calls snf_comm_unique_id and hands the 128 bytes to the other ranks by any
   side channel (a socket, a file, MPI ...), then every rank calls snf_comm_init. */
#define SNF_COMM_ID_BYTES 128
typedef struct snf_comm snf_comm; /* opaque */
int snf_comm_unique_id(void* id128);
int snf_comm_init(const void* id128, int32_t world_size, int32_t rank, int32_t device_id, snf_comm** out);
int snf_comm_rank(const snf_comm* comm);
int snf_comm_world_size(const snf_comm* comm);
int snf_comm_destroy(snf_comm* comm);
/* Variable-length gather of float blocks to `root`, device pointers in and out: rank r contributes
   `send_count` floats; on the root they land in `d_recv` in rank order (`recv_counts[world]`, host, root
   only).  Point-to-point ncclSend / ncclRecv in one group: every peer uses its own xGMI link to the root.
   `stream` NULL: the communicator's stream, synchronised before returning. */
int snf_comm_gatherv(snf_comm* comm, const float* d_send, int64_t send_count, float* d_recv,
                     const int64_t* recv_counts, int32_t root, void* stream);
/* In-place all-reduce of float64 on the device; op 0 = sum, 1 = max. */
int snf_comm_allreduce_f64(snf_comm* comm, double* d_buf, int64_t count, int32_t op, void* stream);

/* Test aid: fills the LDS of every CU of the current device with `pattern` (e.g. 0xFFFFFFFF, a NaN).
   LDS is not cleared between workgroups, so a kernel that reads a word it did not write sees whatever
   the previous kernel left there; the parity tests poison it before they compare against the oracle. */
int snf_debug_fill_lds(uint32_t pattern);
/* Test aid: device pointers of the intermediates the last run of a pitch plan left in its scratch
   (resampled signal [total_down], NCCF at the lag of every state [frames, states], NCCF without
   ballast at the integer lags [frames, lags], Viterbi states [frames]); the parity tests compare
   them stage by stage with the oracle's.  Valid until the next call on the plan. */
int snf_debug_pitch_scratch(snf_plan* plan, void** down, void** nccf_res, void** pov_nccf,
                            void** states);
/* Test aid: the tail of a PLP plan on rows the caller chooses, without the mel front end.  Host arrays:
   `mel` float32 [total_frames, num_bins] linear mel energies, `energy` float64 [total_frames] linear frame
   energies, `frame_offsets` int64 [n_utts + 1] (starting at 0), `out` float32 [total_frames, num_ceps].  Runs
   what the product path runs behind the front end - the RASTA filter if the plan's options ask for it, then
   the PLP tail with the plan's own parameters - on buffers of its own, with the unwarped tables (warp id 0)
   for every utterance, and records the kernels in the plan's timing slots (snf_plan_kernel_name).
   `mel_out` (may be NULL): receives the rows the tail read, float32 [total_frames, num_bins] - the RASTA
   filter's output on a RASTA plan, the input otherwise.  SNF_E_INVALID for a plan of another kind. */
int snf_debug_plp_tail(snf_plan* plan, const float* mel, const double* energy,
                       const int64_t* frame_offsets, int64_t n_utts, float* out, float* mel_out);
/* Test aid: 1 when a batch with these host offset tables (`sample_offsets`, `frame_offsets`: int64
   [n_utts + 1]) runs the 25 ms form of fbank512b_kernel with sample offsets relative to the first frame of
   every frame set (32 bits per lane), 0 when it keeps 64-bit addresses: three consecutive utterances that
   span 2^30 samples or more, or SNF_FBANK512B_ADDR64=1 in the environment.  Negative: an error code. */
int snf_debug_fbank512b_rel32(const int64_t* sample_offsets, const int64_t* frame_offsets, int64_t n_utts);
/* Test aid: the frame sets [*lo, *hi) that workgroup `block` of `blocks` of fbank512b_kernel deals to its waves
   when the batch holds `n_sets` sets of four frames.  The shares tile [0, n_sets) in order and differ by at
   most one set.  Returns the number of workgroups the launcher starts for `n_sets` (min(256, ceil(n_sets /
   16))), or a negative error code. */
int snf_debug_fbank512b_share(int64_t n_sets, int64_t blocks, int64_t block, int64_t* lo, int64_t* hi);
/* Duration in milliseconds of the kernels launched by the last run call on this plan, measured
   with HIP events on the stream the kernels were launched on.  `which` selects a kernel slot:
   0 = whole call, 1.. = per-kernel; returns <0 if the slot was not recorded. */
float snf_plan_last_kernel_ms(const snf_plan* plan, int which);
/* Name of the kernel recorded in slot `which` (NULL if none). */
const char* snf_plan_kernel_name(const snf_plan* plan, int which);

#ifdef __cplusplus
}
#endif
#endif /* SHENNONG_AMD_H_ */
