// C ABI of libshennong_hip.so (include/shennong_amd.h): post-processor plans (delta, pitch post-processing,
// VAD, sliding CMVN), CMVN statistics, and the plan-less column helpers.
#include "plan.h"

using namespace snf;

extern "C" {

int32_t snf_post_ndims(const snf_plan* plan, int32_t in_cols) {
  if (!plan) return -1;
  if (plan->kind == SNF_KIND_DELTA) return in_cols * (plan->o.delta_order + 1);
  if (plan->kind == SNF_KIND_PITCH_POST) return plan->ndims;
  if (plan->kind == SNF_KIND_VAD) return 1;
  if (plan->kind == SNF_KIND_SLIDING_CMVN) return in_cols;
  return -1;
}

int snf_post_run_batch_device(snf_plan* plan, const float* d_in, int32_t in_cols,
                              const int64_t* frame_offsets, int64_t n_utts, float* d_out,
                              void* stream) {
  const uint64_t named_call = take_noise_call();
  if (!plan) return set_error(SNF_E_INVALID, "null plan");
  if (n_utts <= 0) return n_utts == 0 ? SNF_OK : set_error(SNF_E_INVALID, "n_utts < 0");
  if (!frame_offsets) return set_error(SNF_E_INVALID, "null offsets table");
  if (frame_offsets[0] != 0) return set_error(SNF_E_INVALID, "offsets tables must start at 0");
  for (int64_t u = 0; u < n_utts; ++u)
    if (frame_offsets[u + 1] < frame_offsets[u])
      return set_error(SNF_E_INVALID, "offsets tables must be non-decreasing");
  std::lock_guard<std::mutex> lock(plan->mu);
  int rc = guard_device(plan);
  if (rc) return rc;
  const int64_t total_frames = frame_offsets[n_utts];
  if (total_frames == 0) return SNF_OK;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : plan->stream;
  const bool own_stream = (stream == nullptr);
  // the offsets table (and what the delta kernel derives from it) stays on the device between calls
  // with the same table: a pipeline runs the same batch layout call after call
  // (tile_cols is set by delta plans alone: every other kind uploads its table with every call)
  const bool same_table = plan->oc.tile_cols == in_cols && plan->oc.same(nullptr, frame_offsets, n_utts);
  if (!same_table) {
    if ((rc = plan->oc.store(nullptr, frame_offsets, n_utts, s))) return rc;
    SNF_HIP_CHECK(hipStreamSynchronize(s));
  }
  if (own_stream) begin_timing(plan);
  if (plan->kind == SNF_KIND_DELTA) {
    if (in_cols <= 0) return set_error(SNF_E_INVALID, "in_cols must be positive");
    if ((rc = plan->post_s.tile.ensure(4 * sizeof(int64_t) * static_cast<size_t>(total_frames / 32 + 2)))) return rc;
    const char* launched = nullptr;
    if ((rc = launch_deltas(plan->dp, d_in, in_cols, plan->oc.foff.as<int64_t>(), n_utts,
                            total_frames, d_out, plan->post_s.tile.as<int64_t>(), !same_table, s,
                            &launched)))
      return rc;
    // (the tile records are complete before a later call on another stream may use them)
    if (!same_table && !own_stream) SNF_HIP_CHECK(hipStreamSynchronize(s));
    plan->oc.tile_cols = in_cols;
    if (own_stream && launched) mark_kernel(plan, launched);
  } else if (plan->kind == SNF_KIND_PITCH_POST) {
    if (in_cols != 2)
      return set_error(SNF_E_INVALID, "data shape must be (_, 2), but it is (_, " +
                                          std::to_string(in_cols) + ")");
    if (plan->ppost.o.delta_pitch_noise_stddev != 0.0f)
      plan->ppost.seed = plan->o.seed + 0x9E3779B97F4A7C15ull * (named_call ? named_call : ++plan->noise_calls);
    const char* launched = nullptr;
    if ((rc = launch_pitch_post(plan->ppost, d_in, plan->oc.foff.as<int64_t>(), n_utts,
                                total_frames, d_out, s, &launched)))
      return rc;
    if (own_stream && launched) mark_kernel(plan, launched);
  } else if (plan->kind == SNF_KIND_VAD) {
    if (in_cols <= 0) return set_error(SNF_E_INVALID, "in_cols must be positive");
    if ((rc = plan->post_s.stats.ensure(sizeof(float) * static_cast<size_t>(n_utts)))) return rc;
    if ((rc = launch_vad(plan->o.vad, d_in, in_cols, plan->oc.foff.as<int64_t>(), n_utts,
                         total_frames, plan->post_s.stats.as<float>(), d_out, s)))
      return rc;
    if (own_stream) mark_kernel(plan, "vad_kernel");
  } else if (plan->kind == SNF_KIND_SLIDING_CMVN) {
    if (in_cols <= 0) return set_error(SNF_E_INVALID, "in_cols must be positive");
    if ((rc = launch_sliding_cmvn(plan->o.sliding_cmvn, d_in, in_cols, plan->oc.foff.as<int64_t>(),
                                  n_utts, d_out, s)))
      return rc;
    if (own_stream) mark_kernel(plan, "sliding_cmvn_kernel");
  } else {
    return set_error(SNF_E_INVALID, "plan kind is not a post-processor");
  }
  if (own_stream) SNF_HIP_CHECK(hipStreamSynchronize(s));
  return SNF_OK;
}

int snf_post_run_batch(snf_plan* plan, const float* in, int32_t in_cols,
                       const int64_t* frame_offsets, int64_t n_utts, float* out) {
  if (!plan) return set_error(SNF_E_INVALID, "null plan");
  std::lock_guard<std::mutex> host_lock(plan->host_mu);
  if (n_utts <= 0) return n_utts == 0 ? SNF_OK : set_error(SNF_E_INVALID, "n_utts < 0");
  if (!frame_offsets) return set_error(SNF_E_INVALID, "null offsets table");
  const int64_t total_frames = frame_offsets[n_utts];
  const int32_t out_cols = snf_post_ndims(plan, in_cols);
  if (out_cols <= 0 || in_cols <= 0) return set_error(SNF_E_INVALID, "bad column count");
  if (total_frames == 0) return SNF_OK;
  float *d_in, *d_out;
  {
    std::lock_guard<std::mutex> lock(plan->mu);
    int rc = guard_device(plan);
    if (rc) return rc;
    if ((rc = plan->stage.in.ensure(static_cast<size_t>(total_frames) * in_cols, &d_in))) return rc;
    if ((rc = plan->stage.out.ensure(static_cast<size_t>(total_frames) * out_cols, &d_out))) return rc;
    SNF_HIP_CHECK(hipMemcpyAsync(d_in, in, sizeof(float) * total_frames * in_cols, hipMemcpyHostToDevice,
                                 plan->stream));
  }
  int rc = snf_post_run_batch_device(plan, d_in, in_cols, frame_offsets, n_utts, d_out, nullptr);
  return rc ? rc : download(plan, out, d_out, sizeof(float) * total_frames * out_cols);
}

namespace {
int cmvn_check(const snf_plan* plan, int32_t cols, const int64_t* frame_offsets, int64_t n_utts,
               const int32_t* group, int32_t n_groups) {
  if (!plan) return set_error(SNF_E_INVALID, "null plan");
  if (plan->kind != SNF_KIND_CMVN) return set_error(SNF_E_INVALID, "plan kind is not CMVN");
  if (n_utts < 0) return set_error(SNF_E_INVALID, "n_utts < 0");
  if (cols <= 0) return set_error(SNF_E_INVALID, "dimension must be a strictly positive integer");
  if (n_groups <= 0) return set_error(SNF_E_INVALID, "n_groups must be positive");
  if (n_utts > 0 && !frame_offsets) return set_error(SNF_E_INVALID, "null offsets table");
  if (n_utts > 0 && frame_offsets[0] != 0) return set_error(SNF_E_INVALID, "offsets tables must start at 0");
  for (int64_t u = 0; u < n_utts; ++u) {
    if (frame_offsets[u + 1] < frame_offsets[u])
      return set_error(SNF_E_INVALID, "offsets tables must be non-decreasing");
    const int32_t g = group ? group[u] : 0;
    if (g < 0 || g >= n_groups) return set_error(SNF_E_INVALID, "group index out of range");
  }
  return SNF_OK;
}
}  // namespace

int snf_cmvn_accumulate_device(snf_plan* plan, const float* d_in, int32_t cols,
                               const int64_t* frame_offsets, int64_t n_utts, const float* d_weights,
                               const int32_t* group, int32_t n_groups, double* stats) {
  int rc = cmvn_check(plan, cols, frame_offsets, n_utts, group, n_groups);
  if (rc) return rc;
  if (n_utts == 0) return SNF_OK;
  if (!stats) return set_error(SNF_E_INVALID, "null stats");
  std::lock_guard<std::mutex> lock(plan->mu);
  if ((rc = guard_device(plan))) return rc;
  const int64_t total_frames = frame_offsets[n_utts];
  if (total_frames == 0) return SNF_OK;
  if (!d_in) return set_error(SNF_E_INVALID, "null input");
  hipStream_t s = plan->stream;
  const size_t blk = 2 * static_cast<size_t>(cols + 1);
  if ((rc = plan->post_s.stats.ensure(sizeof(double) * blk * static_cast<size_t>(n_utts)))) return rc;
  std::vector<int64_t> foff(frame_offsets, frame_offsets + n_utts + 1);
  if ((rc = plan->oc.foff.upload(foff, s))) return rc;
  begin_timing(plan);
  const char* launched = nullptr;
  if ((rc = launch_cmvn_stats(d_in, cols, plan->oc.foff.as<int64_t>(), d_weights, n_utts,
                              plan->post_s.stats.as<double>(), s, &launched)))
    return rc;
  if (launched) mark_kernel(plan, launched);
  std::vector<double> per_utt(blk * static_cast<size_t>(n_utts));
  SNF_HIP_CHECK(hipMemcpyAsync(per_utt.data(), plan->post_s.stats.p, sizeof(double) * per_utt.size(),
                               hipMemcpyDeviceToHost, s));
  SNF_HIP_CHECK(hipStreamSynchronize(s));
  // the per-speaker sum runs over a handful of [2, cols+1] blocks: host, in utterance order
  for (int64_t u = 0; u < n_utts; ++u) {
    double* dst = stats + blk * static_cast<size_t>(group ? group[u] : 0);
    const double* src = per_utt.data() + blk * static_cast<size_t>(u);
    for (size_t i = 0; i < blk; ++i) dst[i] += src[i];
  }
  return SNF_OK;
}

int snf_cmvn_accumulate(snf_plan* plan, const float* in, int32_t cols, const int64_t* frame_offsets,
                        int64_t n_utts, const float* weights, const int32_t* group,
                        int32_t n_groups, double* stats) {
  int rc = cmvn_check(plan, cols, frame_offsets, n_utts, group, n_groups);
  if (rc) return rc;
  if (n_utts == 0) return SNF_OK;
  const int64_t total_frames = frame_offsets[n_utts];
  if (total_frames == 0) return SNF_OK;
  if (!in) return set_error(SNF_E_INVALID, "null input");
  std::lock_guard<std::mutex> host_lock(plan->host_mu);
  const float *d_in, *d_w = nullptr;
  {
    std::lock_guard<std::mutex> lock(plan->mu);
    if ((rc = guard_device(plan))) return rc;
    if ((rc = plan->stage.in.ensure(static_cast<size_t>(total_frames) * cols, &d_in))) return rc;
    SNF_HIP_CHECK(hipMemcpyAsync(plan->stage.in.p, in, sizeof(float) * total_frames * cols,
                                 hipMemcpyHostToDevice, plan->stream));
    if (weights) {
      if ((rc = plan->post_s.weights.ensure(static_cast<size_t>(total_frames), &d_w))) return rc;
      SNF_HIP_CHECK(hipMemcpyAsync(plan->post_s.weights.p, weights, sizeof(float) * total_frames,
                                   hipMemcpyHostToDevice, plan->stream));
    }
  }
  return snf_cmvn_accumulate_device(plan, d_in, cols, frame_offsets, n_utts, d_w, group, n_groups, stats);
}

int snf_cmvn_apply_device(snf_plan* plan, const float* d_in, int32_t cols,
                          const int64_t* frame_offsets, int64_t n_utts, const double* stats,
                          const int32_t* group, int32_t n_groups, int32_t norm_vars, int32_t reverse,
                          float* d_out) {
  int rc = cmvn_check(plan, cols, frame_offsets, n_utts, group, n_groups);
  if (rc) return rc;
  if (n_utts == 0) return SNF_OK;
  if (!stats) return set_error(SNF_E_INVALID, "null stats");
  // [KALDI-UPSTREAM] transform/cmvn.cc ApplyCmvn / ApplyCmvnReverse: float (offset, scale) per column
  const size_t blk = 2 * static_cast<size_t>(cols + 1);
  std::vector<float> norm(static_cast<size_t>(n_groups) * 2 * cols, 0.0f);
  std::vector<char> used(n_groups, 0);
  for (int64_t u = 0; u < n_utts; ++u) used[group ? group[u] : 0] = 1;
  for (int32_t g = 0; g < n_groups; ++g) {
    if (!used[g]) continue;
    const double* st = stats + blk * static_cast<size_t>(g);
    const double count = st[cols];
    if (count < 1.0)
      return set_error(SNF_E_INVALID, "Insufficient stats for cepstral mean and variance "
                                      "normalization: count = " + std::to_string(count));
    float* off = norm.data() + static_cast<size_t>(g) * 2 * cols;
    float* scl = off + cols;
    for (int d = 0; d < cols; ++d) {
      const double mean = st[d] / count;
      double offset, scale, var = 0.0;
      if (norm_vars) {
        var = st[(cols + 1) + d] / count - mean * mean;
        const double floor = 1.0e-20;
        if (var < floor) var = floor;
      }
      if (!reverse) {
        // without variance normalisation Kaldi adds offset.AddVec(-1.0 / count, mean_stats), whose
        // alpha is a BaseFloat
        offset = static_cast<double>(static_cast<float>(-1.0 / count)) * st[d];
        scale = 1.0;
        if (norm_vars) {
          scale = 1.0 / std::sqrt(var);
          if (scale != scale || 1.0 / scale == 0.0)
            return set_error(SNF_E_RUNTIME, "NaN or infinity in cepstral mean/variance computation");
          offset = -(mean * scale);
        }
      } else {
        offset = mean;
        scale = norm_vars ? std::sqrt(var) : 1.0;
      }
      off[d] = static_cast<float>(offset);
      scl[d] = static_cast<float>(scale);
    }
  }
  std::lock_guard<std::mutex> lock(plan->mu);
  if ((rc = guard_device(plan))) return rc;
  const int64_t total_frames = frame_offsets[n_utts];
  if (total_frames == 0) return SNF_OK;
  if (!d_in || !d_out) return set_error(SNF_E_INVALID, "null buffer");
  hipStream_t s = plan->stream;
  std::vector<int64_t> foff(frame_offsets, frame_offsets + n_utts + 1);
  if ((rc = plan->oc.foff.upload(foff, s))) return rc;
  if ((rc = plan->post_s.norm.upload(norm, s))) return rc;
  const int32_t* d_group = nullptr;
  if (group) {
    std::vector<int32_t> gv(group, group + n_utts);
    if ((rc = plan->post_s.group.upload(gv, s))) return rc;
    d_group = plan->post_s.group.as<int32_t>();
  }
  begin_timing(plan);
  int64_t max_frames = 0;
  for (int64_t k = 0; k < n_utts; ++k)
    max_frames = std::max(max_frames, frame_offsets[k + 1] - frame_offsets[k]);
  if ((rc = launch_cmvn_apply(d_in, cols, plan->oc.foff.as<int64_t>(), n_utts, max_frames, d_group,
                              plan->post_s.norm.as<float>(), norm_vars ? 1 : 0, d_out, s)))
    return rc;
  mark_kernel(plan, "cmvn_apply_kernel");
  SNF_HIP_CHECK(hipStreamSynchronize(s));
  return SNF_OK;
}

int snf_cmvn_apply(snf_plan* plan, const float* in, int32_t cols, const int64_t* frame_offsets,
                   int64_t n_utts, const double* stats, const int32_t* group, int32_t n_groups,
                   int32_t norm_vars, int32_t reverse, float* out) {
  int rc = cmvn_check(plan, cols, frame_offsets, n_utts, group, n_groups);
  if (rc) return rc;
  if (n_utts == 0) return SNF_OK;
  const int64_t total_frames = frame_offsets[n_utts];
  if (total_frames == 0) return SNF_OK;
  if (!in || !out) return set_error(SNF_E_INVALID, "null buffer");
  std::lock_guard<std::mutex> host_lock(plan->host_mu);
  const size_t bytes = sizeof(float) * static_cast<size_t>(total_frames) * cols;
  float *d_in, *d_out;
  {
    std::lock_guard<std::mutex> lock(plan->mu);
    if ((rc = guard_device(plan))) return rc;
    if ((rc = plan->stage.in.ensure(bytes / sizeof(float), &d_in))) return rc;
    if ((rc = plan->stage.out.ensure(bytes / sizeof(float), &d_out))) return rc;
    SNF_HIP_CHECK(hipMemcpyAsync(d_in, in, bytes, hipMemcpyHostToDevice, plan->stream));
  }
  rc = snf_cmvn_apply_device(plan, d_in, cols, frame_offsets, n_utts, stats, group, n_groups, norm_vars,
                             reverse, d_out);
  return rc ? rc : download(plan, out, d_out, bytes);
}

int snf_concat_columns_device(int device_id, const float* d_a, int32_t cols_a,
                              const int64_t* offsets_a, const float* d_b, int32_t cols_b,
                              const int64_t* offsets_b, int64_t n_utts, float* d_out,
                              const int64_t* offsets_out) {
  if (n_utts < 0) return set_error(SNF_E_INVALID, "n_utts < 0");
  if (n_utts == 0) return SNF_OK;
  if (!offsets_a || !offsets_b || !offsets_out) return set_error(SNF_E_INVALID, "null offsets table");
  if (cols_a <= 0 || cols_b <= 0) return set_error(SNF_E_INVALID, "bad column count");
  for (int64_t u = 0; u < n_utts; ++u) {
    const int64_t na = offsets_a[u + 1] - offsets_a[u], nb = offsets_b[u + 1] - offsets_b[u];
    const int64_t no = offsets_out[u + 1] - offsets_out[u];
    if (na < 0 || nb < 0 || no < 0 || no > na || no > nb)
      return set_error(SNF_E_INVALID, "concatenation rows exceed an input for utterance " +
                                          std::to_string(u));
  }
  const int64_t total = offsets_out[n_utts];
  if (total == 0) return SNF_OK;
  if (!d_a || !d_b || !d_out) return set_error(SNF_E_INVALID, "null buffer");
  Planless lay;
  auto d_off = lay.take<int64_t>(3 * (n_utts + 1));   // (the three tables back to back)
  int rc = lay.begin(device_id, nullptr);
  if (rc) return rc;
  // (pageable sources: each copy has read its source when it returns; everything on the thread's own stream,
  // waited for alone - a device-wide wait would also wait for the tracker and the copies of other batches)
  SNF_HIP_CHECK(hipMemcpyAsync(d_off, offsets_a, sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  SNF_HIP_CHECK(hipMemcpyAsync(d_off + (n_utts + 1), offsets_b, sizeof(int64_t) * (n_utts + 1),
                               hipMemcpyHostToDevice, lay.s));
  SNF_HIP_CHECK(hipMemcpyAsync(d_off + 2 * (n_utts + 1), offsets_out, sizeof(int64_t) * (n_utts + 1),
                               hipMemcpyHostToDevice, lay.s));
  rc = launch_concat_columns(d_a, cols_a, d_off, d_b, cols_b, d_off + (n_utts + 1), n_utts, d_out,
                             d_off + 2 * (n_utts + 1), total, lay.s);
  return lay.finish(rc, "concat kernel failed");
}

int snf_count_nonfinite_device(int device_id, const float* d_data, uint64_t n, uint64_t* count) {
  if (!count) return set_error(SNF_E_INVALID, "null count");
  *count = 0;
  if (n == 0) return SNF_OK;
  if (!d_data) return set_error(SNF_E_INVALID, "null buffer");
  if (reinterpret_cast<uintptr_t>(d_data) & 15) return set_error(SNF_E_INVALID, "buffer is not 16-byte aligned");
  Planless lay;
  auto d_count = lay.take<unsigned long long>(1);
  int rc = lay.begin(device_id, nullptr);
  if (rc) return rc;
  unsigned long long host = 0;
  SNF_HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), lay.s));
  rc = launch_count_nonfinite(d_data, n, d_count, lay.s);
  if (!rc && (hipMemcpyAsync(&host, d_count, sizeof(host), hipMemcpyDeviceToHost, lay.s) != hipSuccess ||
              hipStreamSynchronize(lay.s) != hipSuccess))
    rc = set_error(SNF_E_HIP, "non-finite count kernel failed");
  *count = host;
  return rc;
}

}  // extern "C"
