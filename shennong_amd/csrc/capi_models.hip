// C ABI of libshennong_hip.so (include/shennong_amd.h): the plan-less model entry points - diagonal GMM,
// linear VTLN, dense layer, bottleneck extractor.  Each runs on the calling thread's scratch and stream
// (plan.h: Planless).
#include "plan.h"

using namespace snf;

extern "C" {

// ---- diagonal GMM (kernels_gmm.hip) -------------------------------------------------------------
namespace {
int gmm_check_model(int64_t F, int32_t D, int32_t C, const float* d_x, const float* d_gconsts, const float* d_mi,
                    const float* d_iv) {
  if (F < 0) return set_error(SNF_E_INVALID, "gmm: number of frames < 0");
  if (D < 1) return set_error(SNF_E_INVALID, "gmm: feature dimension must be at least 1");
  if (C < 1) return set_error(SNF_E_INVALID, "gmm: number of Gaussians must be at least 1");
  if (!d_gconsts || !d_mi || !d_iv) return set_error(SNF_E_INVALID, "gmm: null model buffer");
  if (F > 0 && !d_x) return set_error(SNF_E_INVALID, "gmm: null frames buffer");
  if (F > (int64_t(1) << 40) / D) return set_error(SNF_E_INVALID, "gmm: frame block too large");
  return SNF_OK;
}

}  // namespace

int snf_gmm_loglikes(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const float* d_gconsts,
                     const float* d_means_invvars, const float* d_inv_vars, int32_t num_gauss, float* d_loglikes,
                     void* stream) {
  int rc = gmm_check_model(n_frames, dim, num_gauss, d_x, d_gconsts, d_means_invvars, d_inv_vars);
  if (rc) return rc;
  if (n_frames > 0 && !d_loglikes) return set_error(SNF_E_INVALID, "gmm: null output buffer");
  if (n_frames == 0) return SNF_OK;
  Planless lay;
  if ((rc = lay.begin(device_id, stream))) return rc;
  rc = launch_gmm_loglikes(d_x, n_frames, dim, d_gconsts, d_means_invvars, d_inv_vars, num_gauss, d_loglikes, lay.s);
  return lay.finish(rc, "gmm loglikes kernel failed");
}

int snf_gmm_accumulate(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const float* d_frame_weights,
                       const float* d_gconsts, const float* d_means_invvars, const float* d_inv_vars,
                       int32_t num_gauss, double* d_stats, double* d_tot_like, float* d_lse, void* stream) {
  int rc = gmm_check_model(n_frames, dim, num_gauss, d_x, d_gconsts, d_means_invvars, d_inv_vars);
  if (rc) return rc;
  if (!d_stats || !d_tot_like) return set_error(SNF_E_INVALID, "gmm: null statistics buffer");
  const int64_t J = 2 * int64_t(dim) + 1, n = num_gauss * J;
  if (n_frames == 0) {
    SNF_HIP_CHECK(hipSetDevice(device_id));
    SNF_HIP_CHECK(hipMemset(d_stats, 0, sizeof(double) * n));
    SNF_HIP_CHECK(hipMemset(d_tot_like, 0, sizeof(double)));
    return SNF_OK;
  }
  const int64_t tiles = gmm_tiles(n_frames), chunks = gmm_stats_chunks(n_frames, num_gauss, dim);
  Planless lay;
  auto part = lay.take<double>(chunks * n);
  auto tl_part = lay.take<double>(tiles);
  auto own_lse = lay.take<float>(d_lse ? 0 : n_frames);
  if ((rc = lay.begin(device_id, stream))) return rc;
  rc = launch_gmm_accumulate(d_x, n_frames, dim, d_frame_weights, d_gconsts, d_means_invvars, d_inv_vars, num_gauss,
                             d_lse ? d_lse : own_lse, tl_part, part, d_stats, d_tot_like, lay.s);
  return lay.finish(rc, "gmm accumulate kernels failed");
}

int snf_gmm_gselect(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const float* d_gconsts,
                    const float* d_means_invvars, const float* d_inv_vars, int32_t num_gauss, int32_t num_gselect,
                    int32_t* d_gselect, float* d_loglike, void* stream) {
  int rc = gmm_check_model(n_frames, dim, num_gauss, d_x, d_gconsts, d_means_invvars, d_inv_vars);
  if (rc) return rc;
  if (num_gselect < 1 || num_gselect > num_gauss)
    return set_error(SNF_E_INVALID, "gmm: num_gselect must be in [1, num_gauss]");
  if (n_frames > 0 && !d_gselect) return set_error(SNF_E_INVALID, "gmm: null output buffer");
  if (n_frames == 0) return SNF_OK;
  // L staged through HBM ~128 MB at a time (multiples of the 64-frame tile)
  int64_t rows = std::max<int64_t>(64, ((int64_t(32) << 20) / num_gauss) & ~int64_t(63));
  rows = std::min(rows, (n_frames + 63) & ~int64_t(63));
  Planless lay;
  auto L = lay.take<float>(rows * num_gauss);
  if ((rc = lay.begin(device_id, stream))) return rc;
  for (int64_t a = 0; a < n_frames && !rc; a += rows) {
    const int64_t r = std::min(rows, n_frames - a);
    rc = launch_gmm_loglikes(d_x + a * dim, r, dim, d_gconsts, d_means_invvars, d_inv_vars, num_gauss, L, lay.s);
    if (!rc)
      rc = launch_gmm_topn(L, nullptr, r, num_gauss, num_gselect, d_gselect + a * num_gselect,
                           d_loglike ? d_loglike + a : nullptr, lay.s);
  }
  return lay.finish(rc, "gmm gselect kernels failed");
}

int snf_gmm_gselect_preselect(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const float* d_gconsts,
                              const float* d_means_invvars, const float* d_inv_vars, int32_t num_gauss,
                              const int32_t* d_preselect, int32_t num_preselect, int32_t num_gselect,
                              int32_t* d_gselect, float* d_loglike, void* stream) {
  int rc = gmm_check_model(n_frames, dim, num_gauss, d_x, d_gconsts, d_means_invvars, d_inv_vars);
  if (rc) return rc;
  if (num_preselect < 1) return set_error(SNF_E_INVALID, "gmm: num_preselect must be at least 1");
  if (num_gselect < 1 || num_gselect > num_preselect)
    return set_error(SNF_E_INVALID, "gmm: num_gselect must be in [1, num_preselect]");
  if (n_frames > 0 && (!d_preselect || !d_gselect)) return set_error(SNF_E_INVALID, "gmm: null selection buffer");
  if (n_frames == 0) return SNF_OK;
  Planless lay;
  auto L = lay.take<float>(n_frames * num_preselect);
  auto d_bad = lay.take<int>(1);
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), lay.s));
  rc = launch_gmm_sel_loglikes(d_x, n_frames, dim, d_gconsts, d_means_invvars, d_inv_vars, num_gauss, d_preselect,
                               num_preselect, L, d_bad, lay.s);
  if (!rc) rc = launch_gmm_topn(L, d_preselect, n_frames, num_preselect, num_gselect, d_gselect, d_loglike, lay.s);
  return lay.finish(rc, "gmm preselect kernels failed", d_bad, "gmm preselect: copy failed",
                    "gmm: preselected Gaussian index out of range");
}

int snf_gmm_selection_posteriors(int device_id, const float* d_x, int64_t n_frames, int32_t dim,
                                 const float* d_gconsts, const float* d_means_invvars, const float* d_inv_vars,
                                 int32_t num_gauss, const int32_t* d_gselect, int32_t num_gselect, float min_post,
                                 float* d_post, float* d_loglike, void* stream) {
  int rc = gmm_check_model(n_frames, dim, num_gauss, d_x, d_gconsts, d_means_invvars, d_inv_vars);
  if (rc) return rc;
  if (num_gselect < 1) return set_error(SNF_E_INVALID, "gmm: num_gselect must be at least 1");
  if (n_frames > 0 && (!d_gselect || !d_post || !d_loglike))
    return set_error(SNF_E_INVALID, "gmm: null selection buffer");
  if (n_frames == 0) return SNF_OK;
  Planless lay;
  auto d_bad = lay.take<int>(1);
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), lay.s));
  rc = launch_gmm_sel_loglikes(d_x, n_frames, dim, d_gconsts, d_means_invvars, d_inv_vars, num_gauss, d_gselect,
                               num_gselect, d_post, d_bad, lay.s);
  if (!rc) rc = launch_gmm_post(d_post, n_frames, num_gselect, min_post, min_post >= 0.0f, d_loglike, lay.s);
  return lay.finish(rc, "gmm posteriors kernels failed", d_bad, "gmm posteriors: copy failed",
                    "gmm: selected Gaussian index out of range");
}

int snf_gmm_posteriors(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const float* d_gconsts,
                       const float* d_means_invvars, const float* d_inv_vars, int32_t num_gauss, float* d_post,
                       float* d_lse, void* stream) {
  int rc = gmm_check_model(n_frames, dim, num_gauss, d_x, d_gconsts, d_means_invvars, d_inv_vars);
  if (rc) return rc;
  if (n_frames > 0 && !d_post) return set_error(SNF_E_INVALID, "gmm: null output buffer");
  if ((reinterpret_cast<uintptr_t>(d_post) & 3) || (reinterpret_cast<uintptr_t>(d_lse) & 3))
    return set_error(SNF_E_INVALID, "gmm: output buffer not aligned to float32");
  if (n_frames > (int64_t(1) << 40) / num_gauss) return set_error(SNF_E_INVALID, "gmm: posterior block too large");
  if (n_frames == 0) return SNF_OK;
  Planless lay;
  auto tl_part = lay.take<double>(gmm_tiles(n_frames));
  auto own_lse = lay.take<float>(d_lse ? 0 : n_frames);
  if ((rc = lay.begin(device_id, stream))) return rc;
  rc = launch_gmm_posteriors(d_x, n_frames, dim, d_gconsts, d_means_invvars, d_inv_vars, num_gauss,
                             d_lse ? d_lse : own_lse, tl_part, d_post, lay.s);
  return lay.finish(rc, "gmm posteriors kernels failed");
}

// ---- linear VTLN (kernels_vtln.hip) -------------------------------------------------------------
namespace {
int vtln_check_segments(const int64_t* off, int64_t S, int64_t F) {
  if (S < 0) return set_error(SNF_E_INVALID, "vtln: number of segments < 0");
  if (!off) return set_error(SNF_E_INVALID, "vtln: null segment offsets");
  if (off[0] != 0 || off[S] != F) return set_error(SNF_E_INVALID, "vtln: segment offsets must run from 0 to n_frames");
  for (int64_t s = 0; s < S; ++s)
    if (off[s + 1] < off[s]) return set_error(SNF_E_INVALID, "vtln: segment offsets must be non-decreasing");
  return SNF_OK;
}

// Items of at most vtln_item_frames() frames per segment: (first, end, slot) with slot = the segment when it
// has one item, else n_segments + its partial's index; red = (segment, first partial, count) per split segment.
void vtln_items(const int64_t* off, int64_t S, std::vector<int64_t>* items, std::vector<int64_t>* red,
                int64_t* n_part) {
  const int64_t chunk = vtln_item_frames();
  *n_part = 0;
  for (int64_t s = 0; s < S; ++s) {
    const int64_t len = off[s + 1] - off[s];
    if (len == 0) continue;
    const int64_t nch = (len + chunk - 1) / chunk;
    if (nch == 1) {
      items->insert(items->end(), {off[s], off[s + 1], s});
      continue;
    }
    red->insert(red->end(), {s, *n_part, nch});
    for (int64_t c = 0; c < nch; ++c) {
      const int64_t a = off[s] + c * chunk;
      items->insert(items->end(), {a, std::min(off[s + 1], a + chunk), S + (*n_part)++});
    }
  }
}
}  // namespace

int snf_fmllr_accumulate(int device_id, const float* d_x, int64_t n_frames, int32_t dim, const int32_t* d_gselect,
                         const float* d_post, int32_t num_gselect, const float* d_means_invvars,
                         const float* d_inv_vars, int32_t num_gauss, const int64_t* h_seg_offsets,
                         int64_t n_segments, double* d_stats, void* stream) {
  if (n_frames < 0) return set_error(SNF_E_INVALID, "vtln: number of frames < 0");
  if (dim < 1 || dim > 64) return set_error(SNF_E_INVALID, "vtln: feature dimension must be in [1, 64]");
  if (num_gauss < 1) return set_error(SNF_E_INVALID, "vtln: number of Gaussians must be at least 1");
  if (num_gselect < 1 || num_gselect > 64) return set_error(SNF_E_INVALID, "vtln: num_gselect must be in [1, 64]");
  if (!d_means_invvars || !d_inv_vars) return set_error(SNF_E_INVALID, "vtln: null model buffer");
  if (n_frames > 0 && (!d_x || !d_gselect || !d_post)) return set_error(SNF_E_INVALID, "vtln: null frames buffer");
  if (n_frames > (int64_t(1) << 28)) return set_error(SNF_E_INVALID, "vtln: frame block too large");
  int rc = vtln_check_segments(h_seg_offsets, n_segments, n_frames);
  if (rc) return rc;
  if (n_segments > 0 && !d_stats) return set_error(SNF_E_INVALID, "vtln: null statistics buffer");
  if (n_segments == 0) return SNF_OK;
  const int64_t V = dim + 1, U = int64_t(dim) * V + dim + 1, uv = U * V;
  std::vector<int64_t> items, red;
  int64_t n_part = 0;
  vtln_items(h_seg_offsets, n_segments, &items, &red, &n_part);
  Planless lay;
  auto rec = lay.take<double>(std::max<int64_t>(1, n_frames) * (3 * dim + 2));
  auto part = lay.take<double>(n_part * uv);
  auto d_items = lay.take<int64_t>(items.size() + 3);
  auto d_red = lay.take<int64_t>(red.size() + 3);
  auto d_bad = lay.take<int>(1);
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int), lay.s));
  SNF_HIP_CHECK(hipMemsetAsync(d_stats, 0, sizeof(double) * n_segments * uv, lay.s));
  if (!items.empty())
    SNF_HIP_CHECK(hipMemcpyAsync(d_items, items.data(), sizeof(int64_t) * items.size(), hipMemcpyHostToDevice, lay.s));
  if (!red.empty())
    SNF_HIP_CHECK(hipMemcpyAsync(d_red, red.data(), sizeof(int64_t) * red.size(), hipMemcpyHostToDevice, lay.s));
  rc = launch_fmllr_accumulate(d_x, n_frames, dim, d_gselect, d_post, num_gselect, d_means_invvars, d_inv_vars,
                               num_gauss, rec, d_bad, d_items, int64_t(items.size() / 3), n_segments, d_stats, part,
                               d_red, int64_t(red.size() / 3), lay.s);
  return lay.finish(rc, "fmllr accumulate kernels failed", d_bad, "fmllr accumulate: copy failed",
                    "vtln: selected Gaussian index out of range");
}

extern "C++" {
namespace {
// The Gram's scratch (records, partials, item and reduction lists) and its one segment's schedule; `records`
// launches the record pre-pass and the product on what it is given.
template <typename Launch>
int vtln_gram_common(int device_id, int64_t n_frames, int32_t dim, double* d_gram, void* stream, Launch records) {
  const int64_t V = 2 * int64_t(dim) + 1, uv = V * V;
  const int64_t off[2] = {0, n_frames};
  std::vector<int64_t> items, red;
  int64_t n_part = 0;
  vtln_items(off, 1, &items, &red, &n_part);
  Planless lay;
  auto rec = lay.take<double>(std::max<int64_t>(1, n_frames) * (2 * dim + 2));
  auto part = lay.take<double>(n_part * uv);
  auto d_items = lay.take<int64_t>(items.size() + 3);
  auto d_red = lay.take<int64_t>(red.size() + 3);
  int rc = lay.begin(device_id, stream);
  if (rc) return rc;
  SNF_HIP_CHECK(hipMemsetAsync(d_gram, 0, sizeof(double) * uv, lay.s));
  if (!items.empty())
    SNF_HIP_CHECK(hipMemcpyAsync(d_items, items.data(), sizeof(int64_t) * items.size(), hipMemcpyHostToDevice, lay.s));
  if (!red.empty())
    SNF_HIP_CHECK(hipMemcpyAsync(d_red, red.data(), sizeof(int64_t) * red.size(), hipMemcpyHostToDevice, lay.s));
  rc = records(rec, d_items, int64_t(items.size() / 3), part, d_red, int64_t(red.size() / 3), lay.s);
  return lay.finish(rc, "vtln gram kernels failed");
}

// `frames`: every frame source is given (checked only when there are frames)
int vtln_gram_check(int64_t n_frames, int32_t dim, bool frames, const double* d_gram) {
  if (n_frames < 0) return set_error(SNF_E_INVALID, "vtln: number of frames < 0");
  if (dim < 1 || dim > 64) return set_error(SNF_E_INVALID, "vtln: feature dimension must be in [1, 64]");
  if (n_frames > 0 && !frames) return set_error(SNF_E_INVALID, "vtln: null frames buffer");
  if (!d_gram) return set_error(SNF_E_INVALID, "vtln: null output buffer");
  if (n_frames > (int64_t(1) << 28)) return set_error(SNF_E_INVALID, "vtln: frame block too large");
  return SNF_OK;
}
}  // namespace
}  // extern "C++"

int snf_vtln_gram(int device_id, const float* d_x, const float* d_y, const float* d_weights, int64_t n_frames,
                  int32_t dim, double* d_gram, void* stream) {
  int rc = vtln_gram_check(n_frames, dim, d_x && d_y, d_gram);
  if (rc) return rc;
  return vtln_gram_common(device_id, n_frames, dim, d_gram, stream,
                          [&](double* rec, const int64_t* items, int64_t n_items, double* part, const int64_t* red,
                              int64_t n_red, hipStream_t s) {
                            return launch_vtln_gram(d_x, d_y, d_weights, n_frames, dim, rec, items, n_items, d_gram,
                                                    part, red, n_red, s);
                          });
}

int snf_vtln_gram_rows(int device_id, const float* const* d_x_blocks, const float* const* d_y_blocks,
                       const int32_t* d_block, const int64_t* d_row, const float* d_weights, int64_t n_frames,
                       int32_t dim, double* d_gram, void* stream) {
  int rc = vtln_gram_check(n_frames, dim, d_x_blocks && d_y_blocks && d_block && d_row, d_gram);
  if (rc) return rc;
  return vtln_gram_common(device_id, n_frames, dim, d_gram, stream,
                          [&](double* rec, const int64_t* items, int64_t n_items, double* part, const int64_t* red,
                              int64_t n_red, hipStream_t s) {
                            return launch_vtln_gram_rows(d_x_blocks, d_y_blocks, d_block, d_row, d_weights, n_frames,
                                                         dim, rec, items, n_items, d_gram, part, red, n_red, s);
                          });
}

int snf_lvtln_select(int device_id, const double* d_stats, int64_t n_segments, int32_t dim, const double* d_A,
                     const double* d_logdets, int32_t num_classes, int32_t norm_type, double logdet_scale,
                     int32_t default_class, double* d_objf, int32_t* d_class, double* d_impr, double* d_count,
                     float* d_transform, void* stream) {
  if (n_segments < 0) return set_error(SNF_E_INVALID, "vtln: number of segments < 0");
  if (dim < 1 || dim > 64) return set_error(SNF_E_INVALID, "vtln: feature dimension must be in [1, 64]");
  if (num_classes < 1) return set_error(SNF_E_INVALID, "vtln: number of classes must be at least 1");
  if (default_class < 0 || default_class >= num_classes)
    return set_error(SNF_E_INVALID, "vtln: default class must be in [0, num_classes)");
  if (norm_type < 0 || norm_type > 2) return set_error(SNF_E_INVALID, "vtln: norm_type must be 0, 1 or 2");
  if (!std::isfinite(logdet_scale)) return set_error(SNF_E_INVALID, "vtln: logdet_scale must be finite");
  if (!d_A || !d_logdets) return set_error(SNF_E_INVALID, "vtln: null model buffer");
  if (n_segments > 0 && (!d_stats || !d_objf || !d_class || !d_impr || !d_count || !d_transform))
    return set_error(SNF_E_INVALID, "vtln: null statistics or output buffer");
  if (n_segments == 0) return SNF_OK;
  Planless lay;
  int rc = lay.begin(device_id, stream);
  if (rc) return rc;
  rc = launch_lvtln_select(d_stats, n_segments, dim, d_A, d_logdets, num_classes, norm_type, logdet_scale,
                           default_class, d_objf, d_class, d_impr, d_count, d_transform, lay.s);
  return lay.finish(rc, "lvtln select kernel failed");
}

int snf_affine_apply_segments(int device_id, const float* d_x, int64_t n_frames, int32_t dim,
                              const int64_t* h_seg_offsets, int64_t n_segments, const float* d_transforms,
                              float* d_y, void* stream) {
  if (n_frames < 0) return set_error(SNF_E_INVALID, "vtln: number of frames < 0");
  if (dim < 1 || dim > 64) return set_error(SNF_E_INVALID, "vtln: feature dimension must be in [1, 64]");
  if (n_frames > (int64_t(1) << 28)) return set_error(SNF_E_INVALID, "vtln: frame block too large");
  int rc = vtln_check_segments(h_seg_offsets, n_segments, n_frames);
  if (rc) return rc;
  if (n_frames > 0 && (!d_x || !d_y || !d_transforms)) return set_error(SNF_E_INVALID, "vtln: null buffer");
  if (n_frames == 0) return SNF_OK;
  Planless lay;
  auto d_off = lay.take<int64_t>(n_segments + 1);
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemcpyAsync(d_off, h_seg_offsets, sizeof(int64_t) * (n_segments + 1), hipMemcpyHostToDevice, lay.s));
  rc = launch_affine_apply_segments(d_x, n_frames, dim, d_off, n_segments, d_transforms, d_y, lay.s);
  return lay.finish(rc, "affine apply kernel failed");
}

// ---- bottleneck extractor (kernels_bottleneck.hip) ------------------------------------------------------
namespace {
constexpr int kBnWin = 200, kBnShift = 80, kBnMel = 24, kBnIn = 144, kBnOut = 80, kBnEdge = 15, kBnStack = 5,
              kBnStackStep = 5, kBnMaxWidth = 1 << 20;

int bn_check_offsets(const int64_t* h_off, int64_t n, const char* what) {
  if (n < 0) return set_error(SNF_E_INVALID, std::string("bottleneck: number of utterances < 0"));
  if (!h_off) return set_error(SNF_E_INVALID, std::string("bottleneck: null ") + what + " offsets table");
  if (h_off[0] != 0) return set_error(SNF_E_INVALID, std::string("bottleneck: ") + what + " offsets must start at 0");
  for (int64_t u = 0; u < n; ++u)
    if (h_off[u + 1] < h_off[u])
      return set_error(SNF_E_INVALID, std::string("bottleneck: ") + what + " offsets must not decrease");
  if (h_off[n] > (int64_t(1) << 40)) return set_error(SNF_E_INVALID, "bottleneck: batch too large");
  return SNF_OK;
}

int64_t bn_frames(int64_t n) { return n < kBnWin ? 0 : (n - kBnWin) / kBnShift + 1; }

// frame offsets of a waveform batch, [n_utts + 1]
void bn_frame_offsets(const int64_t* h_soff, int64_t n_utts, std::vector<int64_t>* foff) {
  foff->assign(n_utts + 1, 0);
  for (int64_t u = 0; u < n_utts; ++u) (*foff)[u + 1] = (*foff)[u] + bn_frames(h_soff[u + 1] - h_soff[u]);
}
}  // namespace

int snf_dense_layer(int device_id, const float* d_x, int64_t m, int32_t k, const float* d_w, const float* d_b,
                    int32_t n, int32_t act, float* d_y, void* stream) {
  if (m < 0) return set_error(SNF_E_INVALID, "dense layer: number of rows < 0");
  if (k < 1 || n < 1) return set_error(SNF_E_INVALID, "dense layer: k and n must be at least 1");
  if (act != 0 && act != 1) return set_error(SNF_E_INVALID, "dense layer: act must be 0 (identity) or 1 (sigmoid)");
  if (!d_w || !d_b) return set_error(SNF_E_INVALID, "dense layer: null weights or bias");
  if (m > 0 && (!d_x || !d_y)) return set_error(SNF_E_INVALID, "dense layer: null buffer");
  if (m > (int64_t(1) << 40) / std::max(k, n)) return set_error(SNF_E_INVALID, "dense layer: matrix too large");
  if (m == 0) return SNF_OK;
  Planless lay;
  int rc = lay.begin(device_id, stream);
  if (rc) return rc;
  rc = launch_bn_dense(d_x, m, k, d_w, d_b, n, act, d_y, nullptr, 0, 0, lay.s);
  return lay.finish(rc, "dense layer kernel failed");
}

int64_t snf_packed_weights_bf16_size(int32_t k, int32_t n) {
  if (k < 1 || n < 1 || k > kBnMaxWidth || n > kBnMaxWidth) return 0;
  return int64_t(n) * bn_bf16_padded_k(k);
}

int snf_pack_weights_bf16(int device_id, const float* d_w, int32_t k, int32_t n, uint16_t* d_packed, void* stream) {
  if (k < 1 || n < 1) return set_error(SNF_E_INVALID, "pack weights: k and n must be at least 1");
  if (k > kBnMaxWidth || n > kBnMaxWidth) return set_error(SNF_E_INVALID, "pack weights: k and n must be at most 2^20");
  if (!d_w || !d_packed) return set_error(SNF_E_INVALID, "pack weights: null buffer");
  if (reinterpret_cast<uintptr_t>(d_packed) & 15)
    return set_error(SNF_E_INVALID, "pack weights: the image is not 16-byte aligned");
  Planless lay;
  int rc = lay.begin(device_id, stream);
  if (rc) return rc;
  rc = launch_bn_pack_bf16(d_w, k, n, d_packed, lay.s);
  return lay.finish(rc, "pack weights kernel failed");
}

int snf_dense_layer_bf16(int device_id, const float* d_x, int64_t m, int32_t k, const uint16_t* d_packed,
                         const float* d_b, int32_t n, int32_t act, float* d_y, void* stream) {
  if (m < 0) return set_error(SNF_E_INVALID, "dense layer: number of rows < 0");
  if (k < 1 || n < 1) return set_error(SNF_E_INVALID, "dense layer: k and n must be at least 1");
  if (k > kBnMaxWidth || n > kBnMaxWidth) return set_error(SNF_E_INVALID, "dense layer: k and n must be at most 2^20");
  if (act != 0 && act != 1) return set_error(SNF_E_INVALID, "dense layer: act must be 0 (identity) or 1 (sigmoid)");
  if (!d_packed || !d_b) return set_error(SNF_E_INVALID, "dense layer: null weights or bias");
  if (reinterpret_cast<uintptr_t>(d_packed) & 15)
    return set_error(SNF_E_INVALID, "dense layer: packed weights are not 16-byte aligned");
  if (m > 0 && (!d_x || !d_y)) return set_error(SNF_E_INVALID, "dense layer: null buffer");
  if (m > (int64_t(1) << 40) / std::max(k, n)) return set_error(SNF_E_INVALID, "dense layer: matrix too large");
  if (m == 0) return SNF_OK;
  Planless lay;
  int rc = lay.begin(device_id, stream);
  if (rc) return rc;
  rc = launch_bn_dense_bf16(d_x, m, k, d_packed, d_b, n, act, d_y, lay.s);
  return lay.finish(rc, "dense layer kernel failed");
}

int snf_bottleneck_vad(int device_id, const int16_t* d_wave, const int64_t* h_sample_offsets, int64_t n_utts,
                       uint8_t* d_mask, int32_t* d_voiced, void* stream) {
  int rc = bn_check_offsets(h_sample_offsets, n_utts, "sample");
  if (rc) return rc;
  if (n_utts == 0) return SNF_OK;
  if (!d_voiced) return set_error(SNF_E_INVALID, "bottleneck: null voiced-count buffer");
  std::vector<int64_t> foff;
  bn_frame_offsets(h_sample_offsets, n_utts, &foff);
  const int64_t total = foff[n_utts];
  if (total > 0 && (!d_wave || !d_mask)) return set_error(SNF_E_INVALID, "bottleneck: null buffer");
  Planless lay;
  auto d_soff = lay.take<int64_t>(n_utts + 1);
  auto d_foff = lay.take<int64_t>(n_utts + 1);
  auto energy = lay.take<double>(std::max<int64_t>(total, 1));
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemcpyAsync(d_soff, h_sample_offsets, sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  SNF_HIP_CHECK(hipMemcpyAsync(d_foff, foff.data(), sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  rc = launch_bn_vad(d_wave, d_soff, d_foff, n_utts, energy, d_mask, d_voiced, lay.s);
  return lay.finish(rc, "bottleneck vad kernel failed");
}

int snf_bottleneck_fbank(int device_id, const int16_t* d_wave, const int64_t* h_sample_offsets, int64_t n_utts,
                         const float* d_tables, float dither, uint64_t seed, float* d_logmel, void* stream) {
  int rc = bn_check_offsets(h_sample_offsets, n_utts, "sample");
  if (rc) return rc;
  if (!(dither >= 0.0f)) return set_error(SNF_E_INVALID, "bottleneck: dither must be >= 0");
  if (n_utts == 0) return SNF_OK;
  std::vector<int64_t> foff;
  bn_frame_offsets(h_sample_offsets, n_utts, &foff);
  const int64_t total = foff[n_utts];
  if (total == 0) return SNF_OK;
  if (!d_wave || !d_tables || !d_logmel) return set_error(SNF_E_INVALID, "bottleneck: null buffer");
  if (reinterpret_cast<uintptr_t>(d_tables) & 7) return set_error(SNF_E_INVALID, "bottleneck: tables are not 8-byte aligned");
  Planless lay;
  auto d_soff = lay.take<int64_t>(n_utts + 1);
  auto d_foff = lay.take<int64_t>(n_utts + 1);
  auto utt_noise = lay.take<uint32_t>(n_utts);
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemcpyAsync(d_soff, h_sample_offsets, sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  SNF_HIP_CHECK(hipMemcpyAsync(d_foff, foff.data(), sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  rc = launch_bn_fbank(d_wave, d_soff, d_foff, n_utts, total, d_tables, dither, seed,
                       utt_noise, d_logmel, lay.s);
  return lay.finish(rc, "bottleneck filterbank kernel failed");
}

int snf_bottleneck_nn_input(int device_id, const float* d_logmel, const uint8_t* d_mask, const int32_t* d_voiced,
                            const int64_t* h_frame_offsets, int64_t n_utts, int32_t context, const float* d_basis,
                            float* d_x, void* stream) {
  int rc = bn_check_offsets(h_frame_offsets, n_utts, "frame");
  if (rc) return rc;
  if (context < 0 || context > bn_max_context())
    return set_error(SNF_E_INVALID, "bottleneck: context must be in [0, " + std::to_string(bn_max_context()) + "]");
  if (n_utts == 0) return SNF_OK;
  std::vector<int64_t> roff(n_utts + 1, 0);
  for (int64_t u = 0; u < n_utts; ++u) {
    const int64_t F = h_frame_offsets[u + 1] - h_frame_offsets[u];
    const int64_t rows = F + 2 * kBnEdge - 2 * context;
    if (F < 1 || rows < 1)
      return set_error(SNF_E_INVALID, "bottleneck: utterance " + std::to_string(u) + " has " + std::to_string(F) +
                                          " frames, too few for one row at context " + std::to_string(context));
    roff[u + 1] = roff[u] + rows;
  }
  if (!d_logmel || !d_mask || !d_voiced || !d_basis || !d_x) return set_error(SNF_E_INVALID, "bottleneck: null buffer");
  Planless lay;
  auto d_foff = lay.take<int64_t>(n_utts + 1);
  auto d_roff = lay.take<int64_t>(n_utts + 1);
  auto mean = lay.take<float>(kBnMel * n_utts);
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemcpyAsync(d_foff, h_frame_offsets, sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  SNF_HIP_CHECK(hipMemcpyAsync(d_roff, roff.data(), sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  rc = launch_bn_nn_input(d_logmel, d_mask, d_voiced, d_foff, d_roff, n_utts, roff[n_utts], context, d_basis,
                          mean, d_x, lay.s);
  return lay.finish(rc, "bottleneck input kernels failed");
}

namespace {
// the stacked networks; `bf16`: W2, W3, W6 and W7 are packed bfloat16 images and run on bn_dense_bf16_kernel
int bn_forward(bool bf16, int device_id, const float* d_x, const int64_t* h_row_offsets, int64_t n_utts,
               const int32_t* h_widths, const void* const* h_params, float* d_bn, float* d_out, void* stream) {
  int rc = bn_check_offsets(h_row_offsets, n_utts, "row");
  if (rc) return rc;
  if (!h_widths || !h_params) return set_error(SNF_E_INVALID, "bottleneck: null layer description");
  for (int i = 0; i < 4; ++i)
    if (h_widths[i] < 1 || h_widths[i] > (1 << 20))
      return set_error(SNF_E_INVALID, "bottleneck: layer width " + std::to_string(i) + " out of range");
  for (int i = 0; i < 12; ++i)
    if (!h_params[i]) return set_error(SNF_E_INVALID, "bottleneck: null parameter buffer " + std::to_string(i));
  if (bf16)
    for (int i : {2, 4, 8, 10})
      if (reinterpret_cast<uintptr_t>(h_params[i]) & 15)
        return set_error(SNF_E_INVALID, "bottleneck: packed weights " + std::to_string(i) + " are not 16-byte aligned");
  if (n_utts == 0) return SNF_OK;
  const int span = kBnStackStep * (kBnStack - 1);   // 20 rows of the first stage under one stacked row
  std::vector<int64_t> ooff(n_utts + 1, 0);
  for (int64_t u = 0; u < n_utts; ++u) {
    const int64_t rows = h_row_offsets[u + 1] - h_row_offsets[u];
    if (rows <= span)
      return set_error(SNF_E_INVALID, "bottleneck: utterance " + std::to_string(u) + " has " + std::to_string(rows) +
                                          " first-stage rows, the stack needs more than " + std::to_string(span));
    ooff[u + 1] = ooff[u] + rows - span;
  }
  const int64_t R0 = h_row_offsets[n_utts], R1 = ooff[n_utts];
  if (!d_x || !d_bn || !d_out) return set_error(SNF_E_INVALID, "bottleneck: null buffer");
  const int wmax = std::max(std::max(h_widths[0], h_widths[1]), std::max(h_widths[2], h_widths[3]));
  // hidden activations live in scratch, one block of rows at a time (rows are independent of each other)
  int64_t chunk = std::max<int64_t>(1024, (int64_t(512) << 20) / (4 * int64_t(wmax))) & ~int64_t(127);
  chunk = std::min(chunk, (R0 + 127) & ~int64_t(127));
  Planless lay;
  auto d_roff = lay.take<int64_t>(n_utts + 1);
  auto d_ooff = lay.take<int64_t>(n_utts + 1);
  auto d_map = lay.take<int64_t>(R1);
  auto h1 = lay.take<float>(chunk * wmax);
  auto h2 = lay.take<float>(chunk * wmax);
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemcpyAsync(d_roff, h_row_offsets, sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  SNF_HIP_CHECK(hipMemcpyAsync(d_ooff, ooff.data(), sizeof(int64_t) * (n_utts + 1), hipMemcpyHostToDevice, lay.s));
  const void* const* P = h_params;
  auto F = [](const void* p) { return static_cast<const float*>(p); };
  // a layer that reads sigmoid outputs: the float32 kernel or the bfloat16 one
  auto hidden = [&](const float* x, int64_t m, int k, int i, int n, int act, float* y) {
    return bf16 ? launch_bn_dense_bf16(x, m, k, static_cast<const uint16_t*>(P[i]), F(P[i + 1]), n, act, y, lay.s)
                : launch_bn_dense(x, m, k, F(P[i]), F(P[i + 1]), n, act, y, nullptr, 0, 0, lay.s);
  };
  for (int64_t a = 0; a < R0 && !rc; a += chunk) {
    const int64_t m = std::min(chunk, R0 - a);
    rc = launch_bn_dense(d_x + a * kBnIn, m, kBnIn, F(P[0]), F(P[1]), h_widths[0], 1, h1, nullptr, 0, 0, lay.s);
    if (!rc) rc = hidden(h1, m, h_widths[0], 2, h_widths[1], 1, h2);
    if (!rc) rc = hidden(h2, m, h_widths[1], 4, kBnOut, 0, d_bn + a * kBnOut);
  }
  if (!rc) rc = launch_bn_row_map(d_roff, d_ooff, n_utts, R1, d_map, lay.s);
  for (int64_t a = 0; a < R1 && !rc; a += chunk) {
    const int64_t m = std::min(chunk, R1 - a);
    rc = launch_bn_dense(d_bn, m, kBnStack * kBnOut, F(P[6]), F(P[7]), h_widths[2], 1, h1, d_map + a, kBnOut, kBnStackStep,
                         lay.s);
    if (!rc) rc = hidden(h1, m, h_widths[2], 8, h_widths[3], 1, h2);
    if (!rc) rc = hidden(h2, m, h_widths[3], 10, kBnOut, 0, d_out + a * kBnOut);
  }
  return lay.finish(rc, "bottleneck network kernels failed");
}
}  // namespace

int snf_bottleneck_forward(int device_id, const float* d_x, const int64_t* h_row_offsets, int64_t n_utts,
                           const int32_t* h_widths, const float* const* h_params, float* d_bn, float* d_out,
                           void* stream) {
  return bn_forward(false, device_id, d_x, h_row_offsets, n_utts, h_widths,
                    reinterpret_cast<const void* const*>(h_params), d_bn, d_out, stream);
}

int snf_bottleneck_forward_bf16(int device_id, const float* d_x, const int64_t* h_row_offsets, int64_t n_utts,
                                const int32_t* h_widths, const void* const* h_params, float* d_bn, float* d_out,
                                void* stream) {
  return bn_forward(true, device_id, d_x, h_row_offsets, n_utts, h_widths, h_params, d_bn, d_out, stream);
}

// ---- the whole extractor in one call ----------------------------------------------------------------------
namespace {
constexpr int64_t kBnExtractScratch = int64_t(1) << 30;   // default bound of the intermediates of one run
constexpr int64_t kBnRunPad = 16 * 256;                   // the 256-byte rounding of a run's pieces

struct BnUtt {
  int64_t F, R0, R1;   // frames, first-stage rows, output rows
};

// bytes of one utterance's intermediates: mask, VAD energies, log-mel energies | x, first stage | row map | the
// voiced mean, the voiced count and the noise word
int64_t bn_utt_bytes(const BnUtt& t) {
  return t.F * (1 + 8 + 4 * kBnMel) + t.R0 * 4 * (kBnIn + kBnOut) + t.R1 * 8 + 4 * kBnMel + 4 + 4;
}

// rows of each of the two hidden buffers: a quarter of the bound each, never less than one tile of 128 rows
int64_t bn_hidden_rows(int64_t bound, int wmax) {
  return std::max<int64_t>(128, (bound / 4 / (4 * int64_t(wmax))) & ~int64_t(127));
}

int bn_extract_check(const int64_t* h_soff, int64_t n_utts, int32_t context, const int32_t* h_widths,
                     int64_t scratch_bytes, std::vector<BnUtt>* utts) {
  int rc = bn_check_offsets(h_soff, n_utts, "sample");
  if (rc) return rc;
  if (context < 0 || context > bn_max_context())
    return set_error(SNF_E_INVALID, "bottleneck: context must be in [0, " + std::to_string(bn_max_context()) + "]");
  if (!h_widths) return set_error(SNF_E_INVALID, "bottleneck: null layer description");
  for (int i = 0; i < 4; ++i)
    if (h_widths[i] < 1 || h_widths[i] > (1 << 20))
      return set_error(SNF_E_INVALID, "bottleneck: layer width " + std::to_string(i) + " out of range");
  if (scratch_bytes < 0) return set_error(SNF_E_INVALID, "bottleneck: scratch_bytes < 0");
  const int span = kBnStackStep * (kBnStack - 1);
  utts->resize(n_utts);
  for (int64_t u = 0; u < n_utts; ++u) {
    const int64_t F = bn_frames(h_soff[u + 1] - h_soff[u]), rows = F + 2 * kBnEdge - 2 * context;
    if (F < 1 || rows < 1)
      return set_error(SNF_E_INVALID, "bottleneck: utterance " + std::to_string(u) + " has " + std::to_string(F) +
                                          " frames, too few for one row at context " + std::to_string(context));
    if (rows <= span)
      return set_error(SNF_E_INVALID, "bottleneck: utterance " + std::to_string(u) + " has " + std::to_string(rows) +
                                          " first-stage rows, the stack needs more than " + std::to_string(span));
    (*utts)[u] = {F, rows, rows - span};
  }
  return SNF_OK;
}

// runs of whole consecutive utterances whose intermediates fit the bound beside the two hidden buffers (an
// utterance that does not fit runs alone): run r is the utterances start[r] .. start[r + 1]
void bn_extract_runs(const std::vector<BnUtt>& utts, const int32_t* h_widths, int64_t scratch_bytes,
                     std::vector<int64_t>* start, int64_t* hidden_rows) {
  const int wmax = std::max(std::max(h_widths[0], h_widths[1]), std::max(h_widths[2], h_widths[3]));
  const int64_t bound = scratch_bytes > 0 ? scratch_bytes : kBnExtractScratch;
  *hidden_rows = bn_hidden_rows(bound, wmax);
  const int64_t room = bound - 2 * *hidden_rows * wmax * 4 - kBnRunPad;
  const int64_t n = static_cast<int64_t>(utts.size());
  start->assign(1, 0);
  int64_t held = 0;
  for (int64_t u = 0; u < n; ++u) {
    const int64_t c = bn_utt_bytes(utts[u]);
    if (u > start->back() && held + c > room) {
      start->push_back(u);
      held = 0;
    }
    held += c;
  }
  if (n > 0) start->push_back(n);
}
}  // namespace

int64_t snf_bottleneck_extract_runs(const int64_t* h_sample_offsets, int64_t n_utts, int32_t context,
                                    const int32_t* h_widths, int64_t scratch_bytes, int64_t* h_run_starts) {
  std::vector<BnUtt> utts;
  int rc = bn_extract_check(h_sample_offsets, n_utts, context, h_widths, scratch_bytes, &utts);
  if (rc) return rc;
  std::vector<int64_t> start;
  int64_t hidden_rows = 0;
  bn_extract_runs(utts, h_widths, scratch_bytes, &start, &hidden_rows);
  if (h_run_starts) std::copy(start.begin(), start.end(), h_run_starts);
  return start.empty() ? 0 : static_cast<int64_t>(start.size()) - 1;
}

int snf_bottleneck_extract(int device_id, const int16_t* d_wave, const int64_t* h_sample_offsets, int64_t n_utts,
                           const float* d_tables, float dither, uint64_t seed, int32_t context, const float* d_basis,
                           const int32_t* h_widths, const void* const* h_params, int32_t bf16, float* d_out,
                           const int64_t* h_out_offsets, int32_t* h_status, int64_t scratch_bytes, void* stream) {
  std::vector<BnUtt> utts;
  int rc = bn_extract_check(h_sample_offsets, n_utts, context, h_widths, scratch_bytes, &utts);
  if (rc) return rc;
  if (!(dither >= 0.0f)) return set_error(SNF_E_INVALID, "bottleneck: dither must be >= 0");
  if (!h_params) return set_error(SNF_E_INVALID, "bottleneck: null layer description");
  for (int i = 0; i < 12; ++i)
    if (!h_params[i]) return set_error(SNF_E_INVALID, "bottleneck: null parameter buffer " + std::to_string(i));
  if (bf16)
    for (int i : {2, 4, 8, 10})
      if (reinterpret_cast<uintptr_t>(h_params[i]) & 15)
        return set_error(SNF_E_INVALID, "bottleneck: packed weights " + std::to_string(i) + " are not 16-byte aligned");
  if (n_utts == 0) return SNF_OK;
  if (!d_wave || !d_tables || !d_basis || !d_out || !h_status) return set_error(SNF_E_INVALID, "bottleneck: null buffer");
  if (reinterpret_cast<uintptr_t>(d_tables) & 7) return set_error(SNF_E_INVALID, "bottleneck: tables are not 8-byte aligned");
  if (!h_out_offsets) return set_error(SNF_E_INVALID, "bottleneck: null output offsets table");
  if (h_out_offsets[0] < 0) return set_error(SNF_E_INVALID, "bottleneck: output offsets must not be negative");
  for (int64_t u = 0; u < n_utts; ++u)
    if (h_out_offsets[u + 1] - h_out_offsets[u] < utts[u].R1)
      return set_error(SNF_E_INVALID, "bottleneck: output offsets leave utterance " + std::to_string(u) +
                                          " fewer than its " + std::to_string(utts[u].R1) + " rows");
  if (h_out_offsets[n_utts] > (int64_t(1) << 40)) return set_error(SNF_E_INVALID, "bottleneck: batch too large");

  std::vector<int64_t> start;
  int64_t hidden_rows = 0;
  bn_extract_runs(utts, h_widths, scratch_bytes, &start, &hidden_rows);
  const int64_t n_runs = static_cast<int64_t>(start.size()) - 1;
  // one table blob: sample offsets | output starts | per run its own frame, first-stage and output offsets from 0
  std::vector<int64_t> tab(h_sample_offsets, h_sample_offsets + n_utts + 1);
  tab.insert(tab.end(), h_out_offsets, h_out_offsets + n_utts + 1);
  std::vector<int64_t> at(n_runs);
  int64_t max_f = 1, max_r0 = 1, max_r1 = 1, max_nu = 1;
  for (int64_t r = 0; r < n_runs; ++r) {
    const int64_t u0 = start[r], nu = start[r + 1] - u0;
    at[r] = static_cast<int64_t>(tab.size());
    tab.resize(tab.size() + 3 * (nu + 1), 0);
    int64_t* foff = tab.data() + at[r];
    int64_t *roff = foff + nu + 1, *ooff = roff + nu + 1;
    for (int64_t u = 0; u < nu; ++u) {
      foff[u + 1] = foff[u] + utts[u0 + u].F;
      roff[u + 1] = roff[u] + utts[u0 + u].R0;
      ooff[u + 1] = ooff[u] + utts[u0 + u].R1;
    }
    max_f = std::max(max_f, foff[nu]);
    max_r0 = std::max(max_r0, roff[nu]);
    max_r1 = std::max(max_r1, ooff[nu]);
    max_nu = std::max(max_nu, nu);
  }
  const int wmax = std::max(std::max(h_widths[0], h_widths[1]), std::max(h_widths[2], h_widths[3]));
  const int64_t chunk = std::min(hidden_rows, (max_r0 + 127) & ~int64_t(127));
  Planless lay;
  auto d_tab = lay.take<int64_t>(tab.size());
  auto d_status = lay.take<int32_t>(n_utts);
  auto mask = lay.take<uint8_t>(max_f);
  auto voiced = lay.take<int32_t>(max_nu);
  auto energy = lay.take<double>(max_f);
  auto logmel = lay.take<float>(kBnMel * max_f);
  auto utt_noise = lay.take<uint32_t>(max_nu);
  auto mean = lay.take<float>(kBnMel * max_nu);
  auto x = lay.take<float>(kBnIn * max_r0);
  auto bn = lay.take<float>(kBnOut * max_r0);
  auto d_map = lay.take<int64_t>(max_r1);
  auto h1 = lay.take<float>(chunk * wmax);
  auto h2 = lay.take<float>(chunk * wmax);
  if ((rc = lay.begin(device_id, stream))) return rc;
  SNF_HIP_CHECK(hipMemcpyAsync(d_tab, tab.data(), sizeof(int64_t) * tab.size(), hipMemcpyHostToDevice, lay.s));
  const int64_t* d_soff = d_tab;
  const int64_t* d_ostart = d_soff + n_utts + 1;
  const void* const* P = h_params;
  auto F = [](const void* p) { return static_cast<const float*>(p); };
  auto hidden = [&](const float* a, int64_t m, int k, int i, int n, int act, float* y) {
    return bf16 ? launch_bn_dense_bf16(a, m, k, static_cast<const uint16_t*>(P[i]), F(P[i + 1]), n, act, y, lay.s)
                : launch_bn_dense(a, m, k, F(P[i]), F(P[i + 1]), n, act, y, nullptr, 0, 0, lay.s);
  };
  for (int64_t r = 0; r < n_runs && !rc; ++r) {
    const int64_t u0 = start[r], nu = start[r + 1] - u0;
    const int64_t* h_ooff = tab.data() + at[r] + 2 * (nu + 1);
    const int64_t* d_foff = d_tab + at[r];
    const int64_t *d_roff = d_foff + nu + 1, *d_ooff = d_roff + nu + 1;
    const int64_t total_f = tab[at[r] + nu], R0 = tab[at[r] + 2 * nu + 1], R1 = h_ooff[nu];
    rc = launch_bn_vad(d_wave, d_soff + u0, d_foff, nu, energy, mask, voiced, lay.s);
    if (!rc)
      rc = launch_bn_fbank(d_wave, d_soff + u0, d_foff, nu, total_f, d_tables, dither, seed, utt_noise, logmel, lay.s);
    if (!rc) rc = launch_bn_nn_input(logmel, mask, voiced, d_foff, d_roff, nu, R0, context, d_basis, mean, x, lay.s);
    if (!rc) rc = launch_bn_row_map(d_roff, d_ooff, nu, R1, d_map, lay.s);
    for (int64_t a = 0; a < R0 && !rc; a += chunk) {
      const int64_t m = std::min(chunk, R0 - a);
      float* xa = x;
      float* ba = bn;
      rc = launch_bn_dense(xa + a * kBnIn, m, kBnIn, F(P[0]), F(P[1]), h_widths[0], 1, h1, nullptr, 0, 0, lay.s);
      if (!rc) rc = hidden(h1, m, h_widths[0], 2, h_widths[1], 1, h2);
      if (!rc) rc = hidden(h2, m, h_widths[1], 4, kBnOut, 0, ba + a * kBnOut);
    }
    int64_t u = 0;   // the utterance of the run that holds the next output row
    for (int64_t a = 0; a < R1 && !rc; a += chunk) {
      const int64_t m = std::min(chunk, R1 - a);
      const int64_t* map = d_map;
      float* h2p = h2;
      rc = launch_bn_dense(bn, m, kBnStack * kBnOut, F(P[6]), F(P[7]), h_widths[2], 1, h1, map + a, kBnOut,
                           kBnStackStep, lay.s);
      if (!rc) rc = hidden(h1, m, h_widths[2], 8, h_widths[3], 1, h2);
      // the last layer writes where the caller wants the rows: one launch per stretch of utterances whose rows
      // follow each other in d_out (a row's value does not depend on the rows beside it)
      for (int64_t p = a; p < a + m && !rc;) {
        while (h_ooff[u + 1] <= p) ++u;
        int64_t dest = h_out_offsets[u0 + u] + (p - h_ooff[u]), v = u, q = std::min(a + m, h_ooff[u + 1]);
        while (q < a + m && h_out_offsets[u0 + v + 1] == h_out_offsets[u0 + v] + utts[u0 + v].R1) {
          ++v;
          q = std::min(a + m, h_ooff[v + 1]);
        }
        rc = hidden(h2p + (p - a) * h_widths[3], q - p, h_widths[3], 10, kBnOut, 0, d_out + dest * kBnOut);
        p = q;
      }
    }
    if (!rc) rc = launch_bn_status(voiced, d_out, d_ostart + u0, d_ooff, nu, static_cast<int32_t*>(d_status) + u0, lay.s);
  }
  if (!rc && hipMemcpyAsync(h_status, d_status, sizeof(int32_t) * n_utts, hipMemcpyDeviceToHost, lay.s) != hipSuccess)
    rc = set_error(SNF_E_HIP, "bottleneck extract: copy of the status failed");
  return lay.finish(rc, "bottleneck extract kernels failed");
}

}  // extern "C"
