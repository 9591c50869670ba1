// C ABI of libshennong_hip.so (include/shennong_amd.h): DTW cost and path length of pairs of feature items
// (snf_dtw_pairs), subsequence DTW search of queries in targets (snf_dtw_search), several detections per such pair
// (snf_dtw_detect) and the best few detections per query (snf_dtw_topk).  Every argument is checked on
// the host before any device is asked for.  The host sorts the pairs by kernel class and, within a class, by the
// cells of their lattice descending (kernels_dtw.hip).  The item and pair tables go up on the calling thread's own
// stream (waited for) into a slot that stays reserved, with the row norms of the call, until the kernels, enqueued
// on the caller's stream, have run - so the call does not wait for the caller's stream.  The pair calls share the
// checks of the tables (check_tables), the sort (sort_pairs) and the slot protocol (enqueue); search and detection
// also the checks of the curves (check_curves).  snf_dtw_topk has group tables in the place of the item and pair
// tables and keeps them in a slot in the same way.
#include <algorithm>
#include <memory>

#include "plan.h"

using namespace snf;

namespace {

// Device tables and scratch that kernels in flight may still be using: `done` is recorded behind them
struct DtwSlot {
  int device = -1;
  DevBuf items, pairs, aux, curves;   // (curves: the curve offsets of a search, in the caller's pair order)
  DevBuf record_first, records;       // (snf_dtw_align: the first record of every sorted pair; the records)
  hipEvent_t done = nullptr;
  bool taken = false;   // between take_slot and the event's record (or the failure that gives it back)
};

std::mutex g_mu;
// (never destroyed: a DevBuf released after the runtime has shut down would call into it)
auto* g_slots = new std::vector<std::unique_ptr<DtwSlot>>;

DtwSlot* take_slot(int device_id) {
  std::lock_guard<std::mutex> lock(g_mu);
  for (auto& slot : *g_slots)
    if (slot->device == device_id && !slot->taken && hipEventQuery(slot->done) == hipSuccess) {
      slot->taken = true;
      return slot.get();
    }
  std::unique_ptr<DtwSlot> fresh(new DtwSlot);
  fresh->device = device_id;
  if (hipEventCreateWithFlags(&fresh->done, hipEventDisableTiming) != hipSuccess) {
    set_error(SNF_E_HIP, "hipEventCreate failed");
    return nullptr;
  }
  fresh->taken = true;
  g_slots->push_back(std::move(fresh));
  return g_slots->back().get();
}

void give_slot(DtwSlot* slot) {
  std::lock_guard<std::mutex> lock(g_mu);
  slot->taken = false;
}

// The host tables of a call, checked
struct DtwTables {
  std::vector<DtwItem> items;
  std::vector<DtwPair> pairs;   // x gives the rows of the lattice, y its columns: the class of the pair
  int64_t class_count[kDtwClasses] = {0, 0, 0};
  int64_t row_lo = INT64_MAX, row_hi = 0;
};

// `who`: the prefix of the messages ("dtw", "dtw_search")
int check_tables(const std::string& who, int32_t dim, int32_t metric, const int64_t* h_item_first,
                 const int32_t* h_item_count, int64_t n_items, const int32_t* h_pairs, int64_t n_pairs,
                 DtwTables& t) {
  if (dim < 1 || dim > kDtwMaxDim)
    return set_error(SNF_E_INVALID, who + ": dim must be in [1, " + std::to_string(kDtwMaxDim) + "]");
  if (metric != SNF_DTW_COSINE && metric != SNF_DTW_SQEUCLIDEAN && metric != SNF_DTW_SYMKL)
    return set_error(SNF_E_INVALID, who + ": metric must be 0 (cosine), 1 (sqeuclidean) or 2 (symkl)");
  if (n_items < 1 || n_items > 0x7fffffff) return set_error(SNF_E_INVALID, who + ": number of items out of range");
  if (n_pairs < 0 || n_pairs > 0x7fffffff) return set_error(SNF_E_INVALID, who + ": number of pairs out of range");
  if (!h_item_first || !h_item_count) return set_error(SNF_E_INVALID, who + ": null item table");
  t.items.resize(static_cast<size_t>(n_items));
  for (int64_t k = 0; k < n_items; ++k) {
    const int64_t first = h_item_first[k];
    const int32_t count = h_item_count[k];
    if (first < 0 || first > (int64_t(1) << 40))
      return set_error(SNF_E_INVALID, who + ": item " + std::to_string(k) + " starts outside the block");
    if (count < 1) return set_error(SNF_E_INVALID, who + ": item " + std::to_string(k) + " has no frames");
    if (count > kDtwMaxFrames)
      return set_error(SNF_E_INVALID, who + ": item " + std::to_string(k) + " has " + std::to_string(count) +
                                          " frames, the limit is " + std::to_string(kDtwMaxFrames));
    t.items[k] = {first, count, 0};
    t.row_lo = std::min(t.row_lo, first);
    t.row_hi = std::max(t.row_hi, first + count);
  }
  if (t.row_hi - t.row_lo > 0x7fffffff)
    return set_error(SNF_E_INVALID, who + ": the items span 2^31 rows or more: compute them in parts");
  if (n_pairs > 0 && !h_pairs) return set_error(SNF_E_INVALID, who + ": null pair table");
  t.pairs.resize(static_cast<size_t>(n_pairs));
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int32_t x = h_pairs[2 * p], y = h_pairs[2 * p + 1];
    if (x < 0 || x >= n_items || y < 0 || y >= n_items)
      return set_error(SNF_E_INVALID, who + ": pair " + std::to_string(p) + " (" + std::to_string(x) + ", " +
                                          std::to_string(y) + ") is out of range for " + std::to_string(n_items) +
                                          " items");
    t.pairs[p] = {x, y, static_cast<int32_t>(p), t.items[x].frames * t.items[y].frames};   // (at most 2^24 cells)
    ++t.class_count[dtw_class_of(t.items[y].frames)];
  }
  return SNF_OK;
}

// by class, within a class the largest lattice first, equal ones in the caller's order: a stable radix sort of
// the 27-bit key (class, 2^24 - cells), 9 bits a pass (a million pairs: milliseconds, where std::sort with a
// comparator that looks the items up takes a tenth of a second)
int sort_pairs(const std::string& who, DtwTables& t) {
  std::vector<DtwPair>& pairs = t.pairs;
  const std::vector<DtwItem>& items = t.items;
  const uint32_t top = uint32_t(kDtwMaxFrames) * kDtwMaxFrames;
  auto key_of = [&](const DtwPair& p) {
    return (uint32_t(dtw_class_of(items[p.y].frames)) << 25) | (top - uint32_t(p.cells));
  };
  std::vector<uint32_t> keys(pairs.size()), keys_next(pairs.size());
  for (size_t p = 0; p < pairs.size(); ++p) keys[p] = key_of(pairs[p]);
  std::vector<DtwPair> next(pairs.size());
  for (int shift = 0; shift < 27; shift += 9) {
    size_t start[513] = {0};
    for (uint32_t k : keys) ++start[((k >> shift) & 511) + 1];
    for (int b = 0; b < 512; ++b) start[b + 1] += start[b];
    for (size_t p = 0; p < pairs.size(); ++p) {
      const size_t to = start[(keys[p] >> shift) & 511]++;
      next[to] = pairs[p];
      keys_next[to] = keys[p];
    }
    pairs.swap(next);
    keys.swap(keys_next);
  }
  // (a kernel class sizes its seam row by the class: no pair may sit in another class's stretch)
  int64_t p = 0;
  for (int c = 0; c < kDtwClasses; ++c)
    for (const int64_t end = p + t.class_count[c]; p < end; ++p)
      if (dtw_class_of(items[pairs[p].y].frames) != c)
        return set_error(SNF_E_RUNTIME, who + ": internal error, the pairs are not sorted by class");
  return SNF_OK;
}

// The records of an alignment are bounded by the caller's scratch_bytes: no head-room, as DevBuf::ensure adds
int ensure_exactly(DevBuf& buf, size_t bytes) {
  if (bytes <= buf.cap) return SNF_OK;
  if (buf.p) (void)hipFree(buf.p);
  buf.p = nullptr;
  buf.cap = 0;
  SNF_HIP_CHECK(malloc_with_hook(&buf.p, bytes));
  buf.cap = bytes;
  return SNF_OK;
}

// Takes a slot, uploads the tables (and `curve_first`, the curve offsets of a search or the path offsets of an
// alignment, where given; `record_first` and `record_bytes` of records, where given: snf_dtw_align), sizes the aux
// block and calls `launch(slot, compute_units, stream)`, which enqueues the kernels; records the slot's event behind
// them
template <class Launch>
int enqueue(const std::string& who, int device_id, void* stream, const DtwTables& t, int32_t dim, int32_t metric,
            const std::vector<int64_t>* curve_first, const std::vector<int64_t>* record_first, size_t record_bytes,
            Launch&& launch) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_error(SNF_E_NODEVICE, "no HIP device visible: libshennong_hip needs an MI355X (gfx950)");
  if (device_id < 0 || device_id >= ndev) return set_error(SNF_E_INVALID, "bad device id");

  SNF_HIP_CHECK(hipSetDevice(device_id));
  int compute_units = 0;
  SNF_HIP_CHECK(hipDeviceGetAttribute(&compute_units, hipDeviceAttributeMultiprocessorCount, device_id));
  if (compute_units < 1) compute_units = 1;
  ThreadScratch* mine = thread_scratch(device_id);
  if (!mine) return SNF_E_HIP;
  DtwSlot* slot = take_slot(device_id);
  if (!slot) return SNF_E_HIP;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : mine->stream;
  // (DevBuf::upload waits for the copy on the thread's own stream: the tables are pageable vectors that go away)
  int rc = slot->items.upload(t.items, mine->stream);
  if (!rc) rc = slot->pairs.upload(t.pairs, mine->stream);
  if (!rc && curve_first) rc = slot->curves.upload(*curve_first, mine->stream);
  if (!rc && record_first) rc = slot->record_first.upload(*record_first, mine->stream);
  if (!rc && record_bytes) rc = ensure_exactly(slot->records, record_bytes);
  // (symkl: the log block of the row range too; a failed allocation ends the call before any kernel)
  if (!rc) rc = slot->aux.ensure(sizeof(float) * dtw_aux_floats(t.row_hi - t.row_lo, dim, metric));
  if (!rc) rc = launch(*slot, compute_units, s);
  if (!rc && hipEventRecord(slot->done, s) != hipSuccess)
    rc = set_error(SNF_E_HIP, who + ": hipEventRecord failed");
  if (rc) {
    // (whatever was enqueued has finished before the slot's tables can be written again)
    (void)hipStreamSynchronize(s);
    give_slot(slot);
    return rc;
  }
  give_slot(slot);   // (free for the next call once `done` has completed: take_slot asks the event)
  if (!stream && hipStreamSynchronize(s) != hipSuccess) return set_error(SNF_E_HIP, who + " kernel failed");
  return SNF_OK;
}

bool bad_word_pointer(const void* p) { return !p || (reinterpret_cast<uintptr_t>(p) & 3); }

// The curves of a search or a detection: pair p owns the elements [first, first + M) of the three curve arrays,
// inside [0, 2^31), and no two overlap
int check_curves(const std::string& who, const DtwTables& t, const int32_t* h_pairs, int64_t n_pairs,
                 const int64_t* h_curve_first, const float* d_curve_cost, const int32_t* d_curve_len,
                 const int32_t* d_curve_start, std::vector<int64_t>& curve_first) {
  if (bad_word_pointer(d_curve_cost) || bad_word_pointer(d_curve_len) || bad_word_pointer(d_curve_start))
    return set_error(SNF_E_INVALID, who + ": a curve array is not 4-byte aligned");
  curve_first.assign(h_curve_first, h_curve_first + n_pairs);
  std::vector<std::pair<int64_t, int32_t>> stretch(static_cast<size_t>(n_pairs));   // (first, pair)
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int64_t first = curve_first[p], columns = t.items[h_pairs[2 * p + 1]].frames;
    if (first < 0 || first + columns > (int64_t(1) << 31))
      return set_error(SNF_E_INVALID, who + ": the curve of pair " + std::to_string(p) + " (" +
                                          std::to_string(columns) + " elements at " + std::to_string(first) +
                                          ") lies outside [0, 2^31)");
    stretch[p] = {first, static_cast<int32_t>(p)};
  }
  std::sort(stretch.begin(), stretch.end());
  for (int64_t k = 0; k + 1 < n_pairs; ++k) {
    const int32_t a = stretch[k].second, b = stretch[k + 1].second;
    if (stretch[k].first + t.items[h_pairs[2 * a + 1]].frames > stretch[k + 1].first)
      return set_error(SNF_E_INVALID, who + ": the curves of the pairs " + std::to_string(std::min(a, b)) +
                                          " and " + std::to_string(std::max(a, b)) + " overlap");
  }
  return SNF_OK;
}

}  // namespace

extern "C" {

int snf_dtw_pairs(int device_id, const float* d_rows, int32_t dim, const int64_t* h_item_first,
                  const int32_t* h_item_count, int64_t n_items, const int32_t* h_pairs, int64_t n_pairs,
                  int32_t metric, float* d_cost, int32_t* d_len, void* stream) {
  const std::string who = "dtw";
  DtwTables t;
  if (const int rc = check_tables(who, dim, metric, h_item_first, h_item_count, n_items, h_pairs, n_pairs, t))
    return rc;
  if (n_pairs == 0) return SNF_OK;
  if (bad_word_pointer(d_rows)) return set_error(SNF_E_INVALID, "dtw: d_rows is null or not aligned to float32");
  if (bad_word_pointer(d_cost) || bad_word_pointer(d_len))
    return set_error(SNF_E_INVALID, "dtw: d_cost or d_len is null or not 4-byte aligned");
  if (const int rc = sort_pairs(who, t)) return rc;
  return enqueue(who, device_id, stream, t, dim, metric, nullptr, nullptr, 0, [&](DtwSlot& slot, int compute_units, hipStream_t s) {
    return launch_dtw_pairs(d_rows, dim, slot.items.as<DtwItem>(), slot.pairs.as<DtwPair>(), t.class_count, t.row_lo,
                            t.row_hi, slot.aux.as<float>(), metric, compute_units, d_cost, d_len, s);
  });
}

int snf_dtw_search(int device_id, const float* d_rows, int32_t dim, const int64_t* h_item_first,
                   const int32_t* h_item_count, int64_t n_items, const int32_t* h_pairs, int64_t n_pairs,
                   int32_t metric, int32_t normalized, float* d_cost, int32_t* d_len, int32_t* d_start,
                   int32_t* d_end, const int64_t* h_curve_first, float* d_curve_cost, int32_t* d_curve_len,
                   int32_t* d_curve_start, void* stream) {
  const std::string who = "dtw_search";
  DtwTables t;
  if (const int rc = check_tables(who, dim, metric, h_item_first, h_item_count, n_items, h_pairs, n_pairs, t))
    return rc;
  if (normalized != 0 && normalized != 1) return set_error(SNF_E_INVALID, who + ": normalized must be 0 or 1");
  const int curve_pointers = (h_curve_first != nullptr) + (d_curve_cost != nullptr) + (d_curve_len != nullptr) +
                             (d_curve_start != nullptr);
  if (curve_pointers != 0 && curve_pointers != 4)
    return set_error(SNF_E_INVALID, who + ": the curve pointers must be all set or all null");
  if (n_pairs == 0) return SNF_OK;
  if (bad_word_pointer(d_rows))
    return set_error(SNF_E_INVALID, who + ": d_rows is null or not aligned to float32");
  if (bad_word_pointer(d_cost) || bad_word_pointer(d_len) || bad_word_pointer(d_start) || bad_word_pointer(d_end))
    return set_error(SNF_E_INVALID, who + ": d_cost, d_len, d_start or d_end is null or not 4-byte aligned");
  std::vector<int64_t> curve_first;
  if (curve_pointers)
    if (const int rc = check_curves(who, t, h_pairs, n_pairs, h_curve_first, d_curve_cost, d_curve_len, d_curve_start,
                                    curve_first))
      return rc;
  if (const int rc = sort_pairs(who, t)) return rc;
  return enqueue(who, device_id, stream, t, dim, metric, curve_pointers ? &curve_first : nullptr, nullptr, 0,
                 [&](DtwSlot& slot, int compute_units, hipStream_t s) {
                   const DtwSearchOut out = {d_cost, d_len, d_start, d_end,
                                             curve_pointers ? slot.curves.as<int64_t>() : nullptr,
                                             d_curve_cost, d_curve_len, d_curve_start};
                   return launch_dtw_search(d_rows, dim, slot.items.as<DtwItem>(), slot.pairs.as<DtwPair>(),
                                            t.class_count, t.row_lo, t.row_hi, slot.aux.as<float>(), metric,
                                            normalized, compute_units, out, s);
                 });
}

int snf_dtw_detect(int device_id, const float* d_rows, int32_t dim, const int64_t* h_item_first,
                   const int32_t* h_item_count, int64_t n_items, const int32_t* h_pairs, int64_t n_pairs,
                   int32_t metric, int32_t normalized, int32_t max_detections, float max_score, int32_t* d_count,
                   float* d_cost, int32_t* d_len, int32_t* d_start, int32_t* d_end, const int64_t* h_curve_first,
                   float* d_curve_cost, int32_t* d_curve_len, int32_t* d_curve_start, void* stream) {
  const std::string who = "dtw_detect";
  DtwTables t;
  if (const int rc = check_tables(who, dim, metric, h_item_first, h_item_count, n_items, h_pairs, n_pairs, t))
    return rc;
  if (normalized != 0 && normalized != 1) return set_error(SNF_E_INVALID, who + ": normalized must be 0 or 1");
  if (max_detections < 1 || max_detections > kDtwMaxDetections)
    return set_error(SNF_E_INVALID, who + ": max_detections must be in [1, " + std::to_string(kDtwMaxDetections) +
                                        "], not " + std::to_string(max_detections));
  if (max_score != max_score) return set_error(SNF_E_INVALID, who + ": max_score is not a number");
  const int curve_pointers = (h_curve_first != nullptr) + (d_curve_cost != nullptr) + (d_curve_len != nullptr) +
                             (d_curve_start != nullptr);
  if (curve_pointers != 0 && curve_pointers != 4)
    return set_error(SNF_E_INVALID, who + ": the curve pointers must be all set or all null");
  if (n_pairs == 0) return SNF_OK;
  if (bad_word_pointer(d_rows))
    return set_error(SNF_E_INVALID, who + ": d_rows is null or not aligned to float32");
  if (bad_word_pointer(d_count) || bad_word_pointer(d_cost) || bad_word_pointer(d_len) || bad_word_pointer(d_start) ||
      bad_word_pointer(d_end))
    return set_error(SNF_E_INVALID,
                     who + ": d_count, d_cost, d_len, d_start or d_end is null or not 4-byte aligned");
  std::vector<int64_t> curve_first;
  if (curve_pointers)
    if (const int rc = check_curves(who, t, h_pairs, n_pairs, h_curve_first, d_curve_cost, d_curve_len, d_curve_start,
                                    curve_first))
      return rc;
  if (const int rc = sort_pairs(who, t)) return rc;
  return enqueue(who, device_id, stream, t, dim, metric, curve_pointers ? &curve_first : nullptr, nullptr, 0,
                 [&](DtwSlot& slot, int compute_units, hipStream_t s) {
                   const DtwDetectOut out = {d_count, d_cost, d_len, d_start, d_end, max_detections, max_score,
                                             curve_pointers ? slot.curves.as<int64_t>() : nullptr,
                                             d_curve_cost, d_curve_len, d_curve_start};
                   return launch_dtw_detect(d_rows, dim, slot.items.as<DtwItem>(), slot.pairs.as<DtwPair>(),
                                            t.class_count, t.row_lo, t.row_hi, slot.aux.as<float>(), metric,
                                            normalized, compute_units, out, s);
                 });
}

int snf_dtw_align(int device_id, const float* d_rows, int32_t dim, const int64_t* h_item_first,
                  const int32_t* h_item_count, int64_t n_items, const int32_t* h_pairs, int64_t n_pairs,
                  int32_t metric, int32_t mode, int32_t normalized, int32_t max_detections, float max_score,
                  int32_t* d_count, float* d_cost, int32_t* d_len, int32_t* d_start, int32_t* d_end,
                  const int64_t* h_path_first, int32_t* d_path_x, int32_t* d_path_y, int64_t scratch_bytes,
                  void* stream) {
  const std::string who = "dtw_align";
  DtwTables t;
  if (const int rc = check_tables(who, dim, metric, h_item_first, h_item_count, n_items, h_pairs, n_pairs, t))
    return rc;
  if (mode != SNF_DTW_ALIGN_GLOBAL && mode != SNF_DTW_ALIGN_SUBSEQUENCE)
    return set_error(SNF_E_INVALID, who + ": mode must be 0 (global) or 1 (subsequence), not " + std::to_string(mode));
  const bool subsequence = mode == SNF_DTW_ALIGN_SUBSEQUENCE;
  if (subsequence) {
    if (normalized != 0 && normalized != 1) return set_error(SNF_E_INVALID, who + ": normalized must be 0 or 1");
    if (max_detections < 1 || max_detections > kDtwMaxDetections)
      return set_error(SNF_E_INVALID, who + ": max_detections must be in [1, " + std::to_string(kDtwMaxDetections) +
                                          "], not " + std::to_string(max_detections));
    if (max_score != max_score) return set_error(SNF_E_INVALID, who + ": max_score is not a number");
  }
  if (scratch_bytes < 0) return set_error(SNF_E_INVALID, who + ": scratch_bytes is negative");
  if (n_pairs == 0) return SNF_OK;
  const int64_t k = subsequence ? max_detections : 1;
  if (bad_word_pointer(d_rows))
    return set_error(SNF_E_INVALID, who + ": d_rows is null or not aligned to float32");
  if (bad_word_pointer(d_cost) || bad_word_pointer(d_len))
    return set_error(SNF_E_INVALID, who + ": d_cost or d_len is null or not 4-byte aligned");
  if (subsequence && (bad_word_pointer(d_count) || bad_word_pointer(d_start) || bad_word_pointer(d_end)))
    return set_error(SNF_E_INVALID, who + ": d_count, d_start or d_end is null or not 4-byte aligned");
  if (!h_path_first) return set_error(SNF_E_INVALID, who + ": null path table");
  if (bad_word_pointer(d_path_x) || bad_word_pointer(d_path_y))
    return set_error(SNF_E_INVALID, who + ": d_path_x or d_path_y is null or not 4-byte aligned");
  // the paths: slot p k + r owns [first, first + N + M - 1), inside [0, 2^31), and no two overlap
  std::vector<int64_t> path_first(h_path_first, h_path_first + n_pairs * k);
  {
    auto room = [&](int64_t slot) {
      const int64_t p = slot / k;
      return int64_t(t.items[h_pairs[2 * p]].frames) + t.items[h_pairs[2 * p + 1]].frames - 1;
    };
    std::vector<std::pair<int64_t, int64_t>> stretch(path_first.size());   // (first, slot)
    bool ascending = true;   // (one stretch behind the other in the order of the slots: nothing to sort)
    for (int64_t s = 0; s < n_pairs * k; ++s) {
      if (s > 0 && path_first[s - 1] + room(s - 1) > path_first[s]) ascending = false;
      if (path_first[s] < 0 || path_first[s] + room(s) > (int64_t(1) << 31))
        return set_error(SNF_E_INVALID, who + ": the path of pair " + std::to_string(s / k) + ", slot " +
                                            std::to_string(s % k) + " (" + std::to_string(room(s)) + " elements at " +
                                            std::to_string(path_first[s]) + ") lies outside [0, 2^31)");
      stretch[s] = {path_first[s], s};
    }
    if (!ascending) std::sort(stretch.begin(), stretch.end());
    for (size_t s = 0; !ascending && s + 1 < stretch.size(); ++s)
      if (stretch[s].first + room(stretch[s].second) > stretch[s + 1].first) {
        const int64_t a = std::min(stretch[s].second, stretch[s + 1].second);
        const int64_t b = std::max(stretch[s].second, stretch[s + 1].second);
        return set_error(SNF_E_INVALID, who + ": the paths of pair " + std::to_string(a / k) + ", slot " +
                                            std::to_string(a % k) + " and pair " + std::to_string(b / k) + ", slot " +
                                            std::to_string(b % k) + " overlap");
      }
  }
  if (const int rc = sort_pairs(who, t)) return rc;
  // The records: the sorted pairs are walked in runs whose records fit the scratch; `record_first` counts from the
  // start of a pair's run
  const int64_t scratch = scratch_bytes ? scratch_bytes : kDtwDefaultScratch;
  std::vector<int64_t> record_first(t.pairs.size());
  std::vector<int64_t> run_first = {0};   // the first pair of every run, and P
  int64_t largest = 0, fill = 0, most = 0;
  for (size_t p = 0; p < t.pairs.size(); ++p) {
    const int64_t need = dtw_record_count(t.items[t.pairs[p].x].frames, t.items[t.pairs[p].y].frames);
    largest = std::max(largest, need);
    if ((fill + need) * kDtwRecordBytes > scratch && fill > 0) {
      run_first.push_back(static_cast<int64_t>(p));
      fill = 0;
    }
    record_first[p] = fill;
    fill += need;
    most = std::max(most, fill);
  }
  run_first.push_back(n_pairs);
  if (largest * kDtwRecordBytes > scratch)
    return set_error(SNF_E_INVALID, who + ": scratch_bytes " + std::to_string(scratch) + " is below the " +
                                        std::to_string(largest * kDtwRecordBytes) +
                                        " bytes of records of the largest pair");
  return enqueue(
      who, device_id, stream, t, dim, metric, &path_first, &record_first, static_cast<size_t>(most * kDtwRecordBytes),
      [&](DtwSlot& slot, int compute_units, hipStream_t s) {
        if (const int rc = launch_dtw_rows(d_rows, dim, t.row_lo, t.row_hi, slot.aux.as<float>(), metric, s))
          return rc;
        const DtwDetectOut out = {d_count,   d_cost, d_len,   d_start, d_end, static_cast<int32_t>(k),
                                  max_score, nullptr, nullptr, nullptr, nullptr};
        const DtwPaths paths = {slot.curves.as<int64_t>(), d_path_x, d_path_y};
        for (size_t r = 0; r + 1 < run_first.size(); ++r) {
          // the pairs [lo, hi) of the run, by class: the classes lie one behind the other in the sorted pairs
          const int64_t lo = run_first[r], hi = run_first[r + 1];
          int64_t run_count[kDtwClasses], class_lo = 0;
          for (int c = 0; c < kDtwClasses; ++c) {
            const int64_t class_hi = class_lo + t.class_count[c];
            run_count[c] = std::max<int64_t>(std::min(hi, class_hi) - std::max(lo, class_lo), 0);
            class_lo = class_hi;
          }
          const DtwRecords records = {slot.records.as<uint4>(), slot.record_first.as<int64_t>() + lo};
          if (const int rc = launch_dtw_align(d_rows, dim, slot.items.as<DtwItem>(), slot.pairs.as<DtwPair>() + lo,
                                              run_count, t.row_lo, slot.aux.as<float>(), metric, subsequence,
                                              normalized, compute_units, out, records, paths, s))
            return rc;
        }
        return static_cast<int>(SNF_OK);
      });
}

int snf_dtw_topk(int device_id, const int32_t* d_count, const float* d_cost, const int32_t* d_len,
                 const int32_t* d_start, const int32_t* d_end, int64_t n_pairs, int32_t max_detections,
                 int32_t normalized, const int32_t* h_group_pairs, const int64_t* h_group_first, int64_t n_queries,
                 int32_t top_k, int32_t* d_top_count, int32_t* d_top_pair, int32_t* d_top_rank, float* d_top_cost,
                 int32_t* d_top_len, int32_t* d_top_start, int32_t* d_top_end, void* stream) {
  const std::string who = "dtw_topk";
  if (n_pairs < 0 || n_pairs > 0x7fffffff) return set_error(SNF_E_INVALID, who + ": number of pairs out of range");
  if (n_queries < 0 || n_queries > 0x7fffffff)
    return set_error(SNF_E_INVALID, who + ": number of queries out of range");
  if (max_detections < 1 || max_detections > kDtwMaxDetections)
    return set_error(SNF_E_INVALID, who + ": max_detections must be in [1, " + std::to_string(kDtwMaxDetections) +
                                        "], not " + std::to_string(max_detections));
  if (normalized != 0 && normalized != 1) return set_error(SNF_E_INVALID, who + ": normalized must be 0 or 1");
  if (top_k < 1 || top_k > kDtwMaxTopk)
    return set_error(SNF_E_INVALID, who + ": top_k must be in [1, " + std::to_string(kDtwMaxTopk) + "], not " +
                                        std::to_string(top_k));
  if (n_queries == 0) return SNF_OK;
  if (!h_group_first) return set_error(SNF_E_INVALID, who + ": null group table");
  if (h_group_first[0] != 0) return set_error(SNF_E_INVALID, who + ": the first group must start at 0");
  for (int64_t q = 0; q < n_queries; ++q)
    if (h_group_first[q + 1] < h_group_first[q] || h_group_first[q + 1] > 0x7fffffff)
      return set_error(SNF_E_INVALID, who + ": the group of query " + std::to_string(q) + " ends before it starts" +
                                          " or beyond 2^31 - 1");
  const int64_t grouped = h_group_first[n_queries];
  if (grouped > 0 && !h_group_pairs) return set_error(SNF_E_INVALID, who + ": null group table");
  for (int64_t g = 0; g < grouped; ++g)
    if (h_group_pairs[g] < 0 || h_group_pairs[g] >= n_pairs)
      return set_error(SNF_E_INVALID, who + ": grouped pair " + std::to_string(g) + " (" +
                                          std::to_string(h_group_pairs[g]) + ") is out of range for " +
                                          std::to_string(n_pairs) + " pairs");
  if (grouped > 0 && (bad_word_pointer(d_count) || bad_word_pointer(d_cost) || bad_word_pointer(d_len) ||
                      bad_word_pointer(d_start) || bad_word_pointer(d_end)))
    return set_error(SNF_E_INVALID,
                     who + ": d_count, d_cost, d_len, d_start or d_end is null or not 4-byte aligned");
  if (bad_word_pointer(d_top_count) || bad_word_pointer(d_top_pair) || bad_word_pointer(d_top_rank) ||
      bad_word_pointer(d_top_cost) || bad_word_pointer(d_top_len) || bad_word_pointer(d_top_start) ||
      bad_word_pointer(d_top_end))
    return set_error(SNF_E_INVALID, who + ": an output array is null or not 4-byte aligned");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_error(SNF_E_NODEVICE, "no HIP device visible: libshennong_hip needs an MI355X (gfx950)");
  if (device_id < 0 || device_id >= ndev) return set_error(SNF_E_INVALID, "bad device id");
  SNF_HIP_CHECK(hipSetDevice(device_id));
  ThreadScratch* mine = thread_scratch(device_id);
  if (!mine) return SNF_E_HIP;
  DtwSlot* slot = take_slot(device_id);
  if (!slot) return SNF_E_HIP;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : mine->stream;
  // (the group tables take the place of the item and pair tables in the slot)
  const std::vector<int32_t> group_pairs(h_group_pairs, h_group_pairs + grouped);
  const std::vector<int64_t> group_first(h_group_first, h_group_first + n_queries + 1);
  int rc = slot->items.upload(group_pairs, mine->stream);
  if (!rc) rc = slot->pairs.upload(group_first, mine->stream);
  if (!rc) {
    const DtwTopkIn in = {d_count, d_cost, d_len, d_start, d_end, max_detections, slot->items.as<int32_t>(),
                          slot->pairs.as<int64_t>()};
    const DtwTopkOut out = {d_top_count, d_top_pair, d_top_rank, d_top_cost, d_top_len, d_top_start, d_top_end};
    rc = launch_dtw_topk(in, n_queries, top_k, normalized, out, s);
  }
  if (!rc && hipEventRecord(slot->done, s) != hipSuccess) rc = set_error(SNF_E_HIP, who + ": hipEventRecord failed");
  if (rc) {
    (void)hipStreamSynchronize(s);
    give_slot(slot);
    return rc;
  }
  give_slot(slot);
  if (!stream && hipStreamSynchronize(s) != hipSuccess) return set_error(SNF_E_HIP, who + " kernel failed");
  return SNF_OK;
}

}  // extern "C"
