// C ABI of libshennong_hip.so (include/shennong_amd.h): DTW cost and path length of pairs of feature items.  Every
// argument is checked on the host before any device is asked for.  The host sorts the pairs by kernel class and,
// within a class, by the cells of their lattice descending (kernels_dtw.hip).  The item and pair tables go up on the
// calling thread's own stream (waited for) into a slot that stays reserved, with the row norms of the call, until
// the kernels, enqueued on the caller's stream, have run - so the call does not wait for the caller's stream.
#include <memory>

#include "plan.h"

using namespace snf;

namespace {

// Device tables and scratch that kernels in flight may still be using: `done` is recorded behind them
struct DtwSlot {
  int device = -1;
  DevBuf items, pairs, aux;
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

}  // namespace

extern "C" {

int snf_dtw_pairs(int device_id, const float* d_rows, int32_t dim, const int64_t* h_item_first,
                  const int32_t* h_item_count, int64_t n_items, const int32_t* h_pairs, int64_t n_pairs,
                  int32_t metric, float* d_cost, int32_t* d_len, void* stream) {
  if (dim < 1 || dim > kDtwMaxDim)
    return set_error(SNF_E_INVALID, "dtw: dim must be in [1, " + std::to_string(kDtwMaxDim) + "]");
  if (metric != SNF_DTW_COSINE && metric != SNF_DTW_SQEUCLIDEAN && metric != SNF_DTW_SYMKL)
    return set_error(SNF_E_INVALID, "dtw: metric must be 0 (cosine), 1 (sqeuclidean) or 2 (symkl)");
  if (n_items < 1 || n_items > 0x7fffffff) return set_error(SNF_E_INVALID, "dtw: number of items out of range");
  if (n_pairs < 0 || n_pairs > 0x7fffffff) return set_error(SNF_E_INVALID, "dtw: number of pairs out of range");
  if (!h_item_first || !h_item_count) return set_error(SNF_E_INVALID, "dtw: null item table");
  std::vector<DtwItem> items(static_cast<size_t>(n_items));
  int64_t row_lo = INT64_MAX, row_hi = 0;
  for (int64_t t = 0; t < n_items; ++t) {
    const int64_t first = h_item_first[t];
    const int32_t count = h_item_count[t];
    if (first < 0 || first > (int64_t(1) << 40))
      return set_error(SNF_E_INVALID, "dtw: item " + std::to_string(t) + " starts outside the block");
    if (count < 1) return set_error(SNF_E_INVALID, "dtw: item " + std::to_string(t) + " has no frames");
    if (count > kDtwMaxFrames)
      return set_error(SNF_E_INVALID, "dtw: item " + std::to_string(t) + " has " + std::to_string(count) +
                                          " frames, the limit is " + std::to_string(kDtwMaxFrames));
    items[t] = {first, count, 0};
    row_lo = std::min(row_lo, first);
    row_hi = std::max(row_hi, first + count);
  }
  if (row_hi - row_lo > 0x7fffffff)
    return set_error(SNF_E_INVALID, "dtw: the items span 2^31 rows or more: compute them in parts");
  if (n_pairs > 0 && !h_pairs) return set_error(SNF_E_INVALID, "dtw: null pair table");
  std::vector<DtwPair> pairs(static_cast<size_t>(n_pairs));
  int64_t class_count[kDtwClasses] = {0, 0, 0};
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int32_t x = h_pairs[2 * p], y = h_pairs[2 * p + 1];
    if (x < 0 || x >= n_items || y < 0 || y >= n_items)
      return set_error(SNF_E_INVALID, "dtw: pair " + std::to_string(p) + " (" + std::to_string(x) + ", " +
                                          std::to_string(y) + ") is out of range for " + std::to_string(n_items) +
                                          " items");
    pairs[p] = {x, y, static_cast<int32_t>(p), items[x].frames * items[y].frames};   // (at most 2^24 cells)
    ++class_count[dtw_class_of(items[y].frames)];
  }
  if (n_pairs == 0) return SNF_OK;
  if (!d_rows || (reinterpret_cast<uintptr_t>(d_rows) & 3))
    return set_error(SNF_E_INVALID, "dtw: d_rows is null or not aligned to float32");
  if (!d_cost || !d_len || (reinterpret_cast<uintptr_t>(d_cost) & 3) || (reinterpret_cast<uintptr_t>(d_len) & 3))
    return set_error(SNF_E_INVALID, "dtw: d_cost or d_len is null or not 4-byte aligned");
  // by class, within a class the largest lattice first, equal ones in the caller's order: a stable radix sort of
  // the 27-bit key (class, 2^24 - cells), 9 bits a pass (a million pairs: milliseconds, where std::sort with a
  // comparator that looks the items up takes a tenth of a second)
  {
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
      for (const int64_t end = p + class_count[c]; p < end; ++p)
        if (dtw_class_of(items[pairs[p].y].frames) != c)
          return set_error(SNF_E_RUNTIME, "dtw: internal error, the pairs are not sorted by class");
  }
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
  int rc = slot->items.upload(items, mine->stream);
  if (!rc) rc = slot->pairs.upload(pairs, mine->stream);
  // (symkl: the log block of the row range too; a failed allocation ends the call before any kernel)
  if (!rc) rc = slot->aux.ensure(sizeof(float) * dtw_aux_floats(row_hi - row_lo, dim, metric));
  if (!rc)
    rc = launch_dtw_pairs(d_rows, dim, slot->items.as<DtwItem>(), slot->pairs.as<DtwPair>(), class_count, row_lo,
                          row_hi, slot->aux.as<float>(), metric, compute_units, d_cost, d_len, s);
  if (!rc && hipEventRecord(slot->done, s) != hipSuccess) rc = set_error(SNF_E_HIP, "dtw: hipEventRecord failed");
  if (rc) {
    // (whatever was enqueued has finished before the slot's tables can be written again)
    (void)hipStreamSynchronize(s);
    give_slot(slot);
    return rc;
  }
  give_slot(slot);   // (free for the next call once `done` has completed: take_slot asks the event)
  if (!stream && hipStreamSynchronize(s) != hipSuccess) return set_error(SNF_E_HIP, "dtw kernel failed");
  return SNF_OK;
}

}  // extern "C"
