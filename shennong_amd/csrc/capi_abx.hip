// C ABI of libshennong_hip.so (include/shennong_amd.h): ABX triplet counts per cell over a table of distances
// that lies in HBM.  Every argument and every cell record is checked on the host before any device is asked for.
// The host sorts the cells by their work nA nB nX: those at or below kSmallWork go, one lane each, to
// abx_small_kernel; the others become wave units, cut over x into stretches of about kSplitWork compares when their
// work exceeds it, sorted by work descending (kernels_abx.hip).  The tables go up on the calling thread's own
// stream (waited for) into a slot that stays reserved until the kernels, enqueued on the caller's stream, have
// run - so the call does not wait for the caller's stream.
#include <stdlib.h>

#include <algorithm>
#include <memory>

#include "plan.h"

using namespace snf;

namespace {

// Both thresholds are measured on an MI355X, kernel durations from a rocprofv3 dispatch trace (tools/time_abx.py
// --sweep and --trace, profiles/abx_timing.jsonl): 200 000 cells of k^3 compares take a lane each
// 0.399 ms and a wave each 0.460 ms at k = 7, 0.579 and 0.519 ms at k = 8 - the two lines cross near 430 compares;
// 64 cells of 256^3 compares take 0.188 / 0.150 / 0.275 / 1.00 ms cut into stretches of 2^16 / 2^18 / 2^20 / 2^22
// compares and 3.96 ms whole.  SNF_ABX_SMALL_WORK and SNF_ABX_SPLIT_WORK in the environment replace them, for
// that measurement.
constexpr int64_t kSmallWork = 384;          // cells of at most this many compares: one lane each
constexpr int64_t kSplitWork = 1 << 18;      // cells above it are cut into stretches of x of about this work
constexpr int64_t kMaxTriplets = int64_t(1) << 62;

int64_t threshold(const char* name, int64_t fallback) {
  const char* text = getenv(name);
  if (!text || !*text) return fallback;
  char* end = nullptr;
  const long long v = strtoll(text, &end, 10);
  // (at most kMaxTriplets, the largest work of a cell: sums of the two stay below 2^63)
  return (end && !*end && v >= 0) ? std::min(static_cast<int64_t>(v), kMaxTriplets) : fallback;
}

// Device tables that kernels in flight may still be using: `done` is recorded behind them
struct AbxSlot {
  int device = -1;
  DevBuf cells, small, units;
  hipEvent_t done = nullptr;
  bool taken = false;   // between take_slot and the event's record (or the failure that gives it back)
};

std::mutex g_mu;
// (never destroyed: a DevBuf released after the runtime has shut down would call into it)
auto* g_slots = new std::vector<std::unique_ptr<AbxSlot>>;

AbxSlot* take_slot(int device_id) {
  std::lock_guard<std::mutex> lock(g_mu);
  for (auto& slot : *g_slots)
    if (slot->device == device_id && !slot->taken && hipEventQuery(slot->done) == hipSuccess) {
      slot->taken = true;
      return slot.get();
    }
  std::unique_ptr<AbxSlot> fresh(new AbxSlot);
  fresh->device = device_id;
  if (hipEventCreateWithFlags(&fresh->done, hipEventDisableTiming) != hipSuccess) {
    set_error(SNF_E_HIP, "hipEventCreate failed");
    return nullptr;
  }
  fresh->taken = true;
  g_slots->push_back(std::move(fresh));
  return g_slots->back().get();
}

void give_slot(AbxSlot* slot) {
  std::lock_guard<std::mutex> lock(g_mu);
  slot->taken = false;
}

}  // namespace

extern "C" {

int snf_abx_cells(int device_id, const float* d_cost, const int32_t* d_len, int64_t n_dist, const int64_t* h_cells,
                  int64_t n_cells, uint64_t* d_counts, void* stream) {
  if (n_dist < 0) return set_error(SNF_E_INVALID, "abx: negative number of distances");
  if (n_cells < 0 || n_cells > 0x7fffffff) return set_error(SNF_E_INVALID, "abx: number of cells out of range");
  if (n_cells > 0 && !h_cells) return set_error(SNF_E_INVALID, "abx: null cell table");
  if (reinterpret_cast<uintptr_t>(h_cells) & 7) return set_error(SNF_E_INVALID, "abx: misaligned cell table");
  const int64_t small_work = threshold("SNF_ABX_SMALL_WORK", kSmallWork);
  const int64_t split_work = std::max<int64_t>(threshold("SNF_ABX_SPLIT_WORK", kSplitWork), 1);
  std::vector<AbxCell> cells(static_cast<size_t>(n_cells));
  std::vector<int64_t> work(static_cast<size_t>(n_cells));
  int64_t n_small = 0;
  for (int64_t c = 0; c < n_cells; ++c) {
    const int64_t* r = h_cells + 8 * c;
    const int64_t offA = r[0], offB = r[1], stride = r[2], nA = r[3], nB = r[4], nX = r[5], same = r[6];
    auto which = [c] { return "abx: cell " + std::to_string(c); };   // (only built for a refusal)
    if (nA < 1 || nB < 1 || nX < 1) return set_error(SNF_E_INVALID, which() + " has an empty A, B or X list");
    if (nA > 0x7fffffff || nB > 0x7fffffff || nX > 0x7fffffff)
      return set_error(SNF_E_INVALID, which() + " has a list of 2^31 items or more");
    if (same && nA != nX) return set_error(SNF_E_INVALID, which() + " is marked same with nA != nX");
    if (r[7] != 0) return set_error(SNF_E_INVALID, which() + ": the last word of the record must be 0");
    // (all of these below n_dist < 2^63 before they are multiplied: no product below overflows 128 bits)
    if (offA < 0 || offB < 0 || stride < 0 || offA >= n_dist || offB >= n_dist || stride > n_dist)
      return set_error(SNF_E_INVALID, which() + " reaches outside the " + std::to_string(n_dist) + " distances");
    const __int128 last = static_cast<__int128>(nX - 1) * stride;
    if (last + offA + (nA - 1) >= n_dist || last + offB + (nB - 1) >= n_dist)
      return set_error(SNF_E_INVALID, which() + " reaches outside the " + std::to_string(n_dist) + " distances");
    const __int128 triplets = static_cast<__int128>(nA) * nB * nX;
    if (triplets > kMaxTriplets) return set_error(SNF_E_INVALID, which() + " has more than 2^62 triplets");
    cells[c] = {offA, offB, stride, static_cast<int32_t>(nA), static_cast<int32_t>(nB), static_cast<int32_t>(nX),
                same ? 1 : 0};
    work[c] = static_cast<int64_t>(triplets);
    n_small += work[c] <= small_work;
  }
  if (n_cells == 0) return SNF_OK;
  if (!d_cost || (reinterpret_cast<uintptr_t>(d_cost) & 3))
    return set_error(SNF_E_INVALID, "abx: d_cost is null or not aligned to float32");
  if (d_len && (reinterpret_cast<uintptr_t>(d_len) & 3))
    return set_error(SNF_E_INVALID, "abx: d_len is not 4-byte aligned");
  if (!d_counts || (reinterpret_cast<uintptr_t>(d_counts) & 7))
    return set_error(SNF_E_INVALID, "abx: d_counts is null or not 8-byte aligned");

  // the small cells in the caller's order (their work differs by at most small_work: nothing to balance); the
  // others as units of at most about split_work compares, the largest first
  std::vector<int32_t> small;
  small.reserve(static_cast<size_t>(n_small));
  struct Keyed {
    int64_t work;
    AbxUnit unit;
  };
  std::vector<Keyed> keyed;
  bool any_split = false;
  for (int64_t c = 0; c < n_cells; ++c) {
    if (work[c] <= small_work) {
      small.push_back(static_cast<int32_t>(c));
      continue;
    }
    const int64_t nX = cells[c].nX, per_x = work[c] / nX;
    int64_t parts = std::min<int64_t>(nX, (work[c] + split_work - 1) / split_work);
    const int64_t step = (nX + parts - 1) / parts;
    parts = (nX + step - 1) / step;
    for (int64_t x0 = 0; x0 < nX; x0 += step) {
      const int64_t x1 = std::min(nX, x0 + step);
      keyed.push_back({per_x * (x1 - x0), {static_cast<int32_t>(c), static_cast<int32_t>(x0),
                                           static_cast<int32_t>(x1), parts > 1 ? 1 : 0}});
    }
    any_split = any_split || parts > 1;
  }
  std::stable_sort(keyed.begin(), keyed.end(), [](const Keyed& a, const Keyed& b) { return a.work > b.work; });
  std::vector<AbxUnit> units(keyed.size());
  for (size_t u = 0; u < keyed.size(); ++u) units[u] = keyed[u].unit;

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
  AbxSlot* slot = take_slot(device_id);
  if (!slot) return SNF_E_HIP;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : mine->stream;
  // (DevBuf::upload waits for the copy on the thread's own stream: the tables are pageable vectors that go away)
  int rc = slot->cells.upload(cells, mine->stream);
  if (!rc) rc = slot->small.upload(small, mine->stream);
  if (!rc) rc = slot->units.upload(units, mine->stream);
  // (a split cell's units add to its counts: zero them, in stream order, ahead of the kernels)
  if (!rc && any_split &&
      hipMemsetAsync(d_counts, 0, 3 * sizeof(uint64_t) * static_cast<size_t>(n_cells), s) != hipSuccess)
    rc = set_error(SNF_E_HIP, "abx: hipMemsetAsync failed");
  if (!rc)
    rc = launch_abx_cells(d_cost, d_len, slot->cells.as<AbxCell>(), slot->small.as<int32_t>(),
                          static_cast<int64_t>(small.size()), slot->units.as<AbxUnit>(),
                          static_cast<int64_t>(units.size()), compute_units,
                          reinterpret_cast<unsigned long long*>(d_counts), s);
  if (!rc && hipEventRecord(slot->done, s) != hipSuccess) rc = set_error(SNF_E_HIP, "abx: hipEventRecord failed");
  if (rc) {
    // (whatever was enqueued has finished before the slot's tables can be written again)
    (void)hipStreamSynchronize(s);
    give_slot(slot);
    return rc;
  }
  give_slot(slot);   // (free for the next call once `done` has completed: take_slot asks the event)
  if (!stream && hipStreamSynchronize(s) != hipSuccess) return set_error(SNF_E_HIP, "abx kernel failed");
  return SNF_OK;
}

}  // extern "C"
