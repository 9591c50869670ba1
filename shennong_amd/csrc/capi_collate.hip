// C ABI of libshennong_hip.so (include/shennong_amd.h): the plan-less collation of a ragged feature block into a
// padded batch.  Every argument is checked on the host before any device is asked for.  The per-utterance table
// goes up on the calling thread's own stream (waited for: a few kilobytes) into a slot that stays reserved until
// the kernel, enqueued on the caller's stream, has run - so the call does not wait for the caller's stream.
#include <memory>

#include "plan.h"

using namespace snf;

namespace {

// A device table that a kernel in flight may still be reading: `done` is recorded behind that kernel
struct TableSlot {
  int device = -1;
  DevBuf table;
  hipEvent_t done = nullptr;
  bool taken = false;   // between take_slot and the event's record (or the failure that gives it back)
};

std::mutex g_mu;
// (never destroyed: a DevBuf released after the runtime has shut down would call into it)
auto* g_slots = new std::vector<std::unique_ptr<TableSlot>>;

// a slot of `device_id` whose last kernel has finished, or a new one
TableSlot* take_slot(int device_id) {
  std::lock_guard<std::mutex> lock(g_mu);
  for (auto& slot : *g_slots)
    if (slot->device == device_id && !slot->taken && hipEventQuery(slot->done) == hipSuccess) {
      slot->taken = true;
      return slot.get();
    }
  std::unique_ptr<TableSlot> fresh(new TableSlot);
  fresh->device = device_id;
  if (hipEventCreateWithFlags(&fresh->done, hipEventDisableTiming) != hipSuccess) {
    set_error(SNF_E_HIP, "hipEventCreate failed");
    return nullptr;
  }
  fresh->taken = true;
  g_slots->push_back(std::move(fresh));
  return g_slots->back().get();
}

void give_slot(TableSlot* slot) {
  std::lock_guard<std::mutex> lock(g_mu);
  slot->taken = false;
}

bool subsampling_ok(int32_t subsample, int32_t offset) { return subsample >= 1 && offset >= 0 && offset < subsample; }

int64_t num_out(int64_t frames, int32_t subsample, int32_t offset) {
  return frames <= offset ? 0 : (frames - offset + subsample - 1) / subsample;
}

}  // namespace

extern "C" {

int64_t snf_collate_num_out(int64_t frames, int32_t subsample, int32_t offset) {
  if (frames < 0) return set_error(SNF_E_INVALID, "collate: negative number of frames");
  if (!subsampling_ok(subsample, offset))
    return set_error(SNF_E_INVALID, "collate: subsample must be at least 1 and offset in [0, subsample)");
  return num_out(frames, subsample, offset);
}

int snf_collate_padded(int device_id, const float* d_in, int32_t dim, const int64_t* h_frame_offsets,
                       int64_t n_utts, int32_t left, int32_t right, int32_t subsample, int32_t offset,
                       int32_t out_type, float pad_value, int64_t t_max, void* d_out, int32_t* d_lengths,
                       void* stream) {
  if (!subsampling_ok(subsample, offset))
    return set_error(SNF_E_INVALID, "collate: subsample must be at least 1 and offset in [0, subsample)");
  if (left < 0 || right < 0) return set_error(SNF_E_INVALID, "collate: a context is negative");
  if (left > (1 << 20) || right > (1 << 20)) return set_error(SNF_E_INVALID, "collate: a context is out of range");
  if (dim < 1) return set_error(SNF_E_INVALID, "collate: dim must be positive");
  if (out_type != SNF_COLLATE_F32 && out_type != SNF_COLLATE_F16 && out_type != SNF_COLLATE_BF16)
    return set_error(SNF_E_INVALID, "collate: out_type must be 0 (float32), 1 (float16) or 2 (bfloat16)");
  if (n_utts < 0 || n_utts > 0x7fffffff) return set_error(SNF_E_INVALID, "collate: number of utterances out of range");
  if (t_max < 0) return set_error(SNF_E_INVALID, "collate: t_max is negative");
  if (n_utts == 0) return SNF_OK;
  if (!h_frame_offsets) return set_error(SNF_E_INVALID, "collate: null offsets table");
  if (h_frame_offsets[0] < 0) return set_error(SNF_E_INVALID, "collate: offsets must not be negative");
  std::vector<CollateUtt> utts(static_cast<size_t>(n_utts));
  int64_t longest = 0;
  for (int64_t u = 0; u < n_utts; ++u) {
    const int64_t frames = h_frame_offsets[u + 1] - h_frame_offsets[u];
    if (frames < 0) return set_error(SNF_E_INVALID, "collate: offsets must not decrease");
    if (frames > 0x7fffffff || h_frame_offsets[u + 1] > (int64_t(1) << 40))
      return set_error(SNF_E_INVALID, "collate: utterance " + std::to_string(u) + " is too long");
    const int64_t n = num_out(frames, subsample, offset);
    utts[u] = {h_frame_offsets[u], static_cast<int32_t>(frames), static_cast<int32_t>(n)};
    longest = std::max(longest, n);
  }
  if (t_max < longest)
    return set_error(SNF_E_INVALID, "collate: t_max is " + std::to_string(t_max) + " but an utterance keeps " +
                                        std::to_string(longest) + " frames");
  // 32-bit indices in the kernel: the whole output below 2^31 elements
  const int64_t width = int64_t(left) + 1 + right, limit = 0x7fffffff;
  const int64_t row_elems = width * dim;
  if (row_elems > limit || (t_max > 0 && (row_elems > limit / t_max || row_elems * t_max > limit / n_utts)))
    return set_error(SNF_E_INVALID,
                     "collate: the padded batch (" + std::to_string(n_utts) + " x " + std::to_string(t_max) + " x " +
                         std::to_string(row_elems) + ") has 2^31 elements or more: collate it in parts");
  if (!d_out || !d_lengths) return set_error(SNF_E_INVALID, "collate: null buffer");
  if ((reinterpret_cast<uintptr_t>(d_out) & 15) || (reinterpret_cast<uintptr_t>(d_lengths) & 3))
    return set_error(SNF_E_INVALID, "collate: d_out must be 16-byte aligned and d_lengths 4-byte aligned");
  if (longest > 0 && (!d_in || (reinterpret_cast<uintptr_t>(d_in) & 3)))
    return set_error(SNF_E_INVALID, "collate: d_in is null or not aligned to float32");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_error(SNF_E_NODEVICE, "no HIP device visible: libshennong_hip needs an MI355X (gfx950)");
  if (device_id < 0 || device_id >= ndev) return set_error(SNF_E_INVALID, "bad device id");

  CollateShape shape{};
  shape.dim = dim;
  shape.width = static_cast<int32_t>(width);
  shape.left = left;
  shape.subsample = subsample;
  shape.offset = offset;
  shape.t_max = static_cast<int32_t>(t_max);
  shape.row_elems = static_cast<uint32_t>(row_elems);
  shape.utt_elems = static_cast<uint32_t>(row_elems * t_max);
  shape.total = static_cast<uint32_t>(row_elems * t_max * n_utts);
  shape.n_utts = static_cast<uint32_t>(n_utts);

  SNF_HIP_CHECK(hipSetDevice(device_id));
  ThreadScratch* mine = thread_scratch(device_id);
  if (!mine) return SNF_E_HIP;
  TableSlot* slot = take_slot(device_id);
  if (!slot) return SNF_E_HIP;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : mine->stream;
  // (DevBuf::upload waits for the copy on the thread's own stream: `utts` is a pageable vector that goes away)
  int rc = slot->table.upload(utts, mine->stream);
  if (!rc)
    rc = launch_collate_padded(d_in, slot->table.as<CollateUtt>(), shape, out_type, pad_value, d_out, d_lengths, s);
  if (!rc && hipEventRecord(slot->done, s) != hipSuccess) rc = set_error(SNF_E_HIP, "collate: hipEventRecord failed");
  if (rc) {
    // (whatever was enqueued has finished before the slot's table can be written again)
    (void)hipStreamSynchronize(s);
    give_slot(slot);
    return rc;
  }
  give_slot(slot);   // (free for the next call once `done` has completed: take_slot asks the event)
  if (!stream && hipStreamSynchronize(s) != hipSuccess) return set_error(SNF_E_HIP, "collate kernel failed");
  return SNF_OK;
}

}  // extern "C"
