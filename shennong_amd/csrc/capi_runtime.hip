// C ABI of libshennong_hip.so (include/shennong_amd.h): version, last error, devices, the frame arithmetic,
// memory / stream / event wrappers, debug exports; and the process-wide pieces behind plan.h (out-of-memory
// hook, per-thread scratch, named noise calls).
#include <atomic>

#include "plan.h"

using namespace snf;

namespace snf {

namespace {
// Out-of-memory hook (snf_set_oom_hook): the host side parks freed device buffers in a pool of its own
// (shennong_amd/_backend.py, up to 8 GiB); an allocation of the library that fails asks it to give them
// back and tries once more.
std::atomic<snf_oom_hook> g_oom_hook{nullptr};
// noise stream of the next call of THIS thread that draws random numbers (0: the plan's own call count)
thread_local uint64_t t_noise_call = 0;
}  // namespace

hipError_t malloc_with_hook(void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipErrorOutOfMemory) {
    if (snf_oom_hook hook = g_oom_hook.load()) {
      (void)hipGetLastError();
      // the hook frees pooled blocks of EVERY device and binds each one to do it: the retry (and the
      // launches of the plan call we are in the middle of) must find the calling thread on its own device
      int dev = -1;
      const bool have_dev = hipGetDevice(&dev) == hipSuccess;
      hook();
      if (have_dev) (void)hipSetDevice(dev);
      (void)hipGetLastError();
      e = hipMalloc(p, bytes);
    }
  }
  return e;
}

ThreadScratch* thread_scratch(int device_id) {
  thread_local std::vector<std::pair<int, ThreadScratch*>> mine;
  for (auto& e : mine)
    if (e.first == device_id) return e.second;
  ThreadScratch* t = new ThreadScratch;
  if (hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking) != hipSuccess) {
    delete t;
    snf::set_error(SNF_E_HIP, "hipStreamCreate failed");
    return nullptr;
  }
  mine.emplace_back(device_id, t);
  return t;
}

uint64_t take_noise_call() {
  const uint64_t pinned = t_noise_call;
  t_noise_call = 0;
  return pinned;
}

}  // namespace snf

extern "C" {

const char* snf_version(void) { return "shennong_amd 0.1 (gfx950)"; }
const char* snf_last_error(void) { return last_error(); }

int snf_set_noise_call(uint64_t call) {
  t_noise_call = call;
  return SNF_OK;
}

int snf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
int snf_set_device(int device_id) {
  SNF_HIP_CHECK(hipSetDevice(device_id));
  return SNF_OK;
}
int snf_device_name(int device_id, char* buf, int buflen) {
  hipDeviceProp_t prop;
  SNF_HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
  snprintf(buf, buflen, "%s (%s)", prop.name, prop.gcnArchName);
  return SNF_OK;
}
int snf_device_synchronize(void) {
  SNF_HIP_CHECK(hipDeviceSynchronize());
  return SNF_OK;
}

int64_t snf_num_frames(const snf_frame_options* o, int64_t n) { return num_frames(*o, n); }
int64_t snf_first_sample_of_frame(const snf_frame_options* o, int64_t f) {
  return first_sample_of_frame(*o, f);
}
int32_t snf_window_size(const snf_frame_options* o) { return window_size(*o); }
int32_t snf_window_shift(const snf_frame_options* o) { return window_shift(*o); }
int32_t snf_padded_window_size(const snf_frame_options* o) { return padded_window_size(*o); }
int snf_window_function(const snf_frame_options* o, float* out) {
  std::vector<float> w;
  int rc = make_window(*o, &w);
  if (rc) return rc;
  std::memcpy(out, w.data(), sizeof(float) * w.size());
  return SNF_OK;
}
int64_t snf_pitch_num_frames(const snf_pitch_options* o, int64_t n) {
  PitchTablesHost t;
  if (make_pitch_tables(*o, &t)) return -1;
  return t.frames_available(t.resample.num_output(n, true), true, o->snip_edges != 0);
}

int snf_malloc(void** dptr, uint64_t bytes) {
  SNF_HIP_CHECK(hipMalloc(dptr, bytes));
  return SNF_OK;
}
int snf_mem_info(uint64_t* free_bytes, uint64_t* total_bytes) {
  size_t f = 0, t = 0;
  SNF_HIP_CHECK(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return SNF_OK;
}
int snf_set_oom_hook(snf_oom_hook hook) {
  g_oom_hook.store(hook);
  return SNF_OK;
}
int snf_free(void* dptr) {
  SNF_HIP_CHECK(hipFree(dptr));
  return SNF_OK;
}
int snf_memcpy_h2d(void* dst, const void* src, uint64_t bytes) {
  SNF_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return SNF_OK;
}
int snf_memcpy_d2h(void* dst, const void* src, uint64_t bytes) {
  SNF_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return SNF_OK;
}
int snf_stream_create(void** stream) {
  if (!stream) return set_error(SNF_E_INVALID, "null pointer");
  hipStream_t s;
  SNF_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = s;
  return SNF_OK;
}
int snf_stream_destroy(void* stream) {
  if (stream) SNF_HIP_CHECK(hipStreamDestroy(static_cast<hipStream_t>(stream)));
  return SNF_OK;
}
int snf_stream_synchronize(void* stream) {
  SNF_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return SNF_OK;
}
int snf_stream_query(void* stream) {
  const hipError_t e = hipStreamQuery(static_cast<hipStream_t>(stream));
  if (e == hipSuccess) return 0;
  if (e == hipErrorNotReady) {
    (void)hipGetLastError();   // (not an error: nothing to leave behind for the next call's check)
    return 1;
  }
  return set_error(SNF_E_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(e));
}
int snf_event_create(void** event) {
  if (!event) return set_error(SNF_E_INVALID, "null pointer");
  hipEvent_t e;
  SNF_HIP_CHECK(hipEventCreate(&e));
  *event = e;
  return SNF_OK;
}
int snf_event_destroy(void* event) {
  if (event) SNF_HIP_CHECK(hipEventDestroy(static_cast<hipEvent_t>(event)));
  return SNF_OK;
}
int snf_event_record(void* event, void* stream) {
  if (!event) return set_error(SNF_E_INVALID, "null event");
  SNF_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(event), static_cast<hipStream_t>(stream)));
  return SNF_OK;
}
int snf_event_synchronize(void* event) {
  if (!event) return set_error(SNF_E_INVALID, "null event");
  SNF_HIP_CHECK(hipEventSynchronize(static_cast<hipEvent_t>(event)));
  return SNF_OK;
}
int snf_stream_wait_event(void* stream, void* event) {
  if (!event) return set_error(SNF_E_INVALID, "null event");
  SNF_HIP_CHECK(hipStreamWaitEvent(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(event), 0));
  return SNF_OK;
}
int snf_event_elapsed_ms(void* start, void* stop, float* ms) {
  if (!start || !stop || !ms) return set_error(SNF_E_INVALID, "null pointer");
  SNF_HIP_CHECK(hipEventSynchronize(static_cast<hipEvent_t>(stop)));
  SNF_HIP_CHECK(hipEventElapsedTime(ms, static_cast<hipEvent_t>(start), static_cast<hipEvent_t>(stop)));
  return SNF_OK;
}
int snf_memcpy_h2d_async(void* dst, const void* src, uint64_t bytes, void* stream) {
  SNF_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream)));
  return SNF_OK;
}
int snf_memcpy_d2h_async(void* dst, const void* src, uint64_t bytes, void* stream) {
  SNF_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
  return SNF_OK;
}
int snf_memset(void* dst, int value, uint64_t bytes) {
  // hipMemset on device memory returns before the fill has run, and the plans' streams are non-blocking:
  // they do not wait for the null stream.  A caller that fills a buffer and then hands it to a plan expects
  // the fill to be over (found by the pipeline fuzzer: the fill landed on top of a kernel's output).
  SNF_HIP_CHECK(hipMemset(dst, value, bytes));
  SNF_HIP_CHECK(hipStreamSynchronize(nullptr));
  return SNF_OK;
}
namespace {
__global__ __launch_bounds__(256) void lds_fill_kernel(unsigned pattern, int words, unsigned* sink) {
  extern __shared__ unsigned fill[];
  for (int i = threadIdx.x; i < words; i += blockDim.x) fill[i] = pattern;
  __syncthreads();
  // (a dependent read keeps the stores from being optimised away)
  if (fill[(threadIdx.x * 97) % words] != pattern) sink[0] = 1;
}
}  // namespace

int snf_debug_pitch_scratch(snf_plan* plan, void** down, void** nccf_res, void** pov_nccf,
                            void** states) {
  if (!plan || plan->kind != SNF_KIND_PITCH) return set_error(SNF_E_INVALID, "not a pitch plan");
  if (down) *down = plan->pitch_s.down.p;
  if (nccf_res) *nccf_res = plan->pitch_s.nccf_res.p;
  if (pov_nccf) *pov_nccf = plan->pitch_s.pov_nccf.p;
  if (states) *states = plan->pitch_s.states.p;
  return SNF_OK;
}
int snf_debug_fill_lds(uint32_t pattern) {
  // two 80 KB workgroups cover the 160 KB of a CU; many more workgroups than CUs so that every CU
  // (and both halves of its LDS) is visited
  const int bytes = 80 * 1024 - 256;
  unsigned* sink = nullptr;
  SNF_HIP_CHECK(hipMalloc(&sink, sizeof(unsigned)));
  SNF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lds_fill_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  hipLaunchKernelGGL(lds_fill_kernel, dim3(256 * 32), dim3(256), bytes, nullptr, pattern, bytes / 4, sink);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  (void)hipFree(sink);
  if (e != hipSuccess) return snf::set_error(SNF_E_HIP, std::string("lds fill: ") + hipGetErrorString(e));
  return SNF_OK;
}

int snf_host_malloc(void** hptr, uint64_t bytes) {
  if (!hptr) return set_error(SNF_E_INVALID, "null pointer");
  SNF_HIP_CHECK(hipHostMalloc(hptr, bytes > 0 ? bytes : 1, hipHostMallocDefault));
  return SNF_OK;
}
int snf_host_free(void* hptr) {
  if (hptr) SNF_HIP_CHECK(hipHostFree(hptr));
  return SNF_OK;
}

float snf_plan_last_kernel_ms(const snf_plan* plan, int which) {
  if (!plan || !plan->events_valid || which < 0 || which > plan->n_slots) return -1.0f;
  float ms = -1.0f;
  if (hipEventSynchronize(plan->ev[plan->n_slots]) != hipSuccess) return -1.0f;
  hipError_t e = which == 0 ? hipEventElapsedTime(&ms, plan->ev[0], plan->ev[plan->n_slots])
                            : hipEventElapsedTime(&ms, plan->ev[which - 1], plan->ev[which]);
  return e == hipSuccess ? ms : -1.0f;
}
const char* snf_plan_kernel_name(const snf_plan* plan, int which) {
  if (!plan || which <= 0 || which > plan->n_slots) return nullptr;
  return plan->slot_name[which];
}

}  // extern "C"
