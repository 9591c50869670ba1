// C ABI of libshennong_hip.so (include/shennong_amd.h): the plan-less resampler entry points.  The rate pair is
// checked and its table sized on the host before any device is asked for; a table is built once per pair and
// uploaded once per (device, pair).  Runs on the calling thread's scratch and stream (plan.h: Planless).
#include <map>
#include <memory>
#include <tuple>

#include "plan.h"

using namespace snf;

namespace {

constexpr int kMaxRate = 1 << 22;          // Hertz: the phase loop of a refused pair stays short
constexpr int64_t kMaxSamples = 0x7fffff00;   // per utterance, on either side

struct PairTable {
  LinearResampleHost host;   // geometry; the weights once `built`
  ResampleTable layout{};
  bool built = false;
};

std::mutex g_mu;
// (never destroyed: a DevBuf released after the runtime has shut down would call into it)
auto* g_pairs = new std::map<std::pair<int, int>, std::unique_ptr<PairTable>>;
auto* g_tables = new std::map<std::tuple<int, int, int>, std::unique_ptr<DevBuf>>;

bool rates_ok(int32_t rate_in, int32_t rate_out) {
  return rate_in >= 1 && rate_out >= 1 && rate_in <= kMaxRate && rate_out <= kMaxRate;
}

// ResampleWaveform's filter: cutoff 0.99 x half the lower rate, 6 zero crossings
float waveform_cutoff(int32_t rate_in, int32_t rate_out) {
  return static_cast<float>(0.99 * 0.5 * std::min(rate_in, rate_out));
}

// the pair's table, sized and checked against the LDS limit (g_mu held)
int pair_table(int32_t rate_in, int32_t rate_out, PairTable** out) {
  auto& slot = (*g_pairs)[{rate_in, rate_out}];
  if (!slot) {
    slot.reset(new PairTable);
    make_linear_resample_geometry(rate_in, rate_out, waveform_cutoff(rate_in, rate_out), 6, &slot->host);
    resample_layout(slot->host, &slot->layout);
  }
  const int64_t table_bytes = static_cast<int64_t>(slot->host.out_unit) * (2 + slot->layout.stride) * 4;
  const int64_t span_bytes = static_cast<int64_t>(slot->layout.span) * 4;
  if (((table_bytes + 15) & ~int64_t(15)) + span_bytes > kResampleLdsBytes)
    return set_error(SNF_E_INVALID, "resample " + std::to_string(rate_in) + " -> " + std::to_string(rate_out) +
                                        " Hz: the phase table (" + std::to_string(slot->host.out_unit) +
                                        " phases, " + std::to_string(table_bytes) + " bytes) and the staged span (" +
                                        std::to_string(span_bytes) + " bytes) do not fit in the " +
                                        std::to_string(kResampleLdsBytes) + " bytes of LDS of a workgroup");
  if (!slot->built) {
    make_linear_resample(rate_in, rate_out, waveform_cutoff(rate_in, rate_out), 6, &slot->host);
    slot->built = true;
  }
  *out = slot.get();
  return SNF_OK;
}

}  // namespace

extern "C" {

int64_t snf_resample_num_out(int32_t rate_in, int32_t rate_out, int64_t n_in) {
  if (!rates_ok(rate_in, rate_out)) return set_error(SNF_E_INVALID, "resample: rates must be in [1, 2^22] Hz");
  if (n_in < 0 || n_in > kMaxSamples) return set_error(SNF_E_INVALID, "resample: number of samples out of range");
  LinearResampleHost r;
  r.rate_in = rate_in;
  r.rate_out = rate_out;
  return r.num_output(n_in, true);
}

int snf_linear_resample(int device_id, int32_t rate_in, int32_t rate_out, int32_t kind, const void* d_src,
                        const int64_t* h_src_offsets, int64_t n_utts, void* d_dst, const int64_t* h_dst_starts,
                        void* stream) {
  if (!rates_ok(rate_in, rate_out)) return set_error(SNF_E_INVALID, "resample: rates must be in [1, 2^22] Hz");
  if (rate_in == rate_out)
    return set_error(SNF_E_INVALID, "resample: both rates are " + std::to_string(rate_in) + " Hz, nothing to do");
  if (kind != 0 && kind != 1) return set_error(SNF_E_INVALID, "resample: kind must be 0 (int16) or 1 (float32)");
  if (n_utts < 0 || n_utts > (int64_t(1) << 31)) return set_error(SNF_E_INVALID, "resample: number of utterances out of range");
  ResampleTable table{};
  LinearResampleHost geometry;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    PairTable* pair = nullptr;
    int rc = pair_table(rate_in, rate_out, &pair);
    if (rc) return rc;
    table = pair->layout;
    geometry.rate_in = rate_in;
    geometry.rate_out = rate_out;
  }
  if (n_utts == 0) return SNF_OK;
  if (!h_src_offsets || !h_dst_starts) return set_error(SNF_E_INVALID, "resample: null offsets table");
  if (h_src_offsets[0] < 0) return set_error(SNF_E_INVALID, "resample: source offsets must not be negative");
  std::vector<ResampleUtt> utts(static_cast<size_t>(n_utts));
  int64_t max_out = 0;
  for (int64_t u = 0; u < n_utts; ++u) {
    const int64_t n_in = h_src_offsets[u + 1] - h_src_offsets[u];
    if (n_in < 0) return set_error(SNF_E_INVALID, "resample: source offsets must not decrease");
    if (n_in > kMaxSamples || h_src_offsets[u + 1] > (int64_t(1) << 40))
      return set_error(SNF_E_INVALID, "resample: utterance " + std::to_string(u) + " is too long");
    const int64_t n_out = geometry.num_output(n_in, true);
    if (n_out > kMaxSamples) return set_error(SNF_E_INVALID, "resample: utterance " + std::to_string(u) + " is too long");
    if (h_dst_starts[u] < 0 || h_dst_starts[u] > (int64_t(1) << 40))
      return set_error(SNF_E_INVALID, "resample: destination start of utterance " + std::to_string(u) + " out of range");
    utts[u] = {h_src_offsets[u], n_in, h_dst_starts[u], n_out};
    max_out = std::max(max_out, n_out);
  }
  if (max_out == 0) return SNF_OK;
  if (!d_src || !d_dst) return set_error(SNF_E_INVALID, "resample: null buffer");
  const uintptr_t align = kind == 0 ? 1 : 3;
  if ((reinterpret_cast<uintptr_t>(d_src) & align) || (reinterpret_cast<uintptr_t>(d_dst) & align))
    return set_error(SNF_E_INVALID, "resample: a buffer is not aligned to its element type");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_error(SNF_E_NODEVICE, "no HIP device visible: libshennong_hip needs an MI355X (gfx950)");
  if (device_id < 0 || device_id >= ndev) return set_error(SNF_E_INVALID, "bad device id");

  Planless lay;
  auto d_utts = lay.take<ResampleUtt>(utts.size());
  int rc = lay.begin(device_id, stream);
  if (rc) return rc;
  {
    // the table of this device: uploaded once, on this stream, waited for under the lock
    std::lock_guard<std::mutex> lock(g_mu);
    auto& buf = (*g_tables)[std::make_tuple(device_id, rate_in, rate_out)];
    if (!buf) {
      std::vector<int32_t> blob;
      resample_blob((*g_pairs)[{rate_in, rate_out}]->host, table, &blob);
      std::unique_ptr<DevBuf> fresh(new DevBuf);
      if ((rc = fresh->upload(blob, lay.s))) return rc;
      buf = std::move(fresh);
    }
    table.blob = buf->as<int32_t>();
  }
  SNF_HIP_CHECK(hipMemcpyAsync(d_utts, utts.data(), sizeof(ResampleUtt) * utts.size(), hipMemcpyHostToDevice, lay.s));
  rc = launch_linear_resample(table, kind, d_src, d_utts, n_utts, max_out, d_dst, lay.s);
  return lay.finish(rc, "resample kernel failed");   // (also: `utts` is no longer read by the copy)
}

}  // extern "C"
