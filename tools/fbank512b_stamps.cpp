// When do the waves of fbank512b_kernel finish?  Runs the benchmark batch (N utterances x 3 s) through the stamp
// build of the library (make -C shennong_amd/csrc stamps: kernels_fbank512b.hip with -DSNF_FBANK512B_STAMPS), in
// which every wave records its workgroup, wave, XCC and hardware ids, s_memtime and s_memrealtime at entry to and
// exit from the set loop and the number of sets it ran, and prints the spread of the finish times inside a SIMD,
// inside a CU and across CUs and XCDs, in % of the launch (profiles/NOTEBOOK.md 4.1g).
//
//   make -C shennong_amd/csrc stamps
//   g++ -O2 -std=c++17 tools/fbank512b_stamps.cpp -Iinclude -Lshennong_amd -lshennong_hip_stamps
//       -Wl,-rpath,'$ORIGIN/../shennong_amd' -o scratch/stamps512b        (one command line)
//   scratch/stamps512b [n_utts] [kind: fbank|mfcc] [settling launches] -- name=ENV1=v,ENV2=v ...
// (variants as in tools/ab_fbank512.cpp: `fixed=SNF_FBANK512B_FIXED=1` is the walk of before)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "shennong_amd.h"

extern "C" void snf_debug_fbank512b_stamps(void* device_buffer);  // the stamp build alone

#define CK(x)                                              \
  do {                                                     \
    int rc_ = (x);                                         \
    if (rc_ != 0) {                                        \
      printf("%s -> %d: %s\n", #x, rc_, snf_last_error()); \
      return 1;                                            \
    }                                                      \
  } while (0)

static void apply_env(const std::string& spec, bool set) {
  size_t pos = spec.find('=');
  if (pos == std::string::npos) return;
  std::string rest = spec.substr(pos + 1);
  while (!rest.empty()) {
    const size_t comma = rest.find(',');
    const std::string item = rest.substr(0, comma);
    const size_t eq = item.find('=');
    if (eq != std::string::npos) {
      if (set) setenv(item.substr(0, eq).c_str(), item.substr(eq + 1).c_str(), 1);
      else unsetenv(item.substr(0, eq).c_str());
    }
    if (comma == std::string::npos) break;
    rest = rest.substr(comma + 1);
  }
}

struct Wave {
  int block, wid, xcc, simd, cu, se;
  long long sets;
  double in, out;  // % of the launch, on the 100 MHz clock all XCDs share
  long long clocks, real;
};

static double median(std::vector<double> v) {
  if (v.empty()) return 0.0;
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}
static double maxof(const std::vector<double>& v) { return v.empty() ? 0.0 : *std::max_element(v.begin(), v.end()); }
static double minof(const std::vector<double>& v) { return v.empty() ? 0.0 : *std::min_element(v.begin(), v.end()); }

int main(int argc, char** argv) {
  int64_t n_utts = 10000;
  std::string kind = "fbank";
  int settle = 300;
  std::vector<std::string> variants;
  int i = 1;
  for (; i < argc && std::strcmp(argv[i], "--") != 0; ++i) {
    if (i == 1) n_utts = atoll(argv[i]);
    if (i == 2) kind = argv[i];
    if (i == 3) settle = atoi(argv[i]);
  }
  for (++i; i < argc; ++i) variants.push_back(argv[i]);
  if (variants.empty()) variants.push_back("default=");

  snf_options o;
  std::memset(&o, 0, sizeof(o));
  o.frame.samp_freq = 16000;
  o.frame.frame_shift_ms = 10;
  o.frame.frame_length_ms = 25;
  o.frame.preemph_coeff = 0.97f;
  o.frame.remove_dc_offset = 1;
  o.frame.window_type = SNF_WINDOW_POVEY;
  o.frame.round_to_power_of_two = 1;
  o.frame.blackman_coeff = 0.42f;
  o.frame.snip_edges = 1;
  o.mel.num_bins = 40;
  o.mel.low_freq = 20;
  o.mel.vtln_low = 100;
  o.mel.vtln_high = -500;
  o.raw_energy = 1;
  o.use_log_fbank = 1;
  o.use_power = 1;
  o.kind = SNF_KIND_FBANK;
  if (kind == "mfcc") {
    o.kind = SNF_KIND_MFCC;
    o.mel.num_bins = 23;
    o.num_ceps = 13;
    o.cepstral_lifter = 22;
    o.use_energy = 1;
  }
  o.delta_order = 2;
  o.delta_window = 2;

  snf_plan* plan = nullptr;
  CK(snf_plan_create(&o, 0, &plan));
  const int cols = snf_plan_ndims(plan);
  std::vector<int64_t> soff(n_utts + 1, 0), foff(n_utts + 1, 0);
  for (int64_t u = 0; u < n_utts; ++u) {
    soff[u + 1] = soff[u] + 48000;
    foff[u + 1] = foff[u] + snf_plan_num_frames(plan, 48000);
  }
  const int64_t total_samples = soff[n_utts], total_frames = foff[n_utts];
  std::vector<int16_t> wave(static_cast<size_t>(total_samples));
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  for (size_t k = 0; k < wave.size(); ++k) {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    wave[k] = static_cast<int16_t>(static_cast<int>((rng >> 40) & 0x3fff) - 0x2000 +
                                   static_cast<int>(6000.0 * std::sin(0.05 * static_cast<double>(k % 48000))));
  }
  constexpr int kWavesMax = 4096, kWords = 8;
  const size_t stamp_bytes = sizeof(uint64_t) * kWavesMax * kWords;
  void *d_wave = nullptr, *d_out = nullptr, *d_stamps = nullptr;
  CK(snf_malloc(&d_wave, static_cast<uint64_t>(total_samples) * 2));
  CK(snf_malloc(&d_out, static_cast<uint64_t>(total_frames) * cols * 4));
  CK(snf_malloc(&d_stamps, stamp_bytes));
  CK(snf_memcpy_h2d(d_wave, wave.data(), static_cast<uint64_t>(total_samples) * 2));
  printf("workload: %lld utterances, %lld frames (%lld sets), %d columns, kind %s, %d settling launches\n",
         (long long)n_utts, (long long)total_frames, (long long)((total_frames + 3) / 4), cols, kind.c_str(), settle);

  for (const std::string& v : variants) {
    const std::string label = v.substr(0, v.find('='));
    apply_env(v, true);
    snf_debug_fbank512b_stamps(nullptr);
    for (int r = 0; r < settle; ++r)
      CK(snf_plan_run_batch_device(plan, static_cast<const int16_t*>(d_wave), soff.data(), n_utts, nullptr,
                                   static_cast<float*>(d_out), foff.data(), nullptr));
    CK(snf_memset(d_stamps, 0, stamp_bytes));
    snf_debug_fbank512b_stamps(d_stamps);
    CK(snf_plan_run_batch_device(plan, static_cast<const int16_t*>(d_wave), soff.data(), n_utts, nullptr,
                                 static_cast<float*>(d_out), foff.data(), nullptr));
    const double kernel_ms = snf_plan_last_kernel_ms(plan, 1);
    const char* kernel_name = snf_plan_kernel_name(plan, 1);
    snf_debug_fbank512b_stamps(nullptr);
    std::vector<uint64_t> raw(static_cast<size_t>(kWavesMax) * kWords);
    CK(snf_memcpy_d2h(raw.data(), d_stamps, stamp_bytes));
    apply_env(v, false);

    uint64_t r0 = ~0ull, r1 = 0;
    int n_waves = 0;
    for (int w = 0; w < kWavesMax; ++w) {
      const uint64_t* m = &raw[static_cast<size_t>(w) * kWords];
      if (!(m[0] >> 63)) continue;
      ++n_waves;
      r0 = std::min(r0, m[6]);
      r1 = std::max(r1, m[7]);
    }
    printf("\n== %s: %s, %.4f ms by the events; %d waves stamped\n", label.c_str(), kernel_name ? kernel_name : "?",
           kernel_ms, n_waves);
    if (n_waves == 0) continue;
    const double span = static_cast<double>(r1 - r0);  // 10 ns ticks from the first entry to the last exit
    std::vector<Wave> waves;
    long long sum_clocks = 0, sum_real = 0, sets_min = 1ll << 60, sets_max = 0, sets_sum = 0;
    int placement[4][4] = {};
    for (int w = 0; w < kWavesMax; ++w) {
      const uint64_t* m = &raw[static_cast<size_t>(w) * kWords];
      if (!(m[0] >> 63)) continue;
      Wave x;
      x.block = static_cast<int>((m[0] >> 8) & 0xffffff);
      x.wid = static_cast<int>(m[0] & 0xff);
      x.xcc = static_cast<int>(m[1] & 0xf);
      x.simd = static_cast<int>((m[2] >> 4) & 3);
      x.cu = static_cast<int>((m[2] >> 8) & 0xf);
      x.se = static_cast<int>((m[2] >> 12) & 0xf);  // (SH and SE bits together: a label, not decoded further)
      x.sets = static_cast<long long>(m[3]);
      x.in = 100.0 * static_cast<double>(m[6] - r0) / span;
      x.out = 100.0 * static_cast<double>(m[7] - r0) / span;
      x.clocks = static_cast<long long>(m[5] - m[4]);
      x.real = static_cast<long long>(m[7] - m[6]);
      sum_clocks += x.clocks;
      sum_real += x.real;
      sets_min = std::min(sets_min, x.sets);
      sets_max = std::max(sets_max, x.sets);
      sets_sum += x.sets;
      ++placement[x.wid & 3][x.simd];
      waves.push_back(x);
    }
    printf("launch by the stamps (first entry to last exit): %.4f ms; shader clock %.3f GHz (sum of s_memtime "
           "ticks / sum of 100 MHz ticks)\n", span * 1e-5, 0.1 * static_cast<double>(sum_clocks) / sum_real);
    printf("sets per wave: min %lld, mean %.2f, max %lld (sum %lld)\n", sets_min,
           static_cast<double>(sets_sum) / n_waves, sets_max, sets_sum);
    printf("placement, waves by (wid & 3) x SIMD id of HW_ID:");
    for (int a = 0; a < 4; ++a) printf("  [%d] %d %d %d %d", a, placement[a][0], placement[a][1], placement[a][2],
                                       placement[a][3]);
    printf("\n");

    // (a) inside a SIMD: the waves wid, wid + 4, wid + 8, wid + 12 of a workgroup; (b) inside a CU
    std::map<int, std::vector<double>> by_simd, by_cu;
    std::map<int, int> xcc_of;
    std::vector<double> entries;
    for (const Wave& x : waves) {
      by_simd[x.block * 4 + (x.wid & 3)].push_back(x.out);
      by_cu[x.block].push_back(x.out);
      xcc_of[x.block] = x.xcc;
      entries.push_back(x.in);
    }
    auto report = [&](const char* what, const std::map<int, std::vector<double>>& groups) {
      std::vector<double> first, last, spread;
      for (const auto& g : groups) {
        first.push_back(minof(g.second));
        last.push_back(maxof(g.second));
        spread.push_back(maxof(g.second) - minof(g.second));
      }
      printf("%s (%zu groups), %% of the launch: first finish median %.2f (min %.2f), last finish median %.2f (max "
             "%.2f), last - first median %.2f, max %.2f\n", what, groups.size(), median(first), minof(first),
             median(last), maxof(last), median(spread), maxof(spread));
    };
    printf("entry to the set loop: median %.2f, max %.2f %% of the launch\n", median(entries), maxof(entries));
    report("(a) inside a SIMD", by_simd);
    report("(b) inside a CU  ", by_cu);
    // (c) per-CU last finish, all and by XCC id
    std::vector<double> cu_last;
    std::map<int, std::vector<double>> by_xcc;
    for (const auto& g : by_cu) {
      cu_last.push_back(maxof(g.second));
      by_xcc[xcc_of[g.first]].push_back(maxof(g.second));
    }
    printf("(c) last finish per CU: min %.2f, median %.2f, max %.2f; max - median %.2f, max - min %.2f\n",
           minof(cu_last), median(cu_last), maxof(cu_last), maxof(cu_last) - median(cu_last),
           maxof(cu_last) - minof(cu_last));
    for (const auto& g : by_xcc)
      printf("    XCC %d: %zu CUs, last finish min %.2f, median %.2f, max %.2f\n", g.first, g.second.size(),
             minof(g.second), median(g.second), maxof(g.second));
    // (d) residency: the waves' time inside the loop against 4096 x the launch
    double idle = 0.0;
    for (const Wave& x : waves) idle += 100.0 - x.out;
    printf("(d) sum of (exit - entry) over the waves = %.2f %% of %d x the launch by the stamps (%.2f %% of %d x the "
           "launch by the events); mean wait for the last wave behind the exit %.2f %% of the launch\n",
           static_cast<double>(sum_real) / (n_waves * span) * 100.0, n_waves,
           static_cast<double>(sum_real) * 1e-5 / (n_waves * kernel_ms) * 100.0, n_waves, idle / n_waves);
    printf("    sum of s_memtime ticks inside the loop: %.4e (SQ_WAVE_CYCLES counts quad-cycles: / 4 = %.4e)\n",
           static_cast<double>(sum_clocks), static_cast<double>(sum_clocks) / 4.0);
    fflush(stdout);
  }
  snf_free(d_wave);
  snf_free(d_out);
  snf_free(d_stamps);
  snf_plan_destroy(plan);
  return 0;
}
