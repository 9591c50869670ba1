// fbank256x2_kernel: the register-resident 512-point kernel (kernels_fbank512.hip: same wave mapping, register
// passes, unpack tile and MFMA mel chain; same table blob, built with `dual` by fast512_tables.cpp) on
// frames that pad to 256 samples (8 kHz audio, 10-16 ms windows at 16 kHz): TWO real frames per 16-lane
// row, packed as one complex signal z[n] = x_a[n] + i x_b[n], n < 256.  The same two register passes as
// there transform it, and the spectra separate without a twiddle: X_a[k] = (Z[k] + conj Z[256 - k]) / 2,
// X_b[k] = (Z[k] - conj Z[256 - k]) / 2i.  A wave64 therefore works on 8 frames per iteration instead of
// the 4 zero-extended ones of the 512-point form (half the transform arithmetic per frame); the mel
// filterbank (129 bins, the same MFMA block tables, built without the zero-tap spreading) and the DCT
// run once per sub-frame.  Flat scheduling only: VTLN batches keep the 512-point form.
// The two real transforms share their roundings (the last bits of X_a depend on x_b), so the pairing is
// a property of the utterance, not of the batch: frames 2 m and 2 m + 1 of one utterance (PairRec table,
// built once per offsets table by build_pair_table_kernel); an odd last frame is transformed with itself.
//
// Restates the same [KALDI-UPSTREAM] per-frame recipe as kernels_mel.hip (feature-window.cc
// ProcessWindow order, feature-fbank.cc, feature-mfcc.cc, MelBanks::Compute), reached by the
// reference at shennong/processor/base.py:429-431.
#include <float.h>

#include "fast512_launch.h"
#include "device_fft.h"

namespace snf {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace {

// the LDS layout of the family (snf_internal.h) under the names the kernel body uses
constexpr int kMaxWaves = kFast512MaxWaves;
constexpr int kTileRow = kFast512TileRow;
constexpr int kFrameTileBytes = kFast512TileBytes;
constexpr int kFastHeaderFloats = kFast512HeaderFloats;

}  // namespace

constexpr int kDualSub = 136;  // float offset of sub-frame b inside a row's power tile (129 bins + pad)

template <int NJ, int KIND, int ENERGY, bool DITHER, bool SNIP>
__global__ __launch_bounds__(kMaxWaves * 64, 4) void fbank256x2_kernel(const Fast512Params p,
                                                                     const BatchArgs b,
                                                                     float* __restrict__ out,
                                                                     double* __restrict__ energy_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tab = reinterpret_cast<float*>(smem);
  for (int i = threadIdx.x; i < p.table_floats; i += blockDim.x) tab[i] = p.tables[i];
  __syncthreads();
  const float2* __restrict__ t_win = reinterpret_cast<const float2*>(tab + kFastHeaderFloats);
  const float2* __restrict__ t_tw16 = t_win + 16 * 18;
  const float4* __restrict__ t_mm_a = reinterpret_cast<const float4*>(tab + p.off_mm_a);
  const float* __restrict__ t_lifter = tab + p.off_lifter;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l = lane & 15, q = lane >> 4;
  const int tab_bytes = (p.table_floats * 4 + 255) & ~255;
  char* wave_base = smem + tab_bytes + (wid * 4 + q) * kFrameTileBytes;
  float2* tile = reinterpret_cast<float2*>(wave_base);
  float* ptile = reinterpret_cast<float*>(wave_base) + q * 16;   // sub-frame a at 0, b at kDualSub
  tile[l * kTileRow + 16] = make_float2(0.0f, 0.0f);  // (padding column: see fbank512_kernel)
  const int mj = lane & 3;
  const float* __restrict__ mm_lane = tab + p.off_mm_lane;
  const int mm_start = reinterpret_cast<const int*>(mm_lane)[lane];
  const int mm_out = reinterpret_cast<const int*>(mm_lane)[64 + lane];
  const float mm_f1 = mm_lane[128 + lane], mm_f2 = mm_lane[192 + lane], mm_f3 = mm_lane[256 + lane];
  float* __restrict__ mtile =
      reinterpret_cast<float*>(smem + tab_bytes + (wid * 4 + mj) * kFrameTileBytes) + mj * 16;

  const float win_len_f = static_cast<float>(p.win_len), inv_win_len = 1.0f / win_len_f;
  const int n_waves = blockDim.x >> 6;
  // (the fix-up launch walks a list whose length only the device knows: BatchArgs::n_pairs_dev)
  const int64_t n_pairs = b.n_pairs_dev ? static_cast<int64_t>(*b.n_pairs_dev) : b.n_pairs;
  const int64_t n_sets = (n_pairs + 3) >> 2;
  const int64_t set_stride = static_cast<int64_t>(gridDim.x) * n_waves;
  const int64_t last_pair = n_pairs - 1;
  // a pair record as two 16-byte halves: {start_a, start_b} and {frame_a, utt1, flags}
  auto starts_of = [&](int64_t pi) -> longlong2 {
    return reinterpret_cast<const longlong2*>(b.pair_tab + (pi < last_pair ? pi : last_pair))[0];
  };
  auto meta_of = [&](int64_t pi) -> int4 {
    return reinterpret_cast<const int4*>(b.pair_tab + (pi < last_pair ? pi : last_pair))[1];
  };
  // NJ = 13: the 25 ms / 8 kHz window (200 samples: only element j = 12 can fall outside the window)
  const bool in_last = l + 16 * (NJ - 1) < p.win_len;
  auto in_window = [&](int j) -> bool {
    if (NJ == 13) return j < NJ - 1 || in_last;
    return l + 16 * j < p.win_len;
  };
  // Sample ingest (round 6; first built for kernels_fbank1024x2.hip): the two frames of a pair lie in ONE span of
  // the utterance - frame b starts `off_b` = start_b - start_a samples (0 ... the frame shift) behind frame a -
  // which comes in as 16-byte pieces, lane l of the row fetching pieces l, l + 16, ... (3 wave instructions for a
  // 25 ms / 10 ms pair at 8 kHz, where a 16-bit load per element and frame took 26: the texture addresser takes a
  // wave instruction per 64 addresses whatever their width), is laid down in the row's LDS tile at the top of
  // the next iteration and read back element by element.  The last bytes of a span that do not fill a piece come
  // through one 16-bit load of the first lanes: no load reaches beyond the span, i.e. beyond the utterance.
  typedef int int4_a2 __attribute__((ext_vector_type(4), aligned(2)));
  constexpr int NP = NJ == 13 ? 3 : 4;   // pieces per lane: spans of up to 384 / 512 samples (launch_fbank512)
  int4_a2 qv[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) qv[i] = int4_a2{0, 0, 0, 0};
  int tailv = 0, offb_next = 0;
  auto load_span = [&](const longlong2 st) __attribute__((always_inline)) {
    const char* __restrict__ pa = reinterpret_cast<const char*>(b.wave + st.x);
    const int ob = static_cast<int>(st.y - st.x);
    const int span_bytes = 2 * (ob + p.win_len);
    const int nf = span_bytes >> 4, nt = (span_bytes & 15) >> 1;
#pragma unroll
    for (int i = 0; i < NP; ++i)
      qv[i] = *reinterpret_cast<const int4_a2*>(pa + (l + 16 * i < nf ? 16 * (l + 16 * i) : 0));
    tailv = *reinterpret_cast<const short*>(pa + (l < nt ? 16 * nf + 2 * l : 0));
    offb_next = ob;
  };
  int64_t set = static_cast<int64_t>(blockIdx.x) * n_waves + wid;
  longlong2 next_starts = {0, 0};
  int4 meta_next = {0, 0, 0, 0};
  if (set < n_sets) {
    load_span(starts_of(set * 4 + q));
    next_starts = starts_of((set + set_stride) * 4 + q);
    meta_next = meta_of(set * 4 + q);
  }
  // Loads and stores share one in-order counter (vmcnt): the wait for the prefetched samples at the top of
  // the loop also covers the output stores issued after them.  Here the prefetch is settled by hand in
  // front of the iteration's first store (and once before the loop, so that no path into the loop head
  // carries a pending load): 0.32 against 0.34 ms per 1.19 M frames.  (The same change on fbank512_kernel
  // measured 5-10 % SLOWER, wherever the settle point was put, and was dropped there.)
  auto settle_prefetch = [&]() {
#pragma unroll
    for (int i = 0; i < NP; ++i) asm volatile("" : "+v"(qv[i]));
    asm volatile("" : "+v"(tailv), "+v"(offb_next));
    asm volatile("" : "+v"(next_starts.x), "+v"(next_starts.y));
    asm volatile("" : "+v"(meta_next.x), "+v"(meta_next.y), "+v"(meta_next.z), "+v"(meta_next.w));
  };
  settle_prefetch();
  for (; set < n_sets; set += set_stride) {
    const int4 meta = meta_next;
    int4 mmeta = meta_of(set * 4 + mj);  // (the MFMA view's pair, below)
    const int64_t ga = static_cast<int64_t>(static_cast<unsigned>(meta.x)) | (static_cast<int64_t>(meta.y) << 32);
    const bool valid_a = set * 4 + q <= last_pair, valid_b = valid_a && (meta.w & 4) != 0;
    const int edge_a = (meta.w & 1) ? meta.z : 0, edge_b = (meta.w & 2) ? meta.z : 0;

    // ---- A: DC removal, pre-emphasis, window (per sub-frame: xe = frame a, xo = frame b) ---------------
    float4 win4[(NJ + 1) / 2];
    read_quads<(NJ + 1) / 2>(t_win + l * 18, win4);
    unsigned dk[4] = {0, 0, 0, 0};
    if (DITHER) {
      // (keyed by the frames' places in their utterance - PairRec.utt1 - not in the batch: snf_internal.h)
      const int64_t du = meta.z > 0 ? meta.z - 1 : 0;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const unsigned long long k =
            wave_noise_id(b, du, ga + s2 - b.frame_offsets[du]) ^ p.seed;
        dk[2 * s2] = fmix32(static_cast<unsigned>(k));
        dk[2 * s2 + 1] = fmix32(static_cast<unsigned>(k >> 32) ^ dk[2 * s2]);
      }
    }
    float xe[NJ], xo[NJ];
    float part_a = 0.0f, part_b = 0.0f;
    constexpr bool kIntSum = !DITHER && SNIP;  // (integer sums are exact: see fbank512_kernel)
    int sum_a = 0, sum_b = 0;
    {
      // the span of this iteration's pair: registers -> the row's tile (whole pieces, then the tail), elements back
      const int ob = offb_next;
      const int span_bytes = 2 * (ob + p.win_len);
      const int nf = span_bytes >> 4, nt = (span_bytes & 15) >> 1;
      char* __restrict__ sb = reinterpret_cast<char*>(tile);
#pragma unroll
      for (int i = 0; i < NP; ++i)
        if (l + 16 * i < nf)
          *reinterpret_cast<int4*>(sb + 16 * (l + 16 * i)) = make_int4(qv[i].x, qv[i].y, qv[i].z, qv[i].w);
      if (l < nt) *reinterpret_cast<short*>(sb + 16 * nf + 2 * l) = static_cast<short>(tailv);
      wave_lds_sync();
      const short* __restrict__ sa = reinterpret_cast<const short*>(tile) + l;
      const short* __restrict__ sbb = sa + ob;
      int va[NJ], vb[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        va[j] = sa[16 * j];
        vb[j] = sbb[16 * j];
      }
      lds_wait();
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        xe[j] = static_cast<float>(va[j]);
        xo[j] = static_cast<float>(vb[j]);
        if (kIntSum) {
          sum_a += in_window(j) ? va[j] : 0;
          sum_b += in_window(j) ? vb[j] : 0;
        }
      }
      wave_lds_sync();
    }
    if (!SNIP && (edge_a | edge_b) != 0) {
      // [KALDI-UPSTREAM] ExtractWindow, snip_edges = false: reflected samples for the frames that reach
      // outside their utterance (their prefetched samples came from a clamped window)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int edge = s2 ? edge_b : edge_a;
        if (edge != 0 && (s2 ? valid_b : valid_a)) {
          const int64_t u = edge - 1;
          const int64_t s0 = b.sample_offsets[u], n = b.sample_offsets[u + 1] - s0;
          const int64_t rel =
              (ga + s2 - b.frame_offsets[u]) * p.win_shift + p.win_shift / 2 - p.win_len / 2;
          const int16_t* __restrict__ w0 = b.wave + s0;
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            if (in_window(j)) {
              int64_t k = rel + l + 16 * j;
              while (k < 0 || k >= n) k = k < 0 ? -k - 1 : 2 * n - 1 - k;
              const float v = static_cast<float>(w0[k]);
              if (s2) xo[j] = v; else xe[j] = v;
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (DITHER) {  // Kaldi dithers before the DC removal
        xe[j] += p.dither * gauss_pair(dk[0], dk[1], static_cast<unsigned>(l + 16 * j)).x;
        xo[j] += p.dither * gauss_pair(dk[2], dk[3], static_cast<unsigned>(l + 16 * j)).x;
      }
      if (!kIntSum) {
        part_a += in_window(j) ? xe[j] : 0.0f;
        part_b += in_window(j) ? xo[j] : 0.0f;
      }
    }
    if (kIntSum) {
      part_a = static_cast<float>(sum_a);
      part_b = static_cast<float>(sum_b);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(xe[j]), "+v"(xo[j]) : : "memory");
    asm volatile("" : "+v"(part_a), "+v"(part_b) : : "memory");
    {  // prefetch: samples of the next set, start offsets of the set after it
      load_span(next_starts);
      next_starts = starts_of((set + 2 * set_stride) * 4 + q);
      meta_next = meta_of((set + set_stride) * 4 + q);
    }
    float nm_a = 0.0f, nm_b = 0.0f;
    if (p.remove_dc) {
      const float sa = row_sum16(part_a), sb = row_sum16(part_b);
      if (kIntSum) {
        const float qa = sa * inv_win_len, qb = sb * inv_win_len;
        nm_a = -__builtin_fmaf(__builtin_fmaf(-qa, win_len_f, sa), inv_win_len, qa);
        nm_b = -__builtin_fmaf(__builtin_fmaf(-qb, win_len_f, sb), inv_win_len, qb);
      } else {
        nm_a = -sa / win_len_f;
        nm_b = -sb / win_len_f;
      }
    }
    lds_wait();
    // the left neighbour x[n-1] is element n-1 = lane l-1 (same j), lane 15 of j-1 for lane 0
    float2 z[16];
    float er_a = 0.0f, er_b = 0.0f, ep_a = 0.0f, ep_b = 0.0f;
    float prev_a = xe[0] + nm_a, prev_b = xo[0] + nm_b;  // lane 0, j = 0: x[-1] := x[0]
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j < NJ) {
        const bool in = in_window(j);
        const float ae = xe[j] + nm_a, ao = xo[j] + nm_b;
        const float rot_a = dpp_row_ror<0x121>(ae), rot_b = dpp_row_ror<0x121>(ao);
        const float pa = l == 0 ? prev_a : rot_a, pb = l == 0 ? prev_b : rot_b;
        prev_a = rot_a;
        prev_b = rot_b;
        const float2 w = (j & 1) ? make_float2(win4[j >> 1].z, win4[j >> 1].w)
                                 : make_float2(win4[j >> 1].x, win4[j >> 1].y);  // (w[n], w[n]); 0 outside
        if (ENERGY == 1 && in) {
          er_a += ae * ae;
          er_b += ao * ao;
        }
        const float ye = (ae - p.preemph * pa) * w.x;
        const float yo = (ao - p.preemph * pb) * w.y;
        z[j] = make_float2(ye, yo);
        ep_a += ye * ye;   // (the energies of the windowed frames: the pairing decision below, ENERGY == 2)
        ep_b += yo * yo;
      } else {
        z[j] = make_float2(0.0f, 0.0f);
      }
    }
    float e_lin_a = 0.0f, e_lin_b = 0.0f;
    {
      const float ew_a = row_sum16(ep_a), ew_b = row_sum16(ep_b);
      if (ENERGY == 2) {
        e_lin_a = ew_a;
        e_lin_b = ew_b;
      } else if (ENERGY == 1) {
        e_lin_a = row_sum16(er_a);
        e_lin_b = row_sum16(er_b);
      }
      // The two frames share the roundings of one transform.  A pair of very different energies (a quiet frame
      // beside an onset, digital silence beside anything) is put down for the fix-up launch, which transforms
      // each of its frames alone and rewrites the two rows (BatchArgs::fix_tab).
      if (b.fix_tab != nullptr && valid_b && l == 0 &&
          fmaxf(ew_a, ew_b) > b.split_ratio * fminf(ew_a, ew_b)) {
        const longlong2 st = starts_of(set * 4 + q);
        const unsigned at = atomicAdd(b.fix_count, 2u);
        longlong2* rec = reinterpret_cast<longlong2*>(b.fix_tab + at);
        int4* rec_meta = reinterpret_cast<int4*>(b.fix_tab + at);
        rec[0] = make_longlong2(st.x, st.x);
        rec_meta[1] = make_int4(meta.x, meta.y, meta.z, meta.w & 1);
        const int64_t gb = ga + 1;
        rec[2] = make_longlong2(st.y, st.y);
        rec_meta[3] = make_int4(static_cast<int>(gb), static_cast<int>(gb >> 32), meta.z, (meta.w >> 1) & 1);
      }
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- B / C: the 256-point complex transform (identical to fbank512_kernel) ------------------------
    fft16_lf(z);
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) tile[k2 * kTileRow + l] = z[k2];
    wave_lds_sync();
    float2 ct[16];
    {
      float4 tw4[8];
      read_tw8_row16(t_tw16 + l * 18, tile + l * kTileRow, tw4, z);  // (cos, tan) pairs + the transposed row
#pragma unroll
      for (int m = 0; m < 16; m += 2) {
        ct[m] = make_float2(tw4[m >> 1].x, tw4[m >> 1].y);
        ct[m + 1] = make_float2(tw4[m >> 1].z, tw4[m >> 1].w);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    fft16_twin(z, ct);
    __builtin_amdgcn_sched_barrier(0);
    wave_lds_sync();

    // ---- D: separate the two spectra, power (x4 like fbank512_kernel): bins k = l + 16 k1 <= 128 --------
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < 8; ++r) tile[r * 16 + l] = z[r + 8];
    wave_lds_sync();
    float2 zpart[8];
    read8_b64_rev128(tile + (16 - l), zpart);   // zpart[k1] = Z[256 - l - 16 k1]
    float pa[8], pb[8];
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) {
      const float2 zk = z[k1], zp = zpart[k1];
      const float c_re = zk.x + zp.x, c_im = zk.y - zp.y;   // 2 X_a[k]
      const float d_re = zk.y + zp.y, d_im = zp.x - zk.x;   // 2 X_b[k]
      pa[k1] = c_re * c_re + c_im * c_im;
      pb[k1] = d_re * d_re + d_im * d_im;
    }
    if (l == 0) {  // k = 0 pairs with itself: X_a[0] = Re Z[0], X_b[0] = Im Z[0]
      pa[0] = 4.0f * z[0].x * z[0].x;
      pb[0] = 4.0f * z[0].y * z[0].y;
    }
    const float p128_a = 4.0f * z[8].x * z[8].x, p128_b = 4.0f * z[8].y * z[8].y;  // lane 0: Z[128]
    wave_lds_sync();
    settle_prefetch();
    asm volatile("" : "+v"(mmeta.x), "+v"(mmeta.y), "+v"(mmeta.w));
    // ---- E: power tiles ----------------------------------------------------------------------------------
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) {
      ptile[l + 16 * k1] = pa[k1];
      ptile[kDualSub + l + 16 * k1] = pb[k1];
    }
    if (l == 0) {
      ptile[128] = p128_a;
      ptile[kDualSub + 128] = p128_b;
    }
    wave_lds_sync();

    // ---- log-energy column ---------------------------------------------------------------------------------
    float log_e[2] = {0.0f, 0.0f};
    if (ENERGY != 0) {
      if (KIND == SNF_KIND_PLP) {
        if (l == 0) {
          if (valid_a) energy_out[ga] = static_cast<double>(e_lin_a);  // (plp_tail_kernel takes the double log)
          if (valid_b) energy_out[ga + 1] = static_cast<double>(e_lin_b);  // (plp_tail_kernel takes the double log)
        }
      } else {
        log_e[0] = fast_log(floor_eps(e_lin_a));
        log_e[1] = fast_log(floor_eps(e_lin_b));
        if (p.has_floor) {
          if (log_e[0] < p.log_energy_floor) log_e[0] = p.log_energy_floor;
          if (log_e[1] < p.log_energy_floor) log_e[1] = p.log_energy_floor;
        }
      }
    }
    float* __restrict__ row = out + ga * static_cast<int64_t>(p.out_cols);  // frame a; frame b: + out_cols

    if (KIND == SNF_KIND_SPECTROGRAM) {
      // the 129 log powers of each frame straight from the registers: lane l of the row holds bins l + 16 k1
      // (16 lanes x 4 bytes per store), lane 0 bin 128 as well; column 0 is the log energy (Kaldi's
      // SpectrogramComputer).  The powers above carry a factor 4 (see fbank512_kernel).
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        if (s2 ? valid_b : valid_a) {
          float* __restrict__ r = row + s2 * p.out_cols;
#pragma unroll
          for (int k1 = 0; k1 < 8; ++k1) {
            float v = fast_log(fmaxf(0.25f * (s2 ? pb[k1] : pa[k1]), FLT_EPSILON));
            if (k1 == 0 && l == 0) v = log_e[s2];
            r[l + 16 * k1] = v;
          }
          if (l == 0) r[128] = fast_log(fmaxf(0.25f * (s2 ? p128_b : p128_a), FLT_EPSILON));
        }
      }
      wave_lds_sync();  // the tile is reused by the next frame set
      continue;
    }
    // ---- F: mel filterbank on the matrix pipe, one chain per sub-frame ------------------------------------
    float mel[2][4];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const float4* __restrict__ bsrc = reinterpret_cast<const float4*>(mtile + kDualSub * s2 + mm_start);
      const float4* __restrict__ asrc = t_mm_a + lane;
      f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
      float4 a0 = asrc[0], x0 = bsrc[0];
      for (int t = 0; t < p.mm_quads; t += 2) {  // (mm_quads is even; the table ends with a row of zeros)
        const float4 a1 = asrc[(t + 1) * 64], x1 = bsrc[t + 1];
        acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.x, x0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.y, x0.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.z, x0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a0.w, x0.w, acc1, 0, 0, 0);
        a0 = asrc[(t + 2) * 64];
        x0 = bsrc[t + 2];
        acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.x, x1.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.y, x1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.z, x1.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a1.w, x1.w, acc1, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) mel[s2][i] = acc0[i] + acc1[i];
      if (p.mm_levels > 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float own = mel[s2][i];
          fmac_row_shl<4>(mel[s2][i], own, mm_f1);
          fmac_row_shl<8>(mel[s2][i], own, mm_f2);
          if (p.mm_levels > 3) fmac_row_shl<12>(mel[s2][i], own, mm_f3);
        }
      }
    }
    // MFMA view: lane 4 b + j -> pair j of the set
    const int64_t mga = static_cast<int64_t>(static_cast<unsigned>(mmeta.x)) | (static_cast<int64_t>(mmeta.y) << 32);
    const bool mvalid[2] = {set * 4 + mj <= last_pair, set * 4 + mj <= last_pair && (mmeta.w & 4) != 0};
    float* __restrict__ mrow = out + mga * static_cast<int64_t>(p.out_cols);
    const int mel_col = (KIND == SNF_KIND_FBANK && p.use_energy && !p.htk_compat) ? 1 : 0;
    if (KIND == SNF_KIND_FBANK || KIND == SNF_KIND_PLP) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        if (KIND == SNF_KIND_FBANK && p.use_log) {
#pragma unroll
          for (int i = 0; i < 4; ++i) mel[s2][i] = fast_log(floor_eps(mel[s2][i]));
        }
        if (mvalid[s2] && mm_out >= 0) {
          float* __restrict__ dst = mrow + s2 * p.out_cols + mel_col + mm_out;
          if (mm_out + 4 <= p.num_bins) {
            __builtin_nontemporal_store(f32x4_a4{mel[s2][0], mel[s2][1], mel[s2][2], mel[s2][3]},
                                        reinterpret_cast<f32x4_a4*>(dst));
          } else {
#pragma unroll
            for (int i = 0; i < 3; ++i)
              if (mm_out + i < p.num_bins) dst[i] = mel[s2][i];
          }
        }
        if (KIND == SNF_KIND_FBANK && p.use_energy && l == 0 && (s2 ? valid_b : valid_a))
          row[s2 * p.out_cols + (p.htk_compat ? p.num_bins : 0)] = log_e[s2];
      }
    }
    if (KIND == SNF_KIND_MFCC) {
      // log-mel of both sub-frames back to their (now idle) power tiles, then the DCT-II chains
      wave_lds_sync();
      if (mm_out >= 0) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
          *reinterpret_cast<float4*>(mtile + kDualSub * s2 + mm_out) =
              make_float4(fast_log(floor_eps(mel[s2][0])), fast_log(floor_eps(mel[s2][1])),
                          fast_log(floor_eps(mel[s2][2])), fast_log(floor_eps(mel[s2][3])));
      }
      wave_lds_sync();
      // DCT-II + lifter on the vector pipe: lane l of a row owns cepstrum l of the row's two sub-frames
      const float4* __restrict__ t_dd_v = reinterpret_cast<const float4*>(tab + p.off_dd_v);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const float4* __restrict__ dw = t_dd_v + l;
        const float4* __restrict__ dx = reinterpret_cast<const float4*>(ptile + kDualSub * s2);
        float v = 0.0f;
#pragma unroll 2
        for (int g4 = 0; g4 < p.dd_groups; ++g4) {
          const float4 w = dw[g4 * 16], x = dx[g4];
          v += w.x * x.x;
          v += w.y * x.y;
          v += w.z * x.z;
          v += w.w * x.w;
        }
        v *= t_lifter[l];
        if (l == 0 && p.use_energy) v = log_e[s2];
        int oc = l;
        if (p.htk_compat) {
          oc = l == 0 ? p.num_ceps - 1 : l - 1;
          if (l == 0 && !p.use_energy)
            v = static_cast<float>(static_cast<double>(v) * 1.4142135623730950488016887);
        }
        if ((s2 ? valid_b : valid_a) && l < p.num_ceps) row[s2 * p.out_cols + oc] = v;
      }
    }
    wave_lds_sync();  // the tile is reused by the next frame set
  }
}

// one thread per frame pair of fbank256x2_kernel (see PairRec): pair_offsets[u] = pairs of the utterances
// before u, an utterance of T frames holding (T + 1) / 2 of them.
__global__ void build_pair_table_kernel(const int64_t* __restrict__ frame_offsets,
                                        const int64_t* __restrict__ sample_offsets,
                                        const int64_t* __restrict__ pair_offsets, int64_t n_utts,
                                        int64_t n_pairs, int win_shift, int win_len, int snip_edges,
                                        PairRec* __restrict__ pairs) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= n_pairs) return;
  const int64_t u = find_utt(pair_offsets, n_utts, g);
  const int64_t s0 = sample_offsets[u], n = sample_offsets[u + 1] - s0;
  const int64_t f0 = frame_offsets[u], n_frames = frame_offsets[u + 1] - f0;
  const int64_t f = 2 * (g - pair_offsets[u]);
  const bool has_b = f + 1 < n_frames;
  PairRec r;
  r.frame_a = f0 + f;
  r.utt1 = static_cast<int32_t>(u + 1);  // (always: the dither stream is keyed per utterance; `flags` marks edges)
  r.flags = has_b ? 4 : 0;
  int64_t start[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const int64_t fr = f + (has_b ? s2 : 0);
    if (snip_edges) {
      start[s2] = s0 + fr * win_shift;
    } else {  // (as build_frame_start_kernel)
      const int64_t rel = fr * win_shift + win_shift / 2 - win_len / 2;
      int64_t safe = rel < 0 ? 0 : rel;
      if (safe + win_len > n) safe = n - win_len;
      start[s2] = s0 + safe;
      if (rel < 0 || rel + win_len > n) r.flags |= 1 << s2;
    }
  }
  r.start_a = start[0];
  r.start_b = start[1];
  pairs[g] = r;
}

int launch_build_pair_table(const int64_t* d_frame_offsets, const int64_t* d_sample_offsets,
                            const int64_t* d_pair_offsets, int64_t n_utts, int64_t n_pairs, int win_shift,
                            int win_len, int snip_edges, PairRec* d_pairs, hipStream_t stream) {
  if (n_pairs <= 0) return SNF_OK;
  hipLaunchKernelGGL(build_pair_table_kernel, dim3(static_cast<unsigned>((n_pairs + 255) / 256)),
                     dim3(256), 0, stream, d_frame_offsets, d_sample_offsets, d_pair_offsets, n_utts,
                     n_pairs, win_shift, win_len, snip_edges, d_pairs);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

// flat batches of FBANK / MFCC / SPECTROGRAM / PLP plans (launch_fbank512 routes here when `p.dual`)
int launch_fbank256x2(const Fast512Params& p, const BatchArgs& b, float* out, int out_cols,
                      double* energy_out, hipStream_t stream) {
  Fast512Params q = p;
  q.out_cols = out_cols;
  const bool per_utt = b.blk_utt != nullptr;
  int n_waves;
  size_t lds;
  if (int rc = fast512_workgroup(p, per_utt, &n_waves, &lds)) return rc;
  if (per_utt || p.fused_delta != 0)
    return set_error(SNF_E_RUNTIME, "fast512: the dual tables serve flat batches only");
  if (!b.pair_tab || b.n_pairs <= 0) return set_error(SNF_E_RUNTIME, "fast512: no frame pair table");
  const int64_t n_sets8 = (b.n_pairs + 3) / 4;
  int64_t blocks8 = (n_sets8 + n_waves - 1) / n_waves;
  const int64_t max_blocks8 = 256 * 4 * (kMaxWaves / n_waves);
  if (blocks8 > max_blocks8) blocks8 = max_blocks8;
  const dim3 block8(n_waves * 64);
  // (the 13-row form fetches spans of up to 384 samples, the 16-row form of up to 512: fast512_dual_eligible)
  const int nj = (p.win_len + 15) / 16 == 13 && p.win_len + p.win_shift <= 384 ? 13 : 16;
  auto run_dual = [&](const BatchArgs& b, const dim3 grid8) -> int {
    return with_nj_kind_energy_dither_snip(nj, p, [&](auto nj_c, auto kind, auto energy, auto dither, auto snip) {
      // (the plan builds dual tables for the four kinds above only; any other has ever meant the PLP form)
      constexpr int KIND = decltype(kind)::value == SNF_KIND_ENERGY ? SNF_KIND_PLP : decltype(kind)::value;
      const auto kernel = fbank256x2_kernel<decltype(nj_c)::value, KIND, decltype(energy)::value,
                                            decltype(dither)::value, decltype(snip)::value>;
      if (lds > 64 * 1024)
        SNF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
      hipLaunchKernelGGL(kernel, grid8, block8, lds, stream, q, b, out, energy_out);
      SNF_HIP_CHECK(hipGetLastError());
      return static_cast<int>(SNF_OK);
    });
  };
  int rc = run_dual(b, dim3(static_cast<unsigned>(blocks8)));
  if (rc != SNF_OK || b.fix_tab == nullptr) return rc;
  // the fix-up launch: the frames of the pairs the first launch put down (two records of one frame each), as
  // many as `fix_count` says when the first launch is done - a grid sized for a twentieth of the pairs walks
  // whatever the list holds
  BatchArgs bf = b;
  bf.pair_tab = b.fix_tab;
  bf.n_pairs_dev = b.fix_count;
  bf.fix_tab = nullptr;
  bf.fix_count = nullptr;
  int64_t blocks_fix = (blocks8 + 9) / 10;
  if (blocks_fix < 16) blocks_fix = blocks8 < 16 ? blocks8 : 16;
  return run_dual(bf, dim3(static_cast<unsigned>(blocks_fix)));
}

}  // namespace snf
