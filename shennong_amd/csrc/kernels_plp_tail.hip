// RASTA filtering and the PLP tail (reference plp.py:64-146, :548-626): rasta_kernel, the three tail kernels -
// plp_tail_kernel for any shape up to 126 bins and order 63, plp_tail_small_kernel up to 32 bins and order 16,
// plp_tail_exact_kernel for the reference's defaults - and their launchers.  Which tail runs: plp_tail_route,
// post_route.h.
#include <float.h>

#include "post_route.h"
#include "snf_internal.h"
#include "utt_search.h"

namespace snf {

// ------------------------------------------------------------------------------------------------
// RASTA: one thread per (utterance, mel bin), sequential over the utterance's frames.  Log domain,
// float64 IIR state, direct form II transposed exactly like scipy.signal.lfilter, first four frames
// emit exp(0) = 1 and prime the FIR state with zi * x[0] (reference plp.py:87-88, :121-146).
// ------------------------------------------------------------------------------------------------
__global__ void rasta_kernel(float* __restrict__ mel, const BatchArgs b, const int nb) {
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (tid >= b.n_utts * nb) return;
  const int64_t u = tid / nb;
  const int bin = static_cast<int>(tid - u * nb);
  const int64_t f0 = b.frame_offsets[u], f1 = b.frame_offsets[u + 1];
  const double b0 = 0.2, b1 = 0.1, b2 = 0.0, b3 = -0.1, b4 = -0.2, a1 = -0.94;
  double zi3 = b4, zi2 = b3 + zi3, zi1 = b2 + zi2, zi0 = b1 + zi1;
  double z0 = 0, z1 = 0, z2 = 0, z3 = 0;
  float first[4];
  int count = 0;
  for (int64_t t = f0; t < f1; ++t, ++count) {
    float* cell = mel + t * nb + bin;
    // (the reference takes numpy's float32 log of its float32 frame, plp.py:126, and the C oracle glibc's logf: both
    // correctly rounded in all but a handful of arguments.  The device's logf errs by up to 2 ulp, 2e-6 on a log
    // energy of 14, which the filter's recursion carries into every later frame: against the float64 statement the
    // filtered rows were up to 7 times as far off as the oracle's, tests/test_plp_tail_gpu.py.  The double logarithm
    // rounded once gives the reference's value, as log_pitch_of does below.)
    const float x = static_cast<float>(log(static_cast<double>(*cell + FLT_EPSILON)));
    double y = 0.0;
    if (count < 4) {
      first[count] = x;
      if (count == 3) {
        const double x0 = first[0];
        z0 = zi0 * x0; z1 = zi1 * x0; z2 = zi2 * x0; z3 = zi3 * x0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double xt = first[k];
          z0 = z1 + xt * b1;
          z1 = z2 + xt * b2;
          z2 = z3 + xt * b3;
          z3 = xt * b4;
        }
      }
    } else {
      const double xd = x;
      y = z0 + b0 * xd;
      z0 = (z1 + xd * b1) - y * a1;
      z1 = z2 + xd * b2;
      z2 = z3 + xd * b3;
      z3 = xd * b4;
    }
    *cell = expf(static_cast<float>(y));
  }
}

int launch_rasta(float* mel, const BatchArgs& b, int num_bins, hipStream_t stream) {
  const int64_t total = b.n_utts * num_bins;
  if (total <= 0 || b.total_frames <= 0) return SNF_OK;
  const int threads = 64;
  hipLaunchKernelGGL(rasta_kernel, dim3(static_cast<unsigned>((total + threads - 1) / threads)),
                     dim3(threads), 0, stream, mel, b, num_bins);
  SNF_HIP_CHECK(hipGetLastError());
  return SNF_OK;
}

// x^e as the reference forms it: numpy's float32 power and glibc's powf are correctly rounded in all but a handful
// of arguments, the device's powf is good to an ulp - and the Durbin recursion behind it amplifies that ulp up to
// 5e4 times on a spectrum nine decades wide.  The double power rounded once gives the reference's value.
__device__ __forceinline__ float pow_rounded_once(float x, float e) {
  return static_cast<float>(pow(static_cast<double>(x), static_cast<double>(e)));
}

// ------------------------------------------------------------------------------------------------
// PLP tail: equal loudness -> cube-root compression -> IDFT to autocorrelation -> Durbin ->
// LPC to cepstrum -> lifter/scale -> energy -> HTK reorder.  One thread per frame
// (reference plp.py:587-626; Durbin / IDFT bases are [KALDI-UPSTREAM] mel-computations.cc /
// feature-functions.cc wrapped at plp.py:601 and :473).
// ------------------------------------------------------------------------------------------------
__global__ void plp_tail_kernel(const PlpParams p, const BatchArgs b,
                                const float* __restrict__ mel, const double* __restrict__ energy,
                                float* __restrict__ out) {
  // The reference's arithmetic, operation by operation (tests/test_plp_tail_gpu.py holds the kernel to the float32
  // oracle at the parity tolerance on spectra where Durbin amplifies a last-place difference past it): no product
  // is fused into the sum behind it, here and in plp_tail_small_kernel.
#pragma clang fp contract(off)
  const int64_t g = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= b.total_frames) return;
  const int nb = p.num_bins, order = p.lpc_order, nc = p.num_ceps;
  int warp_id = 0;
  if (b.utt_warp) warp_id = b.utt_warp[find_utt(b.frame_offsets, b.n_utts, g)];
  const float* __restrict__ eql = p.eql + warp_id * nb;
  float m[kMaxBins + 2];
  for (int i = 0; i < nb; ++i) {
    float v = mel[g * nb + i] * eql[i];
    m[i + 1] = pow_rounded_once(v, p.compress_factor);
  }
  m[0] = m[1];
  m[nb + 1] = m[nb];
  float ac[kMaxLpc + 1], lpc[kMaxLpc], tmp[kMaxLpc], cep[kMaxLpc];
  for (int i = 0; i <= order; ++i) {
    const float* __restrict__ basis = p.idft + i * (nb + 2);
    float s = 0.0f;
    for (int j = 0; j < nb + 2; ++j) s += basis[j] * m[j];
    ac[i] = s;
  }
  // Durbin recursion
  float E = ac[0];
  for (int i = 0; i < order; ++i) lpc[i] = 0.0f;
  for (int i = 0; i < order; ++i) {
    float ki = ac[i + 1];
    for (int j = 0; j < i; ++j) ki += lpc[j] * ac[i - j];
    ki = ki / E;
    float c = 1 - ki * ki;
    if (c < 1.0e-5f) c = 1.0e-5f;
    E *= c;
    tmp[i] = -ki;
    for (int j = 0; j < i; ++j) tmp[j] = lpc[j] - ki * lpc[i - j - 1];
    for (int j = 0; j <= i; ++j) lpc[j] = tmp[j];
  }
  const float res_f = static_cast<float>(-log(1.0 / static_cast<double>(E)));
  const double res = fmax(static_cast<double>(res_f), DBL_EPSILON);
  // LPC -> cepstrum: Python-float (double) accumulation, float32 storage (reference plp.py:149-168)
  for (int i = 0; i < order; ++i) {
    double sum = 0.0;
    for (int j = 0; j < i; ++j)
      sum += static_cast<double>(i - j) * static_cast<double>(lpc[j]) * static_cast<double>(cep[i - j - 1]);
    cep[i] = static_cast<float>(-static_cast<double>(lpc[i]) - sum / static_cast<double>(i + 1));
  }
  float* __restrict__ row = out + g * nc;
  const bool floor_it = p.has_floor;
  for (int c = 0; c < nc; ++c) {
    float v = c == 0 ? static_cast<float>(res) : cep[c - 1];
    if (p.lifter) v *= p.lifter[c];
    if (p.cepstral_scale != 1.0f) v *= p.cepstral_scale;
    if (c == 0 && p.use_energy) {
      // shennong's PLP floors with float64 eps and takes a double log (reference plp.py:191-193); the mel
      // kernels hand over the linear frame energy
      double le = log(fmax(energy[g], DBL_EPSILON));
      if (floor_it && le < p.log_energy_floor) le = p.log_energy_floor;
      v = static_cast<float>(le);
    }
    int oc = c;
    if (p.htk_compat) oc = c == 0 ? nc - 1 : c - 1;
    row[oc] = v;
  }
}

// Same arithmetic, same order, for the usual small shapes (num_bins <= 32, lpc_order <= 16): every
// array has a compile-time bound and stays in registers (the generic kernel above indexes its arrays
// at run time, i.e. from scratch memory), and the 64 mel rows of a workgroup are staged through LDS
// with coalesced loads.
template <int NBMAX, int ORDMAX>
__global__ __launch_bounds__(64) void plp_tail_small_kernel(const PlpParams p, const BatchArgs b,
                                                            const float* __restrict__ mel,
                                                            const double* __restrict__ energy,
                                                            float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float rows[64 * NBMAX];
  const int nb = p.num_bins, order = p.lpc_order, nc = p.num_ceps;
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * 64;
  const int64_t limit = b.total_frames * nb;
  for (int i = threadIdx.x; i < 64 * nb; i += 64) {
    const int64_t a = g0 * nb + i;
    rows[i] = a < limit ? mel[a] : 1.0f;
  }
  __syncthreads();
  const int64_t g = g0 + threadIdx.x;
  if (g >= b.total_frames) return;
  int warp_id = 0;
  if (b.utt_warp) warp_id = b.utt_warp[find_utt(b.frame_offsets, b.n_utts, g)];
  const float* __restrict__ eql = p.eql + warp_id * nb;
  float m[NBMAX + 2];
#pragma unroll
  for (int i = 0; i < NBMAX; ++i) {
    m[i + 1] = 0.0f;
    if (i < nb) {
      const float v = rows[threadIdx.x * nb + i] * eql[i];
      m[i + 1] = pow_rounded_once(v, p.compress_factor);
    }
  }
  m[0] = m[1];
  {
    float last = m[1];
#pragma unroll
    for (int i = 1; i <= NBMAX; ++i) if (i == nb) last = m[i];
#pragma unroll
    for (int i = 1; i <= NBMAX + 1; ++i) if (i == nb + 1) m[i] = last;
  }
  float ac[ORDMAX + 1], lpc[ORDMAX], tmp[ORDMAX], cep[ORDMAX];
#pragma unroll
  for (int i = 0; i <= ORDMAX; ++i) {
    ac[i] = 0.0f;
    if (i <= order) {
      const float* __restrict__ basis = p.idft + i * (nb + 2);
      float s = 0.0f;
#pragma unroll
      for (int j = 0; j < NBMAX + 2; ++j)
        if (j < nb + 2) s += basis[j] * m[j];
      ac[i] = s;
    }
  }
  float E = ac[0];
#pragma unroll
  for (int i = 0; i < ORDMAX; ++i) lpc[i] = tmp[i] = cep[i] = 0.0f;
#pragma unroll
  for (int i = 0; i < ORDMAX; ++i) {
    if (i < order) {
      float ki = ac[i + 1];
#pragma unroll
      for (int j = 0; j < ORDMAX; ++j)
        if (j < i) ki += lpc[j] * ac[i - j];
      ki = ki / E;
      float c = 1 - ki * ki;
      if (c < 1.0e-5f) c = 1.0e-5f;
      E *= c;
      tmp[i] = -ki;
#pragma unroll
      for (int j = 0; j < ORDMAX; ++j)
        if (j < i) tmp[j] = lpc[j] - ki * lpc[i - j - 1];
#pragma unroll
      for (int j = 0; j < ORDMAX; ++j)
        if (j <= i) lpc[j] = tmp[j];
    }
  }
  const float res_f = static_cast<float>(-log(1.0 / static_cast<double>(E)));
  const double res = fmax(static_cast<double>(res_f), DBL_EPSILON);
#pragma unroll
  for (int i = 0; i < ORDMAX; ++i) {
    if (i < order) {
      double sum = 0.0;
#pragma unroll
      for (int j = 0; j < ORDMAX; ++j)
        if (j < i)
          sum += static_cast<double>(i - j) * static_cast<double>(lpc[j]) *
                 static_cast<double>(cep[i - j - 1]);
      cep[i] = static_cast<float>(-static_cast<double>(lpc[i]) - sum / static_cast<double>(i + 1));
    }
  }
  float* __restrict__ row = out + g * nc;
#pragma unroll
  for (int c = 0; c <= ORDMAX; ++c) {
    if (c < nc) {
      float v = static_cast<float>(res);
#pragma unroll
      for (int k = 1; k <= ORDMAX; ++k) if (k == c) v = cep[k - 1];
      if (p.lifter) v *= p.lifter[c];
      if (p.cepstral_scale != 1.0f) v *= p.cepstral_scale;
      if (c == 0 && p.use_energy) {
        double le = log(fmax(energy[g], DBL_EPSILON));  // (linear frame energy from the mel kernel)
        if (p.has_floor && le < p.log_energy_floor) le = p.log_energy_floor;
        v = static_cast<float>(le);
      }
      int oc = c;
      if (p.htk_compat) oc = c == 0 ? nc - 1 : c - 1;
      row[oc] = v;
    }
  }
}

// x^e for the PLP compression exponent e = float(1/3) (the reference's compress_factor, plp.py:588) and
// x >= 0.  Hardware log2 / exp2 give x^(1/3) to ~1e-6; one Newton step on y^3 = x takes it to float
// round-off; a second one with the residual x - y^3 formed exactly (the roundings of y*y and of (y*y)*y
// recovered with fused multiply-adds) leaves half an ulp; the distance of float(1/3) from 1/3 is the factor
// 1 + (e - 1/3) ln x.  ~28 vector instructions against ~120 for the correctly-rounded powf, within 1-2 ulp
// of it.
__device__ __forceinline__ float pow_third(float x, float e) {
  // (the hardware log2 takes a subnormal for zero: an energy below 1e-30 - not reachable from int16 audio -
  // is scaled by 2^96 on the way in and by 2^(-96 e) on the way out; no branch)
  const bool tiny = x < 1.0e-30f;
  x *= tiny ? 7.9228162514264338e28f : 1.0f;
  const float l2 = __builtin_amdgcn_logf(x);                    // log2 x
  const float y0 = __builtin_amdgcn_exp2f(l2 * 0.33333334f);
  const float r = x * __builtin_amdgcn_rcpf(y0 * y0 * y0);      // x / y0^3 = 1 + O(1e-6)
  const float y1 = y0 * __builtin_fmaf(r, 0.33333334f, 0.66666669f);   // y0 (2 + r) / 3
  const float sq = y1 * y1, sq_err = __builtin_fmaf(y1, y1, -sq);
  const float cu = sq * y1, cu_err = __builtin_fmaf(sq, y1, -cu) + sq_err * y1;  // y1^3 = cu + cu_err
  const float res = (x - cu) - cu_err;
  float y = __builtin_fmaf(res, __builtin_amdgcn_rcpf(3.0f * sq), y1);
  const float d = static_cast<float>(static_cast<double>(e) - 1.0 / 3.0);
  y = __builtin_fmaf(y * d, l2 * 0.69314718f, y);
  y *= tiny ? __builtin_amdgcn_exp2f(-96.0f * e) : 1.0f;
  return x > 0.0f ? y : 0.0f;
}

// One frame of the tail in the reference's arithmetic with compile-time bounds: plp_tail_kernel's operations in its
// order (the double power rounded once, products and sums rounded apart, -log(1 / E) and the cepstrum recursion in
// double), for plp_tail_exact_kernel<.., REF = true>.
template <int NB, int ORD>
__device__ __forceinline__ void plp_reference_frame(const float* __restrict__ row, const float* __restrict__ eql,
                                                    const float* __restrict__ basis, float compress_factor,
                                                    double* res_out, float* cep) {
#pragma clang fp contract(off)
  float m[NB + 2];
#pragma unroll 1
  for (int i = 0; i < NB; ++i) m[i + 1] = pow_rounded_once(row[i] * eql[i], compress_factor);
  m[0] = m[1];
  m[NB + 1] = m[NB];
  float ac[ORD + 1], lpc[ORD], tmp[ORD];
#pragma unroll
  for (int i = 0; i <= ORD; ++i) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < NB + 2; ++j) s += basis[i * (NB + 2) + j] * m[j];
    ac[i] = s;
  }
  float E = ac[0];
#pragma unroll
  for (int i = 0; i < ORD; ++i) lpc[i] = tmp[i] = cep[i] = 0.0f;
#pragma unroll
  for (int i = 0; i < ORD; ++i) {
    float ki = ac[i + 1];
#pragma unroll
    for (int j = 0; j < i; ++j) ki += lpc[j] * ac[i - j];
    ki = ki / E;
    float c = 1 - ki * ki;
    if (c < 1.0e-5f) c = 1.0e-5f;
    E *= c;
    tmp[i] = -ki;
#pragma unroll
    for (int j = 0; j < i; ++j) tmp[j] = lpc[j] - ki * lpc[i - j - 1];
#pragma unroll
    for (int j = 0; j <= i; ++j) lpc[j] = tmp[j];
  }
  const float res_f = static_cast<float>(-log(1.0 / static_cast<double>(E)));
  *res_out = fmax(static_cast<double>(res_f), DBL_EPSILON);
#pragma unroll
  for (int i = 0; i < ORD; ++i) {
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < i; ++j)
      sum += static_cast<double>(i - j) * static_cast<double>(lpc[j]) * static_cast<double>(cep[i - j - 1]);
    cep[i] = static_cast<float>(-static_cast<double>(lpc[i]) - sum / static_cast<double>(i + 1));
  }
}

// The same arithmetic in the same order once more, for ONE exact shape (the reference's defaults: 23 mel
// bins, LPC order 12, 13 cepstra; round 4).  plp_tail_small_kernel<32, 16> predicates every loop of the
// 32 x 16 bound on the run-time sizes: 1.8 x the multiply-adds of the 25 x 13 IDFT, 1.8 x those of the
// Durbin and cepstrum recursions, ~1 200 scalar branches and ~580 single-dword scalar loads with their waits
// (tools/count_isa.py).  Here every bound is a template argument, the IDFT bases, the equal-loudness curve
// and the lifter are staged in LDS once per 256-frame workgroup and read as 16-byte broadcasts, and the mel
// rows arrive through the same coalesced LDS staging.
// REF (a compression exponent other than 1/3, where pow_third does not apply and the recipe is worse conditioned):
// the same staging and stores around the reference's arithmetic, operation by operation as in plp_tail_kernel - the
// double power rounded once, no fused products, the double logarithms, the cepstrum recursion as written there.
template <int NB, int ORD, int NC, bool REF>
__global__ __launch_bounds__(256) void plp_tail_exact_kernel(const PlpParams p, const BatchArgs b,
                                                             const float* __restrict__ mel,
                                                             const double* __restrict__ energy,
                                                             float* __restrict__ out) {
  // Round 5: the tail was bound by the LDS pipe, not by its arithmetic (0.205 ms with a seventh of the
  // instructions removed).  Rows 24 floats apart put the 64 lanes of a row read on 4-8 banks (24 t mod 32), and
  // the 325 IDFT bases came as 86 broadcast ds_read_b128 per wave: ~1 800 LDS clocks per wave, 0.14 ms per CU.
  // Now the row pitch is the odd row length itself (23: lane t reads bank 23 t + i, all different; the staging
  // copy is linear) and the bases and the lifter are read where they are used through the scalar cache
  // (uniform addresses with compile-time offsets: s_load_dwordx8/16, an SGPR operand per multiply-add).
  constexpr int kRowPad = NB;
  static_assert(NB % 2 == 1 && NC <= NB, "odd row pitch, output row inside the mel row's slot");
  __shared__ float rows[256 * kRowPad];
  const float* __restrict__ basis = p.idft;
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * 256;
  const int64_t limit = b.total_frames * NB;
  for (int i = threadIdx.x; i < 256 * NB; i += 256) {
    const int64_t a = g0 * NB + i;
    rows[i] = a < limit ? mel[a] : 1.0f;
  }
  __syncthreads();
  // (no early exit: the rows leave through LDS behind a barrier, see the end; a thread past the last frame
  // works on the row of ones the staging loop made and stores nothing)
  const bool live = g0 + threadIdx.x < b.total_frames;
  const int64_t g = live ? g0 + threadIdx.x : b.total_frames - 1;
  int warp_id = 0;
  if (b.utt_warp) warp_id = b.utt_warp[find_utt(b.frame_offsets, b.n_utts, g)];
  const float* __restrict__ eql = p.eql + warp_id * NB;
  float cep[ORD];
  double res;
  if constexpr (REF) {
    plp_reference_frame<NB, ORD>(rows + threadIdx.x * kRowPad, eql, basis, p.compress_factor, &res, cep);
  } else {
    float m[NB + 2];
    if (p.compress_factor == 0.33333334f && !p.exact_pow) {
  #pragma unroll
      for (int i = 0; i < NB; ++i) m[i + 1] = pow_third(rows[threadIdx.x * kRowPad + i] * eql[i], p.compress_factor);
    } else {
  #pragma unroll 1
      for (int i = 0; i < NB; ++i) m[i + 1] = powf(rows[threadIdx.x * kRowPad + i] * eql[i], p.compress_factor);
    }
    m[0] = m[1];
    m[NB + 1] = m[NB];
    float ac[ORD + 1], lpc[ORD], tmp[ORD];
  #pragma unroll
    for (int i = 0; i <= ORD; ++i) {
      float s = 0.0f;
  #pragma unroll
      for (int j = 0; j < NB + 2; ++j) s += basis[i * (NB + 2) + j] * m[j];
      ac[i] = s;
    }
    float E = ac[0];
  #pragma unroll
    for (int i = 0; i < ORD; ++i) lpc[i] = tmp[i] = cep[i] = 0.0f;
  #pragma unroll
    for (int i = 0; i < ORD; ++i) {
      float ki = ac[i + 1];
  #pragma unroll
      for (int j = 0; j < i; ++j) ki += lpc[j] * ac[i - j];
      ki = ki / E;
      float c = 1 - ki * ki;
      if (c < 1.0e-5f) c = 1.0e-5f;
      E *= c;
      tmp[i] = -ki;
  #pragma unroll
      for (int j = 0; j < i; ++j) tmp[j] = lpc[j] - ki * lpc[i - j - 1];
  #pragma unroll
      for (int j = 0; j <= i; ++j) lpc[j] = tmp[j];
    }
    // (round 5) The reference forms -log(1 / E) and the frame's log-energy in float64 and rounds them to float32
    // (plp.py:601-603, :615-620): a float32 logarithm that is good to an ulp gives the same float32 up to its last
    // bit (1e-7 relative on values of 5-20, the parity tolerance is 1e-4) at a fifth of the instructions of the
    // double one.  The LPC -> cepstrum recursion keeps the reference's double accumulation (plp.py:149-168) with
    // the weights (k + 1) c[k] made once per cepstrum and one fused multiply-add per term: 78 double operations
    // instead of 198 + 12 divisions, the same sums up to the last bit of a double that is rounded to float next.
    const float res_f = logf(E);
    res = fmax(static_cast<double>(res_f), DBL_EPSILON);
    double wcep[ORD];
  #pragma unroll
    for (int i = 0; i < ORD; ++i) {
      double sum = 0.0;
  #pragma unroll
      for (int j = 0; j < i; ++j) sum = fma(static_cast<double>(lpc[j]), wcep[i - j - 1], sum);
      cep[i] = static_cast<float>(-static_cast<double>(lpc[i]) - sum * (1.0 / static_cast<double>(i + 1)));
      wcep[i] = static_cast<double>(i + 1) * static_cast<double>(cep[i]);
    }
  }
  // Round 5: the 13 values of a frame used to leave as 13 dword stores per lane, 52 bytes apart from lane to lane
  // - every store instruction touched 52 cache lines, and the kernel took 0.26 ms whatever arithmetic was left in
  // it (ablations without the cube roots, the divisions, the double recursion or the IDFT: 0.24-0.27 ms).  The
  // thread now puts its row where its mel row was (its own slot: nobody else reads it), and the workgroup
  // writes its 256 x 13 floats - one contiguous block of the output - with coalesced stores: 0.21 ms.
  // (Also built: persistent workgroups with the next tile's mel rows requested into registers a tile ahead -
  // 180 registers, 2 waves per SIMD, the same 0.21 ms; capped at 128 / 96 / 80 registers it spills: 0.30-0.33.)
  float* __restrict__ slot = rows + threadIdx.x * kRowPad;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    float v = c == 0 ? static_cast<float>(res) : cep[c > 0 ? c - 1 : 0];
    if (p.lifter) v *= p.lifter[c];
    if (p.cepstral_scale != 1.0f) v *= p.cepstral_scale;
    if (c == 0 && p.use_energy) {
      // (linear frame energy from the mel kernel: a float sum widened to double; the floor of the reference's
      // double logarithm, DBL_EPSILON, is a float32 number too)
      if constexpr (REF) {
        double le = log(fmax(energy[g], DBL_EPSILON));
        if (p.has_floor && le < p.log_energy_floor) le = p.log_energy_floor;
        v = static_cast<float>(le);
      } else {
        float le = logf(fmaxf(static_cast<float>(energy[g]), 2.220446049250313e-16f));
        if (p.has_floor && le < p.log_energy_floor) le = p.log_energy_floor;
        v = le;
      }
    }
    int oc = c;
    if (p.htk_compat) oc = c == 0 ? NC - 1 : c - 1;
    slot[oc] = v;
  }
  __syncthreads();
  const int64_t left = b.total_frames - g0;
  const int count = static_cast<int>(left < 256 ? left : 256) * NC;
  float* __restrict__ block = out + g0 * NC;
  for (int i = threadIdx.x; i < count; i += 256) block[i] = rows[(i / NC) * kRowPad + i % NC];
}

int launch_plp_tail(const PlpParams& p, const BatchArgs& b, const float* mel, const double* energy,
                    float* out, hipStream_t stream, const char** launched) {
  if (launched) *launched = nullptr;
  if (b.total_frames <= 0) return SNF_OK;
  const PostRoute r = plp_tail_route(p.num_bins, p.lpc_order, p.num_ceps, p.compress_factor, post_knobs_from_env());
  if (r.refusal) return set_error(SNF_E_RUNTIME, r.refusal);
  const dim3 grid(static_cast<unsigned>((b.total_frames + r.rows - 1) / r.rows)), block(r.threads);
  switch (r.kernel) {
    case kPlpTailExact:
      if (r.variant)
        hipLaunchKernelGGL((plp_tail_exact_kernel<23, 12, 13, true>), grid, block, 0, stream, p, b, mel, energy, out);
      else
        hipLaunchKernelGGL((plp_tail_exact_kernel<23, 12, 13, false>), grid, block, 0, stream, p, b, mel, energy, out);
      break;
    case kPlpTailSmall:
      hipLaunchKernelGGL((plp_tail_small_kernel<32, 16>), grid, block, 0, stream, p, b, mel, energy, out);
      break;
    default:
      hipLaunchKernelGGL(plp_tail_kernel, grid, block, 0, stream, p, b, mel, energy, out);
  }
  SNF_HIP_CHECK(hipGetLastError());
  if (launched) *launched = r.name();
  return SNF_OK;
}

}  // namespace snf
