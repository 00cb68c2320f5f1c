// Device-side helpers shared by the libhsp kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hsp.h"

#define HSP_WAVE 64

// 16-B addressable: what a float4 access or a 16-B LDS-DMA lane needs of a pointer
inline bool hsp_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Raise a kernel's dynamic-LDS limit to `bytes` once per device.  hipFuncSetAttribute applies to the current
// device only, so the "already raised" flag is kept per device (`flags`: one zero-initialised static array per
// kernel instantiation).  Idempotent and safe from several host threads; kept out of the launch path afterwards
// so that launches stay legal inside a hipGraph stream capture.  Returns 0 or the hipError_t / HSP_EINVAL.
#include <atomic>
constexpr int HSP_MAX_DEVICES = 32;
struct hsp_lds_flags { std::atomic<int> raised[HSP_MAX_DEVICES]; };
inline int hsp_raise_lds_limit(const void* kernel, int bytes, hsp_lds_flags& flags) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= HSP_MAX_DEVICES) return HSP_EINVAL;
  if (flags.raised[dev].load(std::memory_order_acquire)) return 0;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return (int)e;
  flags.raised[dev].store(1, std::memory_order_release);
  return 0;
}

// THE launch of a kernel with dynamic LDS: raise its limit to `lds_max` (once per device, and only when this launch
// needs more than the 32 KB every kernel may have), launch, report.  The flags are a static of this function: every
// call site of a kernel that passes the same argument types shares one set, so there is none to declare and none to
// share between two kernels by mistake (a site with other argument types gets its own set and raises once more, which
// is harmless).  `lds_max` is the most the kernel is ever launched with, not this launch's size: the raise happens
// once.  The caller has checked 0 < blocks <= 0x7fffffff.
template <auto Kernel, class... Args>
int hsp_launch(int64_t blocks, int threads, int lds_bytes, int lds_max, hipStream_t s, Args... args) {
  static hsp_lds_flags flags;
  if (lds_bytes > 32 * 1024)
    if (int e = hsp_raise_lds_limit(reinterpret_cast<const void*>(Kernel), lds_max, flags)) return e;
  hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks), dim3((unsigned)threads), (size_t)lds_bytes, s, args...);
  return (int)hipGetLastError();
}

// C/D map of the 32x32 MFMA forms: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
#define HSP_ACC_ROW(r, half) (((r) & 3) + 8 * ((r) >> 2) + 4 * (half))

__device__ __forceinline__ float hsp_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// exp(x) on the hardware exp2 (v_exp_f32): 2^(x log2 e)
constexpr float HSP_LOG2E = 1.4426950408889634f;
__device__ __forceinline__ float hsp_exp2e(float x) { return __builtin_amdgcn_exp2f(x * HSP_LOG2E); }

// tanh(x) = 1 - 2 / (exp(2x) + 1) on the hardware exp2 (v_exp_f32) and a true division: ~12 instructions
// instead of ocml tanhf's ~100 (which dominated the GELU / WN-gate epilogues).  Absolute error < 2e-7
// (exp2 is accurate to 1 ulp; the subtraction from 1 bounds the error by ulp(1)); saturates to +-1 cleanly
// for large |x| (exp -> inf / 0).
__device__ __forceinline__ float hsp_tanh(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);   // exp(2x) = 2^(2x log2 e)
  return 1.0f - 2.0f / (e + 1.0f);
}

__device__ __forceinline__ float hsp_apply_act(float v, int act) {
  switch (act) {
    case HSP_ACT_TANH: return tanhf(v);   // final waveform tanh: full precision
    case HSP_ACT_GELU_TANH: {
      const float k0 = 0.7978845608028654f, k1 = 0.044715f;
      return 0.5f * v * (1.0f + hsp_tanh(k0 * (v + k1 * v * v * v)));
    }
    case HSP_ACT_RELU: return fmaxf(v, 0.0f);
    case HSP_ACT_MISH: {
      float sp = v > 20.0f ? v : log1pf(expf(v));
      return v * tanhf(sp);
    }
    case HSP_ACT_SILU: return v * hsp_sigmoid(v);
    case HSP_ACT_SOFTPLUS: return v > 20.0f ? v : log1pf(expf(v));
    case HSP_ACT_GELU_ERF: return 0.5f * v * (1.0f + erff(v * 0.7071067811865476f));
    default: return v;
  }
}

// SnakeBeta on one sample: x + binv * sin(x * ea)^2   (activations.py:118)
// sin(y) for the snake argument.  ocml's sinf carries a Payne-Hanek slow path that costs
// 320 B of scratch per lane; the activation argument x*exp(alpha) is O(1..1e3), so a
// three-constant Cody-Waite reduction by pi (k*PI_HI exact for |k| < 2^15) followed by
// the degree-11 odd Taylor polynomial on [-pi/2, pi/2] (remainder < 6e-8) is used
// instead.  sin(y) = (-1)^k sin(r); only sin^2 is consumed, so the sign is dropped.
__device__ __forceinline__ float hsp_sin_abs(float y) {
  const float k = rintf(y * 0.318309886183790672f);
  float r = fmaf(k, -3.140625f, y);
  r = fmaf(k, -9.67502593994140625e-4f, r);
  r = fmaf(k, -1.509957990978376432e-7f, r);
  const float r2 = r * r;
  float p = -2.50521083854417188e-8f;
  p = fmaf(p, r2, 2.75573192239858907e-6f);
  p = fmaf(p, r2, -1.98412698412698413e-4f);
  p = fmaf(p, r2, 8.33333333333333333e-3f);
  p = fmaf(p, r2, -1.66666666666666667e-1f);
  return fmaf(r * r2, p, r);
}

__device__ __forceinline__ float hsp_snake(float x, float ea, float binv) {
  const float s = hsp_sin_abs(x * ea);
  return fmaf(binv, s * s, x);
}

// Hardware-trig form used inside the fused conv prologue, where every VALU cycle is taken
// from the fp32 MFMAs running on the same SIMD:  sin^2(y) = (1 - cos 2y) / 2 with
// v_cos_f32 (argument in revolutions, reduced by v_fract_f32):
//   snake(x) = (x + kb) - kb * cos(2*pi * fract(x * kf)),   kf = exp(alpha)/pi, kb = binv/2
// 5 VALU ops instead of 14.  v_cos_f32 is accurate to ~1e-6 absolute on [0, 1).
__device__ __forceinline__ float hsp_snake_hw(float x, float kf, float kb) {
  const float c = __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(x * kf));
  return fmaf(-kb, c, x + kb);
}

__device__ __forceinline__ int hsp_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The nearest-code arithmetic of EuclideanCodebook.quantize (ttv_v1/core_vq.py:175-183), stated once: |x|^2 and
// dist(x, e) = -((|x|^2 - 2 x.e) + |e|^2) as ascending-d fmaf chains.  x has element stride xs (a [D, T] column in
// global memory or in LDS), e is one contiguous codebook row.  vq_nearest_kernel (csrc/hsp_frontend.hip) and
// prosody_encode_kernel (csrc/hsp_prosody.hip) both call these, so the same x gives both the same distances bit for bit.
__device__ __forceinline__ float hsp_vq_sq(const float* x, int64_t xs, int D) {
  float xx = 0.0f;
  for (int d = 0; d < D; ++d) xx = fmaf(x[d * xs], x[d * xs], xx);
  return xx;
}
__device__ __forceinline__ float hsp_vq_dist(const float* x, int64_t xs, float xx, const float* __restrict__ e, int D) {
  float xe = 0.0f, ee = 0.0f;
  for (int d = 0; d < D; ++d) {
    xe = fmaf(x[d * xs], e[d], xe);
    ee = fmaf(e[d], e[d], ee);
  }
  return -((xx - 2.0f * xe) + ee);
}

// Shared epilogue of both conv kernels for one output element in PLAIN/SHUFFLE row
// modes (GATE modes combine two accumulators before calling with act = NONE).
struct hsp_epi_ctx {
  const hsp_conv1d_args* a;
};

__device__ __forceinline__ void hsp_epilogue_store(const hsp_conv1d_args& a, int b, int co, int t, float v) {
  // v already holds act(acc + bias + cbias)
  float mk = 1.0f;
  if (a.mask_mode != HSP_MASK_NONE) mk = a.mask[(int64_t)b * a.mask_bs + t];
  if (a.mask_mode & HSP_MASK_PRE) v *= mk;
  if (a.cscale) v *= a.cscale[(int64_t)b * a.cscale_bs + co];
  v *= a.scale;
  if (a.res) v += a.res[(int64_t)b * a.res_bs + (int64_t)co * a.res_cs + t];
  if (a.mask_mode & HSP_MASK_POST) v *= mk;
  float* yp = a.y + (int64_t)b * a.y_bs + (int64_t)co * a.y_cs + t;
  if (a.accumulate) v += *yp;
  *yp = v * a.post_scale;
}

// F0 conversion of inference_vc.py:80-81,104-105 for one utterance, by one 256-thread workgroup: voiced statistics of
// both tracks in double (the reference's numpy float32 mean / std differ from the exact values by ~1e-7 relative;
// double keeps this side at the exact ones), then the conversion of src[0, ns) into out[0, ns) and zeros on
// out[ns, n_out).  hsp_f0_convert_f32 and each row of hsp_f0_convert_batch_f32 run this one function, so a batch row is
// bit-identical to the single-utterance call on that row.
__device__ __forceinline__ void hsp_f0_convert_row(const float* src, int ns, const float* trg, int nt, float* out,
                                                   int n_out) {
  __shared__ double red[4][256];
  __shared__ double stat[4];
  double s1 = 0, c1 = 0, s2 = 0, c2 = 0;
  for (int i = threadIdx.x; i < ns; i += 256) if (src[i] != 0.0f) { s1 += src[i]; c1 += 1; }
  for (int i = threadIdx.x; i < nt; i += 256) if (trg[i] != 0.0f) { s2 += trg[i]; c2 += 1; }
  red[0][threadIdx.x] = s1; red[1][threadIdx.x] = c1; red[2][threadIdx.x] = s2; red[3][threadIdx.x] = c2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    __syncthreads();
  }
  const double m1 = red[1][0] > 0 ? red[0][0] / red[1][0] : 0.0, m2 = red[3][0] > 0 ? red[2][0] / red[3][0] : 0.0;
  const double n1 = red[1][0], n2 = red[3][0];
  __syncthreads();
  double v1 = 0, v2 = 0;
  for (int i = threadIdx.x; i < ns; i += 256) if (src[i] != 0.0f) { const double d = src[i] - m1; v1 += d * d; }
  for (int i = threadIdx.x; i < nt; i += 256) if (trg[i] != 0.0f) { const double d = trg[i] - m2; v2 += d * d; }
  red[0][threadIdx.x] = v1; red[2][threadIdx.x] = v2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[2][threadIdx.x] += red[2][threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    stat[0] = m1; stat[1] = n1 > 0 ? sqrt(red[0][0] / n1) : 1.0; stat[2] = m2; stat[3] = n2 > 0 ? sqrt(red[2][0] / n2) : 0.0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_out; i += 256) {
    float o = 0.0f;
    if (i < ns && src[i] != 0.0f) {
      // the reference's steps, in float64 like its numpy arrays (get_yaapt_f0 works on float64), then the float32 cast
      // of torch.FloatTensor(f0 + 1) and a float32 log
      const double z = ((double)src[i] - stat[0]) / stat[1];
      const double f = fmax(z * stat[3] + stat[2], 0.0);
      o = logf((float)(f + 1.0));
    }
    out[i] = o;
  }
}

// max |x[0, n)| of one row by a 1024-thread workgroup (wave64 butterfly, then the 16 wave maxima through LDS)
__device__ __forceinline__ float hsp_block_abs_max_1024(const float* __restrict__ xb, int64_t n) {
  __shared__ float red[16];
  const int tid = threadIdx.x;
  float mx = 0.0f;
  for (int64_t i = tid; i < n; i += 1024) mx = fmaxf(mx, fabsf(xb[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) mx = fmaxf(mx, red[w]);
  return mx;
}

// ob[i] = (int16)(xb[i] / max_{j < L} |xb[j]| * 32767 * gain) for i < L, 0 for L <= i < n, by a 1024-thread workgroup:
// `audio / max(abs(audio)) * 32767.0 * gain` then numpy's truncating astype(int16) (inference_plm.py:186).
// hsp_peak_int16 and hsp_peak_int16_gains both run this function, so equal gains give equal rows.
// A row whose peak is 0 (silence) is written as zeros: the reference expression gives 0 / 0 = NaN there and numpy's
// astype(int16) turns NaN into 0, whereas fmaxf(NaN, -32768) below would make it full-scale negative DC.
__device__ __forceinline__ void hsp_peak_int16_row(const float* __restrict__ xb, int64_t L, float gain,
                                                   int16_t* __restrict__ ob, int64_t n) {
  const float mx = hsp_block_abs_max_1024(xb, L);
  for (int64_t i = threadIdx.x; i < n; i += 1024) {
    float v = 0.0f;
    if (i < L && mx > 0.0f) v = xb[i] / mx * 32767.0f * gain;
    ob[i] = (int16_t)fminf(fmaxf(v, -32768.0f), 32767.0f);
  }
}
