// Kernels of the prompt denoiser (MP-SENet, reference denoiser/: SURVEY.md §8f N4) that are not convolutions or
// GEMMs: the spectrogram front / back end of denoiser/infer.py and the normalisation / gating glue of
// denoiser/generator.py and conformer.py.  Everything here is pointwise or a small reduction over a prompt of a few
// seconds (a [64, T, 201] tensor is 40 MB at 5 s): latency, not throughput.  Reference call sites are listed next
// to each entry point in include/hsp.h.
#include "hsp_rows.h"

namespace {

// block-wide sum of a double (1024 threads at most); every thread receives the total
__device__ __forceinline__ double dn_block_sum(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < nw; ++w) t += sh[w];
  return t;
}

// spec rows [0, nf) real, [nf, 2 nf) imaginary, pitch s_ld  ->  mag[f][t] = |z|^c, pha[f][t] = angle(z)
__global__ __launch_bounds__(256) void mag_pha_kernel(const float* __restrict__ spec, int64_t s_ld, float* __restrict__ mag,
                                                      float* __restrict__ pha, int nf, int T, float c) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)nf * T) return;
  const int f = (int)(i / T), t = (int)(i % T);
  const float re = spec[(int64_t)f * s_ld + t];
  // a real FFT returns exactly +0 for the imaginary part of the DC and Nyquist bins (torch.stft does); the DFT
  // product leaves rounding noise there, whose sign would turn a phase of pi into -pi
  const float im = (f == 0 || f == nf - 1) ? 0.0f : spec[(int64_t)(nf + f) * s_ld + t];
  mag[i] = powf(hypotf(re, im), c);
  pha[i] = atan2f(im, re);
}

// out[t][f] = mag[t][f] * beta * sigmoid(slope[f] * m[t][f])
__global__ __launch_bounds__(256) void lsigmoid_mul_kernel(const float* __restrict__ m, const float* __restrict__ slope,
                                                           float beta, const float* __restrict__ mag, float* __restrict__ out,
                                                           int F, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float s = slope[i % F] * m[i];
  out[i] = mag[i] * (beta / (1.0f + expf(-s)));
}

__global__ __launch_bounds__(256) void atan2_kernel(const float* __restrict__ yy, const float* __restrict__ xx,
                                                    float* __restrict__ out, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) out[i] = atan2f(yy[i], xx[i]);
}

// re = mag^p cos(pha), im = mag^p sin(pha)
__global__ __launch_bounds__(256) void polar_kernel(const float* __restrict__ mag, const float* __restrict__ pha, float p,
                                                    float* __restrict__ re, int64_t re_ld, float* __restrict__ im,
                                                    int64_t im_ld, int T, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t f = i / T, t = i % T;
  const float m = p == 1.0f ? mag[i] : powf(mag[i], p);
  re[f * re_ld + t] = m * cosf(pha[i]);
  im[f * im_ld + t] = m * sinf(pha[i]);
}

// ---------------------------------------------------------------------------------------------------------------
// The T-crossing operations read their bounds from a segment table (dn_seg_of, hsp_rows.h).

// per row: ss = sum x^2 (double accumulation, rounded to fp32), then scale = sqrt(len / ss) and 1 / scale formed in
// double and rounded once; a silent (or empty) row gets 0 for both
__global__ __launch_bounds__(1024) void norm_factor_rows_kernel(const float* __restrict__ x, int64_t x_bs,
                                                                const int64_t* __restrict__ lengths, float* __restrict__ scale,
                                                                float* __restrict__ inv, int64_t L) {
  __shared__ double sh[16];
  const int b = blockIdx.x;
  const int64_t n = hsp_row_len(lengths, b, L);
  const float* p = x + (int64_t)b * x_bs;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) s += (double)p[i] * (double)p[i];
  s = dn_block_sum(s, sh);
  if (threadIdx.x == 0) {
    const float ss = (float)s;
    const bool ok = n > 0 && ss > 0.0f;
    const double norm = ok ? sqrt((double)n / (double)ss) : 0.0;
    scale[b] = (float)norm;
    inv[b] = ok ? (float)(1.0 / norm) : 0.0f;
  }
}

// InstanceNorm2d(affine) + PReLU per (channel, segment): block (c, b) normalises the T_b x F values of segment b in place
// and WRITES zeros on the gap rows that follow it (block b = 0 also on the rows ahead of the first segment), so every
// row of the plane is written by exactly one block and no gap value is ever read
__global__ __launch_bounds__(1024) void instnorm_prelu_seg_kernel(float* __restrict__ x, int64_t cs, int T_tot, int F,
                                                                  const int32_t* __restrict__ seg, int B,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ slope, float eps) {
  __shared__ double sh[16];
  const int c = blockIdx.x, b = blockIdx.y;
  const int t0 = seg[2 * b], Tb = seg[2 * b + 1];
  float* plane = x + (int64_t)c * cs;
  float* p = plane + (int64_t)t0 * F;
  const int64_t N = (int64_t)Tb * F;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += blockDim.x) s += (double)p[i];
  const double mean = dn_block_sum(s, sh) / (double)N;
  double q = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += blockDim.x) {
    const double d = (double)p[i] - mean;
    q += d * d;
  }
  const double var = dn_block_sum(q, sh) / (double)N;   // biased, as F.instance_norm
  const float inv = (float)(1.0 / sqrt(var + (double)eps));
  const float m = (float)mean, g = gamma[c], bt = beta[c], sl = slope[c];
  for (int64_t i = threadIdx.x; i < N; i += blockDim.x) {
    const float y = (p[i] - m) * inv * g + bt;
    p[i] = y > 0.0f ? y : sl * y;
  }
  const int g_hi = b + 1 < B ? seg[2 * b + 2] : T_tot;
  float* z = p + N;
  const int64_t NZ = (int64_t)(g_hi - t0 - Tb) * F;
  for (int64_t i = threadIdx.x; i < NZ; i += blockDim.x) z[i] = 0.0f;
  if (b == 0) {
    const int64_t N0 = (int64_t)t0 * F;
    for (int64_t i = threadIdx.x; i < N0; i += blockDim.x) plane[i] = 0.0f;
  }
}

// zeros on the gap rows of C channel planes [T_tot, F]; rows inside a segment are not touched (nothing is read)
__global__ __launch_bounds__(256) void zero_gaps_kernel(float* __restrict__ x, int64_t cs, int T_tot, int F,
                                                        const int32_t* __restrict__ seg, int B, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t plane = (int64_t)T_tot * F;
  const int64_t c = i / plane, r = i % plane;
  int t0, Tb;
  if (dn_seg_of(seg, B, (int)(r / F), t0, Tb) < 0) x[c * cs + r] = 0.0f;
}

// depthwise Conv1d (same padding, odd K) + BatchNorm1d in eval mode + SiLU over [A, C, N] with N = the packed T axis: taps
// outside the element's own segment read as zero (bounded by the table, whatever the gap width); gap positions are
// written as 0
__global__ __launch_bounds__(256) void dwconv_bn_silu_seg_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, const float* __restrict__ bn_w,
                                                                 const float* __restrict__ bn_b, const float* __restrict__ bn_mean,
                                                                 const float* __restrict__ bn_var, float bn_eps,
                                                                 float* __restrict__ y, int C, int N, int K,
                                                                 const int32_t* __restrict__ seg, int B, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int n = (int)(i % N);
  int t0, Tb;
  if (dn_seg_of(seg, B, n, t0, Tb) < 0) {
    y[i] = 0.0f;
    return;
  }
  const int c = (int)((i / N) % C);
  const float* row = x + (i - n);
  const float* wc = w + (int64_t)c * K;
  const int half = K >> 1;
  float acc = 0.0f;
  for (int j = 0; j < K; ++j) {
    const int m = n + j - half;
    if (m >= t0 && m < t0 + Tb) acc = fmaf(wc[j], row[m], acc);
  }
  acc += bias[c];
  const float alpha = bn_w[c] / sqrtf(bn_var[c] + bn_eps);
  const float v = acc * alpha + (bn_b[c] - bn_mean[c] * alpha);
  y[i] = v / (1.0f + expf(-v));
}

// torch.istft after the inverse DFT, per segment: out[b][n] = sum_t frames[n + N/2 - t hop][t0_b + t] w[.] / sum_t w[.]^2
// over the frames t of segment b (blockIdx.y) only, for n < hop (T_b - 1), times inv[b] (1 when inv is NULL); zeros up
// to n_max
__global__ __launch_bounds__(256) void istft_ola_seg_kernel(const float* __restrict__ frames, int64_t f_ld,
                                                            const float* __restrict__ window, const float* __restrict__ inv,
                                                            float* __restrict__ out, int64_t out_bs, int64_t n_max, int n_fft,
                                                            int hop, const int32_t* __restrict__ seg) {
  const int b = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= n_max) return;
  const int t0 = seg[2 * b], T = seg[2 * b + 1];
  float v = 0.0f;
  if (n < (int64_t)hop * (T - 1)) {
    const int64_t pos = n + (n_fft >> 1);
    int64_t t_hi = pos / hop;
    if (t_hi > T - 1) t_hi = T - 1;
    int64_t t_lo = (pos - n_fft + hop) / hop;
    if (pos - n_fft + 1 <= 0) t_lo = 0;
    float num = 0.0f, den = 0.0f;
    for (int64_t t = t_lo; t <= t_hi; ++t) {
      const int k = (int)(pos - t * hop);
      if (k < 0 || k >= n_fft) continue;
      const float w = window[k];
      num += frames[(int64_t)k * f_ld + t0 + t] * w;
      den += w * w;
    }
    v = num / den * (inv ? inv[b] : 1.0f);
  }
  out[(int64_t)b * out_bs + n] = v;
}

}  // namespace

// declared in hsp_rows.h (hsp_stft_frames_packed_f32 of hsp_mel.hip checks its table with it too)
bool dn_seg_ok(const int32_t* seg, const int32_t* seg_host, int32_t B, int64_t T_tot) {
  if (!seg || !seg_host || B < 1 || B > 65535 || T_tot < 1) return false;
  int64_t end = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t s = seg_host[2 * b], n = seg_host[2 * b + 1];
    if (s < end || n < 1 || s + n > T_tot) return false;
    end = s + n;
  }
  return true;
}

#define HSP_STREAM static_cast<hipStream_t>(stream)

extern "C" int hsp_mag_pha_f32(const float* spec, int64_t s_ld, float* mag, float* pha, int32_t n_freqs, int32_t T,
                               float compress, void* stream) {
  if (!spec || !mag || !pha || n_freqs < 2 || T <= 0 || s_ld < T) return HSP_EINVAL;
  const int64_t total = (int64_t)n_freqs * T;
  if (!hsp_grid_fits(total, 256)) return HSP_EINVAL;
  hipLaunchKernelGGL(mag_pha_kernel, dim3(hsp_flat_grid(total, 256)), dim3(256), 0, HSP_STREAM, spec, s_ld, mag, pha, n_freqs, T,
                     compress);
  return (int)hipGetLastError();
}

extern "C" int hsp_lsigmoid_mul_f32(const float* m, const float* slope, float beta, const float* mag, float* out, int32_t T,
                                    int32_t F, void* stream) {
  if (!m || !slope || !mag || !out || T <= 0 || F <= 0) return HSP_EINVAL;
  const int64_t total = (int64_t)T * F;
  if (!hsp_grid_fits(total, 256)) return HSP_EINVAL;
  hipLaunchKernelGGL(lsigmoid_mul_kernel, dim3(hsp_flat_grid(total, 256)), dim3(256), 0, HSP_STREAM, m, slope, beta, mag, out, F, total);
  return (int)hipGetLastError();
}

extern "C" int hsp_atan2_f32(const float* y, const float* x, float* out, int64_t n, void* stream) {
  if (!y || !x || !out || n <= 0) return HSP_EINVAL;
  if (!hsp_grid_fits(n, 256)) return HSP_EINVAL;
  hipLaunchKernelGGL(atan2_kernel, dim3(hsp_flat_grid(n, 256)), dim3(256), 0, HSP_STREAM, y, x, out, n);
  return (int)hipGetLastError();
}

extern "C" int hsp_polar_f32(const float* mag, const float* pha, float power, float* re, int64_t re_ld, float* im,
                             int64_t im_ld, int32_t F, int32_t T, void* stream) {
  if (!mag || !pha || !re || !im || F <= 0 || T <= 0 || re_ld < T || im_ld < T) return HSP_EINVAL;
  const int64_t total = (int64_t)F * T;
  if (!hsp_grid_fits(total, 256)) return HSP_EINVAL;
  hipLaunchKernelGGL(polar_kernel, dim3(hsp_flat_grid(total, 256)), dim3(256), 0, HSP_STREAM, mag, pha, power, re, re_ld, im, im_ld, T,
                     total);
  return (int)hipGetLastError();
}

extern "C" int hsp_norm_factor_rows_f32(const float* x, int64_t x_bs, const int64_t* lengths, float* scale, float* inv,
                                        int32_t B, int64_t L, void* stream) {
  if (!x || !lengths || !scale || !inv || B < 1 || L <= 0 || x_bs < L) return HSP_EINVAL;
  hipLaunchKernelGGL(norm_factor_rows_kernel, dim3((unsigned)B), dim3(1024), 0, HSP_STREAM, x, x_bs, lengths, scale, inv, L);
  return (int)hipGetLastError();
}

extern "C" int hsp_instnorm_prelu_seg_f32(float* x, int64_t x_cs, int32_t C, int32_t T_tot, int32_t F, const int32_t* seg,
                                          const int32_t* seg_host, int32_t B, const float* gamma, const float* beta,
                                          const float* slope, float eps, void* stream) {
  if (!x || !gamma || !beta || !slope || C <= 0 || F <= 0 || T_tot <= 0) return HSP_EINVAL;
  if (x_cs < (int64_t)T_tot * F || !dn_seg_ok(seg, seg_host, B, T_tot)) return HSP_EINVAL;
  hipLaunchKernelGGL(instnorm_prelu_seg_kernel, dim3((unsigned)C, (unsigned)B), dim3(1024), 0, HSP_STREAM, x, x_cs, T_tot, F,
                     seg, B, gamma, beta, slope, eps);
  return (int)hipGetLastError();
}

extern "C" int hsp_zero_gaps_f32(float* x, int64_t x_cs, int32_t C, int32_t T_tot, int32_t F, const int32_t* seg,
                                 const int32_t* seg_host, int32_t B, void* stream) {
  if (!x || C <= 0 || F <= 0 || T_tot <= 0) return HSP_EINVAL;
  if (x_cs < (int64_t)T_tot * F || !dn_seg_ok(seg, seg_host, B, T_tot)) return HSP_EINVAL;
  const int64_t total = (int64_t)C * T_tot * F;
  if (!hsp_grid_fits(total, 256)) return HSP_EINVAL;
  hipLaunchKernelGGL(zero_gaps_kernel, dim3(hsp_flat_grid(total, 256)), dim3(256), 0, HSP_STREAM, x, x_cs, T_tot, F, seg, B, total);
  return (int)hipGetLastError();
}

extern "C" int hsp_dwconv_bn_silu_seg_f32(const float* x, const float* w, const float* bias, const float* bn_weight,
                                          const float* bn_bias, const float* bn_mean, const float* bn_var, float bn_eps,
                                          float* y, int32_t A, int32_t C, int32_t N, int32_t K, const int32_t* seg,
                                          const int32_t* seg_host, int32_t B, void* stream) {
  if (!x || !w || !bias || !bn_weight || !bn_bias || !bn_mean || !bn_var || !y) return HSP_EINVAL;
  if (A <= 0 || C <= 0 || N <= 0 || K <= 0 || (K & 1) == 0 || !dn_seg_ok(seg, seg_host, B, N)) return HSP_EINVAL;
  const int64_t total = (int64_t)A * C * N;
  if (!hsp_grid_fits(total, 256)) return HSP_EINVAL;
  hipLaunchKernelGGL(dwconv_bn_silu_seg_kernel, dim3(hsp_flat_grid(total, 256)), dim3(256), 0, HSP_STREAM, x, w, bias, bn_weight,
                     bn_bias, bn_mean, bn_var, bn_eps, y, C, N, K, seg, B, total);
  return (int)hipGetLastError();
}

extern "C" int hsp_istft_ola_seg_f32(const float* frames, int64_t f_ld, const float* window, const float* inv, float* out,
                                     int64_t out_bs, int64_t n_max, int32_t n_fft, int32_t hop, const int32_t* seg,
                                     const int32_t* seg_host, int32_t B, int32_t T_tot, void* stream) {
  if (!frames || !window || !out || n_fft <= 0 || (n_fft & 1) || hop <= 0 || hop > n_fft) return HSP_EINVAL;
  if (n_max < 1 || out_bs < n_max || f_ld < T_tot || !dn_seg_ok(seg, seg_host, B, T_tot)) return HSP_EINVAL;
  for (int b = 0; b < B; ++b)
    if ((int64_t)hop * (seg_host[2 * b + 1] - 1) > n_max) return HSP_EINVAL;
  if (!hsp_grid_fits(n_max, 256)) return HSP_EINVAL;
  hipLaunchKernelGGL(istft_ola_seg_kernel, dim3(hsp_flat_grid(n_max, 256), (unsigned)B), dim3(256), 0, HSP_STREAM, frames, f_ld,
                     window, inv, out, out_bs, n_max, n_fft, hop, seg);
  return (int)hipGetLastError();
}
