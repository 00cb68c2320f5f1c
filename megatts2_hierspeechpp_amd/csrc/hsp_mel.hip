// STFT framing in its three forms (plain, ragged rows, rows packed into one matrix) and the power / mel / log step: the
// HBM-bound steps around the DFT GEMM of the prompt front-end (MelSpectrogramFixed,
// Mels_preprocess.py:8-18), of batched voice conversion and of the prompt denoiser.  Declarations and semantics:
// include/hsp.h.
#include "hsp_rows.h"

namespace {

// Frame column t of one row: fcol[n * f_ld] = w[n] * x[reflect(base + n)] for the window positions n in [n0, n0 + 64) of
// the frame whose first sample is `base` = frame * hop - n_fft / 2; with SCALED the sample is multiplied by sc first
// (w[n] * (x * sc): the norm factor folded into the framing).  A column that is not `live` (row pitch padding, past the
// row's last frame, a gap between packed segments) is written as 0 and reads nothing.  Every framing kernel below calls
// this one function, which is why the plain, ragged and packed forms of a row are bit-equal (include/hsp.h).
template <class I>
__device__ __forceinline__ void frame_column(const float* __restrict__ xb, I Lb, I base, bool live, bool scaled, float sc,
                                             const float* __restrict__ w, float* __restrict__ fcol, int f_ld, int n0,
                                             int n_fft) {
  for (int n = n0; n < min(n0 + 64, n_fft); ++n) {
    float v = 0.0f;
    if (live) {
      const float xv = xb[hsp_reflect<I>(base + n, Lb)];
      v = scaled ? w[n] * (xv * sc) : w[n] * xv;
    }
    fcol[(int64_t)n * f_ld] = v;
  }
}

// frames[b][n][t] = w[n] * x[b][reflect(t * hop + n - n_fft / 2)] with row b's own length (NULL lengths: L, the plain
// form): T_b = 1 + len_b / hop frames that reflect at len_b, zero columns on [T_b, f_ld).  One workgroup = 64 frames x 256
// window positions of one row; lanes run along t (the GEMM's column axis, time fastest like every activation of the
// path), so the stores are coalesced and the strided reads of x (lane stride = hop) hit lines that the 4 following n of
// the same thread re-use from L1.
__global__ __launch_bounds__(256) void stft_frames_kernel(const float* __restrict__ x, int64_t x_bs,
                                                          const int64_t* __restrict__ lengths,
                                                          const float* __restrict__ w, float* __restrict__ frames, int L,
                                                          int n_fft, int hop, int T, int f_ld) {
  const int b = blockIdx.z;
  const int t = blockIdx.x * 64 + (threadIdx.x & 63);
  const int n0 = blockIdx.y * 256 + (threadIdx.x >> 6) * 64;
  if (t >= f_ld) return;
  const int Lb = (int)hsp_row_len(lengths, b, L);
  const int Tb = Lb > 0 ? min(T, 1 + Lb / hop) : 0;
  frame_column<int>(x + (int64_t)b * x_bs, Lb, t * hop - (n_fft >> 1), t < Tb, false, 1.0f, w,
                    frames + (int64_t)b * n_fft * f_ld + t, f_ld, n0, n_fft);
}

// The same tile on ONE [n_fft, f_ld] matrix that holds every row: column t belongs to the segment of the table that
// contains it (row b's frames at columns [t0_b, t0_b + T_b), times scale[b] when given); every other column is 0.
__global__ __launch_bounds__(256) void stft_frames_packed_kernel(const float* __restrict__ x, int64_t x_bs,
                                                                 const int64_t* __restrict__ lengths,
                                                                 const float* __restrict__ scale, const float* __restrict__ w,
                                                                 float* __restrict__ frames, const int32_t* __restrict__ seg,
                                                                 int B, int64_t L, int n_fft, int hop, int f_ld) {
  const int t = blockIdx.x * 64 + (threadIdx.x & 63);
  const int n0 = blockIdx.y * 256 + (threadIdx.x >> 6) * 64;
  if (t >= f_ld) return;
  int t0 = 0, Tb = 0;
  const int b = dn_seg_of(seg, B, t, t0, Tb);
  int64_t Lb = 0;
  const float* xb = x;
  float sc = 1.0f;
  if (b >= 0) {
    Lb = hsp_row_len(lengths, b, L);
    xb = x + (int64_t)b * x_bs;
    if (scale) sc = scale[b];
  }
  frame_column<int64_t>(xb, Lb, (int64_t)(t - t0) * hop - (n_fft >> 1), b >= 0 && Lb > 0, scale != nullptr, sc, w,
                        frames + t, f_ld, n0, n_fft);
}

// out[b][m][t] = log(sum_{f in [lo[m], hi[m])} fb[f][m] * (re^2 + im^2) + eps); lanes along t.
__global__ __launch_bounds__(64) void power_mel_log_kernel(const float* __restrict__ spec, int64_t s_bs, int s_ld,
                                                           const float* __restrict__ fbank, const int* __restrict__ f_lo,
                                                           const int* __restrict__ f_hi, float* __restrict__ out,
                                                           int n_freqs, int n_mels, int T_out, float eps) {
  const int b = blockIdx.z, m = blockIdx.y;
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= T_out) return;
  const float* re = spec + (int64_t)b * s_bs + t;
  const float* im = re + (int64_t)n_freqs * s_ld;
  const int lo = f_lo[m], hi = f_hi[m];
  float acc = 0.0f;
  for (int f = lo; f < hi; ++f) {
    const float r = re[(int64_t)f * s_ld], i = im[(int64_t)f * s_ld];
    acc = fmaf(fbank[f * n_mels + m], fmaf(r, r, i * i), acc);
  }
  out[((int64_t)b * n_mels + m) * T_out + t] = logf(acc + eps);
}

}  // namespace

#define HSP_STREAM static_cast<hipStream_t>(stream)

constexpr int FRAME_MAX_Y = 65535;   // grid y (256-position groups of the window) and z (rows)

extern "C" int hsp_stft_frames_f32(const float* x, const float* window, float* frames, int32_t B, int32_t L,
                                   int32_t n_fft, int32_t hop, int32_t T, int32_t f_ld, void* stream) {
  if (!x || !window || !frames || B <= 0 || n_fft <= 0 || hop <= 0 || T <= 0 || f_ld < T) return HSP_EINVAL;
  if (L <= n_fft / 2) return HSP_EINVAL;                       // reflect padding needs L > n_fft / 2 (as torch.stft)
  if ((int64_t)(T - 1) * hop > (int64_t)L) return HSP_EINVAL;  // the last frame's centre lies inside the signal
  if (B > FRAME_MAX_Y || (n_fft + 255) / 256 > FRAME_MAX_Y) return HSP_EINVAL;
  hipLaunchKernelGGL(stft_frames_kernel, dim3((f_ld + 63) / 64, (n_fft + 255) / 256, B), dim3(256), 0, HSP_STREAM, x,
                     (int64_t)L, nullptr, window, frames, L, n_fft, hop, T, f_ld);
  return (int)hipGetLastError();
}

extern "C" int hsp_stft_frames_ragged_f32(const float* x, int64_t x_bs, const int64_t* lengths, const float* window,
                                          float* frames, int32_t B, int32_t L, int32_t n_fft, int32_t hop, int32_t T,
                                          int32_t f_ld, void* stream) {
  if (!x || !lengths || !window || !frames || B <= 0 || n_fft <= 0 || hop <= 0 || T <= 0 || f_ld < T || x_bs < L)
    return HSP_EINVAL;
  if (L <= n_fft / 2 || T != 1 + L / hop) return HSP_EINVAL;
  if (B > FRAME_MAX_Y || (n_fft + 255) / 256 > FRAME_MAX_Y) return HSP_EINVAL;
  hipLaunchKernelGGL(stft_frames_kernel, dim3((f_ld + 63) / 64, (n_fft + 255) / 256, B), dim3(256), 0, HSP_STREAM, x,
                     x_bs, lengths, window, frames, L, n_fft, hop, T, f_ld);
  return (int)hipGetLastError();
}

extern "C" int hsp_stft_frames_packed_f32(const float* x, int64_t x_bs, const int64_t* lengths, const float* scale,
                                          const float* window, float* frames, const int32_t* seg, const int32_t* seg_host,
                                          int32_t B, int64_t L, int32_t n_fft, int32_t hop, int32_t T_tot, int32_t f_ld,
                                          void* stream) {
  if (!x || !lengths || !window || !frames || n_fft <= 0 || hop <= 0 || f_ld < T_tot || x_bs < L) return HSP_EINVAL;
  if (L <= n_fft / 2 || (n_fft + 255) / 256 > FRAME_MAX_Y) return HSP_EINVAL;
  if (!dn_seg_ok(seg, seg_host, B, T_tot)) return HSP_EINVAL;
  for (int b = 0; b < B; ++b)                                  // no row holds more frames than the longest can: 1 + L / hop
    if (seg_host[2 * b + 1] > 1 + L / hop) return HSP_EINVAL;
  hipLaunchKernelGGL(stft_frames_packed_kernel, dim3((f_ld + 63) / 64, (n_fft + 255) / 256), dim3(256), 0, HSP_STREAM, x,
                     x_bs, lengths, scale, window, frames, seg, B, L, n_fft, hop, f_ld);
  return (int)hipGetLastError();
}

extern "C" int hsp_power_mel_log_f32(const float* spec, int64_t s_bs, int32_t s_ld, const float* fb,
                                     const int32_t* f_lo, const int32_t* f_hi, float* out, int32_t B, int32_t n_freqs,
                                     int32_t n_mels, int32_t T_out, float eps, void* stream) {
  if (!spec || !fb || !f_lo || !f_hi || !out || B <= 0 || n_freqs <= 0 || n_mels <= 0 || T_out <= 0) return HSP_EINVAL;
  if (s_ld < T_out || B > 65535 || n_mels > 65535) return HSP_EINVAL;
  hipLaunchKernelGGL(power_mel_log_kernel, dim3((T_out + 63) / 64, n_mels, B), dim3(64), 0, HSP_STREAM, spec, s_bs,
                     s_ld, fb, f_lo, f_hi, out, n_freqs, n_mels, T_out, eps);
  return (int)hipGetLastError();
}
