// Batched voice conversion (inference_vc.vc_batch): the per-row-length forms of the single-utterance steps of the
// harness (inference_vc.py:80-126, 157-160).  Row lengths are device int64 [B] so that a fixed-shape batch can be
// captured in a hipGraph with no host read-back; every length is clamped into the buffer it indexes.  Declarations and
// semantics: include/hsp.h.  None of this is MFMA work: each kernel reads and writes its rows once.
#include "hsp_device.h"

namespace {

__device__ __forceinline__ int64_t clamp_len(const int64_t* len, int b, int64_t cap) {
  return len ? min(cap, max((int64_t)0, len[b])) : cap;
}

// y[b][t] = x[b][reflect(t - pad)] over [0, len_b + 2 pad), zero on [len_b + 2 pad, Lo).  One thread per output
// sample; blockIdx.y = row.  The clamp after the reflection only matters for len_b <= pad (outside the contract).
__global__ __launch_bounds__(256) void reflect_pad_ragged_kernel(const float* __restrict__ x, int64_t x_bs,
                                                                 const int64_t* __restrict__ lengths, float* __restrict__ y,
                                                                 int64_t y_bs, int L, int pad, int Lo) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Lo) return;
  const int n = (int)clamp_len(lengths, b, L);
  float v = 0.0f;
  if (n > 0 && t < n + 2 * pad) {
    int s = t - pad;
    s = s < 0 ? -s : (s >= n ? 2 * (n - 1) - s : s);
    s = min(max(s, 0), n - 1);
    v = x[(int64_t)b * x_bs + s];
  }
  y[(int64_t)b * y_bs + t] = v;
}

// one 256-thread workgroup per row: the single-utterance conversion on that row's tracks (hsp_f0_convert_row)
__global__ __launch_bounds__(256) void f0_convert_batch_kernel(const float* __restrict__ src, int64_t src_bs,
                                                               const int64_t* __restrict__ n_src,
                                                               const float* __restrict__ trg, int64_t trg_bs,
                                                               const int64_t* __restrict__ n_trg, int nt_max,
                                                               float* __restrict__ out, int64_t out_bs, int n_max) {
  const int b = blockIdx.x;
  const int ns = (int)clamp_len(n_src, b, n_max), nt = (int)clamp_len(n_trg, b, nt_max);
  hsp_f0_convert_row(src + (int64_t)b * src_bs, ns, trg + (int64_t)b * trg_bs, nt, out + (int64_t)b * out_bs, n_max);
}

// stft_frames_kernel of hsp_mel.hip with row b's own length: T_b = 1 + len_b / hop frames that reflect at len_b,
// zero columns on [T_b, f_ld).  Block = 64 frames x 256 window positions of one row, lanes along t.
__global__ __launch_bounds__(256) void stft_frames_ragged_kernel(const float* __restrict__ x, int64_t x_bs,
                                                                 const int64_t* __restrict__ lengths,
                                                                 const float* __restrict__ w, float* __restrict__ frames,
                                                                 int L, int n_fft, int hop, int T, int f_ld) {
  const int b = blockIdx.z;
  const int t = blockIdx.x * 64 + (threadIdx.x & 63);
  const int n0 = blockIdx.y * 256 + (threadIdx.x >> 6) * 64;
  if (t >= f_ld) return;
  const int Lb = (int)clamp_len(lengths, b, L);
  const int Tb = Lb > 0 ? min(T, 1 + Lb / hop) : 0;
  const float* xb = x + (int64_t)b * x_bs;
  float* fb = frames + (int64_t)b * n_fft * f_ld;
  const int base = t * hop - (n_fft >> 1);
  for (int n = n0; n < min(n0 + 64, n_fft); ++n) {
    float v = 0.0f;
    if (t < Tb) {
      int i = base + n;
      i = i < 0 ? -i : i;
      i = i >= Lb ? 2 * (Lb - 1) - i : i;
      i = min(max(i, 0), Lb - 1);             // only for Lb <= n_fft / 2 (outside the contract)
      v = w[n] * xb[i];
    }
    fb[(int64_t)n * f_ld + t] = v;
  }
}

__global__ __launch_bounds__(1024) void abs_max_rows_kernel(const float* __restrict__ x, int64_t x_bs,
                                                            const int64_t* __restrict__ len, float* __restrict__ out,
                                                            int64_t n) {
  const int b = blockIdx.x;
  const float mx = hsp_block_abs_max_1024(x + b * x_bs, clamp_len(len, b, n));
  if (threadIdx.x == 0) out[b] = mx;
}

// peak_int16_kernel of hsp_frontend.hip with the gain of row b read from gains[b] (both run hsp_peak_int16_row)
__global__ __launch_bounds__(1024) void peak_int16_gains_kernel(const float* __restrict__ x, int64_t x_bs,
                                                                const int64_t* __restrict__ len,
                                                                const float* __restrict__ gains,
                                                                int16_t* __restrict__ out, int64_t o_bs, int64_t n) {
  const int b = blockIdx.x;
  hsp_peak_int16_row(x + b * x_bs, clamp_len(len, b, n), gains[b], out + b * o_bs, n);
}

}  // namespace

#define HSP_STREAM static_cast<hipStream_t>(stream)

extern "C" int hsp_reflect_pad_ragged_f32(const float* x, int64_t x_bs, const int64_t* lengths, float* y, int64_t y_bs,
                                          int32_t B, int32_t L, int32_t pad, int32_t Lo, void* stream) {
  if (!x || !y || B <= 0 || L <= 0 || pad < 0 || pad >= L || Lo <= 0) return HSP_EINVAL;
  if (x_bs < L || y_bs < Lo || (int64_t)Lo > (int64_t)L + 2 * pad || B > 65535) return HSP_EINVAL;
  hipLaunchKernelGGL(reflect_pad_ragged_kernel, dim3((Lo + 255) / 256, B), dim3(256), 0, HSP_STREAM, x, x_bs, lengths,
                     y, y_bs, L, pad, Lo);
  return (int)hipGetLastError();
}

extern "C" int hsp_f0_convert_batch_f32(const float* f0_src, int64_t src_bs, const int64_t* n_src, const float* f0_trg,
                                        int64_t trg_bs, const int64_t* n_trg, int32_t nt_max, float* out,
                                        int64_t out_bs, int32_t B, int32_t n_max, void* stream) {
  if (!f0_src || !n_src || !f0_trg || !n_trg || !out || B <= 0 || n_max <= 0 || nt_max <= 0) return HSP_EINVAL;
  if (src_bs < n_max || out_bs < n_max || trg_bs < 0 || (trg_bs > 0 && trg_bs < nt_max)) return HSP_EINVAL;
  hipLaunchKernelGGL(f0_convert_batch_kernel, dim3(B), dim3(256), 0, HSP_STREAM, f0_src, src_bs, n_src, f0_trg, trg_bs,
                     n_trg, nt_max, out, out_bs, n_max);
  return (int)hipGetLastError();
}

extern "C" int hsp_stft_frames_ragged_f32(const float* x, int64_t x_bs, const int64_t* lengths, const float* window,
                                          float* frames, int32_t B, int32_t L, int32_t n_fft, int32_t hop, int32_t T,
                                          int32_t f_ld, void* stream) {
  if (!x || !lengths || !window || !frames || B <= 0 || n_fft <= 0 || hop <= 0 || T <= 0 || f_ld < T || x_bs < L)
    return HSP_EINVAL;
  if (L <= n_fft / 2 || T != 1 + L / hop) return HSP_EINVAL;
  if (B > 65535 || (n_fft + 255) / 256 > 65535) return HSP_EINVAL;
  hipLaunchKernelGGL(stft_frames_ragged_kernel, dim3((f_ld + 63) / 64, (n_fft + 255) / 256, B), dim3(256), 0,
                     HSP_STREAM, x, x_bs, lengths, window, frames, L, n_fft, hop, T, f_ld);
  return (int)hipGetLastError();
}

extern "C" int hsp_abs_max_rows_f32(const float* x, int64_t x_bs, const int64_t* lengths, float* out, int32_t B,
                                    int64_t n, void* stream) {
  if (!x || !out || B <= 0 || n <= 0 || x_bs < n) return HSP_EINVAL;
  hipLaunchKernelGGL(abs_max_rows_kernel, dim3((unsigned)B), dim3(1024), 0, HSP_STREAM, x, x_bs, lengths, out, n);
  return (int)hipGetLastError();
}

extern "C" int hsp_peak_int16_gains(const float* x, int64_t x_bs, const int64_t* lengths, const float* gains,
                                    int16_t* out, int64_t o_bs, int32_t B, int64_t n, void* stream) {
  if (!x || !gains || !out || B <= 0 || n <= 0 || x_bs < n || o_bs < n) return HSP_EINVAL;
  hipLaunchKernelGGL(peak_int16_gains_kernel, dim3((unsigned)B), dim3(1024), 0, HSP_STREAM, x, x_bs, lengths, gains, out,
                     o_bs, n);
  return (int)hipGetLastError();
}
