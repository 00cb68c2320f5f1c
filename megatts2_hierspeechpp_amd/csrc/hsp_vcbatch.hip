// Batched voice conversion (inference_vc.vc_batch): the per-row-length forms of the single-utterance steps of the
// harness (inference_vc.py:80-126, 157-160).  Row lengths are device int64 [B] so that a fixed-shape batch can be
// captured in a hipGraph with no host read-back; every length is clamped into the buffer it indexes.  Declarations and
// semantics: include/hsp.h.  None of this is MFMA work: each kernel reads and writes its rows once.
#include "hsp_rows.h"

namespace {

// one 256-thread workgroup per row: the single-utterance conversion on that row's tracks (hsp_f0_convert_row)
__global__ __launch_bounds__(256) void f0_convert_batch_kernel(const float* __restrict__ src, int64_t src_bs,
                                                               const int64_t* __restrict__ n_src,
                                                               const float* __restrict__ trg, int64_t trg_bs,
                                                               const int64_t* __restrict__ n_trg, int nt_max,
                                                               float* __restrict__ out, int64_t out_bs, int n_max) {
  const int b = blockIdx.x;
  const int ns = (int)hsp_row_len(n_src, b, n_max), nt = (int)hsp_row_len(n_trg, b, nt_max);
  hsp_f0_convert_row(src + (int64_t)b * src_bs, ns, trg + (int64_t)b * trg_bs, nt, out + (int64_t)b * out_bs, n_max);
}

__global__ __launch_bounds__(1024) void abs_max_rows_kernel(const float* __restrict__ x, int64_t x_bs,
                                                            const int64_t* __restrict__ len, float* __restrict__ out,
                                                            int64_t n) {
  const int b = blockIdx.x;
  const float mx = hsp_block_abs_max_1024(x + b * x_bs, hsp_row_len(len, b, n));
  if (threadIdx.x == 0) out[b] = mx;
}

// hsp_peak_int16_row (hsp_device.h) with the gain of row b read from gains[b]
__global__ __launch_bounds__(1024) void peak_int16_gains_kernel(const float* __restrict__ x, int64_t x_bs,
                                                                const int64_t* __restrict__ len,
                                                                const float* __restrict__ gains,
                                                                int16_t* __restrict__ out, int64_t o_bs, int64_t n) {
  const int b = blockIdx.x;
  hsp_peak_int16_row(x + b * x_bs, hsp_row_len(len, b, n), gains[b], out + b * o_bs, n);
}

}  // namespace

#define HSP_STREAM static_cast<hipStream_t>(stream)

extern "C" int hsp_f0_convert_batch_f32(const float* f0_src, int64_t src_bs, const int64_t* n_src, const float* f0_trg,
                                        int64_t trg_bs, const int64_t* n_trg, int32_t nt_max, float* out,
                                        int64_t out_bs, int32_t B, int32_t n_max, void* stream) {
  if (!f0_src || !n_src || !f0_trg || !n_trg || !out || B <= 0 || n_max <= 0 || nt_max <= 0) return HSP_EINVAL;
  if (src_bs < n_max || out_bs < n_max || trg_bs < 0 || (trg_bs > 0 && trg_bs < nt_max)) return HSP_EINVAL;
  hipLaunchKernelGGL(f0_convert_batch_kernel, dim3(B), dim3(256), 0, HSP_STREAM, f0_src, src_bs, n_src, f0_trg, trg_bs,
                     n_trg, nt_max, out, out_bs, n_max);
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
