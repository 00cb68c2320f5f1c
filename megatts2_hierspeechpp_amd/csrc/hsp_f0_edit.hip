// Pitch edit of ragged log-F0 rows (PitchEdit of prosody_controls.py).  Declarations and the
// arithmetic: include/hsp.h.
//
// One 256-thread workgroup per row, one launch: the voiced mean of ln Hz (each thread sums its strided frames in
// ascending order, then the halving tree of hsp_f0_convert_row), then the edit of every voiced frame, all in double.
// The order of every sum is fixed by the row alone, so row b of a batch is bit-identical to the call on row b alone.
// A thread reads frame i before it writes frame i and reads no other thread's frames after the reduction, so the output
// may be the input.
#include "hsp_rows.h"

#include <math.h>

namespace {

constexpr int NT = 256;   // threads per workgroup

__global__ __launch_bounds__(NT) void f0_edit_rows_kernel(const float* lf0, int64_t lf0_bs, const int64_t* __restrict__ lengths,
                                                          int64_t n, const float* __restrict__ shift,
                                                          const float* __restrict__ range,
                                                          const float* __restrict__ target_hz,
                                                          const float* __restrict__ offsets, int64_t off_bs, float f_min,
                                                          float f_max, float* out, int64_t out_bs,
                                                          float* __restrict__ mean_hz) {
  __shared__ double red[2][NT];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t nb = hsp_row_len(lengths, b, n);
  const float* lb = lf0 + (int64_t)b * lf0_bs;
  float* ob = out + (int64_t)b * out_bs;
  const float sh = shift ? shift[b] : 0.0f, rg = range ? range[b] : 1.0f, tg = target_hz ? target_hz[b] : 0.0f;
  const bool identity = sh == 0.0f && rg == 1.0f && !(tg > 0.0f) && !offsets;   // the same for every thread of the row
  double m = 0.0;
  if (!identity || mean_hz) {
    double s = 0.0, c = 0.0;
    for (int64_t i = tid; i < nb; i += NT) {
      const float l = lb[i];
      if (l > 0.0f) {
        s += log(expm1((double)l));
        c += 1.0;
      }
    }
    red[0][tid] = s;
    red[1][tid] = c;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
      if (tid < o) {
        red[0][tid] += red[0][tid + o];
        red[1][tid] += red[1][tid + o];
      }
      __syncthreads();
    }
    const double cnt = red[1][0];
    m = cnt > 0.0 ? red[0][0] / cnt : 0.0;
    if (mean_hz && tid == 0) mean_hz[b] = cnt > 0.0 ? (float)exp(m) : 0.0f;
  }
  if (identity) {   // bit for bit, no clamp: such a row takes part in a mixed batch without changing
    for (int64_t i = tid; i < n; i += NT) ob[i] = i < nb ? lb[i] : 0.0f;
    return;
  }
  const double centre = tg > 0.0f ? log((double)tg) : m;
  const double lo = log((double)f_min), hi = log((double)f_max);
  const double semitone = 0.69314718055994530942 / 12.0;
  const float* fb = offsets ? offsets + (int64_t)b * off_bs : nullptr;
  for (int64_t i = tid; i < n; i += NT) {
    float o = 0.0f;
    if (i < nb) {
      const float l = lb[i];
      if (l > 0.0f) {
        const double p = log(expm1((double)l));
        const double steps = (double)sh + (fb ? (double)fb[i] : 0.0);
        double q = centre + (double)rg * (p - m) + steps * semitone;
        q = fmin(fmax(q, lo), hi);
        o = (float)log1p(exp(q));
      }
    }
    ob[i] = o;
  }
}

inline bool finite_f(float v) { return v > -HUGE_VALF && v < HUGE_VALF; }

}  // namespace

#define HSP_STREAM static_cast<hipStream_t>(stream)

extern "C" int hsp_f0_edit_rows_f32(const hsp_f0_edit_args* a, void* stream) {
  if (!a || !a->lf0 || !a->out || a->B < 1 || a->B > 65535 || a->n < 1 || a->lf0_bs < a->n || a->out_bs < a->n)
    return HSP_EINVAL;
  if (a->offsets && a->off_bs < a->n) return HSP_EINVAL;
  if (!finite_f(a->f_min) || !finite_f(a->f_max) || !(a->f_min > 0.0f) || !(a->f_min < a->f_max)) return HSP_EINVAL;
  hipLaunchKernelGGL(f0_edit_rows_kernel, dim3((unsigned)a->B), dim3(NT), 0, HSP_STREAM, a->lf0, a->lf0_bs, a->lengths, a->n,
                     a->shift, a->range, a->target_hz, a->offsets, a->off_bs, a->f_min, a->f_max, a->out, a->out_bs,
                     a->mean_hz);
  return (int)hipGetLastError();
}
