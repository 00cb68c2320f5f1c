// True-peak meter and look-ahead limiter of ragged mono rows (scale_norm="lufs" with limiter=True).
// Declarations and the arithmetic: include/hsp.h.
//
// Everything is a finite window -- a 2Z-tap polyphase FIR, a sliding minimum, a raised-cosine weighted mean -- so a row
// is cut into tiles of TILE samples whose origin is relative to the row start, and one workgroup computes one tile from
// the samples around it alone: s over the tile needs m over +-W around it, m needs r over +-2W, r needs P one sample
// further back, P needs y over the FIR span.  All of it is staged and kept in LDS; x is read once, z is written once.
// The two row reductions (true peak: a max; smallest gain: a min) are order-independent, so the tiles fold their partial
// results with integer atomics on the bit patterns of non-negative floats into outputs the launcher presets on the same
// stream: bit-reproducible, and row b of a batch is bit-identical to the call on row b alone.
#include "hsp_rows.h"

#include <math.h>

namespace {

constexpr int TILE = 2048;                 // samples of a row per workgroup
constexpr int NT = 256;                    // threads per workgroup
constexpr int ZH = 6;                      // Z: half the taps of a phase
constexpr int TAPS = 2 * ZH;               // d = -(Z - 1) ... Z
constexpr int FMAX = 12;                   // phases at 16 kHz
constexpr int WMAX = 480;                  // look-ahead in samples
constexpr int NY_MAX = TILE + 4 * WMAX + TAPS;
constexpr int NP_MAX = TILE + 4 * WMAX + 1;
constexpr int NM_MAX = TILE + 2 * WMAX + 4;     // + 4: the last float4 of a thread's window ends past m
constexpr int NW_MAX = 2 * WMAX + 16;           // the weights, 3 zeros in front, zeros behind to a whole float4
constexpr int QT = TILE / (4 * NT);             // quads of consecutive samples per thread
static_assert((NY_MAX + NP_MAX + NM_MAX + NW_MAX + FMAX * TAPS + 8) * 4 <= 64 * 1024, "static LDS of limiter_kernel");
static_assert(TILE % (4 * NT) == 0, "every thread owns QT quads of the tile");

// ys[k] = y[g0 + k] for k < count: G x inside the row, 0 outside (samples at and after the row's length are never read)
__device__ __forceinline__ void stage_y(const float* __restrict__ xb, int64_t len, float g, int64_t g0, int count,
                                        float* __restrict__ ys) {
  for (int k = threadIdx.x; k < count; k += NT) {
    const int64_t i = g0 + k;
    ys[k] = (i >= 0 && i < len) ? __fmul_rn(g, xb[i]) : 0.0f;
  }
}

// P = max_p |sum_d h_p[d] y[i + d]|, taps ascending, one fma chain per phase from 0; yk = &ys[(i - (Z - 1)) - g0].
// Phase 0 is the unit impulse, so P >= |y[i]| exactly.
__device__ __forceinline__ float fir_peak(const float* __restrict__ yk, const float* __restrict__ bank, int F) {
  float v[TAPS];
#pragma unroll
  for (int d = 0; d < TAPS; ++d) v[d] = yk[d];
  float p = 0.0f;
  for (int ph = 0; ph < F; ++ph) {
    float acc = 0.0f;
#pragma unroll
    for (int d = 0; d < TAPS; ++d) acc = fmaf(bank[ph * TAPS + d], v[d], acc);
    p = fmaxf(p, fabsf(acc));
  }
  return p;
}

// max (MAX) or min of v over the workgroup; valid in thread 0
template <bool MAX>
__device__ __forceinline__ float block_fold(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float u = __shfl_xor(v, o, 64);
    v = MAX ? fmaxf(v, u) : fminf(v, u);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) v = MAX ? fmaxf(v, red[w]) : fminf(v, red[w]);
  return v;
}

__global__ __launch_bounds__(NT) void true_peak_kernel(const float* __restrict__ x, int64_t x_bs,
                                                       const int64_t* __restrict__ lengths,
                                                       const float* __restrict__ gains, int64_t n,
                                                       const float* __restrict__ bank_g, int F, float* __restrict__ tp) {
  __shared__ float ys[TILE + TAPS];
  __shared__ float bank[FMAX * TAPS];
  __shared__ float red[NT / 64];
  const int b = blockIdx.y;
  const int64_t len = hsp_row_len(lengths, b, n);
  const int64_t t0 = (int64_t)blockIdx.x * TILE;
  if (t0 >= len) return;
  const float g = gains ? gains[b] : 1.0f;
  for (int k = threadIdx.x; k < F * TAPS; k += NT) bank[k] = bank_g[k];
  stage_y(x + (int64_t)b * x_bs, len, g, t0 - (ZH - 1), TILE + TAPS - 1, ys);
  __syncthreads();
  float mx = 0.0f;
  for (int k = threadIdx.x; k < TILE; k += NT)
    if (t0 + k < len) mx = fmaxf(mx, fir_peak(ys + k, bank, F));
  mx = block_fold<true>(mx, red);
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned int*>(tp + b), __float_as_uint(mx));
}

__global__ __launch_bounds__(NT) void limiter_kernel(const float* __restrict__ x, int64_t x_bs,
                                                     const int64_t* __restrict__ lengths,
                                                     const float* __restrict__ gains, int64_t n,
                                                     const float* __restrict__ bank_g, int F, int W, float c,
                                                     float* __restrict__ z, int64_t z_bs, float* __restrict__ min_gain,
                                                     float* __restrict__ tp) {
  __shared__ float ys[NY_MAX];             // y  from sample t0 - 2W - Z
  __shared__ float pr[NP_MAX];             // P  from sample t0 - 2W - 1, then r from sample t0 - 2W
  __shared__ __attribute__((aligned(16))) float ms[NM_MAX];   // 1 - m from sample t0 - W
  __shared__ __attribute__((aligned(16))) float wp[NW_MAX];   // wp[k] = w[k - 3 - W], 0 outside |j| <= W
  __shared__ float bank[FMAX * TAPS];
  __shared__ float red[2 * (NT / 64)];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int64_t len = hsp_row_len(lengths, b, n);
  const int64_t t0 = (int64_t)blockIdx.x * TILE;
  float* zb = z + (int64_t)b * z_bs;
  const int cnt = (int)min((int64_t)TILE, n - t0);             // samples of the tile inside the buffer
  if (t0 >= len) {                                             // the whole tile lies past the row's end
    for (int k = tid; k < cnt; k += NT) zb[t0 + k] = 0.0f;
    return;
  }
  const float g = gains ? gains[b] : 1.0f;
  const int NP = TILE + 4 * W + 1, NR = TILE + 4 * W, NM = TILE + 2 * W;
  for (int k = tid; k < F * TAPS; k += NT) bank[k] = bank_g[k];
  // w[j] = (1 + cos(pi j / (W + 1))) / (2 W + 2): the cosines over |j| <= W sum to 1, so the weights sum to 1
  const int NQ = (2 * W + 4 + 3) / 4;                          // float4 steps that cover a quad's window of 2W + 4
  for (int k = tid; k < 4 * (NQ + 1); k += NT) {
    const int j = k - 3 - W;
    wp[k] = (j >= -W && j <= W) ? (float)((1.0 + cospi((double)j / (double)(W + 1))) / (double)(2 * W + 2)) : 0.0f;
  }
  stage_y(x + (int64_t)b * x_bs, len, g, t0 - 2 * W - ZH, NP + TAPS - 1, ys);
  __syncthreads();

  // P[i], 0 outside the row (P[-1] = 0)
  for (int k = tid; k < NP; k += NT) {
    const int64_t i = t0 - 2 * W - 1 + k;
    pr[k] = (i >= 0 && i < len) ? fir_peak(ys + k, bank, F) : 0.0f;
  }
  __syncthreads();
  if (tp) {                                                    // the true peak of y: this tile's own samples
    float mx = 0.0f;
    for (int k = tid; k < TILE; k += NT)
      if (t0 + k < len) mx = fmaxf(mx, pr[k + 2 * W + 1]);
    mx = block_fold<true>(mx, red);
    if (tid == 0) atomicMax(reinterpret_cast<unsigned int*>(tp + b), __float_as_uint(mx));
  }

  // r[i] = min(1, c / max(P[i - 1], P[i])) in place, 1 outside the row.  The quotient is stepped down by one float where
  // its product with p2 rounds above c: then fl(r p2) <= c, and since rounding is monotone, fl(s |y|) <= c for every
  // s <= r and |y| <= p2.
  constexpr int ER = (NP_MAX + NT - 1) / NT;
  float rv[ER];
#pragma unroll
  for (int e = 0; e < ER; ++e) {
    const int k = tid + e * NT;
    const int64_t i = t0 - 2 * W + k;
    float r = 1.0f;
    if (k < NR && i >= 0 && i < len) {
      const float p2 = fmaxf(pr[k], pr[k + 1]);
      if (p2 > c) {
        r = __fdiv_rn(c, p2);
        if (__fmul_rn(r, p2) > c) r = __uint_as_float(__float_as_uint(r) - 1u);
      }
    }
    rv[e] = r;
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < ER; ++e)
    if (tid + e * NT < NR) pr[tid + e * NT] = rv[e];
  __syncthreads();

  // thread t owns the quads of samples 4 t + 1024 e + (0 ... 3): their r, before pr is overwritten
  float rs[QT][4];
#pragma unroll
  for (int e = 0; e < QT; ++e)
#pragma unroll
    for (int o = 0; o < 4; ++o) rs[e][o] = pr[4 * tid + 4 * NT * e + o + 2 * W];
  __syncthreads();

  // m[k] = min_{|j| <= W} r[k + j], on every integer k the tile's weighted means read.  A minimum may count a sample
  // twice, so the window of 2W + 1 is two overlapping windows of `span`, the largest power of two inside it, and those
  // come from doubling in place: pr[i] = min r[i ... i + span - 1].  Kept as 1 - m.
  int span = 1;
  while (2 * span <= 2 * W + 1) {
#pragma unroll
    for (int e = 0; e < ER; ++e) {
      const int k = tid + e * NT;
      if (k < NR) rv[e] = k + span < NR ? fminf(pr[k], pr[k + span]) : pr[k];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < ER; ++e)
      if (tid + e * NT < NR) pr[tid + e * NT] = rv[e];
    __syncthreads();
    span *= 2;
  }
  for (int k = tid; k < NM + 4; k += NT) ms[k] = k < NM ? 1.0f - fminf(pr[k], pr[k + 2 * W + 1 - span]) : 0.0f;
  __syncthreads();

  // s[i] = min(r[i], 1 - sum_j w[j] (1 - m[i + j])), j ascending in one fma chain from 0; z = s y.  A quad's four windows
  // lie in 2W + 4 consecutive values: they are read a float4 at a time, and the weights of a step -- 7 consecutive ones,
  // zero where j falls outside |j| <= W, which leaves a chain as it is -- come from two float4 of wp.
  float acc[QT][4];
#pragma unroll
  for (int e = 0; e < QT; ++e)
#pragma unroll
    for (int o = 0; o < 4; ++o) acc[e][o] = 0.0f;
  const float4* ms4 = reinterpret_cast<const float4*>(ms);
  const float4* wp4 = reinterpret_cast<const float4*>(wp);
  float4 wa = wp4[0];
  for (int q = 0; q < NQ; ++q) {
    const float4 wb = wp4[q + 1];
    const float w7[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
    for (int e = 0; e < QT; ++e) {
      const float4 d4 = ms4[tid + NT * e + q];
      const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[e][o] = fmaf(w7[u - o + 3], dv[u], acc[e][o]);
    }
    wa = wb;
  }
  float mg = 1.0f;
#pragma unroll
  for (int e = 0; e < QT; ++e)
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int k = 4 * tid + 4 * NT * e + o;
      if (k < cnt) {
        float out = 0.0f;
        if (t0 + k < len) {
          const float s = fminf(rs[e][o], 1.0f - acc[e][o]);
          mg = fminf(mg, s);
          out = __fmul_rn(s, ys[k + 2 * W + ZH]);
        }
        zb[t0 + k] = out;
      }
    }
  mg = block_fold<false>(mg, red + NT / 64);
  if (tid == 0) atomicMin(reinterpret_cast<unsigned int*>(min_gain + b), __float_as_uint(mg));
}

// gains_out[b] = gains_in[b] 10^((target - lufs[b]) / 20), formed in double; a loudness that is not finite leaves the
// gain as it is.  gains_in NULL: the first gain of a row, 1 -- and 0 for a row without a loudness, which stays silent.
__global__ __launch_bounds__(256) void gain_update_kernel(const float* __restrict__ gains_in, const float* __restrict__ lufs,
                                                          float target, float* __restrict__ gains_out, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double l = (double)lufs[b];
  const bool fin = l > -HUGE_VAL && l < HUGE_VAL;
  double g = gains_in ? (double)gains_in[b] : (fin ? 1.0 : 0.0);
  if (fin) g *= pow(10.0, ((double)target - l) / 20.0);
  gains_out[b] = (float)g;
}

// the safety scale of the chain and the stats it reports, formed in double
__global__ __launch_bounds__(256) void limiter_stats_kernel(const float* __restrict__ lufs, const float* __restrict__ tp,
                                                            float c, float* __restrict__ q, float* __restrict__ achieved,
                                                            float* __restrict__ true_peak, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float t = tp[b];
  float qv = 1.0f;
  if (t > c) {
    qv = __fdiv_rn(c, t);
    if (__fmul_rn(qv, t) > c) qv = __uint_as_float(__float_as_uint(qv) - 1u);
  }
  q[b] = qv;
  achieved[b] = (float)((double)lufs[b] + 20.0 * log10((double)qv));
  true_peak[b] = __fmul_rn(t, qv);
}

// out[b, i] = (int16)(x[b, i] g_b 32767), truncated toward zero and saturating, zeros from the row's length on
__global__ __launch_bounds__(256) void gain_int16_kernel(const float* __restrict__ x, int64_t x_bs,
                                                         const int64_t* __restrict__ lengths,
                                                         const float* __restrict__ gains, int16_t* __restrict__ out,
                                                         int64_t o_bs, int64_t n) {
  const int b = blockIdx.y;
  const int64_t len = hsp_row_len(lengths, b, n);
  const float g = gains[b];
  const float* xb = x + (int64_t)b * x_bs;
  int16_t* ob = out + (int64_t)b * o_bs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float v = 0.0f;
    if (i < len) v = __fmul_rn(__fmul_rn(xb[i], g), 32767.0f);
    ob[i] = (int16_t)fminf(fmaxf(v, -32768.0f), 32767.0f);
  }
}

bool rows_ok(const float* x, int64_t x_bs, int32_t B, int64_t n) {
  return x && B > 0 && B <= 65535 && n > 0 && x_bs >= n && hsp_grid_fits(n, TILE);
}
bool bank_ok(const float* bank, int32_t F, int32_t Z) { return bank && (F == 4 || F == 8 || F == 12) && Z == ZH; }

}  // namespace

#define HSP_STREAM static_cast<hipStream_t>(stream)

extern "C" int hsp_true_peak_f32(const float* x, int64_t x_bs, const int64_t* lengths, const float* gains, int32_t B,
                                 int64_t n, const float* bank, int32_t F, int32_t Z, float* tp, void* stream) {
  if (!rows_ok(x, x_bs, B, n) || !bank_ok(bank, F, Z) || !tp) return HSP_EINVAL;
  hipError_t e = hipMemsetAsync(tp, 0, (size_t)B * sizeof(float), HSP_STREAM);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(true_peak_kernel, dim3((unsigned)((n + TILE - 1) / TILE), (unsigned)B), dim3(NT), 0, HSP_STREAM, x, x_bs,
                     lengths, gains, n, bank, F, tp);
  return (int)hipGetLastError();
}

extern "C" int hsp_limiter_f32(const hsp_limiter_args* a, void* stream) {
  if (!a || !rows_ok(a->x, a->x_bs, a->B, a->n) || !bank_ok(a->bank, a->F, a->Z) || !a->y || !a->min_gain) return HSP_EINVAL;
  if (a->y_bs < a->n || a->W < 1 || a->W > WMAX || !(a->ceiling > 0.0f && a->ceiling < HUGE_VALF)) return HSP_EINVAL;
  hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a->min_gain), 0x3f800000, (size_t)a->B, HSP_STREAM);   // 1.0f
  if (e == hipSuccess && a->tp) e = hipMemsetAsync(a->tp, 0, (size_t)a->B * sizeof(float), HSP_STREAM);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(limiter_kernel, dim3((unsigned)((a->n + TILE - 1) / TILE), (unsigned)a->B), dim3(NT), 0, HSP_STREAM, a->x,
                     a->x_bs, a->lengths, a->gains, a->n, a->bank, a->F, a->W, a->ceiling, a->y, a->y_bs, a->min_gain,
                     a->tp);
  return (int)hipGetLastError();
}

extern "C" int hsp_gain_update_f32(const float* gains_in, const float* lufs, float target_lufs, float* gains_out,
                                   int32_t B, void* stream) {
  if (!lufs || !gains_out || B <= 0 || !(target_lufs > -HUGE_VALF && target_lufs < HUGE_VALF)) return HSP_EINVAL;
  hipLaunchKernelGGL(gain_update_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, HSP_STREAM, gains_in, lufs,
                     target_lufs, gains_out, B);
  return (int)hipGetLastError();
}

extern "C" int hsp_limiter_stats_f32(const float* lufs, const float* tp, float ceiling, float* q, float* achieved_lufs,
                                     float* true_peak, int32_t B, void* stream) {
  if (!lufs || !tp || !q || !achieved_lufs || !true_peak || B <= 0 || !(ceiling > 0.0f && ceiling < HUGE_VALF))
    return HSP_EINVAL;
  hipLaunchKernelGGL(limiter_stats_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, HSP_STREAM, lufs, tp, ceiling, q,
                     achieved_lufs, true_peak, B);
  return (int)hipGetLastError();
}

extern "C" int hsp_gain_int16_f32(const float* x, int64_t x_bs, const int64_t* lengths, const float* gains, int16_t* out,
                                  int64_t o_bs, int32_t B, int64_t n, void* stream) {
  if (!x || !gains || !out || B <= 0 || B > 65535 || n <= 0 || x_bs < n || o_bs < n) return HSP_EINVAL;
  hipLaunchKernelGGL(gain_int16_kernel, dim3(hsp_flat_grid(n, 256, 4096), (unsigned)B), dim3(256), 0, HSP_STREAM, x, x_bs,
                     lengths, gains, out, o_bs, n);
  return (int)hipGetLastError();
}
