// One pre-LN transformer layer of the Mega-TTS2 prosody LM for ONE new position of B rows, against a K/V cache
// (include/hsp.h "causal PLM decoding"): the step of Megatts2PLM1.infer(causal=True).  Under the causal mask of the
// reference's training forward (ttv_v1/utils_mega.py:21-39) position j's activations never change after step j, so a
// step is one column per row in every layer.
//
// Design: a step's cost is streaming the layer's weights (3 D D + D D + 2 D F floats: 3.66 MB at 276 / 1104), and one
// compute unit pulls ~60 GB/s: one workgroup per row for the whole layer was measured at ~60 us per launch, slower than
// the bidirectional loop at B = 1.  So a row is split over several workgroups, in three launches on the stream:
//   1. attention, grid (B, H): workgroup (b, h) normalises the row, projects q / k / v of ITS head (3 Dh columns of
//      the stacked weight), stores k / v to column t of the cache, runs the head's softmax over keys 0 .. t and writes
//      the head's Dh attention outputs to the workspace;
//   2. feed-forward, grid (B, P), P = HSP_PLM_DECODE_SPLIT: every workgroup repeats the small out-proj + residual +
//      LayerNorm (D D weights), then takes F / P hidden units: their ff.0 rows, ReLU, and their share of ff.3 -- a
//      partial sum over its hidden units for all D outputs, to the workspace (workgroup 0 adds x1 + c2);
//   3. sum, grid (B): y = the P partial sums added in order.
// A workgroup streams 0.23 MB (1) or 0.61 MB (2) instead of 3.66 MB.  Weights are read TRANSPOSED ([K][M], packed at
// finalize): in the GEMVs thread (q, s) owns four outputs over the s-th slice of the K inputs, so a wave reads
// consecutive weights (float4 per lane) and no load of a thread depends on the one before; the S partial sums of an
// output meet in LDS in a fixed order, and so do the P partial sums of launch 3: a row's result does not depend on the
// batch around it.  Attention: one thread per key takes the dot product with lanes running along the cache's time axis
// (unit stride), one wave does the softmax in LDS, then four channels per wave sum p V with lanes along time again.
//
// Two forms of every launch share one body per row (attn_row / ffn_row / sum_row): by value, every row at a.t
// (hsp_plm_decode_layer_f32), and by position, row b at pos[b] read from device memory (hsp_plm_decode_layer_pos_f32;
// hsp.h "per-row positions"), where a row outside [0, a.t] is idle and its workgroups return at once -- the form that lets
// one captured step serve rows of every length (Megatts2PLM1.decode_session).
#include <cmath>

#include "hsp_device.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kPartFloats = 4096;   // S * M partial sums of a GEMV: (kThreads / (M / 4)) * M <= 4 * kThreads

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// out[c] = (in[c] - mean) * rstd * g[c] + b[c] over D channels in LDS; every wave computes the statistics itself (two
// passes, as torch does), so no barrier is needed between them and the normalisation.  Ends with a barrier.
__device__ __forceinline__ void layernorm_lds(const float* in, float* out, const float* __restrict__ g,
                                              const float* __restrict__ b, int D, float eps) {
  const int lane = threadIdx.x & 63;
  float s = 0.0f;
  for (int c = lane; c < D; c += 64) s += in[c];
  const float mean = wave_sum(s) / (float)D;
  float q = 0.0f;
  for (int c = lane; c < D; c += 64) {
    const float d = in[c] - mean;
    q += d * d;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  for (int c = threadIdx.x; c < D; c += kThreads) out[c] = (in[c] - mean) * rstd * g[c] + b[c];
  __syncthreads();
}

// part[s * M + m] = sum over the s-th slice of k of wt[k * ld + m] * in[k]  (wt [K][>= M] with row pitch ld, M % 4 == 0,
// ld % 4 == 0, 16-B aligned).
// Ends with a barrier; the caller then sums part[s * M + m] over s < gemv_splits(M) in order.
__device__ __forceinline__ int gemv_splits(int M) { return kThreads / (M >> 2); }
__device__ __forceinline__ void gemv_partials(const float* __restrict__ wt, int ld, const float* in, float* part, int K,
                                              int M) {
  const int Q = M >> 2, S = kThreads / Q;
  const int tid = threadIdx.x;
  if (tid < Q * S) {
    const int q = tid % Q, s = tid / Q;
    const int kc = (K + S - 1) / S;
    const int k0 = s * kc, k1 = min(K, k0 + kc);
    const int ld4 = ld >> 2;
    const float4* w = reinterpret_cast<const float4*>(wt) + (int64_t)k0 * ld4 + q;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 8
    for (int k = k0; k < k1; ++k, w += ld4) {
      const float4 v = *w;
      const float h = in[k];
      acc.x = fmaf(v.x, h, acc.x);
      acc.y = fmaf(v.y, h, acc.y);
      acc.z = fmaf(v.z, h, acc.z);
      acc.w = fmaf(v.w, h, acc.w);
    }
    *reinterpret_cast<float4*>(part + (int64_t)s * M + 4 * q) = acc;
  }
  __syncthreads();
}

__device__ __forceinline__ float sum_partials(const float* part, int m, int M) {
  const int S = gemv_splits(M);
  float v = part[m];
  for (int s = 1; s < S; ++s) v += part[s * M + m];
  return v;
}

constexpr int kP = HSP_PLM_DECODE_SPLIT;

// workspace: at [B][D] attention outputs, then partial [B][kP][D]
__device__ __forceinline__ float* ws_at(const hsp_plm_decode_args& a, int b) {
  return static_cast<float*>(a.workspace) + (int64_t)b * a.D;
}
__device__ __forceinline__ float* ws_part(const hsp_plm_decode_args& a, int b, int p) {
  return static_cast<float*>(a.workspace) + (int64_t)a.B * a.D + ((int64_t)b * kP + p) * a.D;
}

// launch 1 for row b, head h at position t (the by-value kernel passes a.t, the position form pos[b])
__device__ __forceinline__ void attn_row(const hsp_plm_decode_args& a, int b, int h, int t, float* lds) {
  const int D = a.D, n = t + 1, Dh = a.D / a.H;
  const int Dhp = (Dh + 3) & ~3;
  float* xs = lds;                 // [D]   x
  float* hs = xs + D;              // [D]   LayerNorm(x)
  float* qkv = hs + D;             // [3][Dhp] q | k | v of this head, new position
  float* part = qkv + 3 * Dhp;     // [S][3 Dh] partial sums
  float* linv = part + kPartFloats;   // [4]
  float* sc = linv + 4;            // [n] scores, then exp(score - max)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  const float* xb = a.x + (int64_t)b * a.x_bs;
  for (int c = tid; c < D; c += kThreads) xs[c] = xb[(int64_t)c * a.x_cs];
  __syncthreads();
  layernorm_lds(xs, hs, a.g1, a.b1, D, a.eps);

  // the head's 3 Dh outputs (columns which * D + h Dh + d of wqkv_t), S slices of the D inputs each
  const int M3 = 3 * Dh, S = kThreads / M3, kc = (D + S - 1) / S;
  if (tid < M3 * S) {
    const int o = tid % M3, s = tid / M3;
    const int col = (o / Dh) * D + h * Dh + o % Dh;
    const int k0 = s * kc, k1 = min(D, k0 + kc);
    const float* w = a.wqkv_t + (int64_t)k0 * (3 * D) + col;
    float acc = 0.0f;
#pragma unroll 8
    for (int k = k0; k < k1; ++k, w += 3 * D) acc = fmaf(*w, hs[k], acc);
    part[s * M3 + o] = acc;
  }
  __syncthreads();
  float* kb = a.k_cache + (int64_t)b * a.bs + (int64_t)(h * Dh) * a.cs;
  float* vb = a.v_cache + (int64_t)b * a.bs + (int64_t)(h * Dh) * a.cs;
  if (tid < M3) {
    const int which = tid / Dh, d = tid % Dh;
    float v = part[tid];
    for (int s = 1; s < S; ++s) v += part[s * M3 + tid];
    v += a.bqkv[which * D + h * Dh + d];
    qkv[which * Dhp + d] = v;
    if (which == 1) kb[(int64_t)d * a.cs + t] = v;
    if (which == 2) vb[(int64_t)d * a.cs + t] = v;
  }
  __syncthreads();

  // scores of the new query against keys 0 .. t (column t from LDS: what this workgroup has just stored)
  const float scale = 1.0f / sqrtf((float)Dh);
  const float *qh = qkv, *kh = qkv + Dhp, *vh = qkv + 2 * Dhp;
  for (int j = tid; j < n; j += kThreads) {
    float s = 0.0f;
    if (j == t) {
      for (int d = 0; d < Dh; ++d) s = fmaf(qh[d], kh[d], s);
    } else {
      const float* kp = kb + j;
#pragma unroll 8
      for (int d = 0; d < Dh; ++d) s = fmaf(qh[d], kp[(int64_t)d * a.cs], s);
    }
    sc[j] = s * scale;
  }
  __syncthreads();
  if (wave == 0) {
    float mx = -INFINITY;
    for (int j = lane; j < n; j += 64) mx = fmaxf(mx, sc[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float l = 0.0f;
    for (int j = lane; j < n; j += 64) {
      const float p = hsp_exp2e(sc[j] - mx);
      sc[j] = p;
      l += p;
    }
    l = wave_sum(l);
    if (lane == 0) linv[0] = 1.0f / l;
  }
  __syncthreads();
  // out[d] = sum_j p[j] v[d][j] / l: four channels per wave at a time, lanes along the keys.  (Spreading the Dh = 69
  // channels 5 per wave, so that no wave walks the keys twice, was measured: the loop got 0.8 ms / 1.2 ms slower at
  // 16 x 200 / 1 x 200 -- the per-channel predicate in the inner loop costs more than the second walk of two waves.)
  float* out = ws_at(a, b) + h * Dh;
  for (int d0 = wave * 4; d0 < Dh; d0 += (kThreads / 64) * 4) {
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = lane; j < t; j += 64) {
      const float p = sc[j];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = fmaf(p, vb[(int64_t)min(d0 + u, Dh - 1) * a.cs + j], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float s = wave_sum(acc[u]);
      if (lane == 0 && d0 + u < Dh) out[d0 + u] = (s + sc[t] * vh[d0 + u]) * linv[0];
    }
  }
}

// launch 2 for row b, slice p of the hidden units
__device__ __forceinline__ void ffn_row(const hsp_plm_decode_args& a, int b, int p, float* lds) {
  const int D = a.D, F = a.F, Fs = a.F / kP;
  float* xs = lds;                 // [D]  x, then x1
  float* hs = xs + D;              // [D]  attention output, then LayerNorm(x1)
  float* ff = hs + D;              // [Fs] relu(W1 h + c1), this workgroup's hidden units
  float* part = ff + Fs;           // [kPartFloats]
  const int tid = threadIdx.x;

  const float* xb = a.x + (int64_t)b * a.x_bs;
  const float* at = ws_at(a, b);
  for (int c = tid; c < D; c += kThreads) xs[c] = xb[(int64_t)c * a.x_cs], hs[c] = at[c];
  __syncthreads();
  // x1 = x + Wo at + bo (every workgroup of the row: D D weights)
  gemv_partials(a.wo_t, D, hs, part, D, D);
  for (int m = tid; m < D; m += kThreads) xs[m] += sum_partials(part, m, D) + a.bo[m];
  __syncthreads();
  layernorm_lds(xs, hs, a.g2, a.b2, D, a.eps);
  // hidden units [p Fs, (p + 1) Fs): ff.0 + ReLU, then their share of ff.3
  gemv_partials(a.w1_t + p * Fs, F, hs, part, D, Fs);
  for (int m = tid; m < Fs; m += kThreads) ff[m] = fmaxf(sum_partials(part, m, Fs) + a.c1[p * Fs + m], 0.0f);
  __syncthreads();
  gemv_partials(a.w2_t + (int64_t)p * Fs * D, D, ff, part, Fs, D);
  float* o = ws_part(a, b, p);
  for (int m = tid; m < D; m += kThreads) {
    float v = sum_partials(part, m, D);
    if (p == 0) v += xs[m] + a.c2[m];
    o[m] = v;
  }
}

// launch 3 for row b: y = the kP partial sums in order
__device__ __forceinline__ void sum_row(const hsp_plm_decode_args& a, int b) {
  float* yb = a.y + (int64_t)b * a.y_bs;
  for (int m = threadIdx.x; m < a.D; m += 256) {
    float v = ws_part(a, b, 0)[m];
    for (int p = 1; p < kP; ++p) v += ws_part(a, b, p)[m];
    yb[(int64_t)m * a.y_cs] = v;
  }
}

// The kernels: grid B * H (workgroup b * H + h), B * kP (workgroup b * kP + p) and B.  By value, every row is at a.t.
__global__ __launch_bounds__(kThreads) void plm_decode_attn_kernel(hsp_plm_decode_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  attn_row(a, blockIdx.x / a.H, blockIdx.x % a.H, a.t, lds);
}
__global__ __launch_bounds__(kThreads) void plm_decode_ffn_kernel(hsp_plm_decode_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  ffn_row(a, blockIdx.x / kP, blockIdx.x % kP, lds);
}
__global__ __launch_bounds__(256) void plm_decode_sum_kernel(hsp_plm_decode_args a) {
  sum_row(a, blockIdx.x);
}

// Position form (hsp.h "per-row positions"): row b is at pos[b], read here.  A row whose position is not in [0, a.t] is
// idle: its workgroups return before they touch memory -- the check is what bounds the cache column and the LDS scores
// (sized for a.t + 1 keys by the host).  One row per workgroup, so the branch is uniform.
__device__ __forceinline__ bool row_active(const hsp_plm_decode_args& a, const int32_t* __restrict__ pos, int b, int* t) {
  *t = pos[b];
  return *t >= 0 && *t <= a.t;
}
__global__ __launch_bounds__(kThreads) void plm_decode_attn_pos_kernel(hsp_plm_decode_args a,
                                                                      const int32_t* __restrict__ pos) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int t;
  if (row_active(a, pos, blockIdx.x / a.H, &t)) attn_row(a, blockIdx.x / a.H, blockIdx.x % a.H, t, lds);
}
__global__ __launch_bounds__(kThreads) void plm_decode_ffn_pos_kernel(hsp_plm_decode_args a,
                                                                     const int32_t* __restrict__ pos) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int t;
  if (row_active(a, pos, blockIdx.x / kP, &t)) ffn_row(a, blockIdx.x / kP, blockIdx.x % kP, lds);
}
__global__ __launch_bounds__(256) void plm_decode_sum_pos_kernel(hsp_plm_decode_args a, const int32_t* __restrict__ pos) {
  int t;
  if (row_active(a, pos, blockIdx.x, &t)) sum_row(a, blockIdx.x);
}

constexpr int kLdsMax = 160 * 1024;

// dynamic LDS of the attention launch, or -1 when the geometry is not served
int64_t attn_lds_bytes(int64_t D, int64_t H, int64_t F, int64_t n) {
  if (D < 4 || H < 1 || F < 4 || D % 4 || D % H || F % (4 * kP)) return -1;
  if (D > kThreads || 3 * (D / H) > kThreads || F / kP > kThreads) return -1;   // launch 2 stays within 32 KB of LDS
  const int64_t Dhp = (D / H + 3) & ~3;
  return (2 * D + 3 * Dhp + kPartFloats + 4 + n) * 4;
}

}  // namespace

extern "C" int hsp_plm_decode_supported(int32_t D, int32_t H, int32_t F) {
  const int64_t lds = attn_lds_bytes(D, H, F, 1);
  return lds > 0 && lds <= kLdsMax ? 1 : 0;
}

extern "C" int64_t hsp_plm_decode_workspace_bytes(int32_t B, int32_t D) {
  if (B <= 0 || D <= 0) return 0;
  return (int64_t)B * D * (1 + kP) * 4;
}

namespace {

// the refusals of both layer entry points (hsp.h); the attention launch's LDS bytes for a->t + 1 keys, or -1
int64_t decode_args_lds(const hsp_plm_decode_args* a) {
  if (!a) return -1;
  if (!a->x || !a->y || !a->k_cache || !a->v_cache || !a->workspace) return -1;
  if (!a->g1 || !a->b1 || !a->wqkv_t || !a->bqkv || !a->wo_t || !a->bo || !a->g2 || !a->b2 || !a->w1_t || !a->c1 ||
      !a->w2_t || !a->c2)
    return -1;
  if (a->debug != 0 || a->B <= 0 || a->B > 65535 || a->t < 0 || (int64_t)a->t >= a->cs || a->bs < 0) return -1;
  if (a->x_bs < 0 || a->x_cs < 0 || a->y_bs < 0 || a->y_cs < 0 || !(a->eps >= 0.0f)) return -1;
  if (!hsp_plm_decode_supported(a->D, a->H, a->F)) return -1;
  if (a->workspace_bytes < hsp_plm_decode_workspace_bytes(a->B, a->D) || !hsp_aligned16(a->workspace)) return -1;
  if (!hsp_aligned16(a->wqkv_t) || !hsp_aligned16(a->wo_t) || !hsp_aligned16(a->w1_t) || !hsp_aligned16(a->w2_t)) return -1;
  const int64_t lds = attn_lds_bytes(a->D, a->H, a->F, (int64_t)a->t + 1);
  return lds > kLdsMax ? -1 : lds;   // more keys than one compute unit's LDS holds scores for
}

}  // namespace

extern "C" int hsp_plm_decode_layer_f32(const hsp_plm_decode_args* a, void* stream) {
  const int64_t lds = decode_args_lds(a);
  if (lds < 0) return HSP_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = hsp_launch<plm_decode_attn_kernel>((int64_t)a->B * a->H, kThreads, (int)lds, kLdsMax, s, *a)) return e;
  const int lds2 = (2 * a->D + a->F / kP + kPartFloats) * 4;      // at most 28 KB (decode geometry check)
  if (int e = hsp_launch<plm_decode_ffn_kernel>((int64_t)a->B * kP, kThreads, lds2, lds2, s, *a)) return e;
  return hsp_launch<plm_decode_sum_kernel>(a->B, 256, 0, 0, s, *a);
}

extern "C" int hsp_plm_decode_layer_pos_f32(const hsp_plm_decode_args* a, const int32_t* pos, void* stream) {
  const int64_t lds = decode_args_lds(a);
  if (lds < 0 || !pos) return HSP_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = hsp_launch<plm_decode_attn_pos_kernel>((int64_t)a->B * a->H, kThreads, (int)lds, kLdsMax, s, *a, pos))
    return e;
  const int lds2 = (2 * a->D + a->F / kP + kPartFloats) * 4;
  if (int e = hsp_launch<plm_decode_ffn_pos_kernel>((int64_t)a->B * kP, kThreads, lds2, lds2, s, *a, pos)) return e;
  return hsp_launch<plm_decode_sum_pos_kernel>(a->B, 256, 0, 0, s, *a, pos);
}
