// Causal attention over the first n positions of ONE row of the prosody LM, and that row's K / V into the layer's decode
// caches (include/hsp.h "PLM prefill"): what lets Megatts2PLM1 continue from given codes.  All positions of a prefix are
// known, so every projection of a layer is one GEMM over n columns on the library's token GEMMs; what is left is this
// kernel: the causal softmax over the stacked q | k | v, without a dense [n, n] mask, and the copy of k and v to where
// hsp_plm_decode_layer_f32 reads them.
//
// One workgroup of 256 threads per (tile of kTq = 16 queries, head).  It walks the key blocks of kKb = 64 keys from 0 up
// to the tile's diagonal -- blocks above it are not visited -- with a running maximum and sum per query (scores and
// probabilities live in registers and LDS only).  Per key block:
//   scores   lane = key, wave w = queries 4 w .. 4 w + 3: the Dh-long dot products read k from global memory with the
//            lanes along time (unit stride, as attn_row of hsp_plm_decode.hip) and q from LDS (one 16-byte broadcast);
//            the maximum and the sum of a query's 64 scores are reductions inside its wave;
//   p V      thread = (query, one of 16 channel groups): channels g, g + 16, ... of the head, summed over the block's keys
//            in order from the V block staged in LDS (lanes along time when it is loaded) and the probabilities in LDS
//            (both with rows padded to 65 floats: the 16 queries and the 4 channels of a wave's access fall on
//            different banks).
// Every sum has a fixed order and there are no atomics; column i of the output depends on columns 0 .. i of the head's
// q / k / v only, so neither on n nor on anything outside the row.  At Dh = 69 and n up to a few thousand this is a
// latency item (a 200-position prefix is 13 tiles x 4 heads with at most four key blocks each), so plain HIP C++.
// The workgroup also copies the K / V columns of its own query range for its head into the caches; with out = NULL it
// does only that.
#include <cmath>

#include "hsp_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTq = 16;            // queries per workgroup
constexpr int kKb = 64;            // keys per block = lanes of a wave
constexpr int kPp = kKb + 1;       // pitch of a probability row in LDS
constexpr int kMaxDh = 128;        // head channels: at most kMaxU per p V thread
constexpr int kMaxU = kMaxDh / 16;
constexpr int kLdsMax = (kMaxDh * kTq + kMaxDh * kPp + kTq * kPp + 2 * kTq) * 4;   // 45 760 bytes

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// acc[u] = acc[u] * f + sum over the block's nk keys, in order, of pr[jj] * V[channel og + 16 u][jj] for u < NU.  A channel
// past the head's last is read as the last (and never stored), so the inner loop carries no predicate.
template <int NU>
__device__ __forceinline__ void pv_block(const float* pr, const float* vs, int og, int Dh, int nk, float f, float* acc) {
  const float* vr[NU];
  float sum[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) vr[u] = vs + min(og + 16 * u, Dh - 1) * kPp, sum[u] = 0.0f;
  for (int jj = 0; jj < nk; ++jj) {
    const float p = pr[jj];
#pragma unroll
    for (int u = 0; u < NU; ++u) sum[u] = fmaf(p, vr[u][jj], sum[u]);
  }
#pragma unroll
  for (int u = 0; u < NU; ++u) acc[u] = fmaf(acc[u], f, sum[u]);
}

__global__ __launch_bounds__(kThreads) void plm_prefill_attn_kernel(hsp_plm_prefill_attn_args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int n = a.n, D = a.D, H = a.H, Dh = D / H;
  const int h = blockIdx.x % H, i0 = (blockIdx.x / H) * kTq;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nq = min(kTq, n - i0);                     // valid queries of this tile (>= 1 by the grid)
  const float* qg = a.qkv + (int64_t)(h * Dh) * a.q_rs;
  const float* kg = a.qkv + (int64_t)(D + h * Dh) * a.q_rs;
  const float* vg = a.qkv + (int64_t)(2 * D + h * Dh) * a.q_rs;

  // K / V columns [i0, i0 + nq) of this head into the caches: lanes along time
  {
    float* kc = a.k_cache + (int64_t)(h * Dh) * a.cs;
    float* vc = a.v_cache + (int64_t)(h * Dh) * a.cs;
    for (int e = tid; e < Dh * kTq; e += kThreads) {
      const int d = e / kTq, q = e % kTq;
      if (q < nq) {
        kc[(int64_t)d * a.cs + i0 + q] = kg[(int64_t)d * a.q_rs + i0 + q];
        vc[(int64_t)d * a.cs + i0 + q] = vg[(int64_t)d * a.q_rs + i0 + q];
      }
    }
  }
  if (!a.out) return;                                  // uniform over the grid

  float* qs = lds;                                     // [Dh][kTq]   queries of the tile (0 past n)
  float* vs = qs + Dh * kTq;                           // [Dh][kPp]   V of the key block (0 past the tile's last key)
  float* ps = vs + Dh * kPp;                           // [kTq][kPp]  probabilities of the key block
  float* al = ps + kTq * kPp;                          // [kTq]       exp(old maximum - new maximum)
  float* li = al + kTq;                                // [kTq]       1 / sum
  for (int e = tid; e < Dh * kTq; e += kThreads) {
    const int d = e / kTq, q = e % kTq;
    qs[e] = q < nq ? qg[(int64_t)d * a.q_rs + i0 + q] : 0.0f;
  }

  const float scale = 1.0f / sqrtf((float)Dh);
  float m[4], l[4];                                    // running maximum / sum of queries 4 wave + u (same in every lane)
#pragma unroll
  for (int u = 0; u < 4; ++u) m[u] = -INFINITY, l[u] = 0.0f;
  const int oq = tid & (kTq - 1), og = tid >> 4;       // p V: query, channel group
  float acc[kMaxU];
#pragma unroll
  for (int u = 0; u < kMaxU; ++u) acc[u] = 0.0f;

  const int last = min(i0 + kTq, n) - 1;               // the largest key any query of the tile sees
  for (int j0 = 0; j0 <= last; j0 += kKb) {
    __syncthreads();                                   // qs is written; the previous block's p V has read vs / ps / al
    for (int e = tid; e < Dh * kKb; e += kThreads) {
      const int d = e >> 6, jj = e & 63;
      vs[d * kPp + jj] = j0 + jj <= last ? vg[(int64_t)d * a.q_rs + j0 + jj] : 0.0f;
    }
    // scores of key j0 + lane against queries 4 wave .. 4 wave + 3
    const int j = j0 + lane;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (j <= last) {
      const float* kp = kg + j;
#pragma unroll 4
      for (int d = 0; d < Dh; ++d) {
        const float kv = kp[(int64_t)d * a.q_rs];
        const float4 q4 = *reinterpret_cast<const float4*>(qs + d * kTq + 4 * wave);
        s[0] = fmaf(q4.x, kv, s[0]);
        s[1] = fmaf(q4.y, kv, s[1]);
        s[2] = fmaf(q4.z, kv, s[2]);
        s[3] = fmaf(q4.w, kv, s[3]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = 4 * wave + u;
      // key j is visible to query i0 + q when j <= i0 + q; key 0 is visible to every query, so the maximum is finite
      // from the first block on and exp(-inf - maximum) = 0 is what a hidden key contributes
      const float sv = j <= i0 + q ? s[u] * scale : -INFINITY;
      const float mn = fmaxf(m[u], wave_max(sv));
      const float p = hsp_exp2e(sv - mn);
      const float f = hsp_exp2e(m[u] - mn);
      l[u] = l[u] * f + wave_sum(p);
      m[u] = mn;
      ps[q * kPp + lane] = p;
      if (lane == 0) al[q] = f;
    }
    __syncthreads();
    {
      const float f = al[oq];
      const float* pr = ps + oq * kPp;
      const int nk = min(kKb, last - j0 + 1);
      switch ((Dh + 15) >> 4) {                        // uniform: channels per p V thread
        case 1: pv_block<1>(pr, vs, og, Dh, nk, f, acc); break;
        case 2: pv_block<2>(pr, vs, og, Dh, nk, f, acc); break;
        case 3: pv_block<3>(pr, vs, og, Dh, nk, f, acc); break;
        case 4: pv_block<4>(pr, vs, og, Dh, nk, f, acc); break;
        case 5: pv_block<5>(pr, vs, og, Dh, nk, f, acc); break;
        case 6: pv_block<6>(pr, vs, og, Dh, nk, f, acc); break;
        case 7: pv_block<7>(pr, vs, og, Dh, nk, f, acc); break;
        default: pv_block<8>(pr, vs, og, Dh, nk, f, acc); break;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) li[4 * wave + u] = 1.0f / l[u];
  }
  __syncthreads();
  if (oq < nq) {
    const float inv = li[oq];
    float* ob = a.out + (int64_t)(h * Dh) * a.o_rs + i0 + oq;
#pragma unroll
    for (int u = 0; u < kMaxU; ++u) {
      const int d = og + 16 * u;
      if (d < Dh) ob[(int64_t)d * a.o_rs] = acc[u] * inv;
    }
  }
}

int lds_bytes(int Dh) { return (Dh * kTq + Dh * kPp + kTq * kPp + 2 * kTq) * 4; }

}  // namespace

extern "C" int hsp_plm_prefill_attn_supported(int32_t D, int32_t H) {
  if (D < 1 || H < 1 || D % H) return 0;
  return D / H <= kMaxDh && D <= 8192 ? 1 : 0;
}

extern "C" int hsp_plm_prefill_attn_f32(const hsp_plm_prefill_attn_args* a, void* stream) {
  if (!a || !a->qkv || !a->k_cache || !a->v_cache) return HSP_EINVAL;
  if (a->debug != 0 || a->n < 1 || a->n > HSP_PLM_PREFILL_MAX_N) return HSP_EINVAL;
  if (a->q_rs < 0 || a->o_rs < 0 || a->cs < 0) return HSP_EINVAL;
  if (a->n > a->q_rs || a->n > a->cs || (a->out && a->n > a->o_rs)) return HSP_EINVAL;
  if (!hsp_plm_prefill_attn_supported(a->D, a->H)) return HSP_EINVAL;
  const int64_t tiles = ((int64_t)a->n + kTq - 1) / kTq;
  return hsp_launch<plm_prefill_attn_kernel>(tiles * a->H, kThreads, lds_bytes(a->D / a->H), kLdsMax,
                                             static_cast<hipStream_t>(stream), *a);
}
