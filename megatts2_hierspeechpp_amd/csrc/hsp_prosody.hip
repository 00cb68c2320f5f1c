// Prosody codes of a mel in one launch (include/hsp.h: hsp_prosody_encode_f32; ttv_v1/t2w2v_transformer.py:887-930 of
// the reference): first D mel bins -> PLMConv -> max-pool 8 -> PLMConv -> nearest code, every code held for 8 frames.
// One workgroup = PE_P pooled frames of one row.  Everything between the mel and the codes lives in LDS:
//   pooled frames [j0, j0 + PE_P) need p (the pooled track) on [j0 - 4, j0 + PE_P + 4): two k = 5 convs,
//   i.e. h (the output of the first PLMConv) on 8 (PE_P + 8) mel frames, its first conv on 2 more frames each side and
//   the masked mel on 2 more again.  Column i of every staged array is a fixed frame, stated where the array is declared.
// Frames outside the row (t < 0, t >= length) are ZEROS in every staged array -- the reference's zero padding and its
// `* mask` after every conv are the same thing here -- so no tap is ever skipped and every sum has one fixed order:
// taps k ascending, input channels ascending inside a tap, the bias added last.
#include "hsp_device.h"

namespace {

constexpr int PE_THREADS = 512;
constexpr int PE_P = 4;                       // pooled frames per workgroup (tests read this constant)
constexpr int PE_POOL = 8;                    // MaxPool1d(kernel_size = stride = 8)
constexpr int PE_K = 5;                       // taps of all four convs
constexpr int PE_DMAX = 32;                   // channels
constexpr int PE_NP = PE_P + 8;               // p  : column i = pooled frame j0 - 4 + i
constexpr int PE_NQ1 = PE_P + 4;              // q1 : column i = pooled frame j0 - 2 + i
constexpr int PE_NH2 = PE_POOL * PE_NP;       // h  : column i = mel frame 8 (j0 - 4) + i
constexpr int PE_NH1 = PE_NH2 + 4;            // h1 : column i = mel frame 8 (j0 - 4) - 2 + i
constexpr int PE_NX = PE_NH1 + 4;             // x  : column i = mel frame 8 (j0 - 4) - 4 + i
constexpr int PE_WL = 4096;                   // floats of LDS for the taps of one conv (pe_conv)
static_assert(PE_NH1 <= 128 && PE_NQ1 <= 16, "one lane per column of a conv's output");

// ys[c][i] = lo <= f0 + i < hi ? bias[c] + sum_k sum_ci w[k][ci][c] xs[ci][i + k] : 0   for i < ny, c < D
// (column i of ys is frame f0 + i, column i of xs frame f0 + i - 2).  2^LOGW lanes walk the columns; the threads'
// 512 >> LOGW groups share the output channels.  DT: the channel count at compile time, or 0 for D at run time.
// With DT and at least one whole wave per group (every lane of a wave then wants the same taps) the workgroup first
// copies the taps into LDS (`wl`), coalesced, as [k][ci][group][PERP] with PERP = the group's channels rounded up to 4,
// and the sum reads them from there in 16-byte broadcast reads; otherwise a thread reads its taps from global memory
// where it uses them.  Called by all threads of the workgroup.
template <int LOGW, int DT>
__device__ __forceinline__ void pe_conv(const float* xs, int xld, float* ys, int yld, int ny, int f0, int lo, int hi,
                                        const float* __restrict__ w, const float* __restrict__ bias, int D, int w_ld,
                                        float* wl) {
  constexpr int NG = PE_THREADS >> LOGW;
  constexpr int PER = ((DT ? DT : PE_DMAX) + NG - 1) / NG;       // accumulators of a thread
  constexpr int PERP = (PER + 3) & ~3;
  constexpr bool STAGED = DT > 0 && LOGW >= 6;
  // taps from global memory: unroll everything, so that all loads of a thread are in flight together; from LDS: a few
  // channels at a time (a full unroll has the compiler hoist every read and spill)
  constexpr int UNR_K = STAGED ? 1 : PE_K, UNR_C = STAGED ? 4 : (DT ? DT : 1);
  static_assert(!STAGED || PE_K * DT * NG * PERP <= PE_WL, "taps of one conv in LDS");
  const int i = threadIdx.x & ((1 << LOGW) - 1);
  int g = threadIdx.x >> LOGW;
  if (LOGW >= 6) g = __builtin_amdgcn_readfirstlane(g);
  const int per = (D + NG - 1) / NG, co0 = g * per;
  const int nco = min(per, D - co0);
  if constexpr (STAGED) {
    for (int o = threadIdx.x; o < PE_K * DT * DT; o += PE_THREADS) {
      const int r = o / DT, c = o - r * DT;
      wl[(r * NG + c / PER) * PERP + c % PER] = w[(int64_t)r * w_ld + c];
    }
    __syncthreads();
  }
  if (i >= ny || nco <= 0) return;
  float acc[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) acc[u] = 0.0f;
#pragma unroll UNR_K
  for (int k = 0; k < PE_K; ++k)
#pragma unroll UNR_C
    for (int ci = 0; ci < D; ++ci) {
      const float xv = xs[ci * xld + i + k];
      float wv[PERP];
      if constexpr (STAGED) {
#pragma unroll
        for (int v = 0; v < PERP / 4; ++v) {
          const float4 w4 = reinterpret_cast<const float4*>(wl + ((k * DT + ci) * NG + g) * PERP)[v];
          wv[4 * v] = w4.x; wv[4 * v + 1] = w4.y; wv[4 * v + 2] = w4.z; wv[4 * v + 3] = w4.w;
        }
      } else {
        const float* wr = w + (int64_t)(k * D + ci) * w_ld + co0;
#pragma unroll
        for (int u = 0; u < PER; ++u) wv[u] = u < nco ? wr[u] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < PER; ++u)
        if (u < nco) acc[u] = fmaf(wv[u], xv, acc[u]);
    }
  const bool live = f0 + i >= lo && f0 + i < hi;
#pragma unroll
  for (int u = 0; u < PER; ++u)
    if (u < nco) ys[(co0 + u) * yld + i] = live ? acc[u] + (bias ? bias[co0 + u] : 0.0f) : 0.0f;
}

// larger distance wins, the lower code index on equal distances (torch.max's first maximum)
__device__ __forceinline__ void pe_better(float& best, int& arg, float ob, int oa) {
  if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
}

// DT: the channel count as a compile-time constant (every loop over channels unrolls, so that the codebook loads of a
// thread are all in flight together; pe_conv), or 0 for a.D at run time.  Same statements, same order of every sum.
template <int DT>
__global__ __launch_bounds__(PE_THREADS) void prosody_encode_kernel(const hsp_prosody_args a) {
  __shared__ float bufA[PE_DMAX * PE_NX];     // x, then h
  __shared__ float bufB[PE_DMAX * PE_NH1];    // h1
  __shared__ __attribute__((aligned(16))) float wl[PE_WL];
  __shared__ float ps[PE_DMAX * PE_NP];
  __shared__ float q1[PE_DMAX * PE_NQ1];
  __shared__ float qs[PE_DMAX * PE_P];
  __shared__ float red_d[PE_P][PE_THREADS / 64];
  __shared__ int red_i[PE_P][PE_THREADS / 64];
  __shared__ int code_s[PE_P];
  const int tid = threadIdx.x, b = blockIdx.y, j0 = blockIdx.x * PE_P;
  const int D = DT ? DT : a.D, T = a.T;
  const int n = (int)min((int64_t)T, max((int64_t)0, a.lengths[b]));
  const int Tp = (T + PE_POOL - 1) / PE_POOL, np = (n + PE_POOL - 1) / PE_POOL;
  int64_t* crow = a.codes ? a.codes + (int64_t)b * a.c_bs : nullptr;
  int64_t* prow = a.pooled ? a.pooled + (int64_t)b * a.p_bs : nullptr;
  const int t_out = PE_POOL * j0 + tid;       // threads < 8 PE_P: one mel frame of `codes` each
  if (j0 >= np) {                             // the whole tile is past the row's end: zeros
    if (crow && tid < PE_POOL * PE_P && t_out < T) crow[t_out] = 0;
    if (prow && tid < PE_P && j0 + tid < Tp) prow[j0 + tid] = 0;
    return;
  }
  const int fx = PE_POOL * (j0 - 4) - 4;      // mel frame of x's column 0
  const float* xb = a.x + (int64_t)b * a.x_bs;
  for (int o = tid; o < D * PE_NX; o += PE_THREADS) {
    const int ci = o / PE_NX, i = o - ci * PE_NX, t = fx + i;
    bufA[o] = t >= 0 && t < n ? xb[(int64_t)ci * a.x_cs + t] : 0.0f;
  }
  __syncthreads();
  pe_conv<7, DT>(bufA, PE_NX, bufB, PE_NH1, PE_NH1, fx + 2, 0, n, a.w1a, a.b1a, D, a.w_ld, wl);
  __syncthreads();
  pe_conv<7, DT>(bufB, PE_NH1, bufA, PE_NH2, PE_NH2, fx + 4, 0, n, a.w1b, a.b1b, D, a.w_ld, wl);
  __syncthreads();
  // p = max over each window of 8 columns of h; the frames past the row's end are among them as the zeros they hold
  for (int o = tid; o < D * PE_NP; o += PE_THREADS) {
    const int c = o / PE_NP, i = o - c * PE_NP, j = j0 - 4 + i;
    const float* hp = bufA + c * PE_NH2 + PE_POOL * i;
    float m = hp[0];
#pragma unroll
    for (int r = 1; r < PE_POOL; ++r) m = fmaxf(m, hp[r]);
    ps[o] = j >= 0 && j < np ? m : 0.0f;
  }
  __syncthreads();
  pe_conv<4, DT>(ps, PE_NP, q1, PE_NQ1, PE_NQ1, j0 - 2, 0, np, a.w2a, a.b2a, D, a.w_ld, wl);
  __syncthreads();
  pe_conv<4, DT>(q1, PE_NQ1, qs, PE_P, PE_P, j0, 0, np, a.w2b, a.b2b, D, a.w_ld, wl);
  __syncthreads();
  // nearest code: lanes along the codebook, every thread its codes in ascending order for all PE_P frames
  float xx[PE_P], best[PE_P];
  int arg[PE_P];
#pragma unroll
  for (int f = 0; f < PE_P; ++f) {
    xx[f] = hsp_vq_sq(qs + f, PE_P, D);
    best[f] = -INFINITY;
    arg[f] = INT32_MAX;
  }
  for (int e = tid; e < a.bins; e += PE_THREADS) {
    const float* ep = a.embed + (int64_t)e * D;
    float row[DT ? DT : 1];
    if constexpr (DT > 0 && DT % 4 == 0) {      // the code's row in 16-byte loads (the host checks the alignment)
#pragma unroll
      for (int v = 0; v < DT / 4; ++v) {
        const float4 r4 = reinterpret_cast<const float4*>(ep)[v];
        row[4 * v] = r4.x; row[4 * v + 1] = r4.y; row[4 * v + 2] = r4.z; row[4 * v + 3] = r4.w;
      }
      ep = row;
    }
#pragma unroll
    for (int f = 0; f < PE_P; ++f) {
      const float dist = hsp_vq_dist(qs + f, PE_P, xx[f], ep, D);
      if (dist > best[f]) { best[f] = dist; arg[f] = e; }
    }
  }
#pragma unroll
  for (int f = 0; f < PE_P; ++f) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pe_better(best[f], arg[f], __shfl_xor(best[f], o, 64), __shfl_xor(arg[f], o, 64));
    if ((tid & 63) == 0) { red_d[f][tid >> 6] = best[f]; red_i[f][tid >> 6] = arg[f]; }
  }
  __syncthreads();
  if (tid < PE_P) {
    float bd = red_d[tid][0];
    int bi = red_i[tid][0];
    for (int wv = 1; wv < PE_THREADS / 64; ++wv) pe_better(bd, bi, red_d[tid][wv], red_i[tid][wv]);
    code_s[tid] = bi == INT32_MAX ? 0 : bi;   // no distance above -inf: code 0, as the serial search gives
  }
  __syncthreads();
  if (crow && tid < PE_POOL * PE_P && t_out < T) crow[t_out] = t_out < n ? code_s[tid / PE_POOL] : 0;
  if (prow && tid < PE_P && j0 + tid < Tp) prow[j0 + tid] = j0 + tid < np ? code_s[tid] : 0;
}

}  // namespace

extern "C" int hsp_prosody_encode_f32(const hsp_prosody_args* a, void* stream) {
  if (!a || !a->x || !a->lengths || !a->embed || (!a->codes && !a->pooled)) return HSP_EINVAL;
  if (!a->w1a || !a->w1b || !a->w2a || !a->w2b) return HSP_EINVAL;
  if (a->B <= 0 || a->B > 65535 || a->T <= 0 || a->D <= 0 || a->D > PE_DMAX) return HSP_EINVAL;
  if (a->bins <= 0 || a->bins > 1024 || a->k != PE_K || a->w_ld < a->D) return HSP_EINVAL;
  const int Tp = (a->T + PE_POOL - 1) / PE_POOL;
  const dim3 grid((unsigned)((Tp + PE_P - 1) / PE_P), (unsigned)a->B);
  if (a->D == 20 && (reinterpret_cast<uintptr_t>(a->embed) & 15) == 0) hipLaunchKernelGGL(prosody_encode_kernel<20>, grid, dim3(PE_THREADS), 0, static_cast<hipStream_t>(stream), *a);
  else hipLaunchKernelGGL(prosody_encode_kernel<0>, grid, dim3(PE_THREADS), 0, static_cast<hipStream_t>(stream), *a);
  return (int)hipGetLastError();
}
