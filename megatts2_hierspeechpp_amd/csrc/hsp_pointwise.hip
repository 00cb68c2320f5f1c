// HBM-bound pointwise / reduction kernels of the vocoder path (gfx950).
// Reference call sites are listed next to each entry point in include/hsp.h.
#include "hsp_rows.h"
#include "hsp_act1d_arith.h"
#include "hsp_philox.h"

namespace {

// blocks of 256 threads for the kernels that walk n elements with a grid-stride loop
inline unsigned loop_grid(int64_t n) { return hsp_flat_grid(n, 256, 1048576); }

// ---------------------------------------------------------------- Activation1d
// Stand-alone anti-aliased SnakeBeta (used where no conv follows, and -- measured faster on
// MI355X for wide layers -- in front of a plain conv instead of the fused prologue, because
// VALU work inside the conv kernel is paid in fp32-MFMA time on the same SIMD).
// One workgroup = ACT_TILE outputs of one (b, c) row.  The raw window (aligned float4 loads),
// the 2x-rate snake signal and the result go through LDS, so HBM sees one read and one write
// of the tensor (the eager reference makes ~38 passes).
constexpr int ACT_TILE = 1024;
constexpr int ACT_THREADS = 256;
constexpr int ACT_HALO = 8;  // raw window starts at p0 - 8 (16-B aligned); 5 are needed

__global__ __launch_bounds__(ACT_THREADS) void act1d_kernel(const float* __restrict__ x, float* __restrict__ y, int C,
                                                            int L, const float* __restrict__ alpha_exp,
                                                            const float* __restrict__ beta_inv,
                                                            const float* __restrict__ filt, int n_tiles) {
  __shared__ __attribute__((aligned(16))) float raw[ACT_TILE + 2 * ACT_HALO];
  __shared__ __attribute__((aligned(16))) float a2[2 * ACT_TILE + 16];
  const int tile = blockIdx.x % n_tiles;
  const int row = blockIdx.x / n_tiles;  // b * C + c
  const int c = row % C;
  const int p0 = tile * ACT_TILE;
  const float* xrow = x + (int64_t)row * L;
  float* yrow = y + (int64_t)row * L;
  const float kf = alpha_exp[c] * 0.318309886183790672f, kb = 0.5f * beta_inv[c];
  const int n_out = min(ACT_TILE, L - p0);
  const int tid = threadIdx.x;
  const bool vec = ((L & 3) == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0) &&
                   ((reinterpret_cast<uintptr_t>(y) & 15) == 0);
  // ---- raw[s] = x[clamp(p0 - 8 + s)], s in [0, n_out + 16)
  const int nraw = n_out + 2 * ACT_HALO;
  if (vec && p0 >= ACT_HALO && p0 + n_out + ACT_HALO <= L) {
    for (int v = tid; v < nraw / 4; v += ACT_THREADS)
      *reinterpret_cast<float4*>(raw + 4 * v) = *reinterpret_cast<const float4*>(xrow + p0 - ACT_HALO + 4 * v);
  } else {
    for (int s = tid; s < nraw; s += ACT_THREADS) raw[s] = xrow[hsp_clampi(p0 - ACT_HALO + s, 0, L - 1)];
  }
  __syncthreads();
  // ---- a2[s] = snake(2 * up[clamp(2*p0 - 5 + s)]), s in [0, 2*n_out + 10)
  const int a2w = 2 * n_out + 10;
  const int mlo = 2 * p0 - 5;
  if (mlo >= 0 && mlo + a2w <= 2 * L) {
    // interior: slot 2i+1 <-> m = 2q (q = p0-2+i), slot 2i+2 <-> m = 2q+1; x[q-3 .. q+3] = raw[i+3 .. i+9].
    // Two adjacent pairs per thread share their raw window (8 LDS reads for 4 outputs).
    const int npair = (a2w - 1) >> 1;
    float hu[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) hu[t] = filt[t];
    for (int i = 2 * tid; i < npair; i += 2 * ACT_THREADS) {
      float xv[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) xv[t] = raw[i + 3 + t];
      act_f32x2 u0 = {0.0f, 0.0f}, u1 = {0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        const act_f32x2 hh = {hu[11 - 2 * t], hu[10 - 2 * t]};
        const act_f32x2 x0 = {xv[t], xv[t + 1]};
        const act_f32x2 x1 = {xv[t + 1], xv[t + 2]};
        u0 = __builtin_elementwise_fma(x0, hh, u0);
        u1 = __builtin_elementwise_fma(x1, hh, u1);
      }
      u0 = u0 * 2.0f;
      u1 = u1 * 2.0f;
      a2[2 * i + 1] = hsp_snake_hw(u0.x, kf, kb);
      a2[2 * i + 2] = hsp_snake_hw(u0.y, kf, kb);
      if (i + 1 < npair) {
        a2[2 * i + 3] = hsp_snake_hw(u1.x, kf, kb);
        a2[2 * i + 4] = hsp_snake_hw(u1.y, kf, kb);
      }
    }
    if (tid < 2) {  // slot 0 (odd m, raw[3..8]) and the last slot (even m)
      const float* xr_ = tid ? raw + n_out + 7 : raw + 3;
      float uu = 0.0f;
#pragma unroll
      for (int t = 0; t < 6; ++t) uu = fmaf(xr_[t], tid ? filt[11 - 2 * t] : filt[10 - 2 * t], uu);
      a2[tid ? a2w - 1 : 0] = hsp_snake_hw(2.0f * uu, kf, kb);
    }
  } else {
    for (int s = tid; s < a2w; s += ACT_THREADS) {
      const int m = hsp_clampi(mlo + s, 0, 2 * L - 1);
      const int q = m >> 1, odd = m & 1;
      const float* xr_ = raw + (q - 3 + odd) - (p0 - ACT_HALO);
      float u = 0.0f;
#pragma unroll
      for (int t = 0; t < 6; ++t) u = fmaf(xr_[t], odd ? filt[10 - 2 * t] : filt[11 - 2 * t], u);
      a2[s] = hsp_snake_hw(2.0f * u, kf, kb);
    }
  }
  __syncthreads();
  // ---- y[p0 + s] = sum_k hd[k] * a2[2s + k]
  float hd[12];
#pragma unroll
  for (int t = 0; t < 12; ++t) hd[t] = filt[12 + t];
  if (vec && (n_out & 3) == 0) {
    // four consecutive outputs per thread: their 12-tap windows overlap in 18 a2 values
    for (int v = tid; v < n_out / 4; v += ACT_THREADS) {
      const act_f32x2* ar = reinterpret_cast<const act_f32x2*>(a2 + 8 * v);
      act_f32x2 w[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) w[k] = ar[k];
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        act_f32x2 acc = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const act_f32x2 hh = {hd[2 * k], hd[2 * k + 1]};
          acc = __builtin_elementwise_fma(w[q + k], hh, acc);
        }
        o[q] = acc.x + acc.y;
      }
      *reinterpret_cast<float4*>(yrow + p0 + 4 * v) = make_float4(o[0], o[1], o[2], o[3]);
    }
  } else {
    for (int s = tid; s < n_out; s += ACT_THREADS) {
      const act_f32x2* ar = reinterpret_cast<const act_f32x2*>(a2 + 2 * s);
      act_f32x2 acc = {0.0f, 0.0f};
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const act_f32x2 hh = {hd[2 * k], hd[2 * k + 1]};
        acc = __builtin_elementwise_fma(ar[k], hh, acc);
      }
      yrow[p0 + s] = acc.x + acc.y;
    }
  }
}

// Wave-per-segment form for 16-B addressable rows with L % 4 == 0 (every layer of the vocoder).
// One WAVE owns ACT2_SEG outputs of one (b, c) row and its own LDS slice: no workgroup barrier,
// a wave's LDS instructions retire in order, so phases are separated by compiler fences only.
// Every LDS access is contiguous across lanes (b64 / b128, lane stride = access width), so there
// are no bank conflicts -- the workgroup-tile kernel above reads with lane strides of 2, 4 and 8
// floats and is LDS-conflict bound at 1.7 TB/s.
//   raw[j]  = x[clamp(p0 - 8 + j)]                       j in [0, 512)
//   a2[j]   = a[clamp(2 p0 - 5 + j, 0, 2L - 1)]          j in [0, 1024): slot 4l of lane l is the
//             first tap of outputs (p0 + 2l, p0 + 2l + 1) -> three b128 + one b64 read per pair.
//   phase B: lane pair pi owns a[2q+1 .. 2q+4], q = p0 - 3 + 2 pi (odd(q), even(q+1), odd(q+1),
//            even(q+2)): one b128 write at slot 4 pi; its inputs x[q-2 .. q+4] sit in four aligned
//            b64 reads.  The x2 gain is folded into the taps (exact).
constexpr int ACT2_SEG = 496;   // raw window = SEG + 16 = 512 floats = two float4 per lane
constexpr int ACT2_WAVES = 4;
constexpr int ACT2_ITEMS = 4;   // consecutive segments per wave (software-pipelined loads)
constexpr int ACT2_RAW = 512;
constexpr int ACT2_A2 = 1040;

__device__ __forceinline__ void act2_compiler_fence() { asm volatile("" ::: "memory"); }

// one work item = one segment [p0, p0 + n_out) of one (b, c) row; p0 - 8 and L are multiples of 4, so a
// float4 of the raw window lies wholly inside the row or wholly outside it
struct Act2Item {
  int p0, n_out, c;
  int64_t row_off;
};

__device__ __forceinline__ Act2Item act2_item(unsigned w, int nseg, int C, int L) {
  const unsigned row = w / (unsigned)nseg;  // b * C + c
  const int seg = (int)(w - row * (unsigned)nseg);
  Act2Item it;
  it.p0 = seg * ACT2_SEG;
  it.n_out = min(ACT2_SEG, L - it.p0);  // multiple of 4
  it.c = (int)(row % (unsigned)C);
  it.row_off = (int64_t)row * L;
  return it;
}

// Two unconditional float4 loads per lane (clamped address, so always legal and branch-free: a
// load inside a divergent block gets an s_waitcnt vmcnt(0) right behind it and the round trips
// serialise); the replicate padding is applied when the registers are written to LDS.
__device__ __forceinline__ void act2_load(const float* __restrict__ x, const Act2Item& it, int L, int lane,
                                          float4 (&rv)[2]) {
  const float* xrow = x + it.row_off;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int idx = it.p0 - 8 + 4 * (lane + 64 * k);
    rv[k] = *reinterpret_cast<const float4*>(xrow + hsp_clampi(idx, 0, L - 4));
  }
}

// the valid length of the row of work item w: len[b] clamped to [1, L] (ragged form)
__device__ __forceinline__ int act2_row_len(const int64_t* __restrict__ lens, unsigned w, int nseg, int C, int L) {
  const unsigned b = (w / (unsigned)nseg) / (unsigned)C;
  return (int)hsp_clamp_len(lens[b], L, 1);   // never NULL here (the launcher refuses): no test for it in the hot kernel
}

// RAG (hsp_act1d_snakebeta_ragged_f32): row b is valid over [0, lens[b]).  Reads clamp at lens[b] - 1 -- the replicate
// pad of the call on the row cut to that length -- and the outputs at t >= lens[b] are written as 0.  RAG = false is the
// plain kernel (`lens` unread).
template <bool RAG>
__global__ __launch_bounds__(64 * ACT2_WAVES) void act1d_seg_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                    int C, int L, const float* __restrict__ alpha_exp,
                                                                    const float* __restrict__ beta_inv,
                                                                    const float* __restrict__ filt, int nseg,
                                                                    unsigned nwork, const int64_t* __restrict__ lens) {
  __shared__ __attribute__((aligned(16))) float raw_all[ACT2_WAVES][ACT2_RAW];
  __shared__ __attribute__((aligned(16))) float a2_all[ACT2_WAVES][ACT2_A2];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const unsigned w0 = (blockIdx.x * ACT2_WAVES + wave) * ACT2_ITEMS;
  if (w0 >= nwork) return;  // wave-uniform; the kernel has no workgroup barrier
  const unsigned w1 = min(w0 + ACT2_ITEMS, nwork);
  float* raw = raw_all[wave];
  float* a2 = a2_all[wave];
  act_f32x2 hu[6], hd[6];
  HSP_ACT2_TAPS(filt, hu, hd)   // (hsp_act1d_arith.h)

  // A wave walks ACT2_ITEMS consecutive segments; the raw window of the next one is in flight
  // (registers) while the current one is computed, so HBM latency is off the critical path.
  // The outputs of an item stay in registers and are stored one iteration later, BEFORE the next
  // prefetch is issued: vmcnt retires in order, so the wait for a prefetch would otherwise also wait
  // for the stores issued just before it (a full write round trip per item).
  Act2Item cur = act2_item(w0, nseg, C, L);
  float4 rv[2];
  act2_load(x, cur, L, lane, rv);
  int lb = L;         // (RAG) valid length of the current item's row and its last valid sample
  float rl = 0.0f;
  if constexpr (RAG) {
    lb = act2_row_len(lens, w0, nseg, C, L);
    rl = x[cur.row_off + lb - 1];
  }
  constexpr int NC = (ACT2_SEG / 2 + 63) / 64;  // phase-C iterations of a full segment
  float2 yo[NC];
  float* yprev = nullptr;
  int nprev = 0;
  auto flush = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NC; ++it) {
      const int l2 = lane + 64 * it;
      // non-temporal: the write stream does not displace the read stream's lines in L2 on its way out
      // (round 3, same box: 4.8-5.0 -> 5.5-5.8 TB/s at the vocoder's shapes, step 81.5 -> 81.15 ms)
      if (2 * l2 < nprev) __builtin_nontemporal_store(act_f32x2{yo[it].x, yo[it].y}, reinterpret_cast<act_f32x2*>(yprev + 2 * l2));
    }
  };
  for (unsigned w = w0; w < w1; ++w) {
    const int p0 = cur.p0, n_out = cur.n_out;
    const int lbc = lb;
    const float rlc = rl;
    const int n_in = RAG ? max(0, min(n_out, lbc - p0)) : n_out;   // outputs inside the valid part of the row
    float* yrow = y + cur.row_off;
    const float kf = alpha_exp[cur.c] * 0.318309886183790672f, kb = 0.5f * beta_inv[cur.c];
    // ---- phase A: registers -> LDS, then start the next item's loads
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int v = lane + 64 * k;
      const int idx = p0 - 8 + 4 * v;
      float4 t = rv[k];
      t = idx < 0 ? make_float4(t.x, t.x, t.x, t.x) : t;    // clamped address was 0:     x[0]
      t = idx >= L ? make_float4(t.w, t.w, t.w, t.w) : t;   // clamped address was L - 4: x[L-1]
      if constexpr (RAG) {                                  // replicate x[lb - 1] from the row's valid end on
        t.x = idx >= lbc ? rlc : t.x;
        t.y = idx + 1 >= lbc ? rlc : t.y;
        t.z = idx + 2 >= lbc ? rlc : t.z;
        t.w = idx + 3 >= lbc ? rlc : t.w;
      }
      *reinterpret_cast<float4*>(raw + 4 * v) = t;
    }
    act2_compiler_fence();  // keeps the deferred stores behind the wait for rv (the scheduler hoists them into the latch otherwise)
    if (yprev) flush();     // previous item's outputs: ahead of the prefetch in vmcnt order
    if (w + 1 < w1) {
      cur = act2_item(w + 1, nseg, C, L);
      act2_load(x, cur, L, lane, rv);
      if constexpr (RAG) {
        lb = act2_row_len(lens, w + 1, nseg, C, L);
        rl = x[cur.row_off + lb - 1];
      }
    }
    act2_compiler_fence();

    // ---- phase B
    const int npairs = (2 * n_out + 13) >> 2;  // slots [0, 2 n_out + 10)
#pragma unroll 2
    for (int pi = lane; pi < npairs; pi += 64) {
      HSP_ACT2_UP(a2, raw, pi, hu, kf, kb)   // (hsp_act1d_arith.h)
    }
    act2_compiler_fence();
    // replicate padding of the 2x-rate signal: a[-5 .. -1] = a[0], a[2L .. 2L+4] = a[2L-1]
    if constexpr (RAG) {
      // a[2 lb - 1] sits at slot e; every slot after it that an output of this item reads (up to 2 n_out + 9) takes its
      // value -- in the item that holds the row's end AND in the one before it when the end lies within its taps' reach
      const int e = 2 * (lbc - p0) + 4;
      const bool tail = e >= 0 && e < 2 * n_out + 9;
      if (p0 == 0 || tail) {
        if (p0 == 0 && lane < 5) a2[lane] = a2[5];
        if (tail && lane >= 8 && lane < 13) a2[e + lane - 7] = a2[e];
        act2_compiler_fence();
      }
    } else if (p0 == 0 || p0 + n_out == L) {
      if (p0 == 0 && lane < 5) a2[lane] = a2[5];
      if (p0 + n_out == L && lane >= 8 && lane < 13) a2[2 * n_out + lane - 3] = a2[2 * n_out + 4];
      act2_compiler_fence();
    }

    // ---- phase C: y[p0 + s] = sum_k hd[k] * a2[2 s + k], two outputs per lane
#pragma unroll
    for (int it = 0; it < NC; ++it) {
      const int l2 = lane + 64 * it;
      if (2 * l2 >= n_out) continue;
      HSP_ACT2_DOWN(yo[it], a2, l2, hd)   // (hsp_act1d_arith.h)
      if constexpr (RAG) {
        yo[it].x = 2 * l2 < n_in ? yo[it].x : 0.0f;
        yo[it].y = 2 * l2 + 1 < n_in ? yo[it].y : 0.0f;
      }
    }
    yprev = yrow + p0;
    nprev = n_out;
    act2_compiler_fence();  // raw / a2 are rewritten by the next item
  }
  flush();
}

__global__ void snake_consts_kernel(const float* al, const float* bl, float* ea, float* binv, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < C) {
    ea[i] = expf(al[i]);
    binv[i] = 1.0f / (expf(bl[i]) + 1e-9f);
  }
}

// ---------------------------------------------------------------- weight prep
// one wave per row: ||v_r||_2 by a butterfly reduction, then scale
__global__ __launch_bounds__(256) void fold_weight_norm_kernel(const float* __restrict__ v, const float* __restrict__ g,
                                                               float* __restrict__ w, int rows, int cols) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* vr = v + (int64_t)row * cols;
  float ss = 0.0f;
  for (int i = lane; i < cols; i += 64) ss = fmaf(vr[i], vr[i], ss);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float sc = g[row] / sqrtf(ss);
  float* wr = w + (int64_t)row * cols;
  for (int i = lane; i < cols; i += 64) wr[i] = vr[i] * sc;
}

__global__ void gather_kernel(const float* __restrict__ src, const int32_t* __restrict__ map, float* __restrict__ dst,
                              int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t m = map[i];
    dst[i] = m >= 0 ? src[m] : 0.0f;
  }
}

// ---------------------------------------------------------------- small ops
__global__ void sequence_mask_kernel(const int64_t* length, float* mask, int B, int T) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * T) mask[i] = (i % T) < length[i / T] ? 1.0f : 0.0f;
}

__global__ void flip_channels_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C, int T) {
  const int64_t n = (int64_t)B * C * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i % T);
    const int64_t r = i / T;
    const int c = (int)(r % C);
    const int64_t b = r / C;
    y[i] = x[(b * C + (C - 1 - c)) * T + t];
  }
}

// THE prior sample of one element: (m + n exp(logs) noise_scale) mask, for a given and for a drawn n alike
__device__ __forceinline__ float prior_value(float m, float logs, float n, float noise_scale, float mk) {
  return (m + n * expf(logs) * noise_scale) * mk;
}

__global__ void sample_prior_kernel(const float* __restrict__ stats, const float* __restrict__ noise,
                                    const float* __restrict__ mask, float* __restrict__ z, int B, int C, int T,
                                    float noise_scale) {
  const int64_t n = (int64_t)B * C * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i % T);
    const int64_t r = i / T;
    const int c = (int)(r % C);
    const int64_t b = r / C;
    const float m = stats[(b * 2 * C + c) * T + t];
    const float logs = stats[(b * 2 * C + C + c) * T + t];
    z[i] = prior_value(m, logs, noise[i], noise_scale, mask[b * T + t]);
  }
}

// Seeded prior noise (hsp.h): one thread owns the group of four frames 4 g .. 4 g + 3 of one (b, c) -- one Philox call,
// two Box-Muller pairs (hsp_normal4).  VEC: every row is 16-B addressable (T % 4 == 0 and 16-B aligned bases, so
// every group is whole), and a group moves as one float4; else scalar accesses, cut at the row's end.
template <bool VEC>
__device__ __forceinline__ void group_load(const float* __restrict__ p, int left, float v[4]) {
  if (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < left ? p[k] : 0.0f;
  }
}
template <bool VEC>
__device__ __forceinline__ void group_store(float* __restrict__ p, int left, const float v[4]) {
  if (VEC) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < left) p[k] = v[k];
  }
}

// FUSED: z = prior_value of the drawn noise (hsp_sample_prior_seeded_f32; `out` is z); else out = the noise itself
// (hsp_randn_rows_f32; stats and mask unread).  G = groups per row; `seeds` is read here, when the kernel runs.
template <bool FUSED, bool VEC>
__global__ __launch_bounds__(256) void randn_rows_kernel(const int64_t* __restrict__ seeds,
                                                         const float* __restrict__ stats,
                                                         const float* __restrict__ mask, float* __restrict__ out, int B,
                                                         int C, int T, int G, float noise_scale) {
  const int64_t n = (int64_t)B * C * G;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % G);
    const int64_t r = i / G;
    const int c = (int)(r % C);
    const int64_t b = r / C;
    const int t = 4 * g, left = T - t;   // left >= 1: the frames of this group inside the row
    float v[4];
    hsp_normal4(seeds[b], (unsigned)c, (unsigned)g, v);
    if (FUSED) {
      float m[4], logs[4], mk[4];
      group_load<VEC>(stats + (b * 2 * C + c) * T + t, left, m);
      group_load<VEC>(stats + (b * 2 * C + C + c) * T + t, left, logs);
      group_load<VEC>(mask + b * T + t, left, mk);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = prior_value(m[k], logs[k], v[k], noise_scale, mk[k]);
    }
    group_store<VEC>(out + (b * C + c) * T + t, left, v);
  }
}

__global__ void mask_mul_kernel(const float* __restrict__ x, const float* __restrict__ mask, float* __restrict__ y,
                                int B, int C, int T) {
  const int64_t n = (int64_t)B * C * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i % T);
    const int64_t b = i / ((int64_t)C * T);
    y[i] = x[i] * mask[b * T + t];
  }
}

// F.interpolate(mode='linear', align_corners=False) along T.  torch's CPU kernel evaluates the
// source index in fp32 with ONE rounding, src = fmaf(scale, i + 0.5, -0.5), clamped at 0; a
// separate mul + sub is off by 2e-3 at L = 64000 because ulp(src) ~ 4e-3 there.
// RAG (hsp_linear_interp_ragged_f32): row b holds lin[b] valid inputs and lout[b] valid outputs (rows = B * C, b = r / C).
// Same source position as the call on the row alone (the caller keeps Lin / Lout equal to that call's ratio), the
// neighbours clamped at the row's last valid input, zeros past its last valid output.  RAG = false is the plain kernel
// (`lin`, `lout` and C unread).
template <bool RAG>
__global__ void linear_interp_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t rows, int C, int Lin,
                                     int Lout, float scale, const int64_t* __restrict__ lin,
                                     const int64_t* __restrict__ lout) {
  const int64_t n = rows * Lout;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i % Lout);
    const int64_t r = i / Lout;
    int lb_in = Lin;
    if constexpr (RAG) {
      lb_in = (int)hsp_row_len(lin, r / C, Lin, 1);
      if (t >= (int)hsp_row_len(lout, r / C, Lout)) {
        y[i] = 0.0f;
        continue;
      }
    }
    float src = fmaf(scale, (float)t + 0.5f, -0.5f);
    src = src < 0.0f ? 0.0f : src;
    const int i0 = RAG ? min((int)src, lb_in - 1) : (int)src;
    const int i1 = i0 + (i0 < lb_in - 1 ? 1 : 0);
    const float l1 = src - (float)i0, l0 = 1.0f - l1;
    const float* xr = x + r * Lin;
    y[i] = l0 * xr[i0] + l1 * xr[i1];
  }
}

__global__ void act_kernel(const float* x, float* y, int64_t n, int act) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = hsp_apply_act(x[i], act);
}

// y[b][t] = x[b][reflect(t - pad)] over [0, len_b + 2 pad), zero on [len_b + 2 pad, Lo); NULL lengths: len_b = L (the
// plain form, Lo = L + 2 pad: no zeros).  One thread per output sample of a row; blockIdx.y strides the rows.
__global__ __launch_bounds__(256) void reflect_pad_kernel(const float* __restrict__ x, int64_t x_bs,
                                                          const int64_t* __restrict__ lengths, float* __restrict__ y,
                                                          int64_t y_bs, int B, int L, int pad, int Lo) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Lo) return;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int n = (int)hsp_row_len(lengths, b, L);
    float v = 0.0f;
    if (n > 0 && t < n + 2 * pad) v = x[(int64_t)b * x_bs + hsp_reflect(t - pad, n)];
    y[(int64_t)b * y_bs + t] = v;
  }
}

// one workgroup per call: hsp_f0_convert_row (hsp_device.h), which each row of hsp_f0_convert_batch_f32 runs too
__global__ __launch_bounds__(256) void f0_convert_kernel(const float* src, int ns, const float* trg, int nt, float* out) {
  hsp_f0_convert_row(src, ns, trg, nt, out, ns);
}

__global__ void axpby_kernel(const float* x, const float* z, float* y, float a, float b, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = a * x[i] + b * z[i];
}

// What both LayerNorm kernels do with a loaded value v of channel c, batch b: normalise, the per-channel affine, the
// column's mask factor mk, then the (b, c) modulation.
__device__ __forceinline__ float ln_finish(float v, float mean, float rstd, int c, int b, float mk,
                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                           const float* __restrict__ shift, const float* __restrict__ scale,
                                           int64_t mod_bs) {
  v = (v - mean) * rstd;
  if (gamma) v = v * gamma[c] + beta[c];
  v *= mk;
  if (scale) v = v * (1.0f + scale[(int64_t)b * mod_bs + c]) + shift[(int64_t)b * mod_bs + c];
  return v;
}

// LayerNorm over channels of a (B, C, T) tensor.  Block = 64 time steps x 4 channel
// groups; lanes run along T (coalesced), the 4 waves split C and combine through LDS.
// Two passes (mean, then centred variance) like torch's CPU kernel.
__global__ __launch_bounds__(256) void layernorm_mod_kernel(const float* __restrict__ x, float* __restrict__ y, int C,
                                                            int T, float eps, const float* __restrict__ mask,
                                                            const float* __restrict__ shift,
                                                            const float* __restrict__ scale, int64_t mod_bs,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int n_tt) {
  __shared__ float red[4][64];
  const int tt = blockIdx.x % n_tt, b = blockIdx.x / n_tt;
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int t = tt * 64 + lane;
  const bool live = t < T;
  const float* xb = x + (int64_t)b * C * T;
  float* yb = y + (int64_t)b * C * T;
  float s = 0.0f;
  if (live)
    for (int c = grp; c < C; c += 4) s += xb[(int64_t)c * T + t];
  red[grp][lane] = s;
  __syncthreads();
  const float mean = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)C;
  __syncthreads();
  float ss = 0.0f;
  if (live)
    for (int c = grp; c < C; c += 4) {
      const float d = xb[(int64_t)c * T + t] - mean;
      ss = fmaf(d, d, ss);
    }
  red[grp][lane] = ss;
  __syncthreads();
  const float var = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)C;
  const float rstd = 1.0f / sqrtf(var + eps);
  if (!live) return;
  const float mk = mask ? mask[(int64_t)b * T + t] : 1.0f;
  for (int c = grp; c < C; c += 4)
    yb[(int64_t)c * T + t] = ln_finish(xb[(int64_t)c * T + t], mean, rstd, c, b, mk, gamma, beta, shift, scale, mod_bs);
}

// Register-resident variant for C <= 16 * LN_R = 512: a workgroup owns 16 time columns, its 256 threads
// are 16 columns x 16 channel groups and every thread keeps its <= LN_R channel values in
// registers, so the tile is read once with all loads in flight (the loop kernel above chases
// C/4 dependent loads three times: ~40 us for C = 276 whatever T is).  Short sequences still
// give B * T/16 workgroups.
constexpr int LN_R = 32;
__global__ __launch_bounds__(256) void layernorm_reg_kernel(const float* __restrict__ x, float* __restrict__ y, int C,
                                                            int T, float eps, const float* __restrict__ mask,
                                                            const float* __restrict__ shift,
                                                            const float* __restrict__ scale, int64_t mod_bs,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int n_tt) {
  __shared__ float red[16][17];
  const int tt = blockIdx.x % n_tt, b = blockIdx.x / n_tt;
  const int lt = threadIdx.x & 15, cg = threadIdx.x >> 4;
  const int t = tt * 16 + lt;
  const bool live = t < T;
  const float* xb = x + (int64_t)b * C * T + t;
  float* yb = y + (int64_t)b * C * T + t;
  float v[LN_R];
#pragma unroll
  for (int r = 0; r < LN_R; ++r) {
    const int c = cg + 16 * r;
    v[r] = (live && c < C) ? xb[(int64_t)c * T] : 0.0f;
  }
  float s = 0.0f;
#pragma unroll
  for (int r = 0; r < LN_R; ++r) s += v[r];
  red[cg][lt] = s;
  __syncthreads();
  float tot = 0.0f;
#pragma unroll
  for (int g = 0; g < 16; ++g) tot += red[g][lt];
  const float mean = tot / (float)C;
  __syncthreads();
  float ss = 0.0f;
#pragma unroll
  for (int r = 0; r < LN_R; ++r) {
    const float d = (cg + 16 * r < C) ? v[r] - mean : 0.0f;
    ss = fmaf(d, d, ss);
  }
  red[cg][lt] = ss;
  __syncthreads();
  tot = 0.0f;
#pragma unroll
  for (int g = 0; g < 16; ++g) tot += red[g][lt];
  const float rstd = 1.0f / sqrtf(tot / (float)C + eps);
  if (!live) return;
  const float mk = mask ? mask[(int64_t)b * T + t] : 1.0f;
#pragma unroll
  for (int r = 0; r < LN_R; ++r) {
    const int c = cg + 16 * r;
    if (c >= C) break;
    yb[(int64_t)c * T] = ln_finish(v[r], mean, rstd, c, b, mk, gamma, beta, shift, scale, mod_bs);
  }
}

// out[b, c] = sum_t x[b, c, t] / sum_t mask[b, t]; one wave per (b, c)
__global__ __launch_bounds__(256) void masked_mean_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                          float* __restrict__ out, int B, int C, int T) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B * C) return;
  const int b = row / C;
  float s = 0.0f, m = 0.0f;
  for (int t = lane; t < T; t += 64) {
    s += x[(int64_t)row * T + t];
    m += mask[(int64_t)b * T + t];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    m += __shfl_xor(m, o, 64);
  }
  if (lane == 0) out[row] = s / m;
}

}  // namespace

#define HSP_STREAM static_cast<hipStream_t>(stream)

extern "C" int hsp_version(void) { return HSP_VERSION; }
extern "C" const char* hsp_arch(void) { return "gfx950"; }

// the wave-per-segment form on 16-B addressable rows with L % 4 == 0 (the callers have checked both)
template <bool RAG>
static int act1d_seg_launch(const float* x, float* y, int B, int C, int L, const int64_t* lens, const float* alpha_exp,
                            const float* beta_inv, const float* filt, hipStream_t s) {
  const int nseg = (L + ACT2_SEG - 1) / ACT2_SEG;
  const int64_t nwork = (int64_t)nseg * B * C;
  const int64_t blocks = (nwork + ACT2_WAVES * ACT2_ITEMS - 1) / (ACT2_WAVES * ACT2_ITEMS);
  if (nwork > 0x7fffffff - ACT2_WAVES * ACT2_ITEMS) return HSP_EINVAL;
  hipLaunchKernelGGL(act1d_seg_kernel<RAG>, dim3((unsigned)blocks), dim3(64 * ACT2_WAVES), 0, s, x, y, C, L, alpha_exp,
                     beta_inv, filt, nseg, (unsigned)nwork, lens);
  return (int)hipGetLastError();
}

static bool act1d_seg_rows(const float* x, const float* y, int L) {
  return (L & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
}

extern "C" int hsp_act1d_snakebeta_f32(const float* x, float* y, int32_t B, int32_t C, int32_t L,
                                       const float* alpha_exp, const float* beta_inv, const float* filt, void* stream) {
  if (!x || !y || !alpha_exp || !beta_inv || !filt || B <= 0 || C <= 0 || L <= 0) return HSP_EINVAL;
  if (act1d_seg_rows(x, y, L)) return act1d_seg_launch<false>(x, y, B, C, L, nullptr, alpha_exp, beta_inv, filt, HSP_STREAM);
  const int n_tiles = (L + ACT_TILE - 1) / ACT_TILE;
  const int64_t blocks = (int64_t)n_tiles * B * C;
  if (blocks > 0x7fffffff) return HSP_EINVAL;
  hipLaunchKernelGGL(act1d_kernel, dim3((unsigned)blocks), dim3(ACT_THREADS), 0, HSP_STREAM, x, y, C, L, alpha_exp,
                     beta_inv, filt, n_tiles);
  return (int)hipGetLastError();
}

extern "C" int hsp_act1d_snakebeta_ragged_f32(const float* x, float* y, int32_t B, int32_t C, int32_t L, const int64_t* lens,
                                              const float* alpha_exp, const float* beta_inv, const float* filt,
                                              void* stream) {
  if (!x || !y || !lens || !alpha_exp || !beta_inv || !filt || B <= 0 || C <= 0 || L <= 0) return HSP_EINVAL;
  // the wave-per-segment form only (the caller pads the batch to such a length)
  if (!act1d_seg_rows(x, y, L)) return HSP_EINVAL;
  return act1d_seg_launch<true>(x, y, B, C, L, lens, alpha_exp, beta_inv, filt, HSP_STREAM);
}

extern "C" int hsp_snake_consts_f32(const float* al, const float* bl, float* ea, float* binv, int32_t C, void* stream) {
  if (!al || !bl || !ea || !binv || C <= 0) return HSP_EINVAL;
  hipLaunchKernelGGL(snake_consts_kernel, dim3((C + 255) / 256), dim3(256), 0, HSP_STREAM, al, bl, ea, binv, C);
  return (int)hipGetLastError();
}

extern "C" int hsp_fold_weight_norm_f32(const float* v, const float* g, float* w, int32_t rows, int32_t cols,
                                        void* stream) {
  if (!v || !g || !w || rows <= 0 || cols <= 0) return HSP_EINVAL;
  hipLaunchKernelGGL(fold_weight_norm_kernel, dim3((rows + 3) / 4), dim3(256), 0, HSP_STREAM, v, g, w, rows, cols);
  return (int)hipGetLastError();
}

extern "C" int hsp_gather_f32(const float* src, const int32_t* map, float* dst, int64_t n, void* stream) {
  if (!src || !map || !dst || n <= 0) return HSP_EINVAL;
  hipLaunchKernelGGL(gather_kernel, dim3(loop_grid(n)), dim3(256), 0, HSP_STREAM, src, map, dst, n);
  return (int)hipGetLastError();
}

extern "C" int hsp_sequence_mask_f32(const int64_t* length, float* mask, int32_t B, int32_t T, void* stream) {
  if (!length || !mask || B <= 0 || T <= 0) return HSP_EINVAL;
  hipLaunchKernelGGL(sequence_mask_kernel, dim3((B * T + 255) / 256), dim3(256), 0, HSP_STREAM, length, mask, B, T);
  return (int)hipGetLastError();
}

extern "C" int hsp_flip_channels_f32(const float* x, float* y, int32_t B, int32_t C, int32_t T, void* stream) {
  if (!x || !y || x == y || B <= 0 || C <= 0 || T <= 0) return HSP_EINVAL;
  hipLaunchKernelGGL(flip_channels_kernel, dim3(loop_grid((int64_t)B * C * T)), dim3(256), 0, HSP_STREAM, x, y, B,
                     C, T);
  return (int)hipGetLastError();
}

extern "C" int hsp_sample_prior_f32(const float* stats, const float* noise, const float* mask, float* z, int32_t B,
                                    int32_t C, int32_t T, float noise_scale, void* stream) {
  if (!stats || !noise || !mask || !z || B <= 0 || C <= 0 || T <= 0) return HSP_EINVAL;
  hipLaunchKernelGGL(sample_prior_kernel, dim3(loop_grid((int64_t)B * C * T)), dim3(256), 0, HSP_STREAM, stats,
                     noise, mask, z, B, C, T, noise_scale);
  return (int)hipGetLastError();
}

// both seeded launches: one thread per group of four frames, on the grid of every grid-stride kernel of this file
template <bool FUSED>
static int randn_rows_launch(const int64_t* seeds, const float* stats, const float* mask, float* out, int B, int C, int T,
                             float noise_scale, hipStream_t s) {
  const int G = T / 4 + ((T & 3) != 0);
  const bool vec = (T & 3) == 0 && hsp_aligned16(out) && (!FUSED || (hsp_aligned16(stats) && hsp_aligned16(mask)));
  const auto kernel = vec ? randn_rows_kernel<FUSED, true> : randn_rows_kernel<FUSED, false>;
  hipLaunchKernelGGL(kernel, dim3(loop_grid((int64_t)B * C * G)), dim3(256), 0, s, seeds, stats, mask, out, B, C, T, G,
                     noise_scale);
  return (int)hipGetLastError();
}

extern "C" int hsp_randn_rows_f32(const int64_t* seeds, float* out, int32_t B, int32_t C, int32_t T, void* stream) {
  if (!seeds || !out || B <= 0 || C <= 0 || T <= 0) return HSP_EINVAL;
  return randn_rows_launch<false>(seeds, nullptr, nullptr, out, B, C, T, 0.0f, HSP_STREAM);
}

extern "C" int hsp_sample_prior_seeded_f32(const float* stats, const int64_t* seeds, const float* mask, float* z,
                                           int32_t B, int32_t C, int32_t T, float noise_scale, void* stream) {
  if (!stats || !seeds || !mask || !z || B <= 0 || C <= 0 || T <= 0) return HSP_EINVAL;
  return randn_rows_launch<true>(seeds, stats, mask, z, B, C, T, noise_scale, HSP_STREAM);
}

extern "C" int hsp_mask_mul_f32(const float* x, const float* mask, float* y, int32_t B, int32_t C, int32_t T,
                                void* stream) {
  if (!x || !mask || !y || B <= 0 || C <= 0 || T <= 0) return HSP_EINVAL;
  hipLaunchKernelGGL(mask_mul_kernel, dim3(loop_grid((int64_t)B * C * T)), dim3(256), 0, HSP_STREAM, x, mask, y, B,
                     C, T);
  return (int)hipGetLastError();
}

template <bool RAG>
static int linear_interp_launch(const float* x, float* y, int B, int C, int Lin, int Lout, const int64_t* lin,
                                const int64_t* lout, hipStream_t s) {
  const float scale = (float)Lin / (float)Lout;  // torch: area_pixel_compute_scale, align_corners=False
  hipLaunchKernelGGL(linear_interp_kernel<RAG>, dim3(loop_grid((int64_t)B * C * Lout)), dim3(256), 0,
                     s, x, y, (int64_t)B * C, C, Lin, Lout, scale, lin, lout);
  return (int)hipGetLastError();
}

extern "C" int hsp_linear_interp_f32(const float* x, float* y, int32_t B, int32_t C, int32_t Lin, int32_t Lout,
                                    void* stream) {
  if (!x || !y || B <= 0 || C <= 0 || Lin <= 0 || Lout <= 0) return HSP_EINVAL;
  return linear_interp_launch<false>(x, y, B, C, Lin, Lout, nullptr, nullptr, HSP_STREAM);
}

extern "C" int hsp_linear_interp_ragged_f32(const float* x, float* y, int32_t B, int32_t C, int32_t Lin, int32_t Lout,
                                           const int64_t* lin, const int64_t* lout, void* stream) {
  if (!x || !y || !lin || !lout || B <= 0 || C <= 0 || Lin <= 0 || Lout <= 0) return HSP_EINVAL;
  return linear_interp_launch<true>(x, y, B, C, Lin, Lout, lin, lout, HSP_STREAM);
}

extern "C" int hsp_act_f32(const float* x, float* y, int64_t n, int32_t act, void* stream) {
  if (!x || !y || n <= 0 || act < 0 || act > HSP_ACT_GELU_ERF) return HSP_EINVAL;
  hipLaunchKernelGGL(act_kernel, dim3(loop_grid(n)), dim3(256), 0, HSP_STREAM, x, y, n, act);
  return (int)hipGetLastError();
}

constexpr int PAD_MAX_ROWS = 65535;   // grid y; the kernel strides the rows beyond it

extern "C" int hsp_reflect_pad_f32(const float* x, int64_t x_bs, float* y, int32_t B, int32_t L, int32_t pad, void* stream) {
  if (!x || !y || B <= 0 || L <= 0 || pad < 0 || pad >= L) return HSP_EINVAL;
  const int Lo = L + 2 * pad;
  hipLaunchKernelGGL(reflect_pad_kernel, dim3(((int64_t)Lo + 255) / 256, B < PAD_MAX_ROWS ? B : PAD_MAX_ROWS), dim3(256), 0,
                     HSP_STREAM, x, x_bs, nullptr, y, (int64_t)Lo, B, L, pad, Lo);
  return (int)hipGetLastError();
}

extern "C" int hsp_reflect_pad_ragged_f32(const float* x, int64_t x_bs, const int64_t* lengths, float* y, int64_t y_bs,
                                          int32_t B, int32_t L, int32_t pad, int32_t Lo, void* stream) {
  if (!x || !y || B <= 0 || L <= 0 || pad < 0 || pad >= L || Lo <= 0) return HSP_EINVAL;
  if (x_bs < L || y_bs < Lo || (int64_t)Lo > (int64_t)L + 2 * pad || B > PAD_MAX_ROWS) return HSP_EINVAL;
  hipLaunchKernelGGL(reflect_pad_kernel, dim3((Lo + 255) / 256, B), dim3(256), 0, HSP_STREAM, x, x_bs, lengths, y, y_bs, B,
                     L, pad, Lo);
  return (int)hipGetLastError();
}

extern "C" int hsp_f0_convert_f32(const float* f0_src, int32_t n_src, const float* f0_trg, int32_t n_trg, float* out,
                                  void* stream) {
  if (!f0_src || !f0_trg || !out || n_src <= 0 || n_trg <= 0) return HSP_EINVAL;
  hipLaunchKernelGGL(f0_convert_kernel, dim3(1), dim3(256), 0, HSP_STREAM, f0_src, n_src, f0_trg, n_trg, out);
  return (int)hipGetLastError();
}

extern "C" int hsp_axpby_f32(const float* x, const float* z, float* y, float a, float b, int64_t n, void* stream) {
  if (!x || !z || !y || n <= 0) return HSP_EINVAL;
  hipLaunchKernelGGL(axpby_kernel, dim3(loop_grid(n)), dim3(256), 0, HSP_STREAM, x, z, y, a, b, n);
  return (int)hipGetLastError();
}

extern "C" int hsp_layernorm_mod_f32(const float* x, float* y, int32_t B, int32_t C, int32_t T, float eps,
                                     const float* mask, const float* shift, const float* scale, int64_t mod_bs,
                                     const float* gamma, const float* beta, void* stream) {
  if (!x || !y || B <= 0 || C <= 0 || T <= 0) return HSP_EINVAL;
  if ((shift == nullptr) != (scale == nullptr) || (gamma == nullptr) != (beta == nullptr)) return HSP_EINVAL;
  if (C <= 16 * LN_R) {
    const int n_t16 = (T + 15) / 16;
    hipLaunchKernelGGL(layernorm_reg_kernel, dim3((unsigned)(n_t16 * B)), dim3(256), 0, HSP_STREAM, x, y, C, T, eps,
                       mask, shift, scale, mod_bs, gamma, beta, n_t16);
    return (int)hipGetLastError();
  }
  const int n_tt = (T + 63) / 64;
  hipLaunchKernelGGL(layernorm_mod_kernel, dim3((unsigned)(n_tt * B)), dim3(256), 0, HSP_STREAM, x, y, C, T, eps, mask,
                     shift, scale, mod_bs, gamma, beta, n_tt);
  return (int)hipGetLastError();
}

extern "C" int hsp_masked_mean_f32(const float* x, const float* mask, float* out, int32_t B, int32_t C, int32_t T,
                                   void* stream) {
  if (!x || !mask || !out || B <= 0 || C <= 0 || T <= 0) return HSP_EINVAL;
  hipLaunchKernelGGL(masked_mean_kernel, dim3((B * C + 3) / 4), dim3(256), 0, HSP_STREAM, x, mask, out, B, C, T);
  return (int)hipGetLastError();
}
