// ITU-R BS.1770-4 integrated loudness of ragged mono rows, and the gain that brings a row to a target loudness
// (scale_norm="lufs" of the harnesses).  Declarations and semantics: include/hsp.h.
//
// The K-weighting cascade (two biquads) is a recurrence over up to ~10^6 samples per row with only B rows in parallel,
// so every row is cut into chunks of CHUNK = 800 samples -- a divisor of the 100 ms hop at every supported rate, and
// independent of B and n, so row b of a batch is bit-identical to row b alone -- and run as a chunked scan:
//   (a) kw_chunk_kernel<false>  every chunk filters from a zero state and keeps its 4-value end state z[c];
//   (b) kw_carry_kernel         per row, s[c + 1] = M^800 s[c] + z[c] (M^800: 4 x 4, built on the host in double);
//   (c) kw_chunk_kernel<true>   every chunk filters again from its true start state s[c] and keeps the sum of its
//                               squared outputs and its max |x|;
//   (d) gate_kernel             per row: hop sums -> 400 ms block powers -> absolute and relative gate -> LUFS, peak.
// All sums are taken in a fixed order (no atomics).  The recurrence, the carry and every sum run in fp64: the
// high-pass poles sit at radius ~0.995 (48 kHz), where an fp32 direct form loses the low end of the state first, and
// the scan is bound by the latency of its dependent chain, not by fp64 throughput.
#include "hsp_rows.h"

#include <math.h>

namespace {

constexpr int CHUNK = 800;        // samples per chunk: hop = sample_rate / 10 = CHUNK * (sample_rate / 8000)
constexpr int TILE = 32;          // samples of every chunk staged in LDS at a time (CHUNK % TILE == 0)
constexpr int CPB = 64;           // chunks per workgroup = its threads (one wave)
constexpr int TPAD = TILE + 1;    // LDS row pitch: lane t walks row t, the odd pitch spreads the lanes over the banks
static_assert(CHUNK % TILE == 0 && CPB == 64 && TILE == 32, "kw_chunk_kernel's staging index arithmetic");

// stage 1 (high shelf): b0 b1 b2 / 1 a1 a2; stage 2 (high-pass): 1 -2 1 / 1 c1 c2
struct kw_coef { double b0, b1, b2, a1, a2, c1, c2; };
struct kw_pow { double m[4][4]; };   // M^CHUNK: the state after CHUNK zero-input steps, column j from the unit state e_j

// one sample through both biquads in transposed direct form II; s = (stage 1: s1, s2; stage 2: s1, s2)
__host__ __device__ __forceinline__ double kw_step(const kw_coef& k, double x, double s[4]) {
  const double y1 = fma(k.b0, x, s[0]);
  s[0] = fma(k.b1, x, fma(-k.a1, y1, s[1]));
  s[1] = fma(k.b2, x, -k.a2 * y1);
  const double y2 = y1 + s[2];
  s[2] = fma(-2.0, y1, fma(-k.c1, y2, s[3]));
  s[3] = fma(-k.c2, y2, y1);
  return y2;
}

// Steps (a) and (c).  Workgroup (blockIdx.x, b) = chunks [64 blockIdx.x, +64) of row b, lane t = one chunk.  The 64
// chunks are staged TILE samples at a time: the wave reads 2 chunks x 32 consecutive samples (two full 128-B lines)
// per load instruction into registers while it filters the tile before, then writes them to LDS, where lane t walks
// its own row.  Samples at and after the row's length are never read (they enter as 0 and are not summed).
template <bool FINAL>
__global__ __launch_bounds__(CPB) void kw_chunk_kernel(const float* __restrict__ x, int64_t x_bs,
                                                       const int64_t* __restrict__ lengths, int64_t n, int64_t nc,
                                                       kw_coef k, double* __restrict__ state, double* __restrict__ csum,
                                                       float* __restrict__ cmax) {
  __shared__ float tile[CPB * TPAD];
  const int b = blockIdx.y;
  const int lane = threadIdx.x;
  const int64_t len = hsp_row_len(lengths, b, n);
  const int64_t nch = (len + CHUNK - 1) / CHUNK;
  const int64_t c0 = (int64_t)blockIdx.x * CPB;
  if (c0 >= nch) return;                                     // the whole workgroup lies past the row's end
  const float* xb = x + (int64_t)b * x_bs;
  const int64_t c = c0 + lane;
  const int64_t slot = (int64_t)b * nc + c;
  const int valid = (int)min((int64_t)CHUNK, max((int64_t)0, len - c * CHUNK));   // samples of chunk c inside the row
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (FINAL && c < nch) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = state[slot * 4 + i];
  }
  double acc = 0.0;
  float mx = 0.0f;
  float r[TILE];
  const int64_t g0 = (c0 + (lane >> 5)) * CHUNK + (lane & 31);   // element i of a tile: chunk 2 i + lane / 32, sample lane % 32
#pragma unroll
  for (int i = 0; i < TILE; ++i) {
    const int64_t g = g0 + (int64_t)(2 * i) * CHUNK;
    r[i] = g < len ? xb[g] : 0.0f;
  }
  for (int t = 0; t < CHUNK / TILE; ++t) {
    __syncthreads();                                         // every lane is done with the tile before
#pragma unroll
    for (int i = 0; i < TILE; ++i) tile[(2 * i + (lane >> 5)) * TPAD + (lane & 31)] = r[i];
    __syncthreads();
    if (t + 1 < CHUNK / TILE) {
#pragma unroll
      for (int i = 0; i < TILE; ++i) {
        const int64_t g = g0 + (int64_t)(2 * i) * CHUNK + (t + 1) * TILE;
        r[i] = g < len ? xb[g] : 0.0f;
      }
    }
#pragma unroll 8
    for (int j = 0; j < TILE; ++j) {
      const float xv = tile[lane * TPAD + j];
      const double y = kw_step(k, (double)xv, s);
      if (FINAL && t * TILE + j < valid) {
        acc = fma(y, y, acc);
        mx = fmaxf(mx, fabsf(xv));
      }
    }
  }
  if (c >= nch) return;
  if (FINAL) {
    csum[slot] = acc;
    cmax[slot] = mx;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) state[slot * 4 + i] = s[i];
  }
}

// Step (b), in place: state[b][c] holds z[c] on entry and s[c] (the state chunk c starts from) on exit.  One wave per
// row: the lanes move 64 chunks' states between global memory and LDS, lane 0 walks them.
__global__ __launch_bounds__(64) void kw_carry_kernel(const int64_t* __restrict__ lengths, int64_t n, int64_t nc, kw_pow p,
                                                      double* __restrict__ state) {
  __shared__ double zs[64 * 4];
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t nch = (hsp_row_len(lengths, b, n) + CHUNK - 1) / CHUNK;
  double* st = state + (int64_t)b * nc * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t c0 = 0; c0 < nch; c0 += 64) {
    const int cnt = (int)min((int64_t)64, nch - c0);
    for (int i = lane; i < cnt * 4; i += 64) zs[i] = st[c0 * 4 + i];
    __syncthreads();
    if (lane == 0) {
      for (int i = 0; i < cnt; ++i) {
        double z[4], q[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { z[r] = zs[4 * i + r]; zs[4 * i + r] = s[r]; }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          q[r] = z[r];
#pragma unroll
          for (int j = 0; j < 4; ++j) q[r] = fma(p.m[r][j], s[j], q[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = q[r];
      }
    }
    __syncthreads();
    for (int i = lane; i < cnt * 4; i += 64) st[c0 * 4 + i] = zs[i];
    __syncthreads();
  }
}

// sum over a 256-thread workgroup in a fixed tree order; every thread gets the total
__device__ __forceinline__ double block_sum_256(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// sum of squares of the 400 ms block that starts at hop j: its 4 hop sums, each the sum of its m chunk sums, over 4 hops
__device__ __forceinline__ double block_power(const double* __restrict__ cs, int64_t j, int m, double inv_block) {
  double blk = 0.0;
  for (int h = 0; h < 4; ++h) {
    double hop = 0.0;
    for (int i = 0; i < m; ++i) hop += cs[(j + h) * m + i];
    blk += hop;
  }
  return blk * inv_block;
}

// Step (d): BS.1770-4 gating of one row by one 256-thread workgroup.  Blocks of 4 hops (400 ms, 75 % overlap) that lie
// wholly inside the row; absolute gate at -70 LUFS (block power > abs_thr), relative gate 10 LU below the loudness of
// the absolute-gated blocks (block power > their mean power / 10).  A row shorter than one block is taken whole,
// ungated; a row with no block above the absolute gate reports -inf.
__global__ __launch_bounds__(256) void gate_kernel(const int64_t* __restrict__ lengths, int64_t n, int64_t nc, int m,
                                                   double abs_thr, const double* __restrict__ csum,
                                                   const float* __restrict__ cmax, float* __restrict__ lufs,
                                                   float* __restrict__ peak) {
  __shared__ double red[256];
  __shared__ float redf[256];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t len = hsp_row_len(lengths, b, n);
  const int64_t nch = (len + CHUNK - 1) / CHUNK;
  const double* cs = csum + (int64_t)b * nc;
  const float* cm = cmax + (int64_t)b * nc;

  float mx = 0.0f;
  for (int64_t c = tid; c < nch; c += 256) mx = fmaxf(mx, cm[c]);
  redf[tid] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) redf[tid] = fmaxf(redf[tid], redf[tid + o]);
    __syncthreads();
  }
  if (tid == 0) peak[b] = redf[0];

  const int64_t hop = (int64_t)CHUNK * m;
  const int64_t nh = len / hop;                              // whole hops
  const int64_t nblk = nh >= 4 ? nh - 3 : 0;
  const float ninf = -__builtin_inff();
  if (nblk == 0) {
    if (tid == 0) {
      double tot = 0.0;
      for (int64_t c = 0; c < nch; ++c) tot += cs[c];        // at most 4 m chunks
      lufs[b] = (len > 0 && tot > 0.0) ? (float)(-0.691 + 10.0 * log10(tot / (double)len)) : ninf;
    }
    return;
  }
  const double inv_block = 1.0 / (double)(4 * hop);
  double s1 = 0.0, n1 = 0.0;
  for (int64_t j = tid; j < nblk; j += 256) {
    const double z = block_power(cs, j, m, inv_block);
    if (z > abs_thr) { s1 += z; n1 += 1.0; }
  }
  s1 = block_sum_256(s1, red);
  n1 = block_sum_256(n1, red);
  if (n1 == 0.0) {
    if (tid == 0) lufs[b] = ninf;
    return;
  }
  const double rel_thr = 0.1 * (s1 / n1);                    // -10 LU
  double s2 = 0.0, n2 = 0.0;
  for (int64_t j = tid; j < nblk; j += 256) {
    const double z = block_power(cs, j, m, inv_block);
    if (z > abs_thr && z > rel_thr) { s2 += z; n2 += 1.0; }
  }
  s2 = block_sum_256(s2, red);
  n2 = block_sum_256(n2, red);                               // >= 1: the loudest gated block is above a tenth of the mean
  if (tid == 0) lufs[b] = (float)(-0.691 + 10.0 * log10(s2 / n2));
}

__global__ __launch_bounds__(256) void loudness_gains_kernel(const float* __restrict__ lufs, const float* __restrict__ peak,
                                                             float target, float ceiling, float* __restrict__ gains,
                                                             int32_t* __restrict__ limited, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double l = (double)lufs[b];
  // a row without a loudness (-inf: silence; NaN never leaves the meter) takes the ceiling, the "max" rule
  double g = (double)ceiling;
  int lim = 1;
  if (l > -HUGE_VAL && l < HUGE_VAL) {
    const double want = pow(10.0, ((double)target - l) / 20.0) * (double)peak[b];
    if (want < g) { g = want; lim = 0; }
  }
  gains[b] = (float)g;
  limited[b] = lim;
}

// The analytic design behind the BS.1770-4 table (K = tan(pi fc / fs)); at 48 kHz the standard's own table.
bool kw_design(int32_t fs, kw_coef& k) {
  if (fs < 8000 || fs > 48000 || fs % 8000) return false;
  if (fs == 48000) {
    k = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
         -1.99004745483398, 0.99007225036621};
    return true;
  }
  const double pi = 3.14159265358979323846;
  {
    const double K = tan(pi * 1681.974450955533 / fs), Q = 0.7071752369554196;
    const double Vh = pow(10.0, 3.999843853973347 / 20.0), Vb = pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    k.b0 = (Vh + Vb * K / Q + K * K) / a0;
    k.b1 = 2.0 * (K * K - Vh) / a0;
    k.b2 = (Vh - Vb * K / Q + K * K) / a0;
    k.a1 = 2.0 * (K * K - 1.0) / a0;
    k.a2 = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double K = tan(pi * 38.13547087602444 / fs), Q = 0.5003270373238773;
    const double a0 = 1.0 + K / Q + K * K;
    k.c1 = 2.0 * (K * K - 1.0) / a0;
    k.c2 = (1.0 - K / Q + K * K) / a0;
  }
  return true;
}

int64_t ws_chunks(int64_t n) { return (n + CHUNK - 1) / CHUNK; }
// per chunk: 4 doubles of state, one double of squared outputs, one float of max |x| (the float array last)
int64_t ws_bytes(int32_t B, int64_t n) { return (int64_t)B * ws_chunks(n) * (4 * 8 + 8 + 4); }

}  // namespace

#define HSP_STREAM static_cast<hipStream_t>(stream)

extern "C" int hsp_loudness_coefs_f64(int32_t sample_rate, double* coefs) {
  kw_coef k;
  if (!coefs || !kw_design(sample_rate, k)) return HSP_EINVAL;
  const double out[10] = {k.b0, k.b1, k.b2, k.a1, k.a2, 1.0, -2.0, 1.0, k.c1, k.c2};
  for (int i = 0; i < 10; ++i) coefs[i] = out[i];
  return 0;
}

extern "C" int64_t hsp_loudness_workspace_bytes(int32_t B, int64_t n) {
  if (B <= 0 || B > 65535 || n <= 0 || ws_chunks(n) > (int64_t)CPB * 0x7fffffff) return HSP_EINVAL;
  return ws_bytes(B, n);
}

extern "C" int hsp_loudness_f32(const float* x, int64_t x_bs, const int64_t* lengths, int32_t B, int64_t n,
                                int32_t sample_rate, void* workspace, int64_t workspace_bytes, float* lufs, float* peak,
                                void* stream) {
  kw_coef k;
  if (!x || !workspace || !lufs || !peak || B <= 0 || B > 65535 || n <= 0 || x_bs < n) return HSP_EINVAL;
  if (!kw_design(sample_rate, k)) return HSP_EINVAL;
  const int64_t nc = ws_chunks(n);
  if (nc > (int64_t)CPB * 0x7fffffff || workspace_bytes < ws_bytes(B, n) || ((uintptr_t)workspace & 7)) return HSP_EINVAL;
  kw_pow p;
  for (int j = 0; j < 4; ++j) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    s[j] = 1.0;
    for (int i = 0; i < CHUNK; ++i) kw_step(k, 0.0, s);
    for (int r = 0; r < 4; ++r) p.m[r][j] = s[r];
  }
  double* state = static_cast<double*>(workspace);
  double* csum = state + (int64_t)B * nc * 4;
  float* cmax = reinterpret_cast<float*>(csum + (int64_t)B * nc);
  const int m = sample_rate / 8000;
  const double abs_thr = pow(10.0, (-70.0 + 0.691) / 10.0);
  const dim3 grid((unsigned)((nc + CPB - 1) / CPB), (unsigned)B);
  hipLaunchKernelGGL(kw_chunk_kernel<false>, grid, dim3(CPB), 0, HSP_STREAM, x, x_bs, lengths, n, nc, k, state, csum, cmax);
  hipLaunchKernelGGL(kw_carry_kernel, dim3((unsigned)B), dim3(64), 0, HSP_STREAM, lengths, n, nc, p, state);
  hipLaunchKernelGGL(kw_chunk_kernel<true>, grid, dim3(CPB), 0, HSP_STREAM, x, x_bs, lengths, n, nc, k, state, csum, cmax);
  hipLaunchKernelGGL(gate_kernel, dim3((unsigned)B), dim3(256), 0, HSP_STREAM, lengths, n, nc, m, abs_thr, csum, cmax,
                     lufs, peak);
  return (int)hipGetLastError();
}

extern "C" int hsp_loudness_gains_f32(const float* lufs, const float* peak, float target_lufs, float ceiling, float* gains,
                                      int32_t* limited, int32_t B, void* stream) {
  if (!lufs || !peak || !gains || !limited || B <= 0) return HSP_EINVAL;
  if (!(target_lufs > -HUGE_VALF && target_lufs < HUGE_VALF) || !(ceiling > 0.0f && ceiling < HUGE_VALF)) return HSP_EINVAL;
  hipLaunchKernelGGL(loudness_gains_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, HSP_STREAM, lufs, peak,
                     target_lufs, ceiling, gains, limited, B);
  return (int)hipGetLastError();
}
