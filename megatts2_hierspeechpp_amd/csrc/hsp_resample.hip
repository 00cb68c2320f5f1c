// Band-limited sinc resampling of the prompt ingest (torchaudio 0.13.1 functional.resample, as called by every reference
// harness: inference_plm.py:120-126, inference.py:118-124, inference_vc.py:76-78,98-103, inference_speechsr.py:28-34).
// The filter bank is built on the host (functional.sinc_resample_bank); this file applies it.
//
// y[b, i n + p] = sum_{j < n_taps} bank[p][j] * xz[b, i o + tap0[p] + j - width], xz = x[b] on [0, len_b), zero elsewhere.
//
// One workgroup per (block of F output frames i, row b).  The workgroup stages in LDS
//   - the compacted bank transposed to [n_taps][n] (lanes of a wave run over consecutive phases p of one frame: their
//     bank reads are consecutive words, conflict-free),
//   - tap0[] clamped to [0, K - n_taps] (device data: the clamp keeps every LDS read inside the staged span),
//   - the input span [i0 o - width, (i0 + F - 1) o - width + K) of the block, zero outside [0, len_b).
// Plain fp32 FMAs; not a throughput item (a 10 s 44.1 kHz prompt is ~5 M FMA).
#include "hsp_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int64_t kLdsBudget = 64 * 1024;   // the default dynamic-LDS limit: no hipFuncSetAttribute, capture-safe
constexpr int kMaxOutPerBlock = 2048;       // frames per block: about this many outputs (at least one frame)

__global__ __launch_bounds__(kThreads) void resample_kernel(const float* __restrict__ x, int64_t x_bs,
                                                            const int64_t* __restrict__ lengths, int L,
                                                            const float* __restrict__ bank, const int* __restrict__ tap0,
                                                            int n_taps, int o, int n, int width, int F, int S,
                                                            float* __restrict__ y, int64_t y_bs, int T_out) {
  extern __shared__ float lds[];
  float* sbank = lds;                                   // [n_taps][n]
  int* stap = reinterpret_cast<int*>(lds + (int64_t)n * n_taps);   // [n]
  float* sx = reinterpret_cast<float*>(stap + n);       // [S]
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t len = lengths ? min((int64_t)L, max((int64_t)0, lengths[b])) : (int64_t)L;
  const int64_t Tb = ((int64_t)n * len + o - 1) / o;    // torchaudio's ceil(n len / o) for the row alone
  const int64_t i0 = (int64_t)blockIdx.x * F;
  const int K = 2 * width + o;

  for (int e = tid; e < n * n_taps; e += kThreads) {
    const int p = e / n_taps, j = e - p * n_taps;
    sbank[j * n + p] = bank[e];
  }
  for (int p = tid; p < n; p += kThreads) stap[p] = hsp_clampi(tap0[p], 0, K - n_taps);
  const float* xb = x + (int64_t)b * x_bs;
  const int64_t base = i0 * o - width;
  for (int s = tid; s < S; s += kThreads) {
    const int64_t pos = base + s;
    sx[s] = (pos >= 0 && pos < len) ? xb[pos] : 0.0f;
  }
  __syncthreads();

  float* yb = y + (int64_t)b * y_bs;
  for (int e = tid; e < F * n; e += kThreads) {
    const int fi = e / n, p = e - fi * n;
    const int64_t out = (i0 + fi) * n + p;
    if (out >= T_out) break;                            // e grows with out: the rest of this lane's loop is past T_out
    float acc = 0.0f;
    if (out < Tb) {
      const float* xs = sx + fi * o + stap[p];          // fi o + stap[p] + n_taps - 1 <= (F - 1) o + K - 1 = S - 1
      for (int j = 0; j < n_taps; ++j) acc = fmaf(sbank[j * n + p], xs[j], acc);
    }
    yb[out] = acc;
  }
}

}  // namespace

#define HSP_STREAM static_cast<hipStream_t>(stream)

static int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

extern "C" int hsp_resample_f32(const float* x, int64_t x_bs, const int64_t* lengths, int32_t B, int32_t L,
                                const float* bank, const int32_t* tap0, int32_t n_taps, int32_t o, int32_t n,
                                int32_t width, float* y, int64_t y_bs, int32_t T_out, void* stream) {
  if (!x || !bank || !tap0 || !y || B <= 0 || L <= 0 || o < 1 || n < 1 || width < 0 || n_taps < 1 || T_out < 1)
    return HSP_EINVAL;
  if (B > 65535 || gcd64(o, n) != 1) return HSP_EINVAL;
  const int64_t K = 2 * (int64_t)width + o;
  if (K >= ((int64_t)1 << 31) || n_taps > K) return HSP_EINVAL;
  if (((int64_t)n * L + o - 1) / o > T_out) return HSP_EINVAL;             // T_out >= ceil(n L / o)
  if (x_bs < L || y_bs < T_out) return HSP_EINVAL;
  // LDS: bank + tap0 + the span of F frames; F as large as the budget and kMaxOutPerBlock allow, at least 1
  const int64_t fixed = (int64_t)n * n_taps + n;
  if ((fixed + K) * 4 > kLdsBudget) return HSP_EINVAL;
  int64_t F = (kLdsBudget / 4 - fixed - K) / o + 1;
  F = min(F, max((int64_t)1, (int64_t)kMaxOutPerBlock / n));
  const int64_t frames = ((int64_t)T_out + n - 1) / n;                      // frames holding an output < T_out
  F = min(F, frames);
  const int64_t S = (F - 1) * o + K;
  const int64_t blocks = (frames + F - 1) / F;
  if (blocks >= ((int64_t)1 << 31)) return HSP_EINVAL;
  const size_t lds = (size_t)((fixed + S) * 4);
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(kThreads), lds, HSP_STREAM, x, x_bs,
                     lengths, L, bank, tap0, n_taps, o, n, width, (int)F, (int)S, y, y_bs, T_out);
  return (int)hipGetLastError();
}
