// Kernels specific to the Mega-TTS2 prosody language model loop (SURVEY.md row A18,
// ttv_v1/t2w2v_transformer.py:702-718): the per-step input assembly and the greedy argmax
// that feeds the next step.  Both read/write the code buffer in device memory so that the
// whole T-step loop is a chain of launches without a host round trip (hipGraph-capturable).
// The per-row-position forms at the end (hsp_plm_embed_pos_f32, hsp_plm_choose_advance_f32) also keep each row's position
// in device memory, so that one captured step serves rows of every length.
#include <cmath>

#include "hsp_device.h"
#include "hsp_philox.h"   // philox4x32_10: the stream of the sampled decision

namespace {

// The read-only operands every embed kernel shares (hsp.h "Mega-TTS2 PLM loop").  pe_t is the sinusoid table transposed
// to [D][P] so that lanes (running along j) read it coalesced.  A kernel does NOT take this struct: its parameters are
// the pointers themselves, each `const ... __restrict__` (PLM_EMBED_PARAMS), because that is where the compiler honours
// the qualifier on a pointer.  The kernel builds the struct from its parameters (PLM_EMBED_OPS), which costs nothing
// once the helpers below are inlined; the speed of the fused kernels was measured in this form.
struct EmbedOps {
  const float* tc;
  int64_t tc_bs, tc_cs;
  int Dtc;
  const int64_t* codes;
  int64_t codes_bs;
  const float* emb;
  int Demb, n_emb;
  const float* pe_t;
  int P;
  const float* alpha;
};
// `codes_q`: const in the kernels that only read the codes
#define PLM_EMBED_PARAMS(codes_q)                                                                                   \
  const float *__restrict__ tc, int64_t tc_bs, int64_t tc_cs, int Dtc, codes_q int64_t *__restrict__ codes,         \
      int64_t codes_bs, const float *__restrict__ emb, int Demb, int n_emb, const float *__restrict__ pe_t, int P,  \
      const float *__restrict__ alpha
#define PLM_EMBED_OPS EmbedOps{tc, tc_bs, tc_cs, Dtc, codes, codes_bs, emb, Demb, n_emb, pe_t, P, alpha}
#define PLM_EMBED_ARGS(o) o.tc, o.tc_bs, o.tc_cs, o.Dtc, o.codes, o.codes_bs, o.emb, o.Demb, o.n_emb, o.pe_t, o.P, o.alpha

// x[b, c, j] = (c < Dtc ? tc[b, c, j] : emb[codes[b, j], c - Dtc]) + alpha * pe_t[c, j]
// (torch.cat([tc_latent[:, :t+1], pc_embedding(p_code)], -1) then SinePositionalEmbedding.forward,
//  t2w2v_transformer.py:711-713,510-514; x_scale = 1).  A fused kernel holds the code of its newest column in a
// register before its store is visible: column `newest_j` embeds `newest` instead of codes[b, newest_j] (-1: no such
// column, every code comes from memory).
__device__ __forceinline__ float embed_value(const EmbedOps& o, float al, int b, int c, int j, int newest_j = -1,
                                             int64_t newest = 0) {
  float v;
  if (c < o.Dtc) {
    v = o.tc[b * o.tc_bs + c * o.tc_cs + j];
  } else {
    int64_t id = j == newest_j ? newest : o.codes[b * o.codes_bs + j];
    id = id < 0 ? 0 : (id >= o.n_emb ? o.n_emb - 1 : id);  // a corrupted code must not fault the GPU
    v = o.emb[id * o.Demb + (c - o.Dtc)];
  }
  return fmaf(al, o.pe_t[(int64_t)c * o.P + j], v);
}

// side-by-side layout (x_bs == n) with the row padded to x_cs > B*n columns: zero the padding.  The calling threads
// share the work: each passes its index `first` among them and their number `stride` (unsigned, as gridDim.x * 256 is).
__device__ __forceinline__ void embed_zero_padding(float* __restrict__ x, int64_t x_bs, int64_t x_cs, int D, int B, int n,
                                                   int first, unsigned stride) {
  if (x_bs != n || x_cs <= (int64_t)B * n) return;
  const int padc = (int)(x_cs - (int64_t)B * n);
  for (int e = first; e < D * padc; e += stride) x[(int64_t)(e / padc) * x_cs + (int64_t)B * n + e % padc] = 0.0f;
}

// embed_value for every (b, c, j < n), grid-stride
__global__ __launch_bounds__(256) void plm_embed_kernel(PLM_EMBED_PARAMS(const), float* __restrict__ x, int64_t x_bs,
                                                        int64_t x_cs, int B, int n) {
  const EmbedOps o = PLM_EMBED_OPS;
  const int D = o.Dtc + o.Demb;
  const int64_t total = (int64_t)B * D * n;
  const float al = o.alpha[0];
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int j = (int)(e % n);
    const int64_t bc = e / n;
    const int c = (int)(bc % D), b = (int)(bc / D);
    x[b * x_bs + c * x_cs + j] = embed_value(o, al, b, c, j);
  }
  embed_zero_padding(x, x_bs, x_cs, D, B, n, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// The maximum of the 256 threads' (value, index) pairs: the larger value wins, the LOWER index on equal values, and an
// index of 0x7fffffff (a thread that saw nothing comparable) becomes 0.  A wave64 butterfly, then the four waves' pairs
// through smax / sidx on thread 0: the result is valid on thread 0 only.  Has a barrier.
__device__ __forceinline__ int block_argmax(float best, int bi, float* smax, int* sidx) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) best = ov, bi = oi;
  }
  if (lane == 0) smax[wave] = best, sidx[wave] = bi;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < 4; ++w)
      if (smax[w] > best || (smax[w] == best && sidx[w] < bi)) best = smax[w], bi = sidx[w];
  return bi == 0x7fffffff ? 0 : bi;
}

// argmax_c row[c * l_cs] over c < N by one 256-thread workgroup: ties -> lowest index (torch.argmax on CPU returns the
// first maximal element), 0 when nothing compares (all NaN).  The result is valid on thread 0 only.  Has a barrier.
__device__ __forceinline__ int argmax_row(const float* __restrict__ row, int64_t l_cs, int N, float* smax, int* sidx) {
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = threadIdx.x; c < N; c += 256) {
    const float v = row[(int64_t)c * l_cs];
    if (v > best || (v == best && c < bi)) best = v, bi = c;
  }
  return block_argmax(best, bi, smax, sidx);
}

// out[b * out_bs] = argmax_c logits[b * l_bs + c * l_cs] (argmax_row).  One workgroup per row.
__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ logits, int64_t l_bs, int64_t l_cs, int N,
                                                     int64_t* __restrict__ out, int64_t out_bs) {
  __shared__ float smax[4];
  __shared__ int sidx[4];
  const int b = blockIdx.x;
  const int bi = argmax_row(logits + (int64_t)b * l_bs, l_cs, N, smax, sidx);
  if (threadIdx.x == 0) out[(int64_t)b * out_bs] = bi;
}

// y[b, c, t] (contiguous) = x[b * s_bs + c * s_cs + t * s_ts]
__global__ __launch_bounds__(256) void copy_strided_kernel(const float* __restrict__ x, int64_t s_bs, int64_t s_cs,
                                                           int64_t s_ts, float* __restrict__ y, int B, int C, int T) {
  const int64_t total = (int64_t)B * C * T;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int t = (int)(e % T);
    const int64_t bc = e / T;
    y[e] = x[(bc / C) * s_bs + (bc % C) * s_cs + t * s_ts];
  }
}

// ------------------------------------------------------------------------------------------- sampled decoding
// The decision of hsp.h "sampled PLM decoding" for one row, by one 256-thread workgroup.  Thread t holds the logits
// 4t .. 4t+3 (so its four Philox words are exactly one call at counter t).  No sort: the top-k pivot and the top-p
// boundary are exact radix selects (four 8-bit digit passes) over the order-preserving uint32 key of each float.  The
// top-p mass is carried as 2^-40 fixed point in 64-bit integers, so every sum is exact, order-free and deterministic
// (the fused and the standalone launch agree bit for bit, and re-choosing a column is idempotent).
constexpr int kSampleMaxN = 1024;

struct SampleSmem {
  unsigned long long hist[256];
  unsigned long long wtot[4];
  unsigned long long sel_above;
  unsigned sel_bin;
  int sel_found;
  unsigned bits[kSampleMaxN / 32];
  float redf[4];
  int redi[4];
  int token;
};

__device__ __forceinline__ unsigned order_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// inclusive scan of v over the 256 threads in thread order; every thread gets its own prefix, *total the sum
__device__ __forceinline__ unsigned long long block_scan_u64(unsigned long long v, SampleSmem& s,
                                                            unsigned long long* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  if (lane == 63) s.wtot[wave] = v;
  __syncthreads();
  unsigned long long before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const unsigned long long t = s.wtot[w];
    before += w < wave ? t : 0ull;
    all += t;
  }
  __syncthreads();   // wtot is reused by the next scan
  *total = all;
  return v + before;
}

__device__ __forceinline__ float block_max(float v, SampleSmem& s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) s.redf[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(s.redf[0], s.redf[1]), fmaxf(s.redf[2], s.redf[3]));
  __syncthreads();
  return v;
}

// the same sum on every thread (the butterfly is symmetric, the four waves are added in a fixed order)
__device__ __forceinline__ float block_sum(float v, SampleSmem& s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s.redf[threadIdx.x >> 6] = v;
  __syncthreads();
  v = ((s.redf[0] + s.redf[1]) + s.redf[2]) + s.redf[3];
  __syncthreads();
  return v;
}

// Radix descent: the key v* of the first element, in DESCENDING key order, at which the running sum of the weights w
// exceeds `target`, and the weight of all elements with a key above v*.  Elements with live[r] == false take no part.
// Returns false (nothing crosses) when the total weight is <= target.
__device__ bool radix_descend(const unsigned key[4], const unsigned long long w[4], const bool live[4],
                              unsigned long long target, SampleSmem& s, unsigned* vstar, unsigned long long* above_out) {
  const int tid = threadIdx.x;
  unsigned prefix = 0, mask = 0;
  unsigned long long above = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    s.hist[tid] = 0;
    if (tid == 0) s.sel_found = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (live[r] && (key[r] & mask) == prefix) atomicAdd(&s.hist[(key[r] >> shift) & 255u], w[r]);
    __syncthreads();
    const unsigned bin = 255u - (unsigned)tid;   // thread order = descending digit
    const unsigned long long h = s.hist[bin];
    unsigned long long total;
    const unsigned long long incl = block_scan_u64(h, s, &total);
    const unsigned long long excl = incl - h;
    if (above + excl <= target && above + incl > target) {
      s.sel_bin = bin;
      s.sel_above = above + excl;
      s.sel_found = 1;
    }
    __syncthreads();
    const int found = s.sel_found;
    const unsigned sel_bin = s.sel_bin;
    const unsigned long long sel_above = s.sel_above;
    __syncthreads();   // every wave holds the selection before the next pass (or the next descent) clears it
    if (!found) return false;                    // only possible in the first pass (uniform)
    prefix |= sel_bin << shift;
    mask |= 255u << shift;
    above = sel_above;
  }
  *vstar = prefix;
  *above_out = above;
  return true;
}

// The whole decision for one row; every thread returns the token.  `prev` = the row's n_prev previous codes.
__device__ int sample_decide(const float* __restrict__ row, int64_t l_cs, int N, const int64_t* prev, int n_prev,
                             int j, const hsp_sample_args& a, float* probs, SampleSmem& s) {
  const int tid = threadIdx.x;
  const float rp = a.repetition_penalty;
  const bool penalise = rp != 1.0f;
  if (penalise) {
    if (tid < kSampleMaxN / 32) s.bits[tid] = 0u;
    __syncthreads();
    for (int k = tid; k < n_prev; k += 256) {
      const int64_t c = prev[k];
      if (c >= 0 && c < N) atomicOr(&s.bits[c >> 5], 1u << (c & 31));   // the go token (>= N) is no candidate
    }
    __syncthreads();
  }
  // 1. penalty
  float l[4];
  bool valid[4];
  unsigned key[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = 4 * tid + r;
    valid[r] = i < N;
    float v = valid[r] ? row[(int64_t)i * l_cs] : -INFINITY;
    if (penalise && valid[r] && ((s.bits[i >> 5] >> (i & 31)) & 1u)) v = v < 0.0f ? v * rp : v / rp;
    l[r] = v + 0.0f;                                   // -0 -> +0: equal floats get equal keys
    key[r] = order_key(l[r]);
  }
  // 2. top-p on the penalised logits
  if (a.top_p < 1.0f) {
    const float m = block_max(fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3])), s);
    unsigned long long w[4], mine = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      w[r] = valid[r] ? (unsigned long long)(expf(l[r] - m) * 1099511627776.0f) : 0ull;   // 2^40 fixed point
      mine += w[r];
    }
    unsigned long long S;
    block_scan_u64(mine, s, &S);
    const unsigned long long thresh = (unsigned long long)((double)a.top_p * (double)S);
    unsigned vstar;
    unsigned long long above;
    if (radix_descend(key, w, valid, thresh, s, &vstar, &above)) {
      // ties at v* are kept in index order while their running mass stays <= thresh; the first token always stays
      const bool at_max = vstar == order_key(m);
      int nt = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) nt += valid[r] && key[r] == vstar;
      unsigned long long dummy;
      unsigned long long rank = block_scan_u64((unsigned long long)nt, s, &dummy) - (unsigned long long)nt;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!valid[r]) continue;
        bool keep = key[r] > vstar;
        if (key[r] == vstar) {
          keep = above + (rank + 1) * w[r] <= thresh || (at_max && rank == 0);
          ++rank;
        }
        if (!keep) l[r] = -INFINITY;
      }
    }
  }
  // 3. temperature
  const float temp = fmaxf(a.temperature, 1e-5f);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    l[r] = l[r] / temp;
    key[r] = order_key(l[r]);
  }
  // 4. top-k: pivot = the k-th largest tempered logit (the removed ones count, as -inf); keep everything >= pivot
  if (a.top_k > 0 && a.top_k < N) {
    const unsigned long long one[4] = {1ull, 1ull, 1ull, 1ull};
    unsigned pivot;
    unsigned long long above;
    if (radix_descend(key, one, valid, (unsigned long long)(a.top_k - 1), s, &pivot, &above)) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (key[r] < pivot) l[r] = -INFINITY;
    }
  }
  // 5. softmax (for probs) and the exponential race in log form
  const float mt = block_max(fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3])), s);
  const int64_t seed = a.seeds[blockIdx.x];
  unsigned c[4] = {(unsigned)tid, (unsigned)j, 0u, 0u};
  philox4x32_10(c, (unsigned)(uint64_t)seed, (unsigned)((uint64_t)seed >> 32));
  float best = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (!valid[r] || l[r] == -INFINITY) continue;
    // u = (2 (w >> 8) + 1) 2^-25 needs 25 bits: exact in double only (in float32 the top word rounds to u = 1, q = 0)
    const double u = (double)(2u * (c[r] >> 8) + 1u) * 0x1p-25;
    const float score = (l[r] - mt) - (float)log(-log(u));
    if (score > best) best = score, bi = 4 * tid + r;   // ascending i within the thread: first wins ties
  }
  const int winner = block_argmax(best, bi, s.redf, s.redi);
  if (tid == 0) s.token = winner;
  __syncthreads();
  const int token = s.token;
  if (probs) {
    float e[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) e[r] = valid[r] ? expf(l[r] - mt) : 0.0f;
    const float sum = block_sum((e[0] + e[1]) + (e[2] + e[3]), s);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (valid[r]) probs[(int64_t)blockIdx.x * a.probs_bs + 4 * tid + r] = e[r] / sum;
  }
  return token;
}

// hsp_sample_f32: one workgroup per row
__global__ __launch_bounds__(256) void sample_kernel(const float* __restrict__ logits, int64_t l_bs, int64_t l_cs, int N,
                                                     int64_t* __restrict__ out, int64_t out_bs, int j,
                                                     hsp_sample_args a) {
  __shared__ SampleSmem s;
  const int b = blockIdx.x;
  int64_t* slot = out + (int64_t)b * out_bs;
  const int tok = sample_decide(logits + (int64_t)b * l_bs, l_cs, N, slot - (j - 1), j - 1, j, a, a.probs, s);
  if (threadIdx.x == 0) *slot = tok;
}

// ------------------------------------------------------------------------------------- the fused embedding launch
// How a fused launch takes its newest code.  A choice brings the LDS it needs (`Smem`: the greedy one stays at 36 bytes)
// and is called by the whole workgroup, barriers inside, with the row's logits and the slot codes[b, n - 1] the code
// goes to; every thread gets the code back.
struct GreedyChoice {   // codes[b, n - 1] = argmax_c logits[b * l_bs + c * l_cs] (ties -> lowest index, as argmax_kernel)
  struct Smem {
    float smax[4];
    int sidx[4];
    int code;
  };
  __device__ int operator()(const float* __restrict__ row, int64_t l_cs, int N, const int64_t*, Smem& s) const {
    const int bi = argmax_row(row, l_cs, N, s.smax, s.sidx);
    if (threadIdx.x == 0) s.code = bi;
    __syncthreads();
    return s.code;
  }
};

// the sampled decision for column j; the row's previous codes are the j - 1 entries before the slot.  a.probs is
// ignored here (the fused launch writes no distribution): sample_decide gets a null probs and never reads a.probs_bs
struct SampledChoice {
  using Smem = SampleSmem;
  int j;
  hsp_sample_args a;
  __device__ int operator()(const float* __restrict__ row, int64_t l_cs, int N, const int64_t* slot, Smem& s) const {
    return sample_decide(row, l_cs, N, slot - (j - 1), j - 1, j, a, nullptr, s);
  }
};

// plm_embed_kernel with the choice of the PREVIOUS step folded in (one launch per step less): workgroup (b, 0) first
// takes codes[b, n - 1] = choose(logits of row b), stores it and then writes the code-embedding rows of utterance b;
// the workgroups (b, 1 ...) write the tc_latent rows, which do not depend on any code.
// Grid (B, 1 + ceil(Dtc * n / 1024)).  hsp_plm_embed_step_f32 is the GreedyChoice instantiation,
// hsp_plm_embed_sample_f32 the SampledChoice one (same grid, same writes).
template <class Choice>
__global__ __launch_bounds__(256) void plm_embed_choose_kernel(PLM_EMBED_PARAMS(), float* __restrict__ x,
                                                               int64_t x_bs, int64_t x_cs, int B, int n,
                                                               const float* __restrict__ logits, int64_t l_bs,
                                                               int64_t l_cs, int n_logits, Choice choose) {
  __shared__ typename Choice::Smem s;
  const EmbedOps o = PLM_EMBED_OPS;
  const int b = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
  const float al = o.alpha[0];
  if (part == 0) {
    int64_t* slot = codes + (int64_t)b * o.codes_bs + n - 1;
    const int newest = choose(logits + (int64_t)b * l_bs, l_cs, n_logits, slot, s);
    if (tid == 0) *slot = newest;
    for (int e = tid; e < o.Demb * n; e += 256) {
      const int j = e % n, c = o.Dtc + e / n;
      __builtin_assume(c >= o.Dtc);   // e >= 0: code channels only, so embed_value's tc branch folds away here
      x[b * x_bs + (int64_t)c * x_cs + j] = embed_value(o, al, b, c, j, n - 1, newest);
    }
    if (b == 0) embed_zero_padding(x, x_bs, x_cs, o.Dtc + o.Demb, B, n, tid, 256);
  } else {
    const int total = o.Dtc * n;
    for (int e = (part - 1) * 1024 + tid; e < min(total, part * 1024); e += 256) {
      const int j = e % n, c = e / n;
      __builtin_assume(c < o.Dtc);    // e < Dtc * n: tc channels only; without the hint the loop keeps a branch per
                                      // element and is not unrolled, which measured 0.5 - 1 us per launch at B = 1
      x[b * x_bs + (int64_t)c * x_cs + j] = embed_value(o, al, b, c, j);
    }
  }
}

// ------------------------------------------------------------------------------------- per-row positions (hsp.h)
// hsp_plm_embed_pos_f32: workgroup b embeds position pos[b] of row b -- embed_value for one column of un-shifted
// operands.  An idle row (pos[b] outside [0, max_pos]) returns before it touches memory.
__global__ __launch_bounds__(256) void plm_embed_pos_kernel(PLM_EMBED_PARAMS(const), float* __restrict__ x, int64_t x_bs,
                                                            int64_t x_cs, const int32_t* __restrict__ pos, int max_pos) {
  const EmbedOps o = PLM_EMBED_OPS;
  const int b = blockIdx.x, t = pos[b];
  if (t < 0 || t > max_pos) return;
  const float al = o.alpha[0];
  for (int c = threadIdx.x; c < o.Dtc + o.Demb; c += 256) x[b * x_bs + c * x_cs] = embed_value(o, al, b, c, t);
}

// hsp_plm_choose_advance_f32: workgroup b takes codes[b, t + 1] for t = pos[b] -- argmax_row, or sample_decide for
// column j = t + 1 with the row's codes 1 .. t -- and then moves pos[b] on, to -1 at the row's length.  Every thread
// reads pos[b] before the barriers of the decision, thread 0 writes it after them.  Idle rows return at once.
__global__ __launch_bounds__(256) void plm_choose_advance_kernel(const float* __restrict__ logits, int64_t l_bs,
                                                                 int64_t l_cs, int N, int64_t* __restrict__ codes,
                                                                 int64_t codes_bs, int32_t* pos,
                                                                 const int32_t* __restrict__ len, int max_pos,
                                                                 bool sampled, hsp_sample_args a) {
  __shared__ SampleSmem s;
  const int b = blockIdx.x, t = pos[b];
  if (t < 0 || t > max_pos) return;
  int64_t* row = codes + (int64_t)b * codes_bs;
  int tok;
  if (sampled)
    tok = sample_decide(logits + (int64_t)b * l_bs, l_cs, N, row + 1, t, t + 1, a, a.probs, s);
  else
    tok = argmax_row(logits + (int64_t)b * l_bs, l_cs, N, s.redf, s.redi);
  if (threadIdx.x == 0) {
    row[t + 1] = tok;
    pos[b] = t + 1 < len[b] ? t + 1 : -1;
  }
}

}  // namespace

#define HSP_STREAM static_cast<hipStream_t>(stream)

// What every hsp_plm_embed* entry point refuses: a NULL operand; B, Dtc, Demb or n_emb <= 0; a negative stride; fewer
// than 1 or more than P reachable positions (`n`: the full forms' n, max_pos + 1 of the per-row-position form).  Negative
// tc / codes strides used to be refused by the position form alone; no caller passes one, so all forms refuse them.
// Two differences remain, each at its entry point: the full forms also need x_cs >= n (a row's n columns lie below the
// channel stride; the position form writes one column per channel), and the forms whose grid has one workgroup row per
// utterance need B <= 65535 (hsp_plm_embed_f32 strides a capped grid over any B).
static bool embed_ok(const EmbedOps& o, const float* x, int64_t x_bs, int64_t x_cs, int32_t B, int64_t n) {
  if (!o.tc || !o.codes || !o.emb || !o.pe_t || !o.alpha || !x) return false;
  if (B <= 0 || o.Dtc <= 0 || o.Demb <= 0 || o.n_emb <= 0 || n < 1 || n > o.P) return false;
  return o.tc_bs >= 0 && o.tc_cs >= 0 && o.codes_bs >= 0 && x_bs >= 0 && x_cs >= 0;
}

extern "C" int hsp_plm_embed_f32(const float* tc, int64_t tc_bs, int64_t tc_cs, int32_t Dtc, const int64_t* codes,
                                 int64_t codes_bs, const float* emb, int32_t Demb, int32_t n_emb, const float* pe_t,
                                 int32_t P, const float* alpha, float* x, int64_t x_bs, int64_t x_cs, int32_t B,
                                 int32_t n, void* stream) {
  const EmbedOps o{tc, tc_bs, tc_cs, Dtc, codes, codes_bs, emb, Demb, n_emb, pe_t, P, alpha};
  if (!embed_ok(o, x, x_bs, x_cs, B, n) || x_cs < n) return HSP_EINVAL;
  const int64_t total = (int64_t)B * (Dtc + Demb) * n;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(plm_embed_kernel, dim3((unsigned)blocks), dim3(256), 0, HSP_STREAM, PLM_EMBED_ARGS(o), x,
                     x_bs, x_cs, B, n);
  return (int)hipGetLastError();
}

// The fused pair behind what each refuses of its own: the shared operand check (n == 1 is the one-position form of
// hsp.h), the logits operands, the grid (B, parts), the launch.
template <class Choice>
static int embed_choose(const EmbedOps& o, int64_t* codes, float* x, int64_t x_bs, int64_t x_cs, int32_t B, int32_t n,
                        const float* logits, int64_t l_bs, int64_t l_cs, int32_t n_logits, Choice choose, void* stream) {
  if (!embed_ok(o, x, x_bs, x_cs, B, n) || x_cs < n) return HSP_EINVAL;
  if (!logits || n_logits <= 0 || l_cs <= 0 || l_bs < 0) return HSP_EINVAL;
  const int64_t parts = 1 + ((int64_t)o.Dtc * n + 1023) / 1024;
  if (B > 65535 || parts > 65535) return HSP_EINVAL;
  hipLaunchKernelGGL(plm_embed_choose_kernel<Choice>, dim3((unsigned)B, (unsigned)parts), dim3(256), 0, HSP_STREAM, o.tc,
                     o.tc_bs, o.tc_cs, o.Dtc, codes, o.codes_bs, o.emb, o.Demb, o.n_emb, o.pe_t, o.P, o.alpha, x, x_bs,
                     x_cs, B, n, logits, l_bs, l_cs, n_logits, choose);
  return (int)hipGetLastError();
}

extern "C" int hsp_plm_embed_step_f32(const float* tc, int64_t tc_bs, int64_t tc_cs, int32_t Dtc, int64_t* codes,
                                      int64_t codes_bs, const float* emb, int32_t Demb, int32_t n_emb, const float* pe_t,
                                      int32_t P, const float* alpha, float* x, int64_t x_bs, int64_t x_cs, int32_t B,
                                      int32_t n, const float* logits, int64_t l_bs, int64_t l_cs, int32_t n_logits,
                                      void* stream) {
  const EmbedOps o{tc, tc_bs, tc_cs, Dtc, codes, codes_bs, emb, Demb, n_emb, pe_t, P, alpha};
  return embed_choose(o, codes, x, x_bs, x_cs, B, n, logits, l_bs, l_cs, n_logits, GreedyChoice{}, stream);
}

extern "C" int hsp_argmax_f32(const float* logits, int64_t l_bs, int64_t l_cs, int32_t B, int32_t N, int64_t* out,
                              int64_t out_bs, void* stream) {
  if (!logits || !out || B <= 0 || N <= 0 || l_cs <= 0) return HSP_EINVAL;
  hipLaunchKernelGGL(argmax_kernel, dim3((unsigned)B), dim3(256), 0, HSP_STREAM, logits, l_bs, l_cs, N, out, out_bs);
  return (int)hipGetLastError();
}

extern "C" int hsp_copy_strided_f32(const float* x, int64_t s_bs, int64_t s_cs, int64_t s_ts, float* y, int32_t B,
                                    int32_t C, int32_t T, void* stream) {
  if (!x || !y || B <= 0 || C <= 0 || T <= 0 || s_bs < 0 || s_cs < 0 || s_ts < 0) return HSP_EINVAL;
  int64_t blocks = ((int64_t)B * C * T + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(copy_strided_kernel, dim3((unsigned)blocks), dim3(256), 0, HSP_STREAM, x, s_bs, s_cs, s_ts, y, B, C,
                     T);
  return (int)hipGetLastError();
}


static bool sample_args_ok(const hsp_sample_args* a, int32_t N, int32_t j) {
  if (!a || !a->seeds) return false;
  if (a->top_k < 0 || !(a->top_p > 0.0f) || !(a->repetition_penalty > 0.0f) || !std::isfinite(a->temperature))
    return false;
  if (!std::isfinite(a->repetition_penalty)) return false;
  if (N <= 0 || N > kSampleMaxN || j < 1) return false;
  if (a->probs && a->probs_bs < N) return false;
  return true;
}

extern "C" int hsp_plm_embed_sample_f32(const float* tc, int64_t tc_bs, int64_t tc_cs, int32_t Dtc, int64_t* codes,
                                        int64_t codes_bs, const float* emb, int32_t Demb, int32_t n_emb,
                                        const float* pe_t, int32_t P, const float* alpha, float* x, int64_t x_bs,
                                        int64_t x_cs, int32_t B, int32_t n, const float* logits, int64_t l_bs,
                                        int64_t l_cs, int32_t n_logits, int32_t j, const hsp_sample_args* args,
                                        void* stream) {
  if (!sample_args_ok(args, n_logits, j)) return HSP_EINVAL;
  if (n > 1 && j != n - 1) return HSP_EINVAL;   // the full form chooses column n - 1
  const EmbedOps o{tc, tc_bs, tc_cs, Dtc, codes, codes_bs, emb, Demb, n_emb, pe_t, P, alpha};
  return embed_choose(o, codes, x, x_bs, x_cs, B, n, logits, l_bs, l_cs, n_logits, SampledChoice{j, *args}, stream);
}

extern "C" int hsp_sample_f32(const float* logits, int64_t l_bs, int64_t l_cs, int32_t B, int32_t N, int64_t* out,
                              int64_t out_bs, int32_t j, const hsp_sample_args* args, void* stream) {
  if (!logits || !out || B <= 0 || B > 65535 || l_cs <= 0 || l_bs < 0 || !sample_args_ok(args, N, j)) return HSP_EINVAL;
  hipLaunchKernelGGL(sample_kernel, dim3((unsigned)B), dim3(256), 0, HSP_STREAM, logits, l_bs, l_cs, N, out, out_bs, j,
                     *args);
  return (int)hipGetLastError();
}

extern "C" int hsp_plm_embed_pos_f32(const float* tc, int64_t tc_bs, int64_t tc_cs, int32_t Dtc, const int64_t* codes,
                                     int64_t codes_bs, const float* emb, int32_t Demb, int32_t n_emb, const float* pe_t,
                                     int32_t P, const float* alpha, float* x, int64_t x_bs, int64_t x_cs, int32_t B,
                                     const int32_t* pos, int32_t max_pos, void* stream) {
  const EmbedOps o{tc, tc_bs, tc_cs, Dtc, codes, codes_bs, emb, Demb, n_emb, pe_t, P, alpha};
  if (!embed_ok(o, x, x_bs, x_cs, B, (int64_t)max_pos + 1) || !pos || B > 65535) return HSP_EINVAL;
  hipLaunchKernelGGL(plm_embed_pos_kernel, dim3((unsigned)B), dim3(256), 0, HSP_STREAM, PLM_EMBED_ARGS(o), x, x_bs,
                     x_cs, pos, max_pos);
  return (int)hipGetLastError();
}

extern "C" int hsp_plm_choose_advance_f32(const float* logits, int64_t l_bs, int64_t l_cs, int32_t B, int32_t N,
                                          int64_t* codes, int64_t codes_bs, int32_t* pos, const int32_t* len,
                                          int32_t max_pos, const hsp_sample_args* args, void* stream) {
  if (!logits || !codes || !pos || !len) return HSP_EINVAL;
  if (B <= 0 || B > 65535 || N <= 0 || l_cs <= 0 || l_bs < 0 || codes_bs < 0 || max_pos < 0) return HSP_EINVAL;
  if (args && !sample_args_ok(args, N, 1)) return HSP_EINVAL;   // j = pos[b] + 1 >= 1 for every active row
  hipLaunchKernelGGL(plm_choose_advance_kernel, dim3((unsigned)B), dim3(256), 0, HSP_STREAM, logits, l_bs, l_cs, N,
                     codes, codes_bs, pos, len, max_pos, args != nullptr, args ? *args : hsp_sample_args{});
  return (int)hipGetLastError();
}
