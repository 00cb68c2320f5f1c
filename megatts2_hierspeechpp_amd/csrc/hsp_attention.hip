// Multi-head attention on channel-major (B, H*D, T) tensors, fp32.
//
// Covers timm 0.6.13 Attention as used by DiTConVBlock (modules.py:397,409: no key
// mask, scale D^-0.5), and attentions.MultiHeadAttention (attentions.py:157-188:
// masked_fill(mask == 0, -1e4), optional relative-position window on keys and values).
//
// Whole-row kernels (mha_kernel, mha_mfma_kernel): one workgroup = 16 / 32 queries of one (batch, head), the
// scores for ALL keys are kept in LDS, soft-maxed by rows, then multiplied with V.  They serve every launch
// whose score rows fit the CU's LDS (T <= a few hundred on the 50 Hz path); beyond that the key-streaming
// kernels at the end of this file (online softmax over key blocks) take over, so no launch has a length ceiling.
#include "hsp_device.h"

namespace {

constexpr int QT = 16;       // queries per workgroup of the scalar kernels
constexpr int MQT = 32;      // ... of the MFMA kernels
constexpr int ATT_THREADS = 256;
typedef float mha_f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------
// The steps the kernels share, each said once.

// Where a workgroup works: its batch item and first query, the channel strides (the host fills the defaults) and the
// four planes of its head.  Every kernel starts from mha_head_of<queries per workgroup>.
struct mha_head {
  int b, i0;
  int64_t qcs, kcs, vcs, ocs;
  const float *qh, *kh, *vh;
  float* oh;
};

template <int QTILE>
__device__ __forceinline__ mha_head mha_head_of(const hsp_mha_args& a, int n_qt) {
  int bid = blockIdx.x;
  const int qt = bid % n_qt;
  bid /= n_qt;
  const int h = bid % a.H;
  const int b = bid / a.H;
  mha_head t;
  t.b = b;
  t.i0 = qt * QTILE;
  t.qcs = a.q_cs, t.kcs = a.k_cs, t.vcs = a.v_cs, t.ocs = a.o_cs;
  t.qh = a.q + (int64_t)b * a.q_bs + (int64_t)h * a.D * t.qcs;
  t.kh = a.k + (int64_t)b * a.k_bs + (int64_t)h * a.D * t.kcs;
  t.vh = a.v + (int64_t)b * a.v_bs + (int64_t)h * a.D * t.vcs;
  t.oh = a.o + (int64_t)b * a.o_bs + (int64_t)h * a.D * t.ocs;
  return t;
}

// masked_fill(mask == 0, -1e4) of attentions.py:175, the one statement of it: a score whose mask value is 0 becomes
// the VALUE -1e4.  mha_mask applies it to score s of query i < Tq and key j < Tk of batch item b, for the factor masks
// (mask_q[i] * mask_k[j]; mk = mask_k[b][j] where the caller holds it already) and for the dense mask.
__device__ __forceinline__ bool mha_masked(float m) { return m == 0.0f; }
constexpr float MHA_MASKED = -1e4f;

__device__ __forceinline__ void mha_mask(const hsp_mha_args& a, int b, int i, int j, float& s, float mk) {
  if (a.mask_q && mha_masked(a.mask_q[(int64_t)b * a.Tq + i] * mk)) s = MHA_MASKED;
  if (a.mask_dense && mha_masked(a.mask_dense[(int64_t)b * a.mask_dense_bs + (int64_t)i * a.Tk + j])) s = MHA_MASKED;
}
__device__ __forceinline__ void mha_mask(const hsp_mha_args& a, int b, int i, int j, float& s) {
  mha_mask(a, b, i, j, s, a.mask_q ? a.mask_k[(int64_t)b * a.Tk + j] : 1.0f);
}

// The two exponentials of the online softmax: the scalar kernels keep libm's expf, the MFMA ones the hardware exp2
struct mha_exp_libm { __device__ __forceinline__ float operator()(float x) const { return expf(x); } };
struct mha_exp_hw { __device__ __forceinline__ float operator()(float x) const { return hsp_exp2e(x); } };

// One online-softmax step of a wave on one query row over the 64 NCOL columns of a key block (columns beyond Tk hold
// -3e38 and get weight 0): the row becomes exp(s - m_new), and lane 0 moves the row's running maximum *m and sum *l and
// leaves exp(m_old - m_new), the factor the PV accumulators are rescaled by (0 on the first block), in *al.
template <int NCOL, class Exp>
__device__ __forceinline__ void mha_online_row(float* row, int lane, float* m, float* l, float* al, Exp ex) {
  float sv[NCOL];
  float mx = -3.0e38f;
#pragma unroll
  for (int q = 0; q < NCOL; ++q) { sv[q] = row[lane + 64 * q]; mx = fmaxf(mx, sv[q]); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  const float mo = *m;
  const float mn = fmaxf(mo, mx);
  float sum = 0.0f;
#pragma unroll
  for (int q = 0; q < NCOL; ++q) {
    const float e = sv[q] > -1.0e38f ? ex(sv[q] - mn) : 0.0f;
    row[lane + 64 * q] = e;
    sum += e;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) {
    const float a_ = ex(mo - mn);
    *al = a_;
    *l = *l * a_ + sum;
    *m = mn;
  }
}

// O^T accumulator of head-dim block db (queries on the lanes) -> o[d][i0 + l32] = (acc [+ add]) * inv for the rows
// d < D.  ADD: `add` is this lane's first element of a second partial sum laid out [16][64] (TOK's other key half).
template <bool ADD = false>
__device__ __forceinline__ void mha_store_o(const mha_head& t, int D, int db, int l32, int half, const mha_f32x16& acc, float inv,
                                            const float* add = nullptr) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int d = db * 32 + HSP_ACC_ROW(r, half);
    if (d < D) t.oh[(int64_t)d * t.ocs + t.i0 + l32] = (ADD ? acc[r] + add[r * 64] : acc[r]) * inv;
  }
}

// ---- scalar family (mha_kernel, mha_stream_kernel): 16 queries per workgroup
// LDS in floats: Qs [D][QT] at 0 | S [QT][sp] | Vs [64][dpad] | the streaming form's running max, sum, rescale [3][QT]
template <class I> struct row_lds { I S, Vs, state, total; };
template <class I>
__host__ __device__ constexpr row_lds<I> row_layout(I D, I sp, I dpad, bool stream) {
  row_lds<I> L{};
  L.S = D * QT;
  L.Vs = L.S + QT * sp;
  L.state = L.Vs + 64 * dpad;
  L.total = L.state + (stream ? 3 * QT : 0);
  return L;
}

// Q tile, pre-scaled (attentions.py:164 divides the query; timm scales the product), zero beyond Tq
__device__ __forceinline__ void row_stage_q(const hsp_mha_args& a, const mha_head& t, float* Qs, int tid) {
  for (int e = tid; e < a.D * QT; e += ATT_THREADS) {
    const int i = e % QT, d = e / QT;
    Qs[e] = (t.i0 + i < a.Tq) ? t.qh[(int64_t)d * t.qcs + t.i0 + i] * a.qk_scale : 0.0f;
  }
}

// sv[u] = score of query i0 + iq + u against key j < Tk: the dot over the head dim, the relative-key term of a key
// inside the query's window, the mask
__device__ __forceinline__ void row_score4(const hsp_mha_args& a, const mha_head& t, const float* Qs, int iq, int j, float sv[4]) {
  const int D = a.D;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int d = 0; d < D; ++d) {
    const float kv = t.kh[(int64_t)d * t.kcs + j];
    const float4 qv = *reinterpret_cast<const float4*>(Qs + d * QT + iq);
    s0 = fmaf(qv.x, kv, s0);
    s1 = fmaf(qv.y, kv, s1);
    s2 = fmaf(qv.z, kv, s2);
    s3 = fmaf(qv.w, kv, s3);
  }
  sv[0] = s0; sv[1] = s1; sv[2] = s2; sv[3] = s3;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = t.i0 + iq + u;
    float s = sv[u];
    if (a.rel_k) {
      const int r = j - i;
      if (r >= -a.window && r <= a.window && i < a.Tq) {
        const float* ek = a.rel_k + (int64_t)(r + a.window) * D;
        float e = 0.0f;
        for (int d = 0; d < D; ++d) e = fmaf(Qs[d * QT + iq + u], ek[d], e);
        s += e;
      }
    }
    if (i < a.Tq) mha_mask(a, t.b, i, j, s);
    sv[u] = s;
  }
}

// V slab: keys jb .. jb + 63 (zero from jend on) x head dims d0 .. d0 + 127 -> Vs [64][dpad]; wave w brings dims w, w + 4, ...
__device__ __forceinline__ void row_stage_v(const mha_head& t, float* Vs, int D, int dpad, int d0, int jb, int jend, int lane, int wave) {
  for (int dd = wave; dd < 128 && d0 + dd < D; dd += 4)
    Vs[lane * dpad + dd] = (jb + lane < jend) ? t.vh[(int64_t)(d0 + dd) * t.vcs + jb + lane] : 0.0f;
}

// ---- MFMA family (mha_mfma_kernel, mha_mfma_stream_kernel): 32 queries per workgroup, DP = head dim padded to 32s
// LDS in floats: Qs [DP][32] at 0 | S [32][sp] | Vs [DP][vp] | the streaming form's running max, sum, rescale [3][32]
constexpr int SLAB_VP = 65;   // V pitch of the slab form (64 keys, odd)
template <class I> struct mfma_lds { I S, Vs, state, total; };
template <class I>
__host__ __device__ constexpr mfma_lds<I> mfma_layout(I DP, I sp, I vp, bool stream) {
  mfma_lds<I> L{};
  L.S = DP * 32;
  L.Vs = L.S + 32 * sp;
  L.state = L.Vs + DP * vp;
  L.total = L.state + (stream ? 3 * 32 : 0);
  return L;
}

// Q tile [DP][32] = scale * q, zero rows beyond D and columns beyond Tq
template <int DP>
__device__ __forceinline__ void mfma_stage_q(const hsp_mha_args& a, const mha_head& t, float* Qs, int tid) {
  const int D = a.D, Tq = a.Tq, i0 = t.i0;
  const float* qh = t.qh;
  const int64_t qcs = t.qcs;
#pragma unroll
  for (int u = 0; u < DP * 32 / 256; ++u) {
    const int e = tid + 256 * u;
    const int i = e & 31, d = e >> 5;
    Qs[e] = (d < D && i0 + i < Tq) ? qh[(int64_t)d * qcs + i0 + i] * a.qk_scale : 0.0f;
  }
}

// S[32 queries][32 keys] = (scale Q)^T K for the key block whose key j sits on this lane (zero beyond Tk): the block's K
// fragments are fetched in one batch straight from the channel-major plane, the A fragments come from the Q tile
template <int DP>
__device__ __forceinline__ mha_f32x16 mfma_score_block(const hsp_mha_args& a, const mha_head& t, const float* Qs, int j, int l32, int half) {
  const bool jok = j < a.Tk;
  float kf[DP / 2];
#pragma unroll
  for (int kk = 0; kk < DP / 2; ++kk) {
    const int d = 2 * kk + half;
    kf[kk] = (jok && d < a.D) ? t.kh[(int64_t)d * t.kcs + j] : 0.0f;
  }
  mha_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
  for (int kk = 0; kk < DP / 2; ++kk)
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[(2 * kk + half) * 32 + l32], kf[kk], acc, 0, 0, 0);
  return acc;
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(ATT_THREADS) void mha_kernel(const hsp_mha_args a, int n_qt, int dpad, int spad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const auto L = row_layout<int>(a.D, spad, dpad, false);
  float* Qs = lds;
  float* S = lds + L.S;
  float* Vs = lds + L.Vs;
  const mha_head t = mha_head_of<QT>(a, n_qt);
  const int i0 = t.i0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = a.D, Tq = a.Tq, Tk = a.Tk;

  row_stage_q(a, t, Qs, tid);
  __syncthreads();

  // ---- scores: wave w owns queries 4w..4w+3, lanes run along keys
  for (int j = lane; j < Tk; j += 64) {
    float sv[4];
    row_score4(a, t, Qs, wave * 4, j, sv);
#pragma unroll
    for (int u = 0; u < 4; ++u) S[(wave * 4 + u) * spad + j] = sv[u];
  }
  __syncthreads();

  // ---- row softmax (4 rows per wave)
  for (int u = 0; u < 4; ++u) {
    float* row = S + (wave * 4 + u) * spad;
    float mx = -3.0e38f;
    for (int j = lane; j < Tk; j += 64) mx = fmaxf(mx, row[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.0f;
    for (int j = lane; j < Tk; j += 64) {
      const float e = expf(row[j] - mx);
      row[j] = e;
      sum += e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float inv = 1.0f / sum;
    for (int j = lane; j < Tk; j += 64) row[j] *= inv;
  }

  // ---- O = P V : thread = (head-dim d, query group of 8)
  const int d = tid & 127, ig = tid >> 7;
  float acc[8];
  for (int d0 = 0; d0 < D; d0 += 128) {
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.0f;
    for (int j0 = 0; j0 < Tk; j0 += 64) {
      __syncthreads();  // softmax rows complete (first pass) / previous slab consumed
      row_stage_v(t, Vs, D, dpad, d0, j0, Tk, lane, wave);
      __syncthreads();
      if (d0 + d < D) {
        const int jn = min(64, Tk - j0);
        for (int j = 0; j < jn; ++j) {
          const float vv = Vs[j * dpad + d];
#pragma unroll
          for (int u = 0; u < 8; ++u) acc[u] = fmaf(S[(ig * 8 + u) * spad + j0 + j], vv, acc[u]);
        }
      }
    }
    if (d0 + d < D) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + ig * 8 + u;
        if (i >= Tq) continue;
        float v = acc[u];
        if (a.rel_v) {
          for (int r = -a.window; r <= a.window; ++r) {
            const int j = i + r;
            if (j >= 0 && j < Tk) v = fmaf(S[(ig * 8 + u) * spad + j], a.rel_v[(int64_t)(r + a.window) * D + d0 + d], v);
          }
        }
        t.oh[(int64_t)(d0 + d) * t.ocs + i] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// fp32-MFMA attention (v_mfma_f32_32x32x2_f32, exact fp32) for the no-window case: timm
// Attention of the DiT blocks and the StyleEncoder's self-attention.  One workgroup = 32
// queries of one (batch, head):
//   S^T-free layout: S[32 x Tk] = (scale*Q)^T K  with M = queries, N = keys, k = head dim
//                    (A fragments from the Q tile in LDS, B fragments straight from the
//                    channel-major K plane: 32 consecutive keys per half wave);
//   row softmax in LDS (mask -> -1e4 exactly like attentions.py:175);
//   O^T[D x 32] = V P^T with M = head dim, N = queries, k = keys: V is staged through LDS in
//                    64-key slabs (odd pitch: the column reads of both operands are conflict
//                    free) and the result lands with queries on the lanes -> coalesced stores.

// NDB = ceil(D / 32).  WHOLE_V: all of V (D x Tk) is staged in LDS once, next to the Q tile, so the kernel
// has three global round trips in sequence (Q + V, the K fragments of this wave's key blocks, nothing else)
// instead of one per 4 head-dim steps and two per 64-key slab: at T <= 256 the launch is pure latency.
template <int NDB, bool WHOLE_V>
__global__ __launch_bounds__(256) void mha_mfma_kernel(const hsp_mha_args a, int n_qt, int sp, int vp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int D = a.D, Tq = a.Tq, Tk = a.Tk;
  constexpr int DP = NDB * 32;
  const auto L = mfma_layout<int>(DP, sp, WHOLE_V ? vp : SLAB_VP, false);   // WHOLE_V: vp odd, >= Tk rounded up to 64
  float* Qs = lds;
  float* S = lds + L.S;
  float* Vs = lds + L.Vs;
  const mha_head t = mha_head_of<MQT>(a, n_qt);
  const int b = t.b, i0 = t.i0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, half = lane >> 5;
  const float* vh = t.vh;
  const int64_t vcs = t.vcs;

  if constexpr (WHOLE_V) {
    // V rows straight into LDS (LDS-DMA, 4 B per lane, nothing waits here); padding is zeroed by hand
    const int tkp = (Tk + 63) & ~63;
    for (int d = wave; d < DP; d += 4)
      for (int j0 = 0; j0 < tkp; j0 += 64) {
        if (d < D && j0 + lane < Tk)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vh + (int64_t)d * vcs + j0 + lane),
                                           (__attribute__((address_space(3))) void*)(Vs + d * vp + j0), 4, 0, 0);
        else
          Vs[d * vp + j0 + lane] = 0.0f;
      }
  }
  mfma_stage_q<DP>(a, t, Qs, tid);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- scores: wave w owns key blocks w, w+4, ...; the block's K fragments are fetched in one batch
  // (issuing the first block's fragments together with the Q / V reads saves 1.2 us at T <= 128 but costs
  //  more than that once two workgroups share a CU: measured, not kept)
  const int nkb = (Tk + 31) >> 5;
  for (int jb = wave; jb < nkb; jb += 4) {
    const int j = jb * 32 + l32;
    const mha_f32x16 acc = mfma_score_block<DP>(a, t, Qs, j, l32, half);
#pragma unroll
    for (int r = 0; r < 16; ++r) S[HSP_ACC_ROW(r, half) * sp + j] = acc[r];
  }
  __syncthreads();

  // ---- row softmax over the Tk valid keys (8 rows per wave).  exp on the hardware exp2; the 1 / sum
  // normalisation is applied to the PV output (queries sit on the lanes there), padding columns become 0
  float* inv_s = Qs;   // Qs is dead after the score phase (all waves passed the barrier above): 32 floats reused
  for (int u = 0; u < 8; ++u) {
    const int row_i = wave * 8 + u;
    float* row = S + row_i * sp;
    const int i = i0 + row_i;
    const float mq = (a.mask_q && i < Tq) ? a.mask_q[(int64_t)b * Tq + i] : 1.0f;
    const float* md = (a.mask_dense && i < Tq) ? a.mask_dense + (int64_t)b * a.mask_dense_bs + (int64_t)i * Tk : nullptr;
    float mx = -3.0e38f;
    for (int j = lane; j < Tk; j += 64) {
      float sv = row[j];
      if (a.mask_q && mha_masked(mq * a.mask_k[(int64_t)b * Tk + j])) sv = MHA_MASKED;
      if (md && mha_masked(md[j])) sv = MHA_MASKED;
      row[j] = sv;
      mx = fmaxf(mx, sv);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.0f;
    for (int j = lane; j < nkb * 32 + 32 && j < sp; j += 64) {
      const float e = j < Tk ? hsp_exp2e(row[j] - mx) : 0.0f;
      row[j] = e;
      sum += e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) inv_s[row_i] = 1.0f / sum;
  }

  // ---- O^T = V P^T: wave w owns head-dim block w (D <= 128)
  mha_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  if constexpr (WHOLE_V) {
    __syncthreads();  // softmax rows complete
    if (wave < NDB) {
      const float* va = Vs + (wave * 32 + l32) * vp + half;
      const float* pb = S + l32 * sp + half;
      const int tk2 = (Tk + 1) & ~1;   // S and Vs are zero beyond Tk
#pragma unroll 8
      for (int jj = 0; jj < tk2; jj += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va[jj], pb[jj], acc, 0, 0, 0);
    }
  } else {
    for (int j0 = 0; j0 < Tk; j0 += 64) {
      __syncthreads();  // softmax complete (first slab) / previous slab consumed
      for (int d = wave; d < DP; d += 4)
        Vs[d * SLAB_VP + lane] = (d < D && j0 + lane < Tk) ? vh[(int64_t)d * vcs + j0 + lane] : 0.0f;
      __syncthreads();
      if (wave < NDB) {
        const float* va = Vs + (wave * 32 + l32) * SLAB_VP + half;
        const float* pb = S + l32 * sp + j0 + half;
#pragma unroll 8
        for (int jj = 0; jj < 64; jj += 2)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va[jj], pb[jj], acc, 0, 0, 0);
      }
    }
  }
  if (wave < NDB && i0 + l32 < Tq) mha_store_o(t, D, wave, l32, half, acc, inv_s[l32]);
}

// What mha_decide (end of this file) settled for a launch: the kernel (HSP_MHA_*), its head-dim blocks, the launch
// shape and the LDS pitches.  hsp_mha_f32 only carries it out; hsp_mha_plan reports it.
struct mha_choice {
  int kernel, ndb, n_qt, sp, vp, dpad;
  int64_t lds, blocks;
};

// ---------------------------------------------------------------------------------------
// Key-streaming variants (online softmax): no launch depends on Tk fitting LDS.  Used when the whole-row kernels
// above would need more than the CU's 160 KB (Tk beyond ~1 200 with the MFMA kernel, ~2 200 with the window
// kernel): the denoiser's time conformer on a long prompt (160 frames/s, denoiser/conformer.py:45-60), the
// StyleEncoder / MelEncoder on a minute of mel frames (attentions.py:157-188).  Keys are walked in blocks; a query
// row keeps a running maximum m and sum l, and the PV accumulators are rescaled by exp(m_old - m_new) whenever the
// maximum moves.  masked_fill(-1e4) semantics are unchanged: a masked score is the VALUE -1e4 (a fully masked row
// ends as the uniform average, as in the reference); only keys beyond Tk are excluded (weight 0).
constexpr int SKB = 128;   // keys per block of the MFMA kernel (4 waves x 32)

template <int NDB>
__global__ __launch_bounds__(256) void mha_mfma_stream_kernel(const hsp_mha_args a, int n_qt) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int D = a.D, Tq = a.Tq, Tk = a.Tk;
  constexpr int DP = NDB * 32;
  constexpr int SP = SKB + 1, VP = SKB + 1;
  constexpr auto L = mfma_layout<int>(DP, SP, VP, true);
  float* Qs = lds;
  float* S = lds + L.S;
  float* Vs = lds + L.Vs;
  float* mrow = lds + L.state;     // [32] running maximum
  float* lrow = mrow + 32;         // [32] running sum
  float* arow = lrow + 32;         // [32] rescale factor of the current block
  const mha_head t = mha_head_of<MQT>(a, n_qt);
  const int b = t.b, i0 = t.i0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, half = lane >> 5;
  const float* vh = t.vh;
  const int64_t vcs = t.vcs;

  mfma_stage_q<DP>(a, t, Qs, tid);
  if (tid < 32) { mrow[tid] = -3.0e38f; lrow[tid] = 0.0f; }
  mha_f32x16 oacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) oacc[r] = 0.0f;

  for (int j0 = 0; j0 < Tk; j0 += SKB) {
    __syncthreads();   // Q / state initialised (first block); S and Vs of the previous block consumed
    // V block -> LDS (zero beyond Tk and beyond D)
    for (int d = wave; d < DP; d += 4)
      for (int jj = lane; jj < SKB; jj += 64)
        Vs[d * VP + jj] = (d < D && j0 + jj < Tk) ? vh[(int64_t)d * vcs + j0 + jj] : 0.0f;
    // scores of this wave's 32 keys
    {
      const int j = j0 + wave * 32 + l32;
      const bool jok = j < Tk;
      const mha_f32x16 acc = mfma_score_block<DP>(a, t, Qs, j, l32, half);
      const float mk = (a.mask_k && jok) ? a.mask_k[(int64_t)b * Tk + j] : 1.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row_i = HSP_ACC_ROW(r, half);
        const int i = i0 + row_i;
        float sv = acc[r];
        if (i < Tq && jok) mha_mask(a, b, i, j, sv, mk);
        S[row_i * SP + wave * 32 + l32] = jok ? sv : -3.0e38f;
      }
    }
    __syncthreads();
    // online softmax of rows 8 wave .. 8 wave + 7 over the block's 128 columns (two per lane)
    for (int u = 0; u < 8; ++u) {
      const int row_i = wave * 8 + u;
      mha_online_row<SKB / 64>(S + row_i * SP, lane, mrow + row_i, lrow + row_i, arow + row_i, mha_exp_hw{});
    }
    __syncthreads();
    // O^T += V P^T on the rescaled accumulators: wave w owns head-dim block w, queries sit on the lanes
    if (wave < NDB) {
      const float al = arow[l32];
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[r] *= al;
      const float* va = Vs + (wave * 32 + l32) * VP + half;
      const float* pb = S + l32 * SP + half;
#pragma unroll 8
      for (int jj = 0; jj < SKB; jj += 2) oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(va[jj], pb[jj], oacc, 0, 0, 0);
    }
  }
  if (wave < NDB && i0 + l32 < Tq) mha_store_o(t, D, wave, l32, half, oacc, 1.0f / lrow[l32]);
}

// Window (relative-position) kernel, key-streaming form.  Same thread roles as mha_kernel: wave w scores
// queries 4w .. 4w+3 with lanes along the keys of a block; thread (d, query group) accumulates P V plus the
// relative-value term of the keys of this block that fall inside a query's window.  D <= 256.
constexpr int WKB = 256;   // keys per block

__global__ __launch_bounds__(ATT_THREADS) void mha_stream_kernel(const hsp_mha_args a, int n_qt, int dpad) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int D = a.D, Tq = a.Tq, Tk = a.Tk;
  constexpr int SPW = WKB + 1;
  const auto L = row_layout<int>(D, SPW, dpad, true);
  float* Qs = lds;
  float* S = lds + L.S;
  float* Vs = lds + L.Vs;
  float* mrow = lds + L.state;           // [QT]
  float* lrow = mrow + QT;
  float* arow = lrow + QT;
  const mha_head t = mha_head_of<QT>(a, n_qt);
  const int i0 = t.i0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* oh = t.oh;
  const int64_t ocs = t.ocs;

  row_stage_q(a, t, Qs, tid);
  if (tid < QT) { mrow[tid] = -3.0e38f; lrow[tid] = 0.0f; }
  const int d = tid & 127, ig = tid >> 7;       // PV role: head dims d and d + 128, queries 8 ig .. 8 ig + 7
  float acc0[8], acc1[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) acc0[u] = acc1[u] = 0.0f;

  for (int j0 = 0; j0 < Tk; j0 += WKB) {
    const int jn = min(WKB, Tk - j0);
    __syncthreads();   // Q / state ready; previous block's S consumed
    for (int jj = lane; jj < WKB; jj += 64) {
      float sv[4] = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
      if (jj < jn) row_score4(a, t, Qs, wave * 4, j0 + jj, sv);
#pragma unroll
      for (int u = 0; u < 4; ++u) S[(wave * 4 + u) * SPW + jj] = sv[u];
    }
    __syncthreads();
    for (int u = 0; u < 4; ++u) {
      const int row_i = wave * 4 + u;
      mha_online_row<WKB / 64>(S + row_i * SPW, lane, mrow + row_i, lrow + row_i, arow + row_i, mha_exp_libm{});
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) { const float al = arow[ig * 8 + u]; acc0[u] *= al; acc1[u] *= al; }
    for (int d0 = 0; d0 < D; d0 += 128) {
      for (int js = 0; js < jn; js += 64) {
        __syncthreads();
        row_stage_v(t, Vs, D, dpad, d0, j0 + js, j0 + jn, lane, wave);
        __syncthreads();
        if (d0 + d < D) {
          const int jm = min(64, jn - js);
          for (int j = 0; j < jm; ++j) {
            const float vv = Vs[j * dpad + d];
            if (d0 == 0) {
#pragma unroll
              for (int u = 0; u < 8; ++u) acc0[u] = fmaf(S[(ig * 8 + u) * SPW + js + j], vv, acc0[u]);
            } else {
#pragma unroll
              for (int u = 0; u < 8; ++u) acc1[u] = fmaf(S[(ig * 8 + u) * SPW + js + j], vv, acc1[u]);
            }
          }
        }
      }
      if (a.rel_v && d0 + d < D) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + ig * 8 + u;
          if (i >= Tq) continue;
          float rv = 0.0f;
          for (int r = -a.window; r <= a.window; ++r) {
            const int j = i + r;
            if (j >= j0 && j < j0 + jn) rv = fmaf(S[(ig * 8 + u) * SPW + j - j0], a.rel_v[(int64_t)(r + a.window) * D + d0 + d], rv);
          }
          if (d0 == 0) acc0[u] += rv; else acc1[u] += rv;
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = i0 + ig * 8 + u;
    if (i >= Tq) continue;
    const float inv = 1.0f / lrow[ig * 8 + u];
    if (d < D) oh[(int64_t)d * ocs + i] = acc0[u] * inv;
    if (d + 128 < D) oh[(int64_t)(d + 128) * ocs + i] = acc1[u] * inv;
  }
}

// ---------------------------------------------------------------------------------------
// Short-sequence attention without masks or window (the PLM loop's 4 x 69 heads over a growing prefix, timm
// Attention of the DiT blocks: Tk <= 256): latency-oriented.  The whole-row MFMA kernel above stages V through LDS
// (by LDS-DMA or slab by slab) and spends 20 us on a 10-key problem, 56 us at 200 keys (round-3 trace of the PLM
// loop: 4 launches x 200 steps = a quarter of the loop).  Here nothing but the scores touches LDS:
//   * one workgroup (8 waves) = 32 queries of one (batch, head);
//   * S = (scale Q)^T K: wave w owns key blocks w, w + 8, ...; both fragments are coalesced dword loads from the
//     channel-major planes (lanes along queries / keys), the Q fragments are loaded once and kept in registers;
//   * row softmax in LDS, 4 rows per wave;
//   * O^T = V P^T: six (three, ...) waves = head-dim blocks x two key halves.  The V fragment of lane (d, half) is ONE
//     16-B load of V[d][j0 + 4 half .. + 3] feeding four MFMAs (the k-slots of an MFMA may pair any two keys as
//     long as the P fragment pairs the same ones), so V needs no transpose and no staging; the two key halves
//     are added through LDS.
// LDS = 32 x (Tk + pad) scores + the partial-sum buffer: 45 KB at Tk = 256 -> three workgroups per CU.
constexpr int TQT = 32;
constexpr int TOK_NW = 8;   // eight waves: one key block each, two key halves in the PV phase.  (A four-wave form, of which a
                            // CU holds more, was measured on 448 / 896 workgroups: 38.7 / 53.5 us against 32.6 / 58.1 -- its
                            // per-workgroup chain is twice as long -- and is not built.)

// LDS in floats: S [32][sp] at 0 | red [NDB][16][64], the partial O of the second key half (two key halves only) | inv_s [32]
constexpr int tok_kh(int nw, int ndb) { return nw / ndb >= 2 ? 2 : 1; }   // key halves in the PV phase (8 waves: 2, 4 waves: 1)
constexpr int tok_sp(int Tk) { return ((((Tk + 31) >> 5) * 32 + 7) & ~7) + 1; }
template <class I> struct tok_lds { I red, inv_s, total; };
template <class I>
__host__ __device__ constexpr tok_lds<I> tok_layout(I sp, int ndb, int nw) {
  tok_lds<I> L{};
  L.red = 32 * sp;
  L.inv_s = L.red + (tok_kh(nw, ndb) == 2 ? ndb * 16 * 64 : 0);
  L.total = L.inv_s + 32;
  return L;
}

template <int NDB, int NW>
__global__ __launch_bounds__(64 * NW) void mha_tok_kernel(const hsp_mha_args a, int n_qt, int sp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int KH = tok_kh(NW, NDB);
  const int D = a.D, Tq = a.Tq, Tk = a.Tk;
  const auto L = tok_layout<int>(sp, NDB, NW);
  float* S = lds;
  float* red = lds + L.red;
  float* inv_s = lds + L.inv_s;
  const mha_head t = mha_head_of<TQT>(a, n_qt);
  const int i0 = t.i0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, half = lane >> 5;
  const int64_t qcs = t.qcs, kcs = t.kcs, vcs = t.vcs;
  const float *qh = t.qh, *kh = t.kh, *vh = t.vh;
  const int nkb = (Tk + 31) >> 5;
#ifdef HSP_TUNING
  unsigned long long* stamps = (a.window == 1003 && blockIdx.x == 0 && tid == 0) ? (unsigned long long*)a.rel_v : nullptr;
#define MT_STAMP(i) do { if (stamps) stamps[i] = __builtin_readcyclecounter(); } while (0)
#else
#define MT_STAMP(i) do { } while (0)
#endif
  MT_STAMP(0);

  // ---- scores.  Tk <= 256 = eight key blocks = one (two) per wave, so nothing is reused across blocks: both
  // fragments are loaded per group of U k-steps, all of a group's loads in flight together (the loop of
  // hsp_rgemm.hip).  Only ceil(D / 2) k-steps run (35 of the padded 48 at D = 69).
  {
    constexpr int U = NDB == 3 ? 36 : 32;             // k-steps requested together: all 35 of D = 69 (one round trip; in-kernel stamps:
                                                      // two groups of 18 cost 4 us of a 9-us launch), 48 at D = 96 in two
    const int ksteps = (D + 1) >> 1;
    const bool odd_tail = (D & 1) != 0;
    const int iq = min(i0 + l32, Tq - 1);
    for (int jb = wave; jb < nkb; jb += NW) {
      const int j = jb * 32 + l32;
      const float* qp = qh + iq + (int64_t)half * qcs;
      const float* kp = kh + min(j, Tk - 1) + (int64_t)half * kcs;
      const int64_t qst = 2 * qcs, kst = 2 * kcs;
      mha_f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll 1
      for (int kk = 0; kk < ksteps; kk += U) {
        float fq[U], fk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int k = min(kk + u, ksteps - 1);
          const int kc = (odd_tail && half == 1 && k == ksteps - 1) ? k - 1 : k;   // stay inside the head's rows
          fq[u] = qp[(int64_t)kc * qst];
          fk[u] = kp[(int64_t)kc * kst];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool ok = kk + u < ksteps && !(odd_tail && half == 1 && kk + u == ksteps - 1);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? fq[u] * a.qk_scale : 0.0f, fk[u], acc, 0, 0, 0);
        }
      }
      const bool jok = j < Tk;
#pragma unroll
      for (int r = 0; r < 16; ++r) S[HSP_ACC_ROW(r, half) * sp + j] = jok ? acc[r] : -3.0e38f;
    }
  }
  MT_STAMP(1);
  __syncthreads();
  MT_STAMP(2);
  // ---- V fragments of the first chunk: requested NOW, ahead of the softmax they do not depend on.
  // O^T[d][q] = sum_j V[d][j] P[q][j]: wave = (head-dim block, key part); groups of 8 keys, MAXG groups in flight.
  typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
  constexpr int MAXG = 16;
  const int db = wave % NDB, kh2 = wave / NDB;        // waves >= KH NDB idle in the PV phase
  const int ngrp = (Tk + 7) >> 3;                     // groups of 8 keys
  const int gsplit = KH == 2 ? (ngrp + 1) / 2 : ngrp;
  const int g0 = kh2 == 0 ? 0 : gsplit, g1 = kh2 >= KH ? 0 : (kh2 == 0 ? gsplit : ngrp);
  const int dv = db * 32 + l32;
  const bool dok = dv < D;
  const float* vrow = vh + (int64_t)min(dv, D - 1) * vcs;
  // lane (d, half) wants V[d][jl .. jl + 3], jl = 8 g + 4 half: one 16-B load (4-B aligned: the utterances of a
  // batch sit side by side on the column axis).  A window that would end beyond Tk (last group only) is moved
  // back inside the row -- Tk >= 4 here -- and re-indexed below; what lies beyond Tk is zero.
  f4u v[MAXG];
  auto vload = [&](int gb) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < MAXG; ++u) {
      const int jl = 8 * (gb + u) + 4 * half;
      if (gb + u < g1) v[u] = *reinterpret_cast<const f4u*>(vrow + max(min(jl, Tk - 4), 0));
    }
  };
  vload(g0);
  // ---- row softmax, 32 / NW rows per wave, walked in LOCKSTEP: a wave-wide reduction is six dependent cross-lane
  // steps of ~150 cycles each, and the rows' chains are independent (in-kernel stamps: row after row this phase was
  // 2.9 us of a 9-us launch at 16 keys).  P is left un-normalised, 1 / sum goes to the output.
  const int ncol = nkb * 32;                          // columns written above (the padding holds -3e38 -> 0)
  {
    constexpr int NR = 32 / NW;
    float* rows[NR];
    float mx[NR], sum[NR];
#pragma unroll
    for (int u = 0; u < NR; ++u) {
      rows[u] = S + (wave * NR + u) * sp;
      mx[u] = -3.0e38f;
      sum[u] = 0.0f;
    }
    for (int j = lane; j < ncol; j += 64) {
#pragma unroll
      for (int u = 0; u < NR; ++u) mx[u] = fmaxf(mx[u], rows[u][j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int u = 0; u < NR; ++u) mx[u] = fmaxf(mx[u], __shfl_xor(mx[u], o, 64));
    }
    for (int j = lane; j < ncol; j += 64) {
#pragma unroll
      for (int u = 0; u < NR; ++u) {
        const float sv = rows[u][j];
        const float e = sv > -1.0e38f ? hsp_exp2e(sv - mx[u]) : 0.0f;
        rows[u][j] = e;
        sum[u] += e;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int u = 0; u < NR; ++u) sum[u] += __shfl_xor(sum[u], o, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < NR; ++u) inv_s[wave * NR + u] = 1.0f / sum[u];
    }
  }
  // zero the columns [ncol, ncol8) the PV groups of eight keys may read
  {
    const int ncol8 = (ncol + 7) & ~7;
    for (int e = tid; e < 32 * (ncol8 - ncol); e += 64 * NW) S[(e / (ncol8 - ncol)) * sp + ncol + e % (ncol8 - ncol)] = 0.0f;
  }
  MT_STAMP(3);
  __syncthreads();
  MT_STAMP(4);
  // ---- O^T += V P^T
  mha_f32x16 oacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) oacc[r] = 0.0f;
  if (kh2 < KH) {
    const float* prow = S + l32 * sp + 4 * half;
    const int glast = ngrp - 1;                       // the only group whose window may have been moved back
    for (int gb = g0; gb < g1; gb += MAXG) {
      if (gb > g0) vload(gb);
      if (!dok) {                                     // head-dim rows beyond D (last block only): contribute nothing
#pragma unroll
        for (int u = 0; u < MAXG; ++u) v[u] = f4u{0.0f, 0.0f, 0.0f, 0.0f};
      }
      float pc[4], pn[4];                             // P fragments of the current / next group
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) pc[qq] = prow[8 * gb + qq];
#pragma unroll
      for (int u = 0; u < MAXG; ++u) {
        if (gb + u < g1) {
          if (gb + u + 1 < g1) {
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) pn[qq] = prow[8 * (gb + u + 1) + qq];
          }
          f4u vv = v[u];
          if (gb + u == glast) {                      // wave-uniform: re-index the moved window, zero what lies beyond Tk
            const int jl = 8 * (gb + u) + 4 * half;
            const int sh = jl - max(min(jl, Tk - 4), 0);
            float t4[4];
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
              const int idx = qq + sh;
              t4[qq] = idx == 0 ? vv[0] : idx == 1 ? vv[1] : idx == 2 ? vv[2] : idx == 3 ? vv[3] : 0.0f;
            }
            vv = f4u{t4[0], t4[1], t4[2], t4[3]};
          }
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(vv[qq], pc[qq], oacc, 0, 0, 0);
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) pc[qq] = pn[qq];
        }
      }
    }
    if (KH == 2 && kh2 == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[(db * 16 + r) * 64 + lane] = oacc[r];
    }
  }
  MT_STAMP(5);
  if (KH == 2) __syncthreads();
  MT_STAMP(6);
  if (kh2 == 0 && i0 + l32 < Tq) mha_store_o<KH == 2>(t, D, db, l32, half, oacc, inv_s[l32], red + db * 16 * 64 + lane);
  MT_STAMP(7);
#undef MT_STAMP
}


// ---------------------------------------------------------------------------------------
// THE decision: validation, defaults, and which kernel with which launch shape serves the struct.  hsp_mha_f32 launches
// what this returns and hsp_mha_plan reports it; nothing else chooses.  `a` comes back with the defaults filled in and
// the force-stream hook decoded (window >= 0).
int mha_decide(hsp_mha_args& a, mha_choice& c) {
  if (a.q_cs == 0) a.q_cs = a.Tq;
  if (a.k_cs == 0) a.k_cs = a.Tk;
  if (a.v_cs == 0) a.v_cs = a.Tk;
  if (a.o_cs == 0) a.o_cs = a.Tq;
  if (a.q_cs < a.Tq || a.k_cs < a.Tk || a.v_cs < a.Tk || a.o_cs < a.Tq) return HSP_EINVAL;
  if (!a.q || !a.k || !a.v || !a.o || a.B <= 0 || a.H <= 0 || a.D <= 0 || a.Tq <= 0 || a.Tk <= 0) return HSP_EINVAL;
  if (a.D > 256) return HSP_EINVAL;   // every path: the key-streaming window kernel holds two 128-channel accumulator sets
  if ((a.mask_q == nullptr) != (a.mask_k == nullptr)) return HSP_EINVAL;
  // test hook: window = -(w + 1) selects the key-streaming kernels at any Tk, with window w
  const bool force_stream = a.window < 0;
  if (force_stream) a.window = -(a.window + 1);
  const int ndb32 = (a.D + 31) / 32;
  auto grid = [&](int qt) {
    c.n_qt = (a.Tq + qt - 1) / qt;
    c.blocks = (int64_t)c.n_qt * a.H * a.B;
    return c.blocks > 0 && c.blocks <= 0x7fffffff;
  };
  auto tok = [&]() {
    c.kernel = HSP_MHA_TOK;
    c.ndb = ndb32 < 3 ? ndb32 : 3;
    c.sp = tok_sp(a.Tk);
    c.lds = tok_layout<int64_t>(c.sp, c.ndb, TOK_NW).total * (int64_t)sizeof(float);
    return grid(TQT) ? 0 : HSP_EINVAL;
  };
  c = mha_choice{};
#ifdef HSP_TUNING
  // in-kernel phase stamps of workgroup 0 -> rel_v (8 x uint64): tools/mha_stamps.py.  Inside TOK's own range only: its LDS limit is raised for Tk <= 256
  if (a.window == 1003 && a.rel_v && !a.rel_k && a.Tk >= 4 && a.Tk <= 256 && a.D <= 96) return tok();
#endif
  if ((a.rel_k || a.rel_v) && (a.window <= 0 || a.Tq != a.Tk)) return HSP_EINVAL;
  if (a.mask_dense && a.mask_dense_bs < (int64_t)a.Tq * a.Tk) return HSP_EINVAL;
  // matrix-core path: no relative-position window, head dim <= 128.  The whole-row kernel while the scores of 32
  // queries fit LDS, the key-streaming one (online softmax) beyond
  if (!a.rel_k && !a.rel_v && a.D <= 128) {
    // no masks, at most 256 keys: the latency-oriented kernel
    if (!force_stream && !a.mask_q && !a.mask_dense && a.Tk >= 4 && a.Tk <= 256 && a.D <= 96) return tok();
    if (!grid(MQT)) return HSP_EINVAL;
    c.ndb = ndb32;
    const int DP = ndb32 * 32;
    if (!force_stream) {
      c.sp = ((a.Tk + 31) & ~31) + 33;  // odd pitch, room for one zero slab column block
      const int vp = ((a.Tk + 63) & ~63) + 1;
      const int64_t lds_whole = mfma_layout<int64_t>(DP, c.sp, vp, false).total * (int64_t)sizeof(float);
      const int64_t lds_slab = mfma_layout<int64_t>(DP, c.sp, SLAB_VP, false).total * (int64_t)sizeof(float);
      // whole-V needs one round trip less per 64 keys but more LDS: with more workgroups than CUs prefer the
      // footprint that lets two of them share a CU (their latencies then overlap instead of queueing)
      const bool whole = lds_whole <= 160 * 1024 && (c.blocks <= 256 || lds_whole <= 80 * 1024 || lds_slab > 80 * 1024);
      if (whole || lds_slab <= 160 * 1024) {
        c.kernel = whole ? HSP_MHA_MFMA_WHOLE : HSP_MHA_MFMA_SLAB;
        c.vp = whole ? vp : SLAB_VP;
        c.lds = whole ? lds_whole : lds_slab;
        return 0;
      }
    }
    c.kernel = HSP_MHA_MFMA_STREAM;
    c.sp = SKB + 1;
    c.vp = SKB + 1;
    c.lds = mfma_layout<int64_t>(DP, c.sp, c.vp, true).total * (int64_t)sizeof(float);
    return 0;
  }
  // scalar kernels: a relative-position window, or head dim 129 .. 256
  if (!grid(QT)) return HSP_EINVAL;
  c.ndb = (a.D + 127) / 128;
  c.dpad = (a.D < 128 ? a.D : 128) | 1;
  c.sp = a.Tk + 1;
  c.lds = row_layout<int64_t>(a.D, c.sp, c.dpad, false).total * (int64_t)sizeof(float);
  c.kernel = HSP_MHA_ROW;
  if (c.lds > 160 * 1024 || force_stream) {
    c.kernel = HSP_MHA_ROW_STREAM;
    c.sp = WKB + 1;
    c.lds = row_layout<int64_t>(a.D, c.sp, c.dpad, true).total * (int64_t)sizeof(float);
  }
  return 0;
}

// The kernels that are built per head-dim block count.  TOK is raised once per device, so to its maximum (Tk = 256),
// not to this launch's size; the MFMA streaming kernel's size does not depend on the launch.
template <int NDB>
int mha_launch_ndb(const hsp_mha_args& a, const mha_choice& c, hipStream_t st) {
  const int lds = (int)c.lds;
  switch (c.kernel) {
    case HSP_MHA_TOK:
      if constexpr (NDB <= 3) {
        constexpr int kMaxLds = tok_layout<int>(tok_sp(256), NDB, TOK_NW).total * (int)sizeof(float);
        return hsp_launch<mha_tok_kernel<NDB, TOK_NW>>(c.blocks, 64 * TOK_NW, lds, kMaxLds, st, a, c.n_qt, c.sp);
      }
      return HSP_EINVAL;   // mha_decide gives TOK at most three blocks
    case HSP_MHA_MFMA_WHOLE: return hsp_launch<mha_mfma_kernel<NDB, true>>(c.blocks, 256, lds, 160 * 1024, st, a, c.n_qt, c.sp, c.vp);
    case HSP_MHA_MFMA_SLAB: return hsp_launch<mha_mfma_kernel<NDB, false>>(c.blocks, 256, lds, 160 * 1024, st, a, c.n_qt, c.sp, c.vp);
    default: return hsp_launch<mha_mfma_stream_kernel<NDB>>(c.blocks, 256, lds, lds, st, a, c.n_qt);
  }
}

}  // namespace

extern "C" int hsp_mha_plan(const hsp_mha_args* ap, int32_t out4[4]) {
  if (!ap || !out4) return HSP_EINVAL;
  hsp_mha_args a = *ap;
  mha_choice c;
  if (int e = mha_decide(a, c)) return e;
  out4[0] = c.kernel;
  out4[1] = c.ndb;
  out4[2] = (int32_t)c.lds;
  out4[3] = (int32_t)c.blocks;
  return 0;
}

extern "C" int hsp_mha_f32(const hsp_mha_args* ap, void* stream) {
  if (!ap) return HSP_EINVAL;
  hsp_mha_args a = *ap;
  mha_choice c;
  if (int e = mha_decide(a, c)) return e;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (c.kernel == HSP_MHA_ROW) return hsp_launch<mha_kernel>(c.blocks, ATT_THREADS, (int)c.lds, 160 * 1024, st, a, c.n_qt, c.dpad, c.sp);
  if (c.kernel == HSP_MHA_ROW_STREAM)
    return hsp_launch<mha_stream_kernel>(c.blocks, ATT_THREADS, (int)c.lds, 160 * 1024, st, a, c.n_qt, c.dpad);
  switch (c.ndb) {
    case 1: return mha_launch_ndb<1>(a, c, st);
    case 2: return mha_launch_ndb<2>(a, c, st);
    case 3: return mha_launch_ndb<3>(a, c, st);
    default: return mha_launch_ndb<4>(a, c, st);
  }
}
