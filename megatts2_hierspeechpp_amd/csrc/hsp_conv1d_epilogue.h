// The EPILOGUES of the fused conv kernel, one per HSP_EPI_* kind, on the accumulator registers of a consumer wave
// (part of hsp_conv1d_mfma_kernel.h), with what they share with the rest of the consumer role: where a lane's
// accumulators sit in the output (ConsLane, fold_lane) and the loops over the accumulator file (for_acc and friends).
// HSP_EPI_INIT's stores are in conv_consume (hsp_conv1d_consume.h says why).  HSP_EPI_ACT (EpiAct, at the end) is the one epilogue the producer waves take part in.
#pragma once

namespace hspconv {

// ---- loops over the accumulator file acc[TM][TN] of 32 x 32 blocks, 16 registers each.  Every index reaches `f` as a
// std::integral_constant (`constexpr int i = ii;`): a runtime index into acc[][] would demote the whole accumulator
// file to scratch memory.
template <int TM, int TN, class F>
__device__ __forceinline__ void for_blocks(F&& f) {   // f(i, n): blocks, column block fastest
  static_for<TM>([&](auto ii) __attribute__((always_inline)) {
    static_for<TN>([&](auto nn) __attribute__((always_inline)) { f(ii, nn); });
  });
}
template <class F>
__device__ __forceinline__ void for_regs(F&& f) {     // f(r): the 16 registers (rows HSP_ACC_ROW(r, half)) of a block
  static_for<16>(f);
}
template <int TM, int TN, class F>
__device__ __forceinline__ void for_acc(F&& f) {      // f(i, n, r): every accumulator, register fastest
  for_blocks<TM, TN>([&](auto ii, auto nn) __attribute__((always_inline)) {
    static_for<16>([&](auto rr) __attribute__((always_inline)) { f(ii, nn, rr); });
  });
}
// ---- where a consumer lane works.  Its wave owns a (TM x TN) grid of 32 x 32 blocks at packed rows mw, tile columns
// wcol; register r of block (i, n) is row mw + 32 i + HSP_ACC_ROW(r, half), column tw + 32 n of utterance bl.
struct ConsLane {
  int lane, l32, half;
  int slot;         // the wave's number among its K group's waves: the VEC epilogue's staging slot, the K-split's partner
  int mw, wcol;     // first packed row of the wave; its first column within the tile
  int b, t0, ts0;   // the tile: utterance and first column (FOLD: first VIRTUAL column, at time ts0 of utterance b)
  int bl, tw;       // this lane's utterance and its column in block n = 0
  int xfold;        // FOLD: where the lane's column sits in the LDS window, less the column
};

// Folded columns: utterance `bl` and time `t` of column `col` of the tile, and the piece of the window it lies in.  A
// column past the last virtual column gets a legal address -- the last utterance -- and a time no epilogue stores at.
// Not FOLD: bl and t stay what the caller set (the tile's utterance, t0 + col).
template <bool FOLD>
__device__ __forceinline__ void fold_lane(const hsp_conv1d_args& a, int b, int ts0, int col, int& bl, int& t, int& piece) {
  piece = 0;
  if constexpr (FOLD) {
    fold_col(col, ts0, a.ncols, piece, t);
    bl = b + piece;
    if (bl >= a.B) {
      bl = a.B - 1;
      t = a.ncols;
    }
  }
}

// ---- HSP_EPI_VEC (plain rows, 16-B aligned tensors, any pointwise tail): each 32x32 accumulator
// block is transposed through this wave's LDS staging area (the weight buffers are free after the
// last barrier) so that a lane owns 4 consecutive time steps of 4 rows -> float4 residual /
// accumulate loads and float4 stores.
template <bool FOLD, int TM, int TN>
__device__ __forceinline__ void epi_vec(const hsp_conv1d_args& a, const ConsLane& L, float* const lds,
                                        const f32x16 (&acc)[TM][TN]) {
  constexpr int ESTR = 36;
  float* const stage = lds + L.slot * (32 * ESTR);
  const int er = L.lane >> 3, ec = (L.lane & 7) * 4;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  // utterance and time of this lane's four columns (FOLD: ncols % 4 == 0, a group of four never straddles a seam)
  int bv = L.b, tv = L.t0 + L.wcol + ec, piece;
  fold_lane<FOLD>(a, L.b, L.ts0, L.wcol + ec, bv, tv, piece);
  static_for<TM>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = ii;
    float add[4], cs[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = L.mw + i * 32 + er + 8 * q;
      add[q] = 0.0f;
      cs[q] = a.scale;
      if (co < a.Cout) {
        if (a.bias) add[q] = a.bias[co];
        if (a.cbias) add[q] += a.cbias[(int64_t)bv * a.cbias_bs + co];
        if (a.cscale) cs[q] *= a.cscale[(int64_t)bv * a.cscale_bs + co];
      }
    }
    static_for<TN>([&](auto nn) __attribute__((always_inline)) {
      constexpr int n = nn;
      const int t = tv + n * 32;
      const bool tok = t < a.ncols;
      float4 rs[4], yo[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = L.mw + i * 32 + er + 8 * q;
        const bool ok = tok && co < a.Cout;
        rs[q] = z4;
        yo[q] = z4;
        if (ok && a.res) rs[q] = *reinterpret_cast<const float4*>(a.res + (int64_t)bv * a.res_bs + (int64_t)co * a.res_cs + t);
        if (ok && a.accumulate) yo[q] = *reinterpret_cast<const float4*>(a.y + (int64_t)bv * a.y_bs + (int64_t)co * a.y_cs + t);
      }
      float4 mk = make_float4(1.f, 1.f, 1.f, 1.f);
      if (a.mask_mode != HSP_MASK_NONE && tok) mk = *reinterpret_cast<const float4*>(a.mask + (int64_t)bv * a.mask_bs + t);
      for_regs([&](auto rr) __attribute__((always_inline)) {
        constexpr int r = rr;
        stage[HSP_ACC_ROW(r, L.half) * ESTR + L.l32] = acc[i][n][r];
      });
      wave_lds_fence();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int co = L.mw + i * 32 + er + 8 * q;
        if (tok && co < a.Cout) {
          const float4 v = *reinterpret_cast<const float4*>(stage + (er + 8 * q) * ESTR + ec);
          float e[4] = {v.x, v.y, v.z, v.w};
          const float r4[4] = {rs[q].x, rs[q].y, rs[q].z, rs[q].w};
          const float y4[4] = {yo[q].x, yo[q].y, yo[q].z, yo[q].w};
          const float m4[4] = {mk.x, mk.y, mk.z, mk.w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            float x = hsp_apply_act(e[u] + add[q], a.act);
            if (a.mask_mode & HSP_MASK_PRE) x *= m4[u];
            x = fmaf(x, cs[q], r4[u]);
            if (a.mask_mode & HSP_MASK_POST) x *= m4[u];
            e[u] = (x + y4[u]) * a.post_scale;
          }
          *reinterpret_cast<float4*>(a.y + (int64_t)bv * a.y_bs + (int64_t)co * a.y_cs + t) =
              make_float4(e[0], e[1], e[2], e[3]);
        }
      }
      wave_lds_fence();  // the staging area is rewritten by the next block
    });
  });
}

// ---- HSP_EPI_GATE: gated rows (WN / GLU); blocks i, i + 1 hold the 'a' and 'b' halves of 32 channels
template <int TM, int TN>
__device__ __forceinline__ void epi_gate(const hsp_conv1d_args& a, const ConsLane& L, const f32x16 (&acc)[TM][TN]) {
  static_assert(TM % 2 == 0, "gated rows need both halves of a channel in one wave");
  const int H = a.gate_half;
  static_for<TM / 2>([&](auto ih) __attribute__((always_inline)) {
    constexpr int i = 2 * ih;
    const int mpair = L.mw + i * 32;  // packed row of the 'a' block; multiple of 64
    static_for<TN>([&](auto nn) __attribute__((always_inline)) {
      constexpr int n = nn;
      const int t = L.tw + n * 32;
      if (mpair < a.M && t < a.ncols) {
        for_regs([&](auto rr) __attribute__((always_inline)) {
          constexpr int r = rr;
          const int co = (mpair >> 6) * 32 + HSP_ACC_ROW(r, L.half);
          if (co < H) {
            float va = acc[i][n][r], vb = acc[i + 1][n][r];
            if (a.bias) { va += a.bias[co]; vb += a.bias[H + co]; }
            if (a.cbias) {
              va += a.cbias[(int64_t)L.bl * a.cbias_bs + co];
              vb += a.cbias[(int64_t)L.bl * a.cbias_bs + H + co];
            }
            const float v = (a.rows == HSP_ROWS_GATE_WN ? hsp_tanh(va) : va) * hsp_sigmoid(vb);
            hsp_epilogue_store(a, L.bl, co, t, v);
          }
        });
      }
    });
  });
}

// ---- ConvTranspose (HSP_ROWS_SHUFFLE): packed row m = co * up + phase writes y[co, up * t + phase - shuf_pad].
// The row map for ANY `up`, used by the scalar SHUF path: co = m / up through the float reciprocal (exact for
// m < 2^22, no integer divide).  epi_gen states the same two lines itself: through this helper the GEN kernels with the
// ACT1D prologue compile to one more wait per chunk in the consumer loop's header.  The vector path of epi_shuf
// (up = 2 / 4) takes co = m >> log2(up) instead: different arithmetic on purpose, its groups of `up` adjacent registers
// need no phase at all.
__device__ __forceinline__ void convtr_row(const hsp_conv1d_args& a, float up_inv, int m, int& co, int& phase) {
  co = (int)(((float)m + 0.5f) * up_inv);
  phase = m - co * a.up;
}

// ---- HSP_EPI_SHUF: ConvTranspose fast path, bias only.  Row
// constants (channel, phase, bias, row pointer) are resolved once per accumulator row; the
// store loop has no loads, so nothing ever waits on vmcnt.  The `up` stores of one channel
// (registers r&3 for up = 4, r&1 for up = 2) interleave into full lines in L2.
// (round 4) stride 4 / stride 2 with a whole number of channels per register group: the `up` phases of a channel
// sit in ADJACENT accumulator registers of one lane (rows r & 3 of a group of four) and land on `up` consecutive
// output samples, so they leave as ONE 16-B / 8-B store per lane -- lanes are consecutive t, a store instruction
// covers 512 / 256 contiguous bytes -- instead of `up` scalar stores at a 16-B / 8-B lane stride that only merge
// into full lines in L2 (4 x / 2 x the store instructions; the stride-2 launches of the Generator ran at 57 and 79
// TFLOP/s on them).  The first / last output group of a row (phases shifted outside [0, Lout) by the transposed
// conv's padding) takes scalar stores.
template <int TM, int TN>
__device__ __forceinline__ void epi_shuf_vec(const hsp_conv1d_args& a, const ConsLane& L, const f32x16 (&acc)[TM][TN]) {
  typedef float st4 __attribute__((ext_vector_type(4), aligned(4)));
  typedef float st2 __attribute__((ext_vector_type(2), aligned(4)));
  const float sc = a.scale * a.post_scale;
  const int upl = a.up == 4 ? 2 : 1;               // log2(up)
  static_for<TM>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = ii;
    // register group q = r >> 2 holds rows mw + i * 32 + 8 q + 4 half + (0..3): one channel (up = 4) or two (up = 2)
    float* yrow[4][2];
    float bz[4][2];
    bool rok[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const int m = L.mw + i * 32 + 8 * q + 4 * L.half + 2 * c2;      // up = 2: channel c2 of the group; up = 4: c2 = 0 only
        const int co = m >> upl;
        rok[q][c2] = m < a.M && co < a.Cout;
        yrow[q][c2] = a.y + (int64_t)L.bl * a.y_bs + (int64_t)(rok[q][c2] ? co : 0) * a.y_cs;
        bz[q][c2] = (rok[q][c2] && a.bias) ? a.bias[co] : 0.0f;
      }
    static_for<TN>([&](auto nn) __attribute__((always_inline)) {
      constexpr int n = nn;
      const int t = L.tw + n * 32;
      if (t < a.ncols) {
        const int to0 = a.up * t - a.shuf_pad;
        const bool inside = to0 >= 0 && to0 + a.up <= a.Lout;
        static_for<4>([&](auto qq) __attribute__((always_inline)) {
          constexpr int q = qq;
          if (a.up == 4) {
            if (rok[q][0]) {
              const st4 v = {(acc[i][n][4 * q] + bz[q][0]) * sc, (acc[i][n][4 * q + 1] + bz[q][0]) * sc,
                             (acc[i][n][4 * q + 2] + bz[q][0]) * sc, (acc[i][n][4 * q + 3] + bz[q][0]) * sc};
              if (inside) *reinterpret_cast<st4*>(yrow[q][0] + to0) = v;
              else {
#pragma unroll
                for (int ph = 0; ph < 4; ++ph)
                  if (to0 + ph >= 0 && to0 + ph < a.Lout) yrow[q][0][to0 + ph] = v[ph];
              }
            }
          } else {
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) {
              if (rok[q][c2]) {
                const st2 v = {(acc[i][n][4 * q + 2 * c2] + bz[q][c2]) * sc, (acc[i][n][4 * q + 2 * c2 + 1] + bz[q][c2]) * sc};
                if (inside) *reinterpret_cast<st2*>(yrow[q][c2] + to0) = v;
                else {
#pragma unroll
                  for (int ph = 0; ph < 2; ++ph)
                    if (to0 + ph >= 0 && to0 + ph < a.Lout) yrow[q][c2][to0 + ph] = v[ph];
                }
              }
            }
          }
        });
      }
    });
  });
}

template <int TM, int TN>
__device__ __forceinline__ void epi_shuf(const hsp_conv1d_args& a, const ConsLane& L, const f32x16 (&acc)[TM][TN]) {
  if ((a.up == 4 || a.up == 2) && !HSP_DBG(a, HSP_CV_SHUF_SCALAR)) return epi_shuf_vec(a, L, acc);
  const float up_inv = 1.0f / (float)a.up;
  static_for<TM>([&](auto ii) __attribute__((always_inline)) {
    constexpr int i = ii;
    float* yrow[16];
    float bz[16];
    int toff[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = L.mw + i * 32 + HSP_ACC_ROW(r, L.half);
      int co, phase;
      convtr_row(a, up_inv, m, co, phase);
      const bool ok = m < a.M && co < a.Cout;
      toff[r] = ok ? phase - a.shuf_pad : -(1 << 30);
      yrow[r] = a.y + (int64_t)L.bl * a.y_bs + (int64_t)(ok ? co : 0) * a.y_cs;
      bz[r] = (ok && a.bias) ? a.bias[co] : 0.0f;
    }
    static_for<TN>([&](auto nn) __attribute__((always_inline)) {
      constexpr int n = nn;
      const int t = L.tw + n * 32;
      if (t < a.ncols) {
        for_regs([&](auto rr) __attribute__((always_inline)) {
          constexpr int r = rr;
          const int to = a.up * t + toff[r];
          if (to >= 0 && to < a.Lout) yrow[r][to] = (acc[i][n][r] + bz[r]) * a.scale * a.post_scale;
        });
      }
    });
  });
}

// ---- HSP_EPI_GEN: everything else, one element at a time (hsp_epilogue_store)
template <int TM, int TN>
__device__ __forceinline__ void epi_gen(const hsp_conv1d_args& a, const ConsLane& L, const f32x16 (&acc)[TM][TN]) {
  const float up_inv = a.rows == HSP_ROWS_SHUFFLE ? 1.0f / (float)a.up : 1.0f;
  for_blocks<TM, TN>([&](auto ii, auto nn) __attribute__((always_inline)) {
    constexpr int i = ii, n = nn;
    const int t = L.tw + n * 32;
    if (t < a.ncols) {
      for_regs([&](auto rr) __attribute__((always_inline)) {
        constexpr int r = rr;
        const int m = L.mw + i * 32 + HSP_ACC_ROW(r, L.half);
        int co = m, to = t;
        bool ok = m < a.M;
        if (a.rows == HSP_ROWS_SHUFFLE) {
          co = (int)(((float)m + 0.5f) * up_inv);  // m / up, exact for m < 2^22 (no integer divide)
          to = a.up * t + (m - co * a.up) - a.shuf_pad;
          ok = ok && to >= 0 && to < a.Lout;
        }
        ok = ok && co < a.Cout;
        if (ok) {
          float v = acc[i][n][r];
          if (a.bias) v += a.bias[co];
          if (a.cbias) v += a.cbias[(int64_t)L.bl * a.cbias_bs + co];
          v = hsp_apply_act(v, a.act);
          hsp_epilogue_store(a, L.bl, co, to, v);
        }
      });
    }
  });
}

// ---- HSP_EPI_ACT (hsp_conv1d_args.act == HSP_ACT_ACT1D): the NEXT Activation1d of an AMP pair, applied to the conv's own output
// rows before they leave the workgroup.  Plain direct conv, bias only, on the 32 x 512 / 64 x 256 plain-prologue shapes
// (WM == 1: every consumer wave holds all BM rows of its BN / 4 columns).  Column tiles advance by SEG = BN - 16: the
// tile computes conv columns [p0 - 8, p0 - 8 + BN), p0 = nt SEG -- the raw window of the stand-alone kernel's segment
// [p0, p0 + SEG) (act1d_seg_kernel, hsp_pointwise.hip; at BN = 512 its very geometry) -- and stores the activated columns
// [p0, min(p0 + SEG, L)).  The accumulators start at the bias, as HSP_EPI_INIT's do, and the K loop is the plain one: a
// conv column is bit for bit what the plain launch stores.  The arithmetic behind it is hsp_act1d_arith.h's.
//
// The tile goes through LDS RP rows at a time -- 16 at BN = 512 (registers 8 rh .. 8 rh + 7 of a 32 x 32 block are rows
// 16 rh .. 16 rh + 15), a whole block at BN = 256 -- into the chunk buffers, which are free behind the K loop's last barrier (every fragment read is retired, no
// DMA is in flight).  ALL waves of the workgroup then take rows (the producers stay for this): a wave owns whole rows
// and its own 2x-rate buffer, so the phases of a row need wave-local ordering only, as in the stand-alone kernel.
//   LDS: stage[RP][BN] + a2[waves][RIF][2 BN + 16] floats = 66 048 B at BN = 512 (RP 16, RIF 1), 66 560 B at BN = 256
//   (RP 32, RIF 2: two rows of a wave in flight): under the 80 KB of two workgroups per CU; launch_one requests the larger
//   of this and the K loop's plan.
template <class C>
struct EpiAct {
  static_assert(C::kWM == 1 && C::kKS == 1 && C::BM % 32 == 0 && C::BN % 256 == 0, "whole rows per consumer wave; float4 row images");
  static constexpr int BN = C::BN, SEG = C::BN - 16;   // conv columns / activated columns of a tile
  // Rows of a wave IN FLIGHT: a row is a chain of LDS round trips (raw -> FIR -> a2 -> FIR -> store) and a wave has one
  // neighbour per SIMD to hide them behind.  At BN = 256 a row is half as long and a tile has twice as many: two rows
  // walk the phases together there, each with its own 2x-rate buffer (one row at a time: 64 -> 64 channels k = 3 at
  // 32 x 32 000 was 24 us SLOWER fused than as two launches, profiles/epi_act_bench.txt).  At BN = 512 the second buffer
  // does not fit the 80 KB of two workgroups per CU.
  static constexpr int RIF = BN <= 256 ? 2 : 1;
  static constexpr int RP = BN <= 256 ? 32 : 16;       // rows per pass: a whole 32-row block, or the half of registers 8 rh ...
  static constexpr int NPASS = C::BM / RP;
  static constexpr int NW = C::THREADS / 64;           // waves that take rows: all of them
  static constexpr int A2W = 2 * BN + 16;              // one 2x-rate buffer (ACT2_A2 at BN = 512)
  static constexpr int NV = BN / 256;                  // float4s of a raw row per lane
  static constexpr int NC = (SEG / 2 + 63) / 64;       // phase-C iterations
  static constexpr int LDS_FLOATS = RP * BN + NW * RIF * A2W;
  static_assert(RP % (NW * RIF) == 0 && LDS_FLOATS * 4 <= 80 * 1024, "every wave has RIF rows per round; two workgroups per CU");

  // rows `wave` + NW j, j < RIF, of every round of pass `pass`: replicate padding, up-2 FIR -> SnakeBeta -> down-2 FIR,
  // stores.  A row past Cout (a launch with Cout < BM) walks along on the finite values the MFMAs left and stores nothing.
  static __device__ __forceinline__ void rows(const hsp_conv1d_args& a, float* const lds, int b, int m0, int t0, int pass,
                                              int wave, int lane, const act_f32x2 (&hu)[6], const act_f32x2 (&hd)[6]) {
    const int L = a.ncols;
    const int p0 = t0 + 8;                   // the tile's first activated column; p0 < L (launch_one's tile count)
    const int n_out = min(SEG, L - p0);      // multiple of 4
    for (int rl = wave; rl < RP; rl += NW * RIF) {
      const int co0 = m0 + pass * RP + rl;
      if (co0 >= a.Cout) break;              // wave-uniform
      float* raw[RIF];                       // raw[j][c] = conv column p0 - 8 + c of row co0 + NW j
      float* a2[RIF];
      float kf[RIF], kb[RIF];
      bool ok[RIF];
#pragma unroll
      for (int j = 0; j < RIF; ++j) {
        const int co = co0 + NW * j;
        ok[j] = co < a.Cout;
        raw[j] = lds + (rl + NW * j) * BN;
        a2[j] = lds + RP * BN + (wave * RIF + j) * A2W;
        kf[j] = a.alpha_exp[min(co, a.Cout - 1)] * 0.318309886183790672f;
        kb[j] = 0.5f * a.beta_inv[min(co, a.Cout - 1)];
      }
      // ---- phase A: the replicate padding of the raw row, xt[0] left of column 0 and xt[L - 1] from column L on (the
      // MFMAs computed something there: a conv of the zero padding).  L % 4 == 0 and p0 % 4 == 0: whole float4s.
      if (p0 == 0 || p0 - 8 + BN > L) {      // wave-uniform
#pragma unroll
        for (int j = 0; j < RIF; ++j) {
          const float x0 = raw[j][8];
          const float xl = raw[j][min(L - 1 - p0 + 8, BN - 1)];
          float4 t[NV];
#pragma unroll
          for (int v = 0; v < NV; ++v) t[v] = *reinterpret_cast<const float4*>(raw[j] + 4 * (lane + 64 * v));
          asm volatile("" ::: "memory");
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            const int idx = p0 - 8 + 4 * (lane + 64 * v);
            t[v] = idx < 0 ? make_float4(x0, x0, x0, x0) : t[v];
            t[v] = idx >= L ? make_float4(xl, xl, xl, xl) : t[v];
            *reinterpret_cast<float4*>(raw[j] + 4 * (lane + 64 * v)) = t[v];
          }
        }
        asm volatile("" ::: "memory");
      }
      // ---- phase B: slots [0, 2 n_out + 10) of the 2x-rate signal
      const int npairs = (2 * n_out + 13) >> 2;
#pragma unroll 2
      for (int pi = lane; pi < npairs; pi += 64) {
#pragma unroll
        for (int j = 0; j < RIF; ++j) HSP_ACT2_UP(a2[j], raw[j], pi, hu, kf[j], kb[j])
      }
      asm volatile("" ::: "memory");
      // replicate padding of the 2x-rate signal: a[-5 .. -1] = a[0], a[2L .. 2L+4] = a[2L-1]
      if (p0 == 0 || p0 + n_out == L) {
#pragma unroll
        for (int j = 0; j < RIF; ++j) {
          if (p0 == 0 && lane < 5) a2[j][lane] = a2[j][5];
          if (p0 + n_out == L && lane >= 8 && lane < 13) a2[j][2 * n_out + lane - 3] = a2[j][2 * n_out + 4];
        }
        asm volatile("" ::: "memory");
      }
      // ---- phase C: two outputs per lane, non-temporal (the next conv reads them from HBM / Infinity Cache anyway)
      float* const yrow = a.y + (int64_t)b * a.y_bs + (int64_t)co0 * a.y_cs + p0;
#pragma unroll
      for (int it = 0; it < NC; ++it) {
        const int l2 = lane + 64 * it;
        if (2 * l2 >= n_out) continue;
#pragma unroll
        for (int j = 0; j < RIF; ++j) {
          float2 yo;
          HSP_ACT2_DOWN(yo, a2[j], l2, hd)
          if (ok[j])
            __builtin_nontemporal_store(act_f32x2{yo.x, yo.y}, reinterpret_cast<act_f32x2*>(yrow + (int64_t)(NW * j) * a.y_cs + 2 * l2));
        }
      }
      asm volatile("" ::: "memory");   // raw / a2 are rewritten by the next round
    }
  }

  // the producer waves' part: the consumers' barriers, and their share of the rows
  static __device__ __forceinline__ void producer(const hsp_conv1d_args& a, float* const lds, int b, int m0, int t0,
                                                  int wave, int lane) {
    act_f32x2 hu[6], hd[6];
    HSP_ACT2_TAPS(a.filt, hu, hd)
    for (int pass = 0; pass < NPASS; ++pass) {
      lds_barrier();                           // the pass's rows are staged
      rows(a, lds, b, m0, t0, pass, wave, lane, hu, hd);
      if (pass + 1 < NPASS) lds_barrier();     // ... and read: the stage may be rewritten
    }
  }

  // the consumer waves' part: stage RP rows of the accumulators -- registers RP / 2 of a 32 x 32 block -- then rows like
  // everybody
  template <int TM, int TN>
  static __device__ __forceinline__ void consumer(const hsp_conv1d_args& a, const ConsLane& L, float* const lds, int m0,
                                                  int wave, const f32x16 (&acc)[TM][TN]) {
    static_assert(TM * 32 == NPASS * RP, "the passes cover the wave's blocks");
    act_f32x2 hu[6], hd[6];
    HSP_ACT2_TAPS(a.filt, hu, hd)
    float* const col = lds + L.wcol + L.l32;
    static_for<NPASS>([&](auto pp) __attribute__((always_inline)) {
      constexpr int pass = pp, i = (pass * RP) / 32, row0 = (pass * RP) % 32;   // block and first row of the pass in it
      static_for<TN>([&](auto nn) __attribute__((always_inline)) {
        constexpr int n = nn;
        static_for<RP / 2>([&](auto rr) __attribute__((always_inline)) {
          constexpr int r = row0 / 2 + rr;
          col[(HSP_ACC_ROW(r, L.half) - row0) * BN + 32 * n] = acc[i][n][r];
        });
      });
      lds_barrier();
      rows(a, lds, L.b, m0, L.t0, pass, wave, L.lane, hu, hd);
      if (pass + 1 < NPASS) lds_barrier();
    });
  }
};

}  // namespace hspconv
