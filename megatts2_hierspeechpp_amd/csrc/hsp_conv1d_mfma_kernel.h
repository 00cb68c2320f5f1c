// Fused Conv1d / ConvTranspose1d as an implicit GEMM on the fp32-input matrix cores
// (v_mfma_f32_32x32x2_f32: exact fp32, k-ordered fmaf chain, same 157 TFLOP/s peak as
// the fp32 vector pipe -- MI355X_MICROARCH.md "Matrix cores").
//
//   acc[m, t] = sum_j sum_ci W[j][ci][m] * xin[ci, t + j*dil - pad]
//
// GEMM view: M = packed output rows, N = time, K = (taps x input channels).
// One workgroup owns a BM x BN output tile of one utterance and walks the input
// channels in chunks of KC.  Its waves are SPECIALISED:
//
//   waves 0-3   "consumers": each owns a (TM x TN) grid of 32x32 MFMA blocks and does
//               nothing but read A (weights) / B (shifted input window) fragments from
//               LDS -- one k-step ahead of the MFMAs that use them -- and issue MFMAs;
//   waves 4..   "producers": stage the NEXT chunk into the other half of a double
//               buffer -- the weight slab Ws[K][KC][BM] and the input window
//               Xa[KC][BN + (K-1)*dil] -- applying the PROLOGUE on the way: nothing,
//               leaky-ReLU, or the whole anti-aliased SnakeBeta activation (2x polyphase
//               up-sample -> snake -> 2x low-pass down-sample, replicate-padded at the
//               sequence ends exactly like alias_free_torch).  Each producer wave owns
//               whole channel rows, so the activation phases need only wave-local
//               ordering, and the activated tensor never exists in HBM.
//               Global loads are issued one chunk AHEAD into registers (issue early /
//               commit late), so their latency is covered by a whole chunk of MFMAs.
//
// Wave w and wave w+4 share a SIMD, so the producers' VALU/LDS/global work fills the
// issue slots between the consumers' 64-cycle MFMAs; the only workgroup-wide
// synchronisation is one barrier per chunk.  The EPILOGUE (bias, conditioning bias,
// gate / pointwise function, masks, per-channel scale, residual, running accumulation,
// ConvTranspose phase shuffle) runs on the accumulator registers of the consumers.
//
// Reference call sites: see include/hsp.h (hsp_conv1d_args).
//
// This header is the one to include: tile configuration (Cfg), LDS plan, the kernel, the host-side launch (launch_one,
// select_epilogue) and the tile list.  It includes the kernel's three parts:
//   hsp_conv1d_produce.h    producer waves: the staging routines of a chunk (the chunk loops are in the kernel below)
//   hsp_conv1d_epilogue.h   consumer waves: lane map, accumulator loops, the VEC / GATE / SHUF / GEN epilogues, the activation epilogue (all waves)
//   hsp_conv1d_consume.h    consumer waves: fragment reads, conv_consume with the INIT preload and stores and the MFMA loop
// hsp_conv1d_tile.hip instantiates the kernel once per tile shape (one translation unit each, so the build
// parallelises) and hsp_conv1d_mfma.hip holds validation and the shape / epilogue selection.
#pragma once
#include <atomic>
#include <type_traits>
#include "hsp_device.h"
#include "hsp_act1d_arith.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Tuning switches (hsp_conv1d_args.debug) exist only in the -DHSP_TUNING build (libhsp_tune.so); the
// release library refuses a non-zero debug word in validate().
#ifdef HSP_TUNING
#define HSP_DBG(a, bit) (((a).debug & (bit)) != 0)
#else
#define HSP_DBG(a, bit) false
#endif
// The conv tiles' bits of that word.  Tools, DESIGN.md and the profiles name them by NUMBER: the values stay.  The token
// GEMMs read the same word (HSP_TG_* of hsp_token_gemm.h); "TG:" marks a value that family uses too.
enum : int32_t {
  HSP_CV_ONE_CHUNK = 1,            // producers stage chunk 0 only (wrong results).  TG: HSP_TG_NO_DMA, the same meaning
  HSP_CV_NO_MFMA = 2,              // consumers skip the main loop (wrong results).  TG: HSP_TG_NO_MFMA, the same meaning
  HSP_CV_NO_EPILOGUE = 16,         // consumers skip the epilogue (wrong results).  TG: HSP_TG_RG_32x32, ANOTHER meaning
  HSP_CV_NO_INIT = 32,             // select_epilogue: VEC / GEN where INIT would do
  HSP_CV_NO_XVEC = 64,             // the 4-B window DMA whatever the input's alignment
  HSP_CV_TILE_M128 = 256,          // dispatcher: force the 128 x 128 shape (plain rows; results stay right)
  HSP_CV_NO_FAST_STAGE = 512,      // producers: never the fast staging
  HSP_CV_TILE_M64 = 1024,          // dispatcher: force the 64 x 256 shape (likewise)
  HSP_CV_NO_BARRIER = 2048,        // drop the chunk barriers (wrong results; what do they cost?  nothing measurable)
  HSP_CV_TILE_S64 = 4096,          // dispatcher: force the 64 x 64 shape (likewise)
  HSP_CV_TILE_M64P = 8192,         // dispatcher: force the 64 x 256 shape with four producer waves (likewise)
  HSP_CV_XCD_GROUPS = 16384,       // launch_one: XCD-grouped row tiles (g > 0), a measured loss
  HSP_CV_NO_TAIL = 32768,          // launch_one: no narrow consumer for the last column tile of the 128 x 128 shape
  HSP_CV_NT_STORES = 65536,        // INIT epilogue: non-temporal stores -- measured: k = 3 launches +2-4 % in isolation, step unchanged
  HSP_CV_SHUF_SCALAR = 262144,     // SHUF epilogue: the scalar phase stores of round 3.  TG: HSP_TG_BG_128x128, ANOTHER meaning
  HSP_CV_NO_HALF_CU = 1 << 21,     // launch_one: no half-CU chunk for 257 ... 512 tiles.  TG: HSP_TG_BG_64x128, ANOTHER meaning
  HSP_CV_HALF_CU_ANY = 1 << 26,    // launch_one: the half-CU chunk for ANY launch of up to 512 tiles, so that launches of different streams can share a CU
  HSP_CV_NO_S64G2 = 1 << 27,       // dispatcher: never the K-split gated tile
  HSP_CV_S64G2_512 = 1 << 28,      // dispatcher: the K-split gated tile up to 512 tiles of 64 x 128
  HSP_CV_DEEP_K3 = 1 << 29,        // launch_one: a k <= 3 conv takes the deepest chunk the whole CU can stage
};

// epilogue kinds (template parameter of the kernel: one epilogue per instantiation keeps the register
// allocation of the main loop free of the other variants' live ranges)
enum {
  HSP_EPI_INIT = 0,  // plain rows, no act / mask / cscale, scale == 1: bias + cbias + residual + running sum are
                     // loaded INTO the accumulators before the main loop; the epilogue is stores only
  HSP_EPI_VEC = 1,   // plain rows, any pointwise epilogue, 16-B addressable tensors: LDS transpose + float4
  HSP_EPI_GATE = 2,  // gated rows (WN / GLU)
  HSP_EPI_SHUF = 3,  // ConvTranspose phase shuffle, bias only
  HSP_EPI_GEN = 4,   // everything else (scalar)
  HSP_EPI_ACT = 5    // plain rows, bias only, then the next Activation1d on the tile's rows (act == HSP_ACT_ACT1D;
                     // overlapping column tiles: hsp_conv1d_epilogue.h, EpiAct)
};

namespace hspconv {

template <int WM, int WN, int TM, int TN, int NPW_, int MINW_, int XSLACK_ = 64, int KS_ = 1, bool FOLD_ = false>
struct Cfg {
  // FOLD_: the shape also carries the folded-columns form of its kernels (hsp_conv1d_args.fold_cols; "folded columns"
  // below).  The short-sequence shapes of the 50 Hz part only: every other shape compiles to what it was.
  static constexpr bool kFOLD = FOLD_;
  // KS_ > 1 (round 5): the K range of every chunk is split between KS_ groups of WM x WN consumer waves; their partial
  // sums meet in LDS behind the loop and group 0 runs the epilogue.  A short-sequence launch with fewer tiles than the chip
  // has CUs is bound by ONE tile's MFMA chain per SIMD; halving the tile and splitting its K range puts the same four SIMDs
  // of twice as many CUs on half the chain each (S64G2 below).
  static constexpr int kKS = KS_;
  static constexpr int NCW = WM * WN * KS_;        // consumer waves (4, or 8 = two per SIMD)
  static constexpr int kWM = WM, kWN = WN, kTM = TM, kTN = TN;
  static constexpr int BM = WM * TM * 32;
  static constexpr int BN = WN * TN * 32;
  static constexpr int NPW = NPW_;                 // producer waves
  static constexpr int NPT = NPW_ * 64;            // producer threads
  static constexpr int THREADS = 64 * (WM * WN * KS_ + NPW_);
  static constexpr int MINW = MINW_;               // waves per SIMD the register allocation must allow
  // LDS row pitch of the input window, a compile-time constant so that the consumer loop can reach the next
  // channel pair through ds_read immediates: BN columns + halo (K-1)*dil + 3 (the 16-B window DMA starts at the
  // aligned position below p0) must fit; a multiple of 64 (DMA instructions never straddle rows)
  static constexpr int XWP = BN + XSLACK_;
};

struct LdsPlan {
  int kc, lkc;  // chunk depth (power of two) and its log2
  int rpw;      // channel rows per producer wave and chunk
  int xw;       // activated window width  = BN + (K-1)*dil
  int xwp;      // its LDS row pitch (Cfg::XWP)
  int xrw;      // raw window width        = xw + 10        (ACT1D)
  int xrwp;     // raw row pitch in the producer scratch (multiple of 64)
  int a2w;      // 2x-rate window width    = 2*xw + 10      (ACT1D)
  int ws_sz, xa_sz, scr_sz;  // floats: one weight slab, one window buffer, one producer scratch
  int xa_off, scr_off, total;
};

template <class C>
__host__ __device__ inline LdsPlan make_plan(int K, int dil, int prologue, int lkc) {
  LdsPlan p;
  p.lkc = lkc;
  p.kc = 1 << lkc;
  p.rpw = (p.kc + C::NPW - 1) / C::NPW;
  p.xw = C::BN + (K - 1) * dil;
  p.xwp = C::XWP;  // valid only while xw + 3 <= XWP (pick_lkc checks)
  p.xrw = p.xw + 10;
  p.xrwp = (p.xrw + 63) & ~63;
  p.a2w = 2 * p.xw + 10;
  p.ws_sz = K * p.kc * C::BM;
  p.xa_sz = p.kc * p.xwp;
  // scratch of one producer wave: double-buffered raw rows + one 2x-rate row
  p.scr_sz = prologue == HSP_PRO_ACT1D ? 2 * p.rpw * p.xrwp + ((p.a2w + 3) & ~3) : 0;
  p.xa_off = 2 * p.ws_sz;
  p.scr_off = p.xa_off + 2 * p.xa_sz;
  p.total = p.scr_off + C::NPW * p.scr_sz;
  return p;
}

template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (N > 0) {
    static_for<N - 1>(f);
    f(std::integral_constant<int, N - 1>{});
  }
}

// workgroup barrier that does NOT drain outstanding global loads: only this wave's LDS
// traffic has to be complete before the other role touches the buffer (__syncthreads()
// would add s_waitcnt vmcnt(0) and expose the latency of the prefetched chunk)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
#define HSP_BARRIER(a) do { if (!HSP_DBG(a, HSP_CV_NO_BARRIER)) lds_barrier(); } while (0)

// wave-local LDS ordering: all earlier LDS ops of this wave are complete and the
// compiler may not move memory accesses across this point
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ------------------------------------------------------------------- folded columns
// hsp_conv1d_args.fold_cols: the column tiles of a launch are cut from the B * T virtual columns v = b T + t (T = ncols
// = Lin, a "same" conv), so a tile of BN columns starting at v0 = b0 T + ts0 may run over the seams between utterances
// b0, b0 + 1, ...  Its LDS window is the concatenation of those utterances' pieces, each with a halo of 4 floats on
// either side (pad <= 4 and (K - 1) dil - pad <= 4): window index e holds position q - 4 of utterance b0 + i, where
// q = e + ts0 - i (T + 8) in [0, T + 8); positions outside [0, T) -- the conv's own zero padding -- and utterances past
// the last one are zeros.  T % 4 == 0 and ts0 % 4 == 0, so every 16-B group of the window is wholly one utterance's
// data or wholly zeros (the zero buffer is its DMA source), and column `col` of the tile, in piece i, reads tap j at
// col + 8 i + 4 - pad + j dil: the tap offsets stay what they are, the B-fragment base moves by 8 floats per seam.
// K order per output element is unchanged: bit-identical to the per-utterance tiling.
//
// column `col` of the tile -> the piece i it lies in and its time t there
__device__ __forceinline__ void fold_col(int col, int ts0, int T, int& i, int& t) {
  i = 0;
  t = ts0 + col;
  while (t >= T) {
    t -= T;
    ++i;
  }
}

}  // namespace hspconv

#include "hsp_conv1d_produce.h"
#include "hsp_conv1d_epilogue.h"
#include "hsp_conv1d_consume.h"

namespace hspconv {

// ------------------------------------------------------------------------ kernel
// (HSP_ACC_ROW, the C/D map of the 32x32 MFMA forms, is hsp_device.h's)

// does this instantiation carry the narrow-tail consumer (a last column tile with at most 32 valid columns is
// computed as 4 waves x (32 rows x 32 columns) instead of 4 waves x (64 x 64): a quarter of the MFMAs)?
template <class C, int EPI, bool ACT>
constexpr bool has_tail_path() {
  return EPI == HSP_EPI_INIT && !ACT && C::kWM * C::kWN == 4 && C::kTM * C::kWM == 4 && C::kTN * C::kWN == 4;  // 128 x 128
}

// `sched` = g | tail << 8 (host: launch_one).
//   g = 0: blockIdx.x = mt + n_mt * ct, row tiles fastest: the blocks that round-robin onto one XCD keep hitting the
//          same weight slab in that XCD's L2 -- but the input window of a column tile is then fetched once per row
//          tile, by a different XCD each time.
//   g > 0: XCD-grouped.  Blocks b and b + 8 share an XCD (observed dispatch order; speed only, never correctness).
//          XCD x = blockIdx.x % 8 owns row group (x % (n_mt / g)) = g consecutive row tiles, whose weight slabs fit
//          its L2 together, and walks its column tiles with those g row tiles adjacent in time: the window is
//          fetched from HBM / Infinity Cache once per XCD group instead of once per row tile.
//   tail:  the last column tile of every utterance holds <= 32 valid columns; those tiles are enumerated LAST
//          (short jobs at the end of the grid) and take the narrow consumer.
// FOLD (folded columns, launch_one decides): n_nt column tiles over the B * ncols virtual columns; sched == 0.
template <class C, int EPI, bool ACT, bool FOLD = false>
__global__ __launch_bounds__(C::THREADS, C::MINW) void conv1d_mfma_kernel(const hsp_conv1d_args a, const int n_mt,
                                                                          const int n_nt, const int lkc,
                                                                          const int xvec, const int sched) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int BM = C::BM, BN = C::BN, TM = C::kTM, TN = C::kTN;
  const LdsPlan P = make_plan<C>(a.K, a.dil, ACT ? HSP_PRO_ACT1D : HSP_PRO_NONE, lkc);
  const int KC = P.kc;

  int mt, ct;
  {
    const int g = sched & 255;
    const int bid = blockIdx.x;
    if (g == 0) {
      mt = bid % n_mt;
      ct = bid / n_mt;
    } else {
      const int x = bid & 7, q = bid >> 3;
      const int groups_m = n_mt / g, nx = 8 / groups_m;
      mt = (x % groups_m) * g + q % g;
      ct = (q / g) * nx + x / groups_m;
      if (ct >= n_nt * a.B) return;  // grid padding (whole workgroup, before any barrier)
    }
  }
  int nt, b;
  bool tail_tile = false;
  if constexpr (FOLD) {
    nt = ct;
    b = (nt * BN) / a.ncols;   // the utterance of the tile's first column: the workgroup's one division
  } else if (sched >> 8) {
    const int n_main = (n_nt - 1) * a.B;
    if (ct < n_main) {
      nt = ct % (n_nt - 1);
      b = ct / (n_nt - 1);
    } else {
      nt = n_nt - 1;
      b = ct - n_main;
      tail_tile = true;
    }
  } else {
    nt = ct % n_nt;
    b = ct / n_nt;
  }
  int t0c = nt * BN;
  if constexpr (EPI == HSP_EPI_ACT) t0c = nt * (BN - 16) - 8;   // overlapping tiles: 8 halo columns of the activation on either side
  const int m0 = mt * BM, t0 = t0c;
  const int p0 = t0 - a.pad;  // first activated-input position of the window
  const int ts0 = FOLD ? t0 - b * a.ncols : 0;   // FOLD: t0 is a virtual column, at time ts0 of utterance b

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nchunks = (a.Cin + KC - 1) >> lkc;

  if (wave >= C::NCW) {
    // ------------------------------------------------------------ producers
    const int pw = wave - C::NCW;
    using PR = Prod<C>;
    const float* const wb = a.w + (int64_t)b * a.w_bs;   // per-"utterance" weights (frequency bins, hsp.h: w_bs), else w_bs == 0
    const ProdArgs pa{wb, a.zeros, a.alpha_exp, a.beta_inv, a.filt, a.K, a.Cin, a.Lin, a.M, a.w_ld, (int)a.x_cs,
                      (int)a.x_ts, a.prologue, a.slope};
    const float* xb = a.x + (int64_t)b * a.x_bs;
    float* const Ws0 = lds;
    float* const Xa0 = lds + P.xa_off;
    // One chunk loop per staging form -- "stage chunk 0; barrier; per chunk: stage the next one into the other buffer;
    // barrier" -- written out four times: with the fast and plain forms sharing a loop (or only the wait + leaky-ReLU tail)
    // the plain-row kernels of the 128 x 128, 64 x 256 and 32 x 512 shapes compile to other register and scratch counts
    // and an SGPR spill in the consumers' chunk handover; ACT1D as a stage body changes every ACT1D kernel.
    if constexpr (FOLD) {
      // folded columns: lane g stages 16-B group g of every window row ("folded columns" above)
      const int T = a.ncols;
      const int ngrp = (BN + 8 * ((BN + T - 1) / T + 1)) >> 2;   // <= 64 (launch_one: the window fits the pitch)
      int q = 4 * lane + ts0, piece = 0;
      while (q >= T + 8) {
        q -= T + 8;
        ++piece;
      }
      const bool inside = b + piece < a.B && q >= 4 && q < T + 4;
      const float* const xl = inside ? a.x + (int64_t)(b + piece) * a.x_bs + (q - 4) : a.zeros;
      const int xs = inside ? (int)a.x_cs : 0;
      const bool wfast = m0 + BM <= a.M && (a.Cin & (KC - 1)) == 0;   // wave-uniform (dma_w_fast's preconditions)
      const float* const wtile = wb + m0;
      const unsigned wofs = PR::w_lane_ofs(lane, a.w_ld);
      auto stage = [&](int c0, float* Ws, float* Xa) __attribute__((always_inline)) {
        if (wfast) PR::dma_w_fast(wtile, a.w_ld, a.Cin, a.K, P, Ws, c0, pw, wofs);
        else PR::dma_w(pa, P, Ws, c0, m0, pw, lane);
        PR::dma_x_fold(xl, xs, a.zeros, a.Cin, P, Xa, c0, pw, lane < ngrp);
        wait_vm0();
        if (a.prologue == HSP_PRO_LRELU) PR::lrelu_x(pa, P, Xa, pw, lane);
      };
      stage(0, Ws0, Xa0);
      HSP_BARRIER(a);
      for (int c = 0; c < nchunks; ++c) {
        const int nb = (c + 1) & 1;
        if (c + 1 < nchunks && !HSP_DBG(a, HSP_CV_ONE_CHUNK)) stage((c + 1) << lkc, Ws0 + nb * P.ws_sz, Xa0 + nb * P.xa_sz);
        HSP_BARRIER(a);
      }
    } else if constexpr (!ACT) {
      const int p0a = p0 & ~3;
      const bool fast = xvec && m0 + BM <= a.M && (a.Cin & (KC - 1)) == 0 && !HSP_DBG(a, HSP_CV_NO_FAST_STAGE);  // wave-uniform
      if (fast) {
        const float* const wtile = wb + m0;
        const float* const xtile = xb + p0a;
        const int xcs = (int)a.x_cs;
        const unsigned wofs = PR::w_lane_ofs(lane, a.w_ld);
        if (p0a < 0 || p0a + 4 * ((P.xw + 3 + 3) >> 2) > a.Lin) PR::zero_x_rows(P, Xa0, pw, lane);
        PR::dma_w_fast(wtile, a.w_ld, a.Cin, a.K, P, Ws0, 0, pw, wofs);
        PR::dma_x16_fast(xtile, xcs, a.Lin, P, Xa0, 0, p0a, pw, lane);
        wait_vm0();
        if (a.prologue == HSP_PRO_LRELU) PR::lrelu_x(pa, P, Xa0, pw, lane);
        HSP_BARRIER(a);
        for (int c = 0; c < nchunks; ++c) {
          const int nb = (c + 1) & 1;
          if (c + 1 < nchunks && !HSP_DBG(a, HSP_CV_ONE_CHUNK)) {
            PR::dma_w_fast(wtile, a.w_ld, a.Cin, a.K, P, Ws0 + nb * P.ws_sz, (c + 1) << lkc, pw, wofs);
            PR::dma_x16_fast(xtile, xcs, a.Lin, P, Xa0 + nb * P.xa_sz, (c + 1) << lkc, p0a, pw, lane);
            wait_vm0();
            if (a.prologue == HSP_PRO_LRELU) PR::lrelu_x(pa, P, Xa0 + nb * P.xa_sz, pw, lane);
          }
          HSP_BARRIER(a);
        }
        if constexpr (EPI == HSP_EPI_ACT) EpiAct<C>::producer(a, lds, b, m0, t0, wave, lane);
        return;
      }
      PR::dma_w(pa, P, Ws0, 0, m0, pw, lane);
      if (xvec) PR::dma_x16(pa, P, Xa0, xb, 0, p0a, pw, lane); else PR::dma_x(pa, P, Xa0, xb, 0, p0, pw, lane);
      wait_vm0();
      if (a.prologue == HSP_PRO_LRELU) PR::lrelu_x(pa, P, Xa0, pw, lane);
      HSP_BARRIER(a);
      for (int c = 0; c < nchunks; ++c) {
        const int nb = (c + 1) & 1;
        if (c + 1 < nchunks && !HSP_DBG(a, HSP_CV_ONE_CHUNK)) {
          PR::dma_w(pa, P, Ws0 + nb * P.ws_sz, (c + 1) << lkc, m0, pw, lane);
          if (xvec) PR::dma_x16(pa, P, Xa0 + nb * P.xa_sz, xb, (c + 1) << lkc, p0a, pw, lane);
          else PR::dma_x(pa, P, Xa0 + nb * P.xa_sz, xb, (c + 1) << lkc, p0, pw, lane);
          wait_vm0();
          if (a.prologue == HSP_PRO_LRELU) PR::lrelu_x(pa, P, Xa0 + nb * P.xa_sz, pw, lane);
        }
        HSP_BARRIER(a);
      }
    } else {
      // ACT1D, the one form with a look-ahead: the raw rows of chunk c + 2 are requested while chunk c + 1 is activated,
      // into the other half of this wave's scratch, and land under a whole chunk of MFMAs.
      float* const scr = lds + P.scr_off + pw * P.scr_sz;   // raw[2][rpw][xrwp], a2[a2w]
      float* const a2 = scr + 2 * P.rpw * P.xrwp;
      const int rsz = P.rpw * P.xrwp;
      PR::dma_raw(pa, P, scr, xb, 0, p0, pw, lane);
      PR::dma_w(pa, P, Ws0, 0, m0, pw, lane);
      wait_vm0();
      PR::act_rows(pa, P, scr, a2, Xa0, 0, p0, pw, lane);
      if (nchunks > 1) PR::dma_raw(pa, P, scr + rsz, xb, KC, p0, pw, lane);
      wait_vm0();
      HSP_BARRIER(a);
      for (int c = 0; c < nchunks; ++c) {
        const int nb = (c + 1) & 1;
        if (c + 1 < nchunks && !HSP_DBG(a, HSP_CV_ONE_CHUNK)) {
          PR::dma_w(pa, P, Ws0 + nb * P.ws_sz, (c + 1) << lkc, m0, pw, lane);
          if (c + 2 < nchunks) PR::dma_raw(pa, P, scr + (c & 1) * rsz, xb, (c + 2) << lkc, p0, pw, lane);
          PR::act_rows(pa, P, scr + nb * rsz, a2, Xa0 + nb * P.xa_sz, (c + 1) << lkc, p0, pw, lane);
          wait_vm0();
        }
        HSP_BARRIER(a);
      }
    }
    if constexpr (EPI == HSP_EPI_ACT) EpiAct<C>::producer(a, lds, b, m0, t0, wave, lane);
    return;
  }

  // -------------------------------------------------------------- consumers
  if constexpr (has_tail_path<C, EPI, ACT>()) {
    if (tail_tile) {
      // <= 32 valid columns: wave w takes rows 32 w .. 32 w + 31 of the tile and the first 32 columns
      conv_consume<C, EPI, ACT, 1, 1>(a, P, lds, b, m0, t0, p0, wave, 0, lane, nchunks, lkc, xvec);
      return;
    }
  }
  if constexpr (FOLD) {
    conv_consume<C, EPI, ACT, TM, TN, true>(a, P, lds, b, m0, t0, p0, wave / C::kWN, wave % C::kWN, lane, nchunks, lkc, xvec, 0, ts0);
  } else if constexpr (C::kKS > 1) {
    const int ks = wave / (C::kWM * C::kWN), w2 = wave % (C::kWM * C::kWN);
    conv_consume<C, EPI, ACT, TM, TN>(a, P, lds, b, m0, t0, p0, w2 / C::kWN, w2 % C::kWN, lane, nchunks, lkc, xvec, ks);
  } else {
    conv_consume<C, EPI, ACT, TM, TN>(a, P, lds, b, m0, t0, p0, wave / C::kWN, wave % C::kWN, lane, nchunks, lkc, xvec);
  }
}

// -------------------------------------------------------------------- host side
constexpr int kMaxLdsBytes = 160 * 1024;
constexpr int kLdsTarget = 80 * 1024;  // two workgroups per CU when possible

// largest chunk depth (log2) this tile shape can stage for the launch, or -1
template <class C>
int pick_lkc(const hsp_conv1d_args& a, int lds_limit) {
  const bool act = a.prologue == HSP_PRO_ACT1D;
  if (C::BN + (a.K - 1) * a.dil + 3 > C::XWP) return -1;  // halo beyond this shape's window pitch
  int cin_p2 = 2;
  while ((1 << cin_p2) < a.Cin && cin_p2 < 6) ++cin_p2;  // no point staging past Cin
  for (int lkc = cin_p2; lkc >= 2; --lkc) {
    const LdsPlan P = make_plan<C>(a.K, a.dil, a.prologue, lkc);
    if (P.total * (int)sizeof(float) > lds_limit) continue;
    if (P.kc < Prod<C>::RPI) continue;   // a weight DMA instruction must stay inside one tap
    if (C::kKS > 1 && (((a.K * P.kc) >> 1) % (2 * C::kKS) != 0 || P.total < C::kWM * C::kWN * (32 * 36 + C::kTM * C::kTN * 16 * 64))) continue;  // even shares; room for the partial sums
    if (act && P.rpw > 2) continue;      // activation work per producer wave and chunk
    return lkc;
  }
  return -1;
}

// does this instantiation carry the folded-columns form?
template <class C, int EPI, bool ACT>
constexpr bool has_fold_path() {
  return C::kFOLD && !ACT && EPI != HSP_EPI_SHUF;
}

// the 16-B window DMA: a plain prologue on a 16-B addressable input whose length is a multiple of 4 (else the 4-B one)
inline bool window_dma16(const hsp_conv1d_args& a, bool act) {
  return !act && a.x_ts == 1 && (a.Lin & 3) == 0 && (a.x_cs & 3) == 0 && (a.x_bs & 3) == 0 && hsp_aligned16(a.x) &&
         !HSP_DBG(a, HSP_CV_NO_XVEC);
}

// folded columns: does the launch's geometry fit the form ("folded columns" above)?  Otherwise the per-utterance tiling.
template <class C>
bool fold_fits(const hsp_conv1d_args& a, bool xvec) {
  const int T = a.ncols;
  if (!a.fold_cols || a.B < 2 || !xvec || (T & 3) || (T % C::BN) == 0 || a.w_bs) return false;
  if (a.Lin != T || a.Lout != T || a.pad > 4 || (a.K - 1) * a.dil - a.pad > 4) return false;   // a "same" conv, halo within the rounding
  if (C::BN + 8 * ((C::BN + T - 1) / T + 1) > C::XWP) return false;   // the window with its worst-case seam count
  return (int64_t)a.B * T <= 0x3fffffff;
}

// the activation epilogue: does the launch ask for it (hsp_conv1d_args.act == HSP_ACT_ACT1D)?
inline bool epi_act_set(const hsp_conv1d_args& a) { return a.act == HSP_ACT_ACT1D; }

// Launch one instantiation.  EPI / ACT must already match the arguments (select_epilogue()).
template <class C, int EPI, bool ACT>
int launch_one(const hsp_conv1d_args& a, hipStream_t s, int32_t* plan_out) {
  if (a.fold_cols && !has_fold_path<C, EPI, ACT>()) return HSP_EINVAL;   // this kernel does not implement the form
  if (epi_act_set(a) != (EPI == HSP_EPI_ACT)) return HSP_EINVAL;         // likewise (dispatch() has checked the form's conditions)
  // a shape whose register budget admits two workgroups per CU keeps its LDS under half the
  // CU's; the others take the deepest chunk the whole 160 KB can stage (fewer barriers, and the
  // DMA of a chunk gets a longer MFMA phase to land under)
  // Round 3: the short-sequence shapes (64 x 64, 64 x 128-gated, 32 x 128: <= 87 VGPRs, one workgroup per CU with the deep
  // chunk) take the half-CU chunk as well once the launch has more tiles than the chip has CUs: the FFN fc1 of an
  // 8-utterance front group is 384 tiles -- two rounds of lone workgroups at 52 us, one round of pairs at ~40.
  const int64_t tiles = (int64_t)((a.M + C::BM - 1) / C::BM) * ((a.ncols + C::BN - 1) / C::BN) * a.B;
  // (same box: 42.4 -> 39.3 us per launch, step 81.05 -> 80.77 ms; beyond 512 tiles the deep chunk wins again: 67.8 vs 69.7)
  // (HSP_CV_DEEP_K3, round 6 / VERDICT r05 item 8: twice the MFMAs per barrier and window DMA, ONE workgroup per CU;
  // measured in profiles/r06_k3_deep_chunk.txt)
  const bool deep_k3 = HSP_DBG(a, HSP_CV_DEEP_K3) && a.K <= 3;
  const bool two_per_cu = !deep_k3 && (C::MINW * 256 >= 2 * C::THREADS || ((tiles > 256 || HSP_DBG(a, HSP_CV_HALF_CU_ANY)) && tiles <= 512 && !HSP_DBG(a, HSP_CV_NO_HALF_CU)));
  int lkc = pick_lkc<C>(a, two_per_cu ? kLdsTarget : kMaxLdsBytes);
  if (lkc < 0) lkc = pick_lkc<C>(a, kMaxLdsBytes);
  if (lkc < 0) return HSP_EINVAL;
  int lds_bytes = make_plan<C>(a.K, a.dil, a.prologue, lkc).total * (int)sizeof(float);
  if constexpr (EPI == HSP_EPI_ACT) lds_bytes = lds_bytes > EpiAct<C>::LDS_FLOATS * (int)sizeof(float) ? lds_bytes : EpiAct<C>::LDS_FLOATS * (int)sizeof(float);
  if (plan_out) {
    plan_out[0] = C::BM; plan_out[1] = C::BN; plan_out[2] = 1 << lkc; plan_out[3] = lds_bytes;
    return 0;
  }
  const int n_mt = (a.M + C::BM - 1) / C::BM;
  constexpr int kColStep = EPI == HSP_EPI_ACT ? C::BN - 16 : C::BN;   // HSP_EPI_ACT: overlapping column tiles
  const int n_nt = (a.ncols + kColStep - 1) / kColStep;
  // block schedule (see the kernel): row tiles per XCD group, narrow tail tiles
  const int64_t n_ct = (int64_t)n_nt * a.B;
  // g > 0 (XCD-grouped row tiles) is a measured LOSS and exists in the tuning build only (HSP_CV_XCD_GROUPS):
  // k = 3 convs run 4-5 % slower with it (C = 512 / L = 800: 114.5 vs 119.9 TFLOP/s, C = 256 / L = 4000: 120.9 vs
  // 126.2), k = 7 / 11 are unchanged (profiles/r03_sched_sweep.txt) -- the blocks of one XCD sharing ONE weight slab
  // matters more than fetching a window once.
  int g = 0;
  if (HSP_DBG(a, HSP_CV_XCD_GROUPS) && n_mt >= 1 && n_mt <= 8 && (8 % n_mt) == 0) {
    // the largest group of row tiles whose weight slabs share one XCD's 4-MB L2 with room for the streamed windows
    const int64_t slab = (int64_t)a.K * a.Cin * C::BM * (int64_t)sizeof(float);
    g = 1;
    for (int cand = n_mt; cand > 1; cand >>= 1)
      if (n_mt % cand == 0 && (int64_t)cand * slab <= (int64_t)3200 * 1024) { g = cand; break; }
  }
  const int rem = a.ncols - (n_nt - 1) * C::BN;
  const int tail = (has_tail_path<C, EPI, ACT>() && n_nt >= 2 && rem <= 32 && !HSP_DBG(a, HSP_CV_NO_TAIL)) ? 1 : 0;
  int64_t blocks = (int64_t)n_mt * n_ct;
  if (g > 0) {
    const int nx = 8 / (n_mt / g);
    blocks = 8 * (int64_t)g * ((n_ct + nx - 1) / nx);
  }
  if (blocks <= 0 || blocks > 0x7fffffff) return HSP_EINVAL;
  const int sched = g | (tail << 8);
  auto kern = conv1d_mfma_kernel<C, EPI, ACT>;
  // raise the kernel's dynamic-LDS cap once per device (the attribute is per device; kept out of the
  // launch path afterwards so that launches are legal inside a hipGraph stream capture)
  static hsp_lds_flags flags;
  if (lds_bytes > 32 * 1024)
    if (int e = hsp_raise_lds_limit(reinterpret_cast<const void*>(kern), kMaxLdsBytes, flags)) return e;
  if (EPI == HSP_EPI_VEC && lds_bytes < C::NCW * 32 * 36 * 4) lds_bytes = C::NCW * 32 * 36 * 4;  // staging area
  const bool xvec = window_dma16(a, ACT);
  if constexpr (has_fold_path<C, EPI, ACT>()) {
    // the chunk depth above came from the per-utterance tile count: the folded launch keeps the tile configuration, and
    // with it the order of every output element's sum
    if (fold_fits<C>(a, xvec)) {
      auto kfold = conv1d_mfma_kernel<C, EPI, ACT, true>;
      static hsp_lds_flags fflags;
      if (lds_bytes > 32 * 1024)
        if (int e = hsp_raise_lds_limit(reinterpret_cast<const void*>(kfold), kMaxLdsBytes, fflags)) return e;
      const int n_vt = (int)(((int64_t)a.B * a.ncols + C::BN - 1) / C::BN);
      hipLaunchKernelGGL(kfold, dim3((unsigned)(n_mt * n_vt)), dim3(C::THREADS), lds_bytes, s, a, n_mt, n_vt, lkc, 1, 0);
      return (int)hipGetLastError();
    }
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(C::THREADS), lds_bytes, s, a, n_mt, n_nt, lkc, xvec ? 1 : 0, sched);
  return (int)hipGetLastError();
}

// the epilogue kind the arguments ask for
inline int select_epilogue(const hsp_conv1d_args& a) {
  if (a.rows == HSP_ROWS_GATE_WN || a.rows == HSP_ROWS_GATE_GLU) return HSP_EPI_GATE;
  const bool pointwise = a.act != HSP_ACT_NONE || a.mask_mode != HSP_MASK_NONE || a.cscale;
  if (a.rows == HSP_ROWS_SHUFFLE)
    return (!pointwise && !a.cbias && !a.res && !a.accumulate) ? HSP_EPI_SHUF : HSP_EPI_GEN;
  if (!pointwise && a.scale == 1.0f && !HSP_DBG(a, HSP_CV_NO_INIT)) return HSP_EPI_INIT;
  const bool vec = (a.ncols & 3) == 0 && hsp_aligned16(a.y) && (a.y_bs & 3) == 0 && (a.y_cs & 3) == 0 &&
                   (!a.res || (hsp_aligned16(a.res) && (a.res_bs & 3) == 0 && (a.res_cs & 3) == 0)) &&
                   (a.mask_mode == HSP_MASK_NONE || (hsp_aligned16(a.mask) && (a.mask_bs & 3) == 0));
  return vec ? HSP_EPI_VEC : HSP_EPI_GEN;
}

// tile shapes <WM, WN, TM, TN, producer waves, min waves per SIMD>
using M128 = Cfg<2, 2, 2, 2, 4, 4>;    // 128 x 128, two workgroups per CU
using M64 = Cfg<1, 4, 2, 2, 8, 3>;     //  64 x 256, eight producer waves (fused activation prologue)
using M32 = Cfg<1, 4, 1, 4, 8, 3>;     //  32 x 512, likewise
using M64P = Cfg<1, 4, 2, 2, 4, 4>;    //  64 x 256, plain prologue: four producer waves, two workgroups per CU
using M32P = Cfg<1, 4, 1, 4, 4, 4>;    //  32 x 512, likewise
using S64 = Cfg<2, 2, 1, 1, 4, 2, 64, 1, true>;    //  64 x 64   short sequences: many small, deep-chunk tiles; folded columns
using S64G = Cfg<1, 4, 2, 1, 4, 2, 64, 1, true>;   //  64 x 128  short sequences, gated rows (needs TM even); folded columns
using S32 = Cfg<1, 4, 1, 1, 4, 2>;     //  32 x 128
using S64W = Cfg<2, 2, 1, 1, 4, 2, 128>;   //  64 x 64 with a 192-float window pitch: halos of 62 ... 125 columns
using S64GW = Cfg<1, 4, 2, 1, 4, 2, 128>;  //  64 x 128 gated rows with a 256-float pitch (WN with dilation_rate > 1)
using S64G2 = Cfg<1, 2, 2, 1, 4, 2, 64, 2>;  // 64 x 64 gated rows, the K range of a chunk split between two wave pairs (round 5)

}  // namespace hspconv

// One function per tile shape (hsp_conv1d_tile.hip, compiled once per shape): launches the instantiation
// for (epi, act) or returns HSP_EINVAL when the shape does not carry that combination.
#define HSP_TILE_LIST(X) X(M128) X(M64) X(M32) X(M64P) X(M32P) X(S64) X(S64G) X(S32) X(S64W) X(S64GW) X(S64G2)
#define HSP_TILE_DECL(name) \
  int hsp_conv_tile_##name(const hsp_conv1d_args& a, int epi, bool act, hipStream_t s, int32_t* plan_out);
HSP_TILE_LIST(HSP_TILE_DECL)
#undef HSP_TILE_DECL
