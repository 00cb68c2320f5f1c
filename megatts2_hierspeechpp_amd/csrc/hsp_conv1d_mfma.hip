// hsp_conv1d_mfma_f32: argument validation and the choice of kernel, tile shape and epilogue kind.
// The kernel itself is the template in hsp_conv1d_mfma_kernel.h, instantiated per tile shape by
// hsp_conv1d_tile.hip; 1x1 convs over token columns go to one of the two token GEMMs (hsp_token_gemm.h).
//
// Reference call sites: see include/hsp.h (hsp_conv1d_args).
#include "hsp_conv1d_mfma_kernel.h"
#include "hsp_token_gemm.h"

namespace {
using namespace hspconv;

int validate(const hsp_conv1d_args& a) {
  if (!a.x || !a.w || !a.y) return HSP_EINVAL;
#ifndef HSP_TUNING
  if (a.debug != 0) return HSP_EINVAL;  // tuning switches exist only in libhsp_tune.so
#endif
  if (a.B <= 0 || a.Cin <= 0 || a.Lin <= 0 || a.K <= 0 || a.M <= 0 || a.Cout <= 0 || a.Lout <= 0 || a.ncols <= 0)
    return HSP_EINVAL;
  if (a.stride != 1 || (a.M & 3) || (a.w_ld & 3) || a.w_ld < a.M || a.dil < 1) return HSP_EINVAL;
  if ((reinterpret_cast<uintptr_t>(a.w) & 15) != 0 || a.w_bs < 0 || (a.w_bs & 3)) return HSP_EINVAL;
  if (a.w_bs && (a.ln_c1 || a.split_row || (a.res && a.res_ts > 1))) return HSP_EINVAL;   // per-batch weights: conv tiles only
  // the kernel indexes one utterance / the weight matrix with 32-bit element offsets
  if ((int64_t)a.K * a.Cin * a.w_ld >= (1ll << 31)) return HSP_EINVAL;
  if ((int64_t)a.Cin * a.x_cs + (int64_t)a.Lin * a.x_ts >= (1ll << 31) || a.x_cs < 0 || a.x_ts < 0) return HSP_EINVAL;
  if (a.y_cs < 0 || (int64_t)a.Cout * a.y_cs + a.Lout >= (1ll << 31)) return HSP_EINVAL;
  if (a.res && (a.res_cs < 0 || (int64_t)a.Cout * a.res_cs + a.Lout >= (1ll << 31))) return HSP_EINVAL;
  if (a.res_ts < 0 || (a.res && a.res_ts > 1 && (int64_t)a.Cout * a.res_cs + (int64_t)a.Lout * a.res_ts >= (1ll << 31))) return HSP_EINVAL;
  if (a.prologue == HSP_PRO_ACT1D && (!a.alpha_exp || !a.beta_inv || !a.filt || a.x_ts != 1)) return HSP_EINVAL;
  if (!a.zeros || (reinterpret_cast<uintptr_t>(a.zeros) & 15) != 0) return HSP_EINVAL;
  if (a.prologue != HSP_PRO_NONE && a.prologue != HSP_PRO_LRELU && a.prologue != HSP_PRO_ACT1D) return HSP_EINVAL;
  if (a.mask_mode != HSP_MASK_NONE && !a.mask) return HSP_EINVAL;
  if (a.fold_cols != 0 && a.fold_cols != 1) return HSP_EINVAL;
  if (a.rows == HSP_ROWS_GATE_WN || a.rows == HSP_ROWS_GATE_GLU) {
    if (a.gate_half <= 0 || (a.gate_half & 31) || a.M != 2 * a.gate_half || a.Cout != a.gate_half) return HSP_EINVAL;
    if (a.prologue == HSP_PRO_ACT1D) return HSP_EINVAL;
  } else if (a.rows == HSP_ROWS_SHUFFLE) {
    // M = Cout * up rounded up to a multiple of 4 (hip_layers.convtr_pack_map): the up to three padding rows hold
    // zero weights and are never stored (every SHUFFLE epilogue checks co < Cout)
    if (a.up <= 0 || a.up > 16 || a.M < a.Cout * a.up || a.M - a.Cout * a.up > 3 || a.M > (1 << 16)) return HSP_EINVAL;
  } else if (a.rows != HSP_ROWS_PLAIN) {
    return HSP_EINVAL;
  }
  return 0;
}

// The activation epilogue (hsp_conv1d_args.act == HSP_ACT_ACT1D, include/hsp.h): a launch with that value takes the form or is
// refused -- no other kernel behind this entry point (token GEMMs, gated / ConvTranspose rows, K-split, folded columns,
// the wide shapes) ever sees it.
int dispatch_epi_act(const hsp_conv1d_args& a, hipStream_t s, int32_t* plan_out) {
  if (!a.alpha_exp || !a.beta_inv || !a.filt) return HSP_EINVAL;
  if (a.rows != HSP_ROWS_PLAIN || a.M > 64 || a.Cout > a.M || a.prologue != HSP_PRO_NONE) return HSP_EINVAL;
  if (a.Lin != a.ncols || a.Lout != a.ncols || 2 * a.pad != (a.K - 1) * a.dil || (a.K - 1) * a.dil > 61 || (a.ncols & 3))
    return HSP_EINVAL;   // stride 1 (validate), "same" padding, a halo within the window pitch, whole float4s
  if (!hsp_aligned16(a.y) || (a.y_bs & 3) || (a.y_cs & 3)) return HSP_EINVAL;
  if (a.cbias || a.mask_mode != HSP_MASK_NONE || a.cscale || a.res || a.accumulate ||
      a.scale != 1.0f || a.post_scale != 1.0f)
    return HSP_EINVAL;   // bias alone
  if (a.fold_cols || a.w_bs || a.ln_c1 || a.split_row) return HSP_EINVAL;
  return a.M > 32 ? hsp_conv_tile_M64P(a, HSP_EPI_ACT, false, s, plan_out) : hsp_conv_tile_M32P(a, HSP_EPI_ACT, false, s, plan_out);
}

int dispatch(const hsp_conv1d_args& a, hipStream_t s, int32_t* plan_out) {
  if (epi_act_set(a)) return dispatch_epi_act(a, s, plan_out);
  const bool gated = a.rows == HSP_ROWS_GATE_WN || a.rows == HSP_ROWS_GATE_GLU;
  const bool act = a.prologue == HSP_PRO_ACT1D;
  // "short": 128 x 128 tiles would leave at least half of the 256 CUs idle; prefer 64 x 64 tiles with deep
  // chunks so that more CUs get work.  A lone 64 x 64 tile takes half as long as a lone 128 x 128 one (measured:
  // 36 us against 67 us at C = 128, k = 7) for a quarter of the work, so the small shape wins up to 64 big tiles,
  // ties up to 128 and loses 2x beyond (tools/conv_sweep.py, profiles/r02_tile_threshold.txt).
  const bool short_seq = hsp_tile_count(a, 128, 128) <= 128;
  // a residual read at a column stride: the register-path token GEMM or nothing
  if (a.res && a.res_ts > 1) {
    if (a.fold_cols) return HSP_EINVAL;
    const int e = hsp_rgemm_try(a, s, plan_out);
    return e >= 0 ? e : HSP_EINVAL;
  }
  // 1x1 GEMMs with enough outputs for about one 128 x 128 / 128 x 64 tile per CU (the PLM loop beyond ~60 prefix
  // positions): the throughput-oriented token GEMM (hsp_bgemm.hip)
  if (a.K == 1 && !a.w_bs && !HSP_TG_DBG(a, HSP_TG_OFF)) {
    const int e = hsp_bgemm_try(a, s, plan_out);
    if (e >= 0) return e;
  }
  // Folded columns (hsp_conv1d_args.fold_cols): the block token GEMM above and the conv tiles S64 / S64G implement the
  // form, every other kernel refuses the field -- launch_one does for the conv tiles.  Where a refusal would make way for
  // the next kernel in line (register-path GEMM, K-split gated tile), that kernel is asked first, WITHOUT the field,
  // whether it takes the launch: the field never moves a launch to another kernel.
  hsp_conv1d_args plain = a;
  plain.fold_cols = 0;
  int32_t probe[4];
  // (HSP_TG_RG_ANY_SIZE: try the register-path token GEMM whatever the launch size -- tools/gemm_sweep.py)
  if ((short_seq || a.ln_c1 || a.split_row || HSP_TG_DBG(a, HSP_TG_RG_ANY_SIZE)) && !a.w_bs && !HSP_TG_DBG(a, HSP_TG_OFF)) {
    if (a.fold_cols && hsp_rgemm_try(plain, nullptr, probe) >= 0) return HSP_EINVAL;
    // 1x1 GEMMs over a few thousand token columns: the register-path kernel (hsp_rgemm.hip).  (The LDS-DMA token GEMM
    // of rounds 1-3 was retired in round 4: tools/gemm_sweep.py found no (shape, B, T) cell of
    // profiles/r04_gemm_dispatch_table.txt where it beat the block GEMM or the register path by more than 2 %.)
    const int e = hsp_rgemm_try(a, s, plan_out);
    if (e >= 0) return e;
  }
  if (a.ln_c1 || a.split_row) return HSP_EINVAL;  // fused input LayerNorm / second output: token-GEMM path only
  int epi = select_epilogue(a);
  if (act && epi != HSP_EPI_INIT) epi = HSP_EPI_GEN;  // the activation shapes carry INIT and GEN only
  // the window pitch is a compile-time constant of the shape (tile columns + 64): halos beyond 61 columns
  // (the 64-tap blocks of the wav2vec2 positional conv; WN in-layers with dilation_rate > 1) go to the two
  // shapes with a wider pitch (plain / gated rows; up to 125 columns, beyond: HSP_EINVAL from pick_lkc)
  if ((a.K - 1) * a.dil + 3 > 64)
    return gated ? hsp_conv_tile_S64GW(a, epi, act, s, plan_out) : hsp_conv_tile_S64W(a, epi, act, s, plan_out);
#ifdef HSP_TUNING
  // force a tile shape (results stay right)
  if (!gated && HSP_DBG(a, HSP_CV_TILE_M128)) return hsp_conv_tile_M128(a, epi, act, s, plan_out);
  if (!gated && HSP_DBG(a, HSP_CV_TILE_M64)) return hsp_conv_tile_M64(a, epi, act, s, plan_out);
  if (!gated && HSP_DBG(a, HSP_CV_TILE_S64)) return hsp_conv_tile_S64(a, epi, act, s, plan_out);
  if (!gated && HSP_DBG(a, HSP_CV_TILE_M64P)) return hsp_conv_tile_M64P(a, epi, act, s, plan_out);
#endif
  if (short_seq) {
    if (gated) {
      // (round 5) a launch of a few 64 x 128 tiles is bound by ONE tile's MFMA chain per SIMD: 64 x 64 tiles whose
      // chunk's K range is split between two wave pairs put twice the CUs on half the chain each (one WN layer of H = 192
      // at 8 x 200 frames: 57.9 -> 40.3 us, at 1 x 200: 56.3 -> 39.0).  Only up to 48 such tiles (a request of up to four
      // utterances): in the 32-utterance step the four batch groups of the front part run on four streams and fill the idle
      // CUs with each other's launches -- there the wider footprint LOSES (same box: 57.5-57.6 -> 57.8 ms per step with
      // the split tile on the 96-tile in-layers, profiles/r05_ab_s64g2*.json).  Tuning bits: HSP_CV_NO_S64G2 never,
      // HSP_CV_S64G2_512 up to 512 tiles.
      const int64_t t128 = hsp_tile_count(a, 64, 128);
      if ((t128 <= 48 || (HSP_DBG(a, HSP_CV_S64G2_512) && t128 <= 512)) && !HSP_DBG(a, HSP_CV_NO_S64G2)) {
        if (a.fold_cols && hsp_conv_tile_S64G2(plain, epi, act, nullptr, probe) != HSP_EINVAL) return HSP_EINVAL;
        const int e = hsp_conv_tile_S64G2(a, epi, act, s, plan_out);
        if (e != HSP_EINVAL) return e;
      }
      return hsp_conv_tile_S64G(a, epi, act, s, plan_out);
    }
    if (a.M > 32) return hsp_conv_tile_S64(a, epi, act, s, plan_out);
    return hsp_conv_tile_S32(a, epi, act, s, plan_out);
  }
  if (gated) return hsp_conv_tile_M128(a, epi, act, s, plan_out);
  // M > 128: 128 x 128 tiles at two workgroups per CU.  (A 256 x 128 one-per-CU shape existed in round 1; in
  // units of one 128 x 128 tile's MFMA time a CU spends 2 ceil(n256 / 256) against ceil(n128 / 256) <= that, and
  // it lost or tied on every layer of the path, so it is gone.)
  if (a.M > 64) return hsp_conv_tile_M128(a, epi, act, s, plan_out);
  if (a.M > 32) return act ? hsp_conv_tile_M64(a, epi, act, s, plan_out) : hsp_conv_tile_M64P(a, epi, act, s, plan_out);
  return act ? hsp_conv_tile_M32(a, epi, act, s, plan_out) : hsp_conv_tile_M32P(a, epi, act, s, plan_out);
}

}  // namespace

extern "C" int hsp_conv1d_mfma_f32(const hsp_conv1d_args* a, void* stream) {
  if (!a) return HSP_EINVAL;
  if (int e = validate(*a)) return e;
  return dispatch(*a, static_cast<hipStream_t>(stream), nullptr);
}

extern "C" int hsp_conv1d_mfma_plan(const hsp_conv1d_args* a, int32_t out4[4]) {
  if (!a || !out4) return HSP_EINVAL;
  if (int e = validate(*a)) return e;
  return dispatch(*a, nullptr, out4);
}
