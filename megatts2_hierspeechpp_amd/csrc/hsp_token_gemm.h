// What the two token GEMMs share -- hsp_rgemm.hip (register path, plan KC = -1) and hsp_bgemm.hip (block GEMM, plan
// KC = -2): Y[M x N] = epilogue(W[M x K] X[K x N]) for the 1x1 convs over token columns behind hsp_conv1d_mfma_f32.
// (A third, LDS-DMA token GEMM of rounds 1-3 was retired in round 4: DESIGN.md 4.4.)
//
// Operands.  W is the packed weight [K][w_ld] (rows fastest, a launch takes rows [0, M)); X is channel-major, read at
// x + b x_bs + k x_cs + n x_ts (the block GEMM needs x_ts = 1 and 16-B addressable rows, and stages out-of-range 16-B
// groups from the zero buffer; the register path takes any column stride and clamps its addresses).  Both kernels run
// v_mfma_f32_32x32x2_f32, so an accumulator register r of lane (l32, half) is row HSP_ACC_ROW(r, half), column l32.
//
// Epilogue, per output element, on operands already in registers (hsp_conv1d_args of include/hsp.h):
//   v = acc + (bias[row] + cbias[b][row])            or, with ln_c1:  hsp_tg_ln_apply below
//   v = act(v)
//   v *= mask (PRE);  v *= cscale;  v *= scale;  v += res;  v *= mask (POST);  v += y (accumulate);  y = v post_scale
// A residual or running sum that is not asked for is added as 0.0f (hsp_epilogue_store of the conv kernels skips the
// addition instead, which keeps a -0.0).  The seven steps are NOT one function of the two kernels: the block GEMM
// multiplies by a mask factor that is 1.0f when the mask is off, so the compiler contracts `v * mask + y` into one fma;
// the register path multiplies under a branch and rounds the product first.  For a mask that is not a power of two
// the two differ in the last bit, so each kernel keeps its own lines.
#pragma once
#include "hsp_device.h"

// ---- tuning bits of this family (hsp_conv1d_args.debug; libhsp_tune.so only, libhsp.so refuses a non-zero word)
// The conv tiles read the same word (HSP_CV_* of hsp_conv1d_mfma_kernel.h); "CV:" marks a value that family uses too.
enum : int32_t {
  HSP_TG_NO_DMA = 1,             // block GEMM: no re-issue of a stage slot (wrong results).  CV: HSP_CV_ONE_CHUNK, the same meaning
  HSP_TG_NO_MFMA = 2,            // both kernels: skip the main loop (wrong results).  CV: HSP_CV_NO_MFMA, the same meaning
  HSP_TG_RG_64x32 = 8,           // register path: force the 64 x 32 tile
  HSP_TG_RG_32x32 = 16,          // register path: force the 32 x 32 tile.  CV: HSP_CV_NO_EPILOGUE, ANOTHER meaning
  HSP_TG_OFF = 128,              // dispatcher: no token GEMM at all (conv tiles)
  HSP_TG_BG_128x128 = 1 << 18, HSP_TG_BG_128x64 = 1 << 19, HSP_TG_BG_64x128 = 1 << 21, HSP_TG_BG_64x64 = 1 << 23,   // block GEMM: force a tile shape
                                 // CV: 1 << 18 is HSP_CV_SHUF_SCALAR and 1 << 21 is HSP_CV_NO_HALF_CU, OTHER meanings
  HSP_TG_STAMPS = 1 << 20,       // both kernels: cycle-counter stamps of one workgroup -> a.filt
  HSP_TG_BG_OFF = 1 << 22,       // block GEMM: takes nothing
  HSP_TG_RG_ANY_SIZE = 1 << 24,  // dispatcher: ask the register path whatever the launch size
  HSP_TG_BG_LN_NO_STATS = 1 << 25,   // block GEMM: the LayerNorm variant without its statistics (wrong results)
};
#ifdef HSP_TUNING
#define HSP_TG_DBG(a, bit) (((a).debug & (bit)) != 0)
#else
#define HSP_TG_DBG(a, bit) false
#endif

// ---- host side
int hsp_rgemm_try(const hsp_conv1d_args& a, hipStream_t s, int32_t* plan_out);    // hsp_rgemm.hip
int hsp_bgemm_try(const hsp_conv1d_args& a, hipStream_t s, int32_t* plan_out);    // hsp_bgemm.hip

// tiles of bm x bn outputs in the launch, every utterance tiled on its own
inline int64_t hsp_tile_count(const hsp_conv1d_args& a, int bm, int bn) {
  return (int64_t)((a.M + bm - 1) / bm) * ((a.ncols + bn - 1) / bn) * a.B;
}

// a 1x1 token GEMM: plain rows, no prologue, one output column per column of x, a complete LayerNorm / mask request
inline bool hsp_tg_eligible(const hsp_conv1d_args& a) {
  return a.K == 1 && a.stride == 1 && a.pad == 0 && a.prologue == HSP_PRO_NONE && a.rows == HSP_ROWS_PLAIN &&
         a.x_ts >= 1 && a.Lin == a.ncols && a.Lout == a.ncols && (!a.ln_c1 || a.ln_eps > 0.0f) &&
         (a.mask_mode == HSP_MASK_NONE || a.mask);
}

// ---- device side
// Fused input LayerNorm.  t1 / t2 = sums of (x - pivot) and (x - pivot)^2 over the K channels of a column (pivot =
// the column's channel 0: the shift keeps t2 / K - dm^2 from cancelling at a large mean).
__device__ __forceinline__ void hsp_tg_ln_finish(float t1, float t2, int K, float pivot, float eps, float& mean, float& rstd) {
  const float dm = t1 / (float)K;
  mean = pivot + dm;
  const float var = fmaxf(t2 / (float)K - dm * dm, 0.0f);
  rstd = 1.0f / sqrtf(var + eps);
}
// v = rstd (acc - mean ln_c1[row]) + (bias + cbias)
__device__ __forceinline__ float hsp_tg_ln_apply(float rstd, float mean, float c1, float acc, float bv) {
  return fmaf(rstd, fmaf(-mean, c1, acc), bv);
}
