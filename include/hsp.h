/*
 * hsp.h -- C ABI of libhsp.so, the MI355X (gfx950) kernel library behind the
 * HierSpeech++ waveform-generation hot path.
 *
 * The reference (liuhuang31/Megatts2_HierSpeechpp) has no FFI/plugin layer: its hot
 * path is a chain of torch ops called from Python nn.Modules.  The
 * entry points below are therefore "what the reference's FFI for this path would
 * bind": one launcher per fused op, plain pointers + sizes + a hipStream_t, no torch
 * types.  Each one names the reference code it replaces.  The Python host side
 * (megatts2_hierspeechpp_amd/_lib.py) binds them with ctypes; INTEGRATION.md shows the
 * stub a maintainer of the reference would add.
 *
 * Conventions
 *   - all tensors fp32, device pointers, layout (B, C, T) with T fastest unless stated;
 *     strides are in ELEMENTS
 *   - launchers never allocate, never synchronise, never throw; they return 0 on
 *     success, HSP_EINVAL (-1) on bad arguments, or the positive hipError_t of the launch
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream)
 *   - thread-compatible: the only global state is a per-device "dynamic LDS limit raised" flag per kernel
 *     (atomic, idempotent); the first launch of a kernel on a device must not happen inside a stream capture
 *
 * Limits a caller can reach (each is checked: the entry point returns HSP_EINVAL, it never computes garbage)
 *   - first launch outside a capture: run one eager pass of a model before capturing it into a hipGraph (the
 *     dynamic-LDS limit of a kernel is raised with hipFuncSetAttribute on its first launch per device)
 *   - hsp_conv1d_mfma_f32: stride 1; halo (K - 1) * dil + 3 <= 125 columns (plain and gated rows); one utterance of
 *     a tensor and the packed weight each below 2^31 elements
 *   - hsp_mha_f32: no sequence-length ceiling (score rows that do not fit LDS are walked in key blocks); head dim
 *     <= 256, with or without a relative-position window (the matrix-core kernels serve D <= 128 without a window)
 *   - hsp_lstm_bidir_f32: hidden size H <= 256 (one workgroup of 4 H <= 1024 threads holds the gate rows)
 */
#ifndef HSP_H_
#define HSP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libhsp.so is built with -fvisibility=hidden: exactly the functions declared between this push and the pop at the end
 * of the header are exported (`nm -D --defined-only libhsp.so` lists these names and nothing else; tests/test_host_logic.py). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define HSP_VERSION 104 /* 0.1.4: hsp_sum_sq_f32, hsp_instnorm_prelu_f32, hsp_dwconv_bn_silu_f32 and hsp_istft_ola_f32 are
                           * removed: one prompt is a segment table with one row (hsp_norm_factor_rows_f32 with B = 1 and
                           * the _seg entry points give the same bits); a caller of the four names must move to those.
                           * 0.1.3: hsp_conv1d_args lost the five trailing fields of the modulated input LayerNorm (the
                           * round-6 experiment that 0.1.2 added after w_bs) -- a caller compiled against 102 passes a longer
                           * struct and must be rebuilt; hsp_dftseg_pair_f32 no longer takes inv->y / inv->res (refused).
                           * 0.1.2: hsp_conv1d_args grew those five fields; hsp_dftseg_pair_f32 took inv->y / inv->res and
                           * wrote inv->y; hsp_mha_proj_args and hsp_dftseg_args grew a trailing field each (key_len,
                           * act_len; NULL = the former behaviour) for the row-exact ragged vocoder (hsp_resample_f32 and
                           * hsp_act1d_snakebeta_ragged_f32 only add to the ABI).  0.1.1: hsp_dftseg_args grew a field
                           * (prod3); hsp_cprod3_f32, hsp_cprod3_supported, hsp_dftseg_weight_spectrum_f32,
                           * hsp_dftseg_supported are new.  The version number is pinned by the suite's ABI test. */
#define HSP_EINVAL (-1)

int hsp_version(void);
/* gfx arch string the library was compiled for ("gfx950") */
const char* hsp_arch(void);

/* ---------------------------------------------------------------- conv1d (fused) */

/* prologue applied to the conv INPUT while it is staged in LDS */
enum {
  HSP_PRO_NONE = 0,
  HSP_PRO_LRELU = 1, /* F.leaky_relu(x, slope): DBlock, hierspeechpp_speechsynthesizer.py:336 */
  HSP_PRO_ACT1D = 2, /* Activation1d(SnakeBeta): alias_free_torch/act.py:23-28 + activations.py:107-119 */
  HSP_PRO_SILU = 3   /* nn.SiLU before a Linear: modules.py:402-405 (direct kernel only) */
};

/* pointwise function applied to (acc + bias) in the epilogue */
enum {
  HSP_ACT_NONE = 0,
  HSP_ACT_TANH = 1,      /* Generator tail, hierspeechpp_speechsynthesizer.py:450 */
  HSP_ACT_GELU_TANH = 2, /* FFN_Conv, modules.py:384,400 */
  HSP_ACT_RELU = 3,      /* attentions.FFN, attentions.py:292 */
  HSP_ACT_MISH = 4,      /* StyleEncoder, styleencoder.py:9-10 */
  HSP_ACT_SILU = 5,      /* cond_block, hierspeechpp_speechsynthesizer.py:72 */
  HSP_ACT_SOFTPLUS = 6,
  HSP_ACT_GELU_ERF = 7,  /* exact GELU x Phi(x) of the wav2vec2 producer (HF ACT2FN["gelu"]) */
  /* Not pointwise: the whole anti-aliased Activation1d(SnakeBeta) of hsp_act1d_snakebeta_f32 (2x polyphase up-sample ->
   * snake -> 2x low-pass down-sample, replicate-padded at both ends of every row), applied to the conv's own OUTPUT rows
   * before they leave the workgroup:  y = Activation1d(conv(x) + bias).  It is what the NEXT conv of an AMP pair reads
   * (hierspeechpp_speechsynthesizer.py:380-384: xt = c1(a1(x)); xt = a2(xt)), so xt itself is never written.
   * alpha_exp, beta_inv (per OUTPUT channel, [Cout]) and filt are the activation's; the prologue must be NONE.
   * Column tiles overlap by 16: a tile of BN columns computes conv columns [t (BN - 16) - 8, t (BN - 16) + BN - 8) and
   * stores the BN - 16 activated columns from t (BN - 16) on.  The order of the sum behind every conv column is the
   * plain launch's on the same tile shape and the activation runs the stand-alone kernel's arithmetic: the result is
   * bit-identical to that launch followed by hsp_act1d_snakebeta_f32.
   * hsp_conv1d_mfma_f32 only, on its 32 x 512 and 64 x 256 plain-prologue tiles: a launch with this value always takes
   * one of them (hsp_conv1d_mfma_plan reports it).  Required, else HSP_EINVAL: alpha_exp, beta_inv and filt set;
   * PLAIN rows with M <= 64; stride 1 and "same" padding (Lin == Lout == ncols, 2 pad == (K - 1) dil, (K - 1) dil <= 61);
   * ncols % 4 == 0; y 16-B addressable (y, y_bs, y_cs); an epilogue of bias alone (no cbias, mask, cscale, res,
   * accumulate; scale == post_scale == 1); no fold_cols, w_bs, ln_c1, split_row.  Every other entry point that takes
   * an `act` refuses the value. */
  HSP_ACT_ACT1D = 8
};

/* how packed weight rows map to output channels */
enum {
  HSP_ROWS_PLAIN = 0,    /* row m -> channel m */
  HSP_ROWS_GATE_WN = 1,  /* rows come in 32-blocks (a, b): out = tanh(a)*sigmoid(b); commons.py:107-114 */
  HSP_ROWS_GATE_GLU = 2, /* out = a*sigmoid(b); styleencoder.py:26-31 */
  HSP_ROWS_SHUFFLE = 3   /* ConvTranspose1d as polyphase conv: row m -> (co = m / up, phase = m % up) */
};

enum { HSP_MASK_NONE = 0, HSP_MASK_PRE = 1, HSP_MASK_POST = 2, HSP_MASK_BOTH = 3 };

/*
 * y = epilogue( conv1d( prologue(x) ) )
 *
 * Replaces torch Conv1d / ConvTranspose1d / Linear call sites together with the
 * elementwise work around them: hierspeechpp_speechsynthesizer.py:195-200 (Posterior
 * SF encoder), :292-307 (SourceNetwork), :331-339 (DBlock), :380-384 (AMPBlock1),
 * :430-450 (Generator); modules.py:156-175 (WN), :383-386 (FFN_Conv), :409-410 (DiT
 * residuals), :461,473,486 (coupling); styleencoder.py:26-31,66-78.
 *
 * Weights are pre-folded (weight-norm) and packed by the host as w[K][Cin][w_ld] (w_ld =
 * packed row count, a multiple of 4; a launch computes rows [0, M) of it) in the row
 * order `rows` names.
 *
 * conv:     acc[m, t] = sum_{j<K} sum_{ci<Cin} w[j][ci][m] * xin[ci, t*stride + j*dil - pad]
 *           xin = prologue(x) inside [0, Lin), 0 outside; x is read at
 *           x + b*x_bs + ci*x_cs + i*x_ts
 * epilogue: v = acc + bias[row] + cbias[b*cbias_bs + row]          (row = channel index
 *               of the un-packed layer; GATE modes add both halves before gating)
 *           v = act(v)                       | gate(v_a, v_b) in GATE modes
 *           v *= mask[b*mask_bs + t]         if mask_mode & PRE
 *           v *= cscale[b*cscale_bs + co]    if cscale
 *           v *= scale
 *           v += res[b*res_bs + co*res_cs + t]   if res
 *           v *= mask[...]                   if mask_mode & POST
 *           v += y[...]                      if accumulate
 *           y[b*y_bs + co*y_cs + t] = v * post_scale
 *           (SHUFFLE: co = m / up, t -> up*t + m % up - shuf_pad, bounds-checked to Lout; bias, cbias and cscale
 *            are indexed by co.  M = Cout * up rounded up to a multiple of 4: rows m >= Cout * up are padding and
 *            write nothing.  GATE modes: Cout == gate_half and M == 2 * gate_half, anything else is refused.)
 */
typedef struct hsp_conv1d_args {
  /* input */
  const float* x;
  int64_t x_bs, x_cs, x_ts;
  int32_t B, Cin, Lin;
  /* packed weights */
  const float* w;
  int32_t K, M, dil, pad, stride;
  const float* zeros; /* >= 16 B of zeros, 16-B aligned (MFMA path: source of out-of-range DMA lanes) */
  int32_t w_ld; /* row count of the packed matrix w points into (>= M): lets a launch
                   use a row sub-range [r0, r0+M) by passing w + r0 (r0 % 4 == 0) */
  /* output */
  float* y;
  int64_t y_bs, y_cs;
  int32_t Cout, Lout; /* logical output tensor [B, Cout, Lout] */
  int32_t ncols;      /* conv columns to compute (== Lout except SHUFFLE) */
  /* prologue */
  int32_t prologue;
  float slope;
  const float* alpha_exp; /* [Cin] exp(alpha)              (ACT1D) */
  const float* beta_inv;  /* [Cin] 1/(exp(beta)+1e-9)      (ACT1D) */
  const float* filt;      /* [24]  up filter then down filter (ACT1D) */
  /* epilogue */
  int32_t rows, gate_half, up, shuf_pad;
  const float* bias;
  const float* cbias;
  int64_t cbias_bs;
  int32_t act;
  const float* mask;
  int64_t mask_bs;
  int32_t mask_mode;
  const float* cscale;
  int64_t cscale_bs;
  float scale;
  const float* res;
  int64_t res_bs, res_cs;
  int32_t accumulate;
  float post_scale;
  int32_t debug; /* must be 0: libhsp.so returns HSP_EINVAL otherwise.  The kernel tuning switches this word
                    selects (skip staging / MFMAs / epilogue, force a tile shape) are compiled only into the
                    separate libhsp_tune.so (make tune, -DHSP_TUNING), which tools/ load through HSP_LIB. */
  /* Fused input LayerNorm (1x1 token GEMMs only; any other shape is refused with HSP_EINVAL):
   * y = W LN(x) + b with LN over the Cin channels of every column.  The caller packs
   * w = W diag(gamma), bias = W beta + b and ln_c1[row] = sum_ci w[ci][row]; the kernel takes the
   * column statistics from the staged input tile and applies
   *   v = rstd[t] * (acc[m, t] - mean[t] * ln_c1[row]) + bias[row]      before the activation.
   * nn.LayerNorm -> nn.Linear pairs of ttv_v1/transformer_mega.py:125-131.  NULL = off. */
  const float* ln_c1;
  float ln_eps;
  /* Second output of a 1x1 token GEMM (token-GEMM path only; any other shape is refused with HSP_EINVAL).
   * With split_row > 0 (a multiple of 64) the rows [split_row, Cout) are written to
   *   y2[b][m - split_row][t] = (accumulate2 ? y2 : 0) + (acc[m, t] + bias[m]) [* mask per mask_mode2]
   * while the rows [0, split_row) keep y / res / accumulate / mask_mode (indexed by m).  One GEMM then serves the
   * two halves of modules.WN's res_skip_layers (modules.py:166-174): x = (x + rs[:H]) * mask and out += rs[H:]. */
  int32_t split_row;
  int32_t accumulate2;
  int32_t mask_mode2;
  float* y2;
  int64_t y2_bs, y2_cs;
  /* Column stride of `res` in elements (0 or 1: unit).  Only the register-path token GEMM reads a residual at another
   * stride -- the last layer of the PLM loop adds the last position of every utterance, columns T-1, 2T-1, ... of the
   * layer input, to a [D, B] output without a gather launch in between (ttv_v1/transformer_mega.py:118-131 on the
   * last position only); any other kernel / shape refuses res_ts > 1 with HSP_EINVAL. */
  int64_t res_ts;
  /* Weight stride between the B "utterances" of the batch (elements; 0 = one weight matrix for all of them, as every
   * layer of the reference has).  Non-zero only for the frequency-domain form of a long dilated conv (round 4,
   * hsp_dftseg_*_f32 below), where the batch index is the frequency BIN and every bin has its own [Cin][M] matrix.
   * The implicit-GEMM conv kernel only (the token GEMMs refuse it). */
  int64_t w_bs;
  /* Folded columns (0 = off, 1 = on; additive: HSP_VERSION unchanged).  The column tiles of the launch are cut from the
   * B * ncols virtual columns v = b * ncols + t instead of from every utterance on its own: ceil(B ncols / BN) column
   * tiles where the per-utterance form has B ceil(ncols / BN), i.e. no padded tile at the end of every utterance.
   * Tensors, strides and the order of the sum behind every output element are unchanged: with the same tile shape the
   * result is bit-identical to the launch with 0.  Only the kernels that implement the form take the field -- the block
   * token GEMM (hsp_conv1d_mfma_plan: KC = -2) and the short-sequence conv tiles 64 x 64 / gated 64 x 128 at the 64-
   * column window slack (plan: BM = 64, KC > 0, LDS pitch BN + 64); any other kernel refuses 1 with HSP_EINVAL.  A
   * kernel that implements it falls back to the per-utterance tiling, silently, where the geometry does not fit
   * (ncols % 4 != 0, a window of seams wider than the tile's LDS pitch, ...). */
  int32_t fold_cols;
} hsp_conv1d_args;

/* MFMA (v_mfma_f32_32x32x2_f32, exact fp32) path; stride must be 1, M % 4 == 0.  Behind this entry point: the
 * implicit-GEMM conv kernel (any K / dilation / prologue / row mode) and, for 1x1 convs over token columns (or with
 * ln_c1 / split_row), two token GEMMs -- the register-path kernel (latency-oriented, up to about 1.4 M outputs) and
 * the block token GEMM (64 x 64 / 128 x 128 tiles, from ~96 tiles of 64 x 64 upward, or any size with split_row);
 * hsp_conv1d_mfma_plan tells which one a launch takes. */
int hsp_conv1d_mfma_f32(const hsp_conv1d_args* a, void* stream);
/* VALU path: any shape (Cin = 1, Cout = 1, stride > 1, L = 1 "Linear" cases);
 * rows must be PLAIN; prologue NONE/LRELU/SILU. */
int hsp_conv1d_direct_f32(const hsp_conv1d_args* a, void* stream);
/* which kernel / tile configuration hsp_conv1d_mfma_f32 would pick: writes BM, BN, KC, LDS bytes
 * (KC > 0: the conv kernel's chunk depth; KC = -1: the register-path token GEMM of hsp_rgemm.hip, 32 x 32 or 64 x 32
 * tiles; KC = -2: the block token GEMM of hsp_bgemm.hip, 64 x 64 or 128 x 128 tiles) */
int hsp_conv1d_mfma_plan(const hsp_conv1d_args* a, int32_t out4[4]);

/* --------------------------------------- feature producer of inference_vc.py */
/* y[i] = act(x[i]) (HSP_ACT_*): the GELU that follows the channel LayerNorm of every wav2vec2 feature-encoder
 * layer (HF Wav2Vec2LayerNormConvLayer.forward: conv -> LayerNorm -> GELU). */
int hsp_act_f32(const float* x, float* y, int64_t n, int32_t act, void* stream);
/* y[b, t] = x[b, reflect(t - pad)], t < L + 2 pad : F.pad(audio, (40, 40), "reflect") at inference_vc.py:85.
 * x rows of stride x_bs, y contiguous [B, L + 2 pad]; pad < L. */
int hsp_reflect_pad_f32(const float* x, int64_t x_bs, float* y, int32_t B, int32_t L, int32_t pad, void* stream);
/* F0 conversion of inference_vc.py:80-81,104-105: with V = {f0_src != 0}, W = {f0_trg != 0} (population statistics,
 * numpy's default ddof = 0): out = log(max((f0_src - mean_V) / std_V * std_W + mean_W, 0) + 1) on V and log(1) = 0
 * elsewhere.  One utterance per call (the statistics are per utterance): f0_src [n_src], f0_trg [n_trg]. */
int hsp_f0_convert_f32(const float* f0_src, int32_t n_src, const float* f0_trg, int32_t n_trg, float* out, void* stream);

/* ------------------------------------------------ batched voice conversion (inference_vc.vc_batch; csrc/hsp_vcbatch.hip, and
 * the ragged forms next to their plain ones in csrc/hsp_pointwise.hip and csrc/hsp_mel.hip)
 * Per-row-length forms of the single-utterance steps above and below.  A plain entry point launches the kernel of its
 * ragged form with NULL lengths, so a row of full length is bit-equal through both.  Row lengths are device int64 [B] (values are
 * clamped into [0, the buffer's capacity]), so a fixed-shape batch is capturable with no host read-back.
 * hsp_reflect_pad_ragged_f32: y[b, t] = x[b, reflect(t - pad)] over t < len_b + 2 pad with the reflection at row b's
 *   own end len_b (F.pad(x[b, :len_b], (pad, pad), "reflect")), y[b, t] = 0 on [len_b + 2 pad, Lo).  x rows of stride
 *   x_bs >= L, y rows of stride y_bs >= Lo; Lo <= L + 2 pad, pad < L; lengths NULL = all L; pad < len_b is the
 *   caller's contract.
 * hsp_f0_convert_batch_f32: hsp_f0_convert_f32 on row b = (f0_src[b, :n_src[b]], f0_trg[b, :n_trg[b]]) into
 *   out[b, :n_src[b]], zeros on out[b, n_src[b] : n_max); one launch, row b bit-identical to the single call.
 *   f0_src rows of stride src_bs >= n_max, out rows of stride out_bs >= n_max, f0_trg rows of stride trg_bs
 *   (0 = one track shared by every row; else >= nt_max) holding up to nt_max samples.
 * hsp_stft_frames_ragged_f32: hsp_stft_frames_f32 with row b's own length len_b <= L: T_b = 1 + len_b / hop frames
 *   reflecting at len_b, zero columns on [T_b, f_ld).  T = 1 + L / hop, x rows of stride x_bs >= L; len_b > n_fft / 2
 *   is the caller's contract.  After hsp_power_mel_log_f32 (T_out = T - 1) mel row b has T_b - 1 valid frames.
 * hsp_abs_max_rows_f32: out[b] = max_{i < len_b} |x[b, i]| (0 for an empty row); lengths NULL = all n.
 * hsp_peak_int16_gains: hsp_peak_int16 with row b's gain read from gains[b] (device fp32 [B]). */
int hsp_reflect_pad_ragged_f32(const float* x, int64_t x_bs, const int64_t* lengths, float* y, int64_t y_bs, int32_t B,
                               int32_t L, int32_t pad, int32_t Lo, void* stream);
int hsp_f0_convert_batch_f32(const float* f0_src, int64_t src_bs, const int64_t* n_src, const float* f0_trg,
                             int64_t trg_bs, const int64_t* n_trg, int32_t nt_max, float* out, int64_t out_bs,
                             int32_t B, int32_t n_max, void* stream);
int hsp_stft_frames_ragged_f32(const float* x, int64_t x_bs, const int64_t* lengths, const float* window, float* frames,
                               int32_t B, int32_t L, int32_t n_fft, int32_t hop, int32_t T, int32_t f_ld, void* stream);
int hsp_abs_max_rows_f32(const float* x, int64_t x_bs, const int64_t* lengths, float* out, int32_t B, int64_t n,
                         void* stream);
int hsp_peak_int16_gains(const float* x, int64_t x_bs, const int64_t* lengths, const float* gains, int16_t* out,
                         int64_t o_bs, int32_t B, int64_t n, void* stream);

/* ----------------------------------------------- prompt denoiser (MP-SENet) */
/* The parts of denoiser/ that are neither convolutions nor GEMMs (those run on hsp_conv1d_mfma_f32 /
 * hsp_conv1d_direct_f32 / hsp_mha_f32 / hsp_layernorm_mod_f32).  These four are pointwise; the operations that read
 * across frames take a segment table and follow below. */
/* mag[f][t] = |z|^compress, pha[f][t] = angle(z) for z = spec[f][t] + i spec[n_freqs + f][t] (row pitch s_ld):
 * mag_pha_stft of denoiser/infer.py:12-24 after the DFT product; the imaginary part of the DC and Nyquist rows is
 * taken as +0, as a real FFT returns it.  mag, pha contiguous [n_freqs, T]. */
int hsp_mag_pha_f32(const float* spec, int64_t s_ld, float* mag, float* pha, int32_t n_freqs, int32_t T, float compress,
                    void* stream);
/* out[t][f] = mag[t][f] * beta * sigmoid(slope[f] * m[t][f]): LearnableSigmoid_2d (denoiser/utils.py:44-53) and the
 * mask product of generator.py:140; all [T, F] contiguous. */
int hsp_lsigmoid_mul_f32(const float* m, const float* slope, float beta, const float* mag, float* out, int32_t T,
                         int32_t F, void* stream);
/* out[i] = atan2(y[i], x[i]): PhaseDecoder.forward (denoiser/generator.py:96). */
int hsp_atan2_f32(const float* y, const float* x, float* out, int64_t n, void* stream);
/* re[f][t] = mag[f][t]^power cos(pha[f][t]), im likewise with sin (row pitches re_ld / im_ld): denoised_com of
 * generator.py:142-143 (power 1) and the decompression of mag_pha_istft (infer.py:26-29, power 1 / compress). */
int hsp_polar_f32(const float* mag, const float* pha, float power, float* re, int64_t re_ld, float* im, int64_t im_ld,
                  int32_t F, int32_t T, void* stream);

/* ---- the operations of the prompt denoiser that read across frames.  B utterances lie end to end
 * along T in one [C, T_tot, F] tensor with zero gap rows between neighbours (denoiser.infer.denoise_batch); one prompt
 * (denoiser.infer.denoise) is the table with one row (0, T) and no gap.  The segment table holds (first row, T_b) per
 * utterance as int32 [B][2], ascending and disjoint: `seg` is the device copy the kernels read, `seg_host` the host
 * copy the launcher checks -- HSP_EINVAL, before any HIP call, for a null pointer, B < 1, T_b < 1, a negative,
 * descending or overlapping segment or one past T_tot.  Both copies must hold the same values.  Row lengths in samples
 * are device int64 [B], clamped into [0, L] as in the batched voice conversion above.  Nothing here reads back, so a
 * fixed set of lengths can be captured in a hipGraph. */
/* scale[b] = sqrt(len_b / sum_i x[b][i]^2) and inv[b] = 1 / scale[b]: the norm factor of denoiser/infer.py:4 per row
 * (the sum accumulated in double and rounded to fp32, both factors formed in double from it and rounded once).  A
 * silent or empty row gets scale = inv = 0 (denoise() reads scale[0] back and raises there). */
int hsp_norm_factor_rows_f32(const float* x, int64_t x_bs, const int64_t* lengths, float* scale, float* inv, int32_t B,
                             int64_t L, void* stream);
/* hsp_stft_frames_ragged_f32 into ONE frame matrix [n_fft, f_ld]: row b's T_b = 1 + len_b / hop frames, reflected at
 * len_b and multiplied by scale[b] (NULL = no scaling; bit-equal to hsp_stft_frames_f32 on the row then: the three
 * framing entry points compute a column with one device function, csrc/hsp_mel.hip), at columns
 * [first_b, first_b + T_b); every other column, gaps included, is written as 0.  x rows of stride x_bs >= L. */
int hsp_stft_frames_packed_f32(const float* x, int64_t x_bs, const int64_t* lengths, const float* scale,
                               const float* window, float* frames, const int32_t* seg, const int32_t* seg_host, int32_t B,
                               int64_t L, int32_t n_fft, int32_t hop, int32_t T_tot, int32_t f_ld, void* stream);
/* In place: nn.InstanceNorm2d(C, affine=True) then nn.PReLU(C) with statistics over the T_b x F values of each
 * (segment, channel) of the C planes [T_tot, F] at x + c * x_cs (biased variance, double accumulation as torch's CPU
 * path): denoiser/generator.py:22-23,40-41,47-48,65-66,83-84.  Every row outside the segments is WRITTEN as 0 (never
 * read). */
int hsp_instnorm_prelu_seg_f32(float* x, int64_t x_cs, int32_t C, int32_t T_tot, int32_t F, const int32_t* seg,
                               const int32_t* seg_host, int32_t B, const float* gamma, const float* beta,
                               const float* slope, float eps, void* stream);
/* Zeros on every row outside the segments of the C planes [T_tot, F] at x + c * x_cs; nothing is read. */
int hsp_zero_gaps_f32(float* x, int64_t x_cs, int32_t C, int32_t T_tot, int32_t F, const int32_t* seg,
                      const int32_t* seg_host, int32_t B, void* stream);
/* y = SiLU(BatchNorm1d_eval(depthwise Conv1d(x))) over contiguous [A, C, N] with N the packed axis (T_tot = N); w [C, K]
 * (K odd, padding K / 2), batch-norm as y = x alpha + (bias - mean alpha), alpha = weight / sqrt(var + eps):
 * denoiser/conformer.py:34-37.  Taps outside the element's own segment read as 0 whatever the gap width; positions
 * outside the segments are written as 0. */
int hsp_dwconv_bn_silu_seg_f32(const float* x, const float* w, const float* bias, const float* bn_weight,
                               const float* bn_bias, const float* bn_mean, const float* bn_var, float bn_eps, float* y,
                               int32_t A, int32_t C, int32_t N, int32_t K, const int32_t* seg, const int32_t* seg_host,
                               int32_t B, void* stream);
/* torch.istft(center=True) after the inverse DFT, per segment of frames [n_fft, f_ld >= T_tot]: out[b][n] = inv[b] *
 * sum_t frames[k][first_b + t] w[k] / sum_t w[k]^2 with k = n + n_fft / 2 - t hop in [0, n_fft) over the frames t of
 * segment b only, n < hop (T_b - 1) (denoiser/infer.py:30-31 and the division by the norm factor at :9; inv device
 * fp32 [B], NULL = 1); zeros on [hop (T_b - 1), n_max).  out rows of stride out_bs >= n_max >= hop (T_b - 1). */
int hsp_istft_ola_seg_f32(const float* frames, int64_t f_ld, const float* window, const float* inv, float* out,
                          int64_t out_bs, int64_t n_max, int32_t n_fft, int32_t hop, const int32_t* seg,
                          const int32_t* seg_host, int32_t B, int32_t T_tot, void* stream);

/* ------------------------------------------------------- anti-aliased activation */
/* y = DownSample2x(SnakeBeta(UpSample2x(x))): alias_free_torch/act.py:23-28,
 * resample.py:25-33,47-49, filter.py:86-95, activations.py:107-119.  x, y contiguous
 * [B, C, L]; filt = 12 up taps then 12 down taps. */
int hsp_act1d_snakebeta_f32(const float* x, float* y, int32_t B, int32_t C, int32_t L,
                            const float* alpha_exp, const float* beta_inv, const float* filt,
                            void* stream);
/* The same on a ragged batch: row b is valid over [0, lens[b]) (device int64 [B], clamped to [1, L]).  Reads clamp at
 * lens[b] - 1 -- the replicate pad of the call on the row cut to that length, which row b then equals -- and the
 * outputs at t >= lens[b] are written as 0.  Needs L % 4 == 0 and 16-B aligned x, y (else HSP_EINVAL). */
int hsp_act1d_snakebeta_ragged_f32(const float* x, float* y, int32_t B, int32_t C, int32_t L, const int64_t* lens,
                                   const float* alpha_exp, const float* beta_inv, const float* filt, void* stream);
/* per-channel constants of SnakeBeta(alpha_logscale=True): activations.py:113-117 */
int hsp_snake_consts_f32(const float* alpha_log, const float* beta_log, float* alpha_exp,
                         float* beta_inv, int32_t C, void* stream);

/* ------------------------------------------------------------------ weight prep */
/* w[r, :] = g[r] * v[r, :] / ||v[r, :]||_2 : torch.nn.utils.weight_norm (dim 0), recomputed
 * on every forward by the reference; folded once here. */
int hsp_fold_weight_norm_f32(const float* v, const float* g, float* w, int32_t rows, int32_t cols,
                             void* stream);
/* dst[i] = map[i] >= 0 ? src[map[i]] : 0   (weight re-layout with a host-built index map) */
int hsp_gather_f32(const float* src, const int32_t* map, float* dst, int64_t n, void* stream);

/* ------------------------------------------------------------------- small ops */
/* mask[b, t] = t < length[b] : commons.sequence_mask commons.py:128-132 (as float) */
int hsp_sequence_mask_f32(const int64_t* length, float* mask, int32_t B, int32_t T, void* stream);
/* y[b, c, t] = x[b, C-1-c, t] : modules.Flip modules.py:270-277 */
int hsp_flip_channels_f32(const float* x, float* y, int32_t B, int32_t C, int32_t T, void* stream);
/* z = (m + noise * exp(logs) * noise_scale) * mask; stats = [B, 2C, T] (m then logs):
 * hierspeechpp_speechsynthesizer.py:201-202, 687 */
int hsp_sample_prior_f32(const float* stats, const float* noise, const float* mask, float* z,
                         int32_t B, int32_t C, int32_t T, float noise_scale, void* stream);

/* ------------------------------------------------ seeded prior noise (additive: HSP_VERSION unchanged)
 * The standard-normal noise n[b, c, t] of the prior sample as a counter-based stream.  Row b, channel c (0-based),
 * frame t (0-based), seed s = seeds[b] (int64, two's complement):
 *   key     = (low 32 bits of s, high 32 bits of s)
 *   counter = (t >> 2, c, 0, 1).  The last word names this stream: the draws of "sampled PLM decoding" below use
 *             (i >> 2, j, 0, 0), so one seed serves both without a shared counter.
 *   w0..w3  = Philox4x32-10(counter, key).  Frames with t & 3 in {0, 1} use the pair (w0, w1), frames with t & 3 in
 *             {2, 3} the pair (w2, w3).  For a pair (wa, wb):
 *               u1 = ((wa >> 9) + 0.5) 2^-23   in (0, 1), exact in fp32
 *               u2 = (wb >> 8) 2^-24           in [0, 1), exact
 *               r  = sqrt(-2 ln u1)            <= sqrt(48 ln 2) = 5.768
 *             the even frame of the pair gets r cos(2 pi u2), the odd frame r sin(2 pi u2) (Box-Muller).  The device
 *             evaluates these in fp32 as cospi / sinpi of 2 u2, so no rounded 2 pi enters.
 * n[b, c, t] depends on (s, c, t) only: not on B, T, the row's position in the batch, the launch geometry or the call
 * history; frames 0 .. T - 1 of a longer row are its first T frames.  `seeds` is read from device memory when the
 * kernel runs (a captured graph replays with new seeds after a copy).  One thread owns a group of four frames of one
 * (b, c) and moves it with one 16-byte access where every row is 16-byte addressable (T % 4 == 0, 16-byte aligned
 * bases), with scalar accesses otherwise.  HSP_EINVAL (nothing launched) on a NULL pointer or a size <= 0.
 *
 * out[b, c, t] = n[b, c, t], contiguous [B, C, T]. */
int hsp_randn_rows_f32(const int64_t* seeds, float* out, int32_t B, int32_t C, int32_t T, void* stream);
/* hsp_sample_prior_f32 with the noise drawn in registers: z = (m + n * exp(logs) * noise_scale) * mask with n as above;
 * no noise tensor is written or read.  The draw and the formula are the functions the two launches above run, so the
 * result equals hsp_sample_prior_f32 on the output of hsp_randn_rows_f32 for the same seeds bit for bit. */
int hsp_sample_prior_seeded_f32(const float* stats, const int64_t* seeds, const float* mask, float* z,
                                int32_t B, int32_t C, int32_t T, float noise_scale, void* stream);
/* LayerNorm over C (no affine) then optional mask, then x*(1+scale)+shift with per-(b,c)
 * scale/shift: modules.py:346-347, 396, 398, 409-410.  gamma/beta (per-channel affine,
 * modules.py:19-31) optional. */
int hsp_layernorm_mod_f32(const float* x, float* y, int32_t B, int32_t C, int32_t T, float eps,
                          const float* mask, const float* shift, const float* scale, int64_t mod_bs,
                          const float* gamma, const float* beta, void* stream);
/* softmax(q^T k * qk_scale [masked]) v per (b, head); q,k,v,o are channel-major
 * [B, H*D, T] views (strides in elements).  mask, if given, is the key/query validity
 * [B, T]: scores where mask_q*mask_k == 0 are set to -1e4 (attentions.py:174-175).
 * Without mask: timm 0.6.13 Attention (modules.py:409).  Optional relative-position
 * window (emb_rel_k/v [2w+1, D]): attentions.py:165-170,183-186.
 * No length ceiling: score rows that do not fit the CU's LDS are walked in key blocks with an online softmax.
 * Head dim D <= 256 on every path (D > 256 is refused with HSP_EINVAL, windowed or not, at any length): the
 * matrix-core kernels serve D <= 128 without a window, the scalar kernels a window or D in 129 .. 256. */
typedef struct hsp_mha_args {
  const float *q, *k, *v;
  float* o;
  int64_t q_bs, k_bs, v_bs, o_bs; /* batch strides; channel stride is Tq / Tk (contiguous rows) */
  int32_t B, H, D, Tq, Tk;
  float qk_scale;
  const float* mask_q;
  const float* mask_k; /* [B, Tq], [B, Tk] or NULL */
  const float* rel_k;
  const float* rel_v;
  int32_t window;                 /* w > 0 with rel_k / rel_v.  Negative = test hook: -(w + 1) forces the key-streaming
                                     kernels (which otherwise serve only the lengths the whole-row kernels cannot hold) */
  int64_t q_cs, k_cs, v_cs, o_cs; /* channel strides; 0 = contiguous rows (Tq / Tk).  A larger stride lets the
                                     utterances of a batch sit side by side on the column axis of one
                                     [C][B*T] matrix (batch stride T): the layout of the PLM loop */
  const float* mask_dense;        /* optional [B][Tq][Tk] (batch stride mask_dense_bs >= Tq * Tk, shared by the heads):
                                     the reference's general ``attn_mask`` (attentions.py:147-155,174-175): scores where
                                     it is 0 become -1e4.  NULL = none.  May be combined with mask_q / mask_k. */
  int64_t mask_dense_bs;
} hsp_mha_args;
int hsp_mha_f32(const hsp_mha_args* a, void* stream);
/* Which kernel hsp_mha_f32 would launch for the struct, without launching (host only): 0 or the refusal
 * hsp_mha_f32 gives, and out4 = {kernel (HSP_MHA_*), NDB, dynamic LDS bytes, workgroups}.  NDB = head-dim blocks the
 * kernel is built for: ceil(D / 32) of the matrix-core kernels (TOK 1..3, the MFMA kernels 1..4), the passes over 128
 * channels (1 or 2) of the scalar ROW kernels.  Both entry points read one decision function. */
#define HSP_MHA_TOK 0         /* mha_tok_kernel: no mask, no window, 4 <= Tk <= 256, D <= 96 */
#define HSP_MHA_MFMA_WHOLE 1  /* mha_mfma_kernel, all of V staged in LDS */
#define HSP_MHA_MFMA_SLAB 2   /* mha_mfma_kernel, V in 64-key slabs */
#define HSP_MHA_MFMA_STREAM 3 /* mha_mfma_stream_kernel: online softmax over 128-key blocks */
#define HSP_MHA_ROW 4         /* mha_kernel: relative-position window, or D > 128 */
#define HSP_MHA_ROW_STREAM 5  /* mha_stream_kernel: the same over 256-key blocks */
int hsp_mha_plan(const hsp_mha_args* a, int32_t out4[4]);
/* Self-attention over ALL heads + the output projection + its epilogue in ONE launch (csrc/hsp_mhaproj.hip):
 *   o[b, h D + d, i] = sum_j softmax_j(qk_scale q[b, h D + :, i] . k[b, h D + :, j]) v[b, h D + d, j]
 *   y[b, m, i] = ((sum_c wt[m, c] o[b, c, i] + bias[m]) * mask[b, i]) * cscale[b, m] + res[b, m, i]
 * = scaled_dot_product_attention + out_proj + the residual add of the Mega-TTS2 PLM layer
 * (ttv_v1/transformer_mega.py:63-87,121-123: 4 heads x 69) and timm Attention's softmax(q k^T) v + proj followed by
 * `x + gate_msa * attn(.)` of a DiT block (modules.py:397,409: 2 heads x 96).  Any Tk >= 4 (up to 2^20): rows of up to 256
 * keys take the one-pass form, longer ones stream the keys in groups with an online softmax (tested to 1 000 keys).
 * key_len (optional, device int64 [B]): the softmax of utterance b covers keys [0, key_len[b]) only (clamped to [1, Tk]);
 * 64-key groups past it are skipped -- a ragged batch whose rows equal their B = 1 runs; what k / v hold past key_len[b]
 * never reaches a sum (rows of fewer than 4 keys included).  No other mask inside the
 * softmax -- neither query masks nor a dense or causal attn_mask: a caller that needs one uses hsp_mha_f32
 * (mask_q / mask_k / mask_dense) and the projection as two launches.
 * q / k / v: element (b, c, t) at base + b * bs + c * cs + t (channel-major; a batch may sit side by side on the columns
 * of one [C][B * T] matrix: bs = T, cs = row pitch).  wt = the nn.Linear / 1x1-conv weight AS STORED, [M][H D] row-major
 * with row pitch wt_ld (M == H D).  y / res: element (b, m, i) at base + b * bs + m * cs + i * ts, so that the
 * "last position of every utterance" form of the PLM's final layer (Tq = 1, q pointing at column T - 1) writes a
 * [M][B] matrix and reads its residual in place.  mask [B][Tq], cscale [B][M], bias [M], res: optional (NULL).
 * hsp_mha_proj_supported: 1 when a kernel exists for (H, D, M, Tk) -- otherwise the caller issues hsp_mha_f32 and
 * the projection as two launches (hsp_mha_proj_f32 returns HSP_EINVAL). */
typedef struct hsp_mha_proj_args {
  const float *q, *k, *v;
  int64_t q_bs, q_cs, k_bs, k_cs, v_bs, v_cs;
  int32_t B, H, D, Tq, Tk;
  float qk_scale;
  const float* wt;
  int32_t M, wt_ld;
  const float* bias;
  const float* mask;
  int64_t mask_bs;
  const float* cscale;
  int64_t cscale_bs;
  const float* res;
  int64_t res_bs, res_cs, res_ts;
  float* y;
  int64_t y_bs, y_cs, y_ts;
  int32_t debug; /* must be 0 (tuning build only, as hsp_conv1d_args.debug) */
  const int64_t* key_len; /* [B] keys per utterance, or NULL: all Tk */
} hsp_mha_proj_args;
int hsp_mha_proj_f32(const hsp_mha_proj_args* a, void* stream);
int hsp_mha_proj_supported(int32_t H, int32_t D, int32_t M, int32_t Tk);
/* out[b, c] = sum_t x[b, c, t] / sum_t mask[b, t] : styleencoder.py:83-91.  The numerator runs over ALL T frames, the
 * padded ones included, as the reference's temporal_avg_pool does (a caller that wants the padding left out masks x
 * first; a 0/1 mask is not applied to x here).  A row whose mask sums to
 * 0 gets the IEEE quotient the reference's torch.div gives (+-inf, or NaN for 0 / 0); the other rows are unaffected. */
int hsp_masked_mean_f32(const float* x, const float* mask, float* out, int32_t B, int32_t C,
                        int32_t T, void* stream);
/* y[b, c, t] = x[b, c, t] * mask[b, t] : the `x * x_mask` steps (modules.py:407) */
int hsp_mask_mul_f32(const float* x, const float* mask, float* y, int32_t B, int32_t C, int32_t T, void* stream);
/* y = F.interpolate(x, Lout, mode='linear') along T (align_corners=False), fp32 index arithmetic
 * bit-compatible with torch-CPU: speechsr48k/speechsr.py:96 */
int hsp_linear_interp_f32(const float* x, float* y, int32_t B, int32_t C, int32_t Lin, int32_t Lout, void* stream);
/* The same on a ragged batch (SpeechSR in row-exact mode): row b has lin[b] valid inputs and lout[b] valid outputs
 * (device int64 [B]); output t < lout[b] is the call on the row alone when Lin / Lout is that call's ratio (its upper
 * neighbour clamps at lin[b] - 1), outputs t >= lout[b] are 0.  lin[b] is clamped into [1, Lin] and lout[b] into
 * [0, Lout] before use, so no length reads or writes outside the two buffers. */
int hsp_linear_interp_ragged_f32(const float* x, float* y, int32_t B, int32_t C, int32_t Lin, int32_t Lout,
                                 const int64_t* lin, const int64_t* lout, void* stream);
/* y = a*x + b*z elementwise (style interpolation, hierspeechpp_speechsynthesizer.py:682) */
int hsp_axpby_f32(const float* x, const float* z, float* y, float a, float b, int64_t n, void* stream);


/* -------------------------------------------------- Mega-TTS2 PLM loop */
/* x[b, c, j] = cat(tc[b, :, j], emb[codes[b, j]])[c] + alpha[0] * pe_t[c, j] for j < n :
 * the body of Megatts2PLM1.infer up to pos_emb (ttv_v1/t2w2v_transformer.py:710-713) with
 * SinePositionalEmbedding.forward (:510-514).  tc is channel-major with strides (tc_bs, tc_cs, 1);
 * codes is int64 [B, >= n] with row stride codes_bs and holds the go token at column 0;
 * pe_t is the sinusoid table transposed to [Dtc + Demb][P]; x has strides (x_bs, x_cs, 1):
 * (n, B*n) lays the batch side by side on the columns of one [D][B*n] matrix; with x_bs == n and
 * x_cs > B*n the columns [B*n, x_cs) of every row are zeroed (row padding to a multiple of 4). */
int hsp_plm_embed_f32(const float* tc, int64_t tc_bs, int64_t tc_cs, int32_t Dtc, const int64_t* codes,
                      int64_t codes_bs, const float* emb, int32_t Demb, int32_t n_emb, const float* pe_t,
                      int32_t P, const float* alpha, float* x, int64_t x_bs, int64_t x_cs, int32_t B, int32_t n,
                      void* stream);
/* The same for step n >= 2 of the greedy loop with the choice of the PREVIOUS step folded in (one launch per step less):
 * first codes[b, n - 1] = argmax_c logits[b * l_bs + c * l_cs] (first maximal index on ties, as hsp_argmax_f32; the
 * value is also stored to `codes`), then x as above.  `logits` = the n_logits scores of step n - 1
 * (ttv_v1/t2w2v_transformer.py:716-717 followed by :710-713 of the next iteration).
 * n == 1 (round 6) is the ONE-POSITION form of the loop's layer-0 cache: every per-position operand (tc, codes, pe_t, x)
 * points at position t and only that position is chosen and embedded -- a caller that passes n == 1 with un-shifted
 * pointers overwrites its go token. */
int hsp_plm_embed_step_f32(const float* tc, int64_t tc_bs, int64_t tc_cs, int32_t Dtc, int64_t* codes,
                           int64_t codes_bs, const float* emb, int32_t Demb, int32_t n_emb, const float* pe_t,
                           int32_t P, const float* alpha, float* x, int64_t x_bs, int64_t x_cs, int32_t B, int32_t n,
                           const float* logits, int64_t l_bs, int64_t l_cs, int32_t n_logits, void* stream);
/* out[b * out_bs] = argmax_c logits[b * l_bs + c * l_cs], first maximal index on ties :
 * logits.argmax(dim=-1) of the greedy loop (ttv_v1/t2w2v_transformer.py:716-717) */
int hsp_argmax_f32(const float* logits, int64_t l_bs, int64_t l_cs, int32_t B, int32_t N, int64_t* out,
                   int64_t out_bs, void* stream);

/* ------------------------------------------------ sampled PLM decoding (additive: HSP_VERSION unchanged)
 * The decision for row b choosing code column j (go token at column 0) from that step's N <= 1024 logits l, in the
 * order of the GPT-SoVITS sampler logits_to_probs + multinomial_sample_one_no_sync (ttv_v1/utils_gptsovits.py):
 *  1. repetition penalty r (1 = off): for every DISTINCT token c < N among the row's previous codes (columns 1 .. j-1),
 *     l_c <- l_c < 0 ? l_c * r : l_c / r (once per token, however often it occurs);
 *  2. top-p p (>= 1 = off) on the penalised logits: in descending order, ties ordered by LOWER INDEX FIRST (a stable
 *     sort), a token is removed when the inclusive cumulative softmax mass exceeds p (no shift: the crossing token goes
 *     too); the first token is always kept;
 *  3. temperature: divide by max(T, 1e-5);
 *  4. top-k k (0 = off): pivot = the min(k, N)-th largest tempered logit; only tokens strictly BELOW it are removed
 *     (ties with the pivot stay);
 *  5. draw: token = argmax over the kept tokens of (l'_i - ln q_i), lowest index on ties, q_i = -ln u_i ~ Exp(1) with
 *     u_i = (w >> 8) 2^-24 + 2^-25 and w = word (i & 3) of Philox4x32-10(counter (i >> 2, j, 0, 0), key (low, high
 *     32 bits of seeds[b])); u_i = (2 (w >> 8) + 1) 2^-25 is exact in float64, where q_i is computed (never 0).  A draw
 *     depends on (seeds[b], j, i) only: independent of the batch and idempotent.
 * `seeds` is read from device memory when the kernel runs (a captured graph replays with new seeds after a copy).
 * probs (optional, NULL on the product path): probs[b * probs_bs + i] = the kept, normalised distribution after 4. */
typedef struct hsp_sample_args {
  float temperature;
  int32_t top_k;               /* 0 = off */
  float top_p;                 /* >= 1 = off */
  float repetition_penalty;    /* 1 = off */
  const int64_t* seeds;        /* [B] device int64 */
  float* probs;                /* [B, N] or NULL */
  int64_t probs_bs;
} hsp_sample_args;
/* The sampled twin of hsp_plm_embed_step_f32 (both its full and its n == 1 forms): workgroup (b, 0) takes
 * codes[b, n - 1] = the decision above for column j (j = n - 1 in the full form, the position t in the n == 1 form),
 * reading the row's previous codes from the j - 1 entries just before that slot, stores it and embeds.
 * HSP_EINVAL (nothing launched) on top_k < 0, top_p <= 0, repetition_penalty <= 0, a non-finite temperature,
 * n_logits > 1024, j < 1 or NULL seeds. */
int hsp_plm_embed_sample_f32(const float* tc, int64_t tc_bs, int64_t tc_cs, int32_t Dtc, int64_t* codes,
                             int64_t codes_bs, const float* emb, int32_t Demb, int32_t n_emb, const float* pe_t,
                             int32_t P, const float* alpha, float* x, int64_t x_bs, int64_t x_cs, int32_t B, int32_t n,
                             const float* logits, int64_t l_bs, int64_t l_cs, int32_t n_logits, int32_t j,
                             const hsp_sample_args* args, void* stream);
/* The sampled twin of hsp_argmax_f32: out[b * out_bs] = the decision above for column j; the row's previous codes are
 * the j - 1 entries just before out[b * out_bs] (out = &codes[0, j]).  One workgroup per row.  Same refusals. */
int hsp_sample_f32(const float* logits, int64_t l_bs, int64_t l_cs, int32_t B, int32_t N, int64_t* out, int64_t out_bs,
                   int32_t j, const hsp_sample_args* args, void* stream);

/* ------------------------------------------------ causal PLM decoding (additive: HSP_VERSION unchanged)
 * One pre-LN transformer layer of the prosody LM for ONE new position t of B rows, against a K/V cache
 * (csrc/hsp_plm_decode.hip): the layer of ttv_v1/transformer_mega.py:118-132 under the causal mask the reference trains
 * with (ttv_v1/utils_mega.py:21-39, t2w2v_transformer.py:691), where position t attends to positions 0 .. t only and
 * so nothing computed for an older position ever changes.  Per row b, with Dh = D / H:
 *   h       = LayerNorm(x[b]; g1, b1, eps)                               (biased variance, as torch.nn.LayerNorm)
 *   q, k, v = Wq h + bq, Wk h + bk, Wv h + bv
 *   k_cache[b, :, t] = k ;  v_cache[b, :, t] = v
 *   a[h Dh + d] = sum_{j <= t} softmax_j(q_h . k_cache[b, h Dh + :, j] / sqrt(Dh)) v_cache[b, h Dh + d, j]
 *   x1      = x[b] + Wo a + bo
 *   y[b]    = x1 + W2 relu(W1 LayerNorm(x1; g2, b2, eps) + c1) + c2
 * x / y: element (b, c) at base + b * bs + c * cs -- a [1, D, B] matrix is (1, B), column t of a [D, B, Tp] buffer is
 * (Tp, B Tp); y may be x (a row is read whole before it is written).  k_cache / v_cache: element (b, c, j) at
 * base + b * bs + c * cs + j, one pair of buffers per layer, written by the calls for t = 0, 1, ... in order; this call
 * writes column t and reads columns 0 .. t - 1: columns > t are never read (they may hold anything, NaN included),
 * columns < t are never written.  t travels by value, so a captured graph of a fixed-length loop replays.
 * Weights: TRANSPOSED copies of the nn.Linear weights, packed once at finalize, each [in][out] row-major and 16-byte
 * aligned: wqkv_t [D][3 D] = cat(w_q.weight, w_k.weight, w_v.weight)^T with bqkv [3 D] the three biases in that order,
 * wo_t [D][D] = out_proj.0.weight^T, w1_t [D][F] = ff.0.weight^T, w2_t [F][D] = ff.3.weight^T; g1 / b1 / g2 / b2 [D]
 * the two LayerNorms' weight and bias (NOT folded into the GEMMs), bo [D], c1 [F], c2 [D].
 * Three launches on the stream (attention per (row, head); out-proj + feed-forward per (row, slice of F /
 * HSP_PLM_DECODE_SPLIT hidden units); the sum of the slices' partial results), so that a row's weights stream through
 * 4 and then 12 compute units instead of one; every sum of a row is taken in an order that does not depend on B, so row
 * b of a batch equals the call on that row alone bit for bit.  No allocation, no host synchronisation, no global state.
 * The attention launch needs more than 32 KB of LDS from about 3 000 keys on; the first such call on a device raises
 * the kernel's limit (a function attribute, set once), which is not legal inside a stream capture: a graph that reaches
 * such a t is captured after one eager call at a t that large (the loop of Megatts2PLM1.infer run once eagerly does).
 * workspace: caller-provided device scratch, 16-byte aligned, at least the bytes hsp_plm_decode_workspace_bytes gives
 * for (B, D) = 4 B D (1 + HSP_PLM_DECODE_SPLIT); it carries nothing between calls (the calls of one stream may share it).
 * hsp_plm_decode_supported: 1 when kernels exist for the geometry: D a multiple of 4 up to 1024, H dividing D with
 * 3 D / H <= 1024, F a multiple of 4 HSP_PLM_DECODE_SPLIT up to 12288 (the PLM's 276 / 4 / 1104 among them).
 * HSP_EINVAL, nothing launched: a NULL operand (the workspace included); B <= 0 or > 65535; t < 0; t >= cs; a negative
 * stride; an unsupported geometry; a workspace that is too small or not 16-byte aligned; a weight matrix that is not
 * 16-byte aligned; a non-zero debug; t + 1 keys whose scores do not fit one compute unit's LDS (about 36 000 keys at
 * the PLM geometry; its position table ends at 4 000). */
#define HSP_PLM_DECODE_SPLIT 12
typedef struct hsp_plm_decode_args {
  const float* x;
  int64_t x_bs, x_cs;
  float* y;
  int64_t y_bs, y_cs;
  float *k_cache, *v_cache;
  int64_t bs, cs; /* both caches: batch and channel strides; the time stride is 1 */
  int32_t t, B, D, H, F;
  float eps;
  const float *g1, *b1, *wqkv_t, *bqkv, *wo_t, *bo, *g2, *b2, *w1_t, *c1, *w2_t, *c2;
  void* workspace;
  int64_t workspace_bytes;
  int32_t debug; /* must be 0 (as hsp_conv1d_args.debug) */
} hsp_plm_decode_args;
int hsp_plm_decode_supported(int32_t D, int32_t H, int32_t F);
int64_t hsp_plm_decode_workspace_bytes(int32_t B, int32_t D);
int hsp_plm_decode_layer_f32(const hsp_plm_decode_args* a, void* stream);
/* Per-row positions (ragged request streams from one captured step; additive: HSP_VERSION unchanged).  The three entry
 * points below take the position from device memory, pos int32 [B], read when the kernels run, so one captured graph of
 * a single step serves rows of every length side by side.  Row b is ACTIVE when 0 <= pos[b] <= the call's largest
 * position (a->t / max_pos) and IDLE for every other value (negative ones, INT32_MIN and values above the bound
 * included): an idle row's workgroups return before they touch memory -- nothing of the row (x, y, cache, workspace,
 * codes, pos) is read or written.  That bound check is part of the contract: it is what keeps a stale or wrong
 * position from becoming a store out of range.  The branch is uniform over a workgroup.
 *  - hsp_plm_decode_layer_pos_f32: the layer above with t = pos[b] per row.  a->t is the LARGEST position a row may
 *    hold: it sizes the attention launch's LDS and is checked against cs as above.  An active row runs the device
 *    functions of hsp_plm_decode_layer_f32 with t = pos[b] and equals that call on the row alone bit for bit (y and
 *    column pos[b] of both caches; no other cache column is written).  Refusals as above, plus NULL pos.
 *  - hsp_plm_embed_pos_f32: x[b * x_bs + c * x_cs] = cat(tc[b, :, t], emb[codes[b, t]])[c] + alpha[0] * pe_t[c, t] with
 *    t = pos[b]: hsp_plm_embed_f32 in its one-position form, with UN-shifted tc (strides tc_bs, tc_cs, 1; more than
 *    max_pos columns), codes (row stride codes_bs; clamped into [0, n_emb) as there) and pe_t [Dtc + Demb][P].
 *    HSP_EINVAL: a NULL operand, B <= 0 or > 65535, Dtc / Demb / n_emb <= 0, a negative stride, max_pos < 0 or >= P.
 *  - hsp_plm_choose_advance_f32, after the predict layer: for an active row at t = pos[b], codes[b, t + 1] = the
 *    decision for column j = t + 1 from logits[b * l_bs + c * l_cs], c < N -- args NULL: the first maximal index, by the
 *    device function of hsp_argmax_f32; else the sampled decision above, by the device function of hsp_sample_f32,
 *    with seeds[b] and the row's previous codes (columns 1 .. t) -- and then pos[b] = t + 1 < len[b] ? t + 1 : -1
 *    (len int32 [B], device): pos advances IN PLACE, which is what makes a replayed graph step, and a row that has
 *    chosen column len[b] is finished and idle.  A codes row holds at least max_pos + 2 entries.  HSP_EINVAL: NULL
 *    logits / codes / pos / len, B <= 0 or > 65535, N <= 0, l_cs <= 0, l_bs < 0, max_pos < 0, and with args the
 *    refusals of hsp_sample_f32.
 * All refusals are decided before any HIP call; nothing is launched on one. */
int hsp_plm_decode_layer_pos_f32(const hsp_plm_decode_args* a, const int32_t* pos, void* stream);
int hsp_plm_embed_pos_f32(const float* tc, int64_t tc_bs, int64_t tc_cs, int32_t Dtc, const int64_t* codes,
                          int64_t codes_bs, const float* emb, int32_t Demb, int32_t n_emb, const float* pe_t, int32_t P,
                          const float* alpha, float* x, int64_t x_bs, int64_t x_cs, int32_t B, const int32_t* pos,
                          int32_t max_pos, void* stream);
int hsp_plm_choose_advance_f32(const float* logits, int64_t l_bs, int64_t l_cs, int32_t B, int32_t N, int64_t* codes,
                               int64_t codes_bs, int32_t* pos, const int32_t* len, int32_t max_pos,
                               const hsp_sample_args* args, void* stream);
/* PLM prefill (continue from given codes; additive: HSP_VERSION unchanged).  csrc/hsp_plm_prefill.hip.  When the first n
 * codes of a row are given, every position of that prefix is known at once: each projection of a layer is one GEMM over
 * n columns, and what remains is this entry point.  For ONE row, given the stacked projection q | k | v of its first n
 * positions, it fills the row's slice of the layer's decode caches
 *   k_cache[c, j] = k[c, j] ;  v_cache[c, j] = v[c, j]                                     for j < n, c < D
 * and computes the causal attention output, with Dh = D / H,
 *   out[h Dh + d, i] = sum_{j <= i} softmax_{j <= i}(q[h Dh + :, i] . k[h Dh + :, j] / sqrt(Dh)) v[h Dh + d, j]   for i < n
 * -- what hsp_plm_decode_layer_f32 computes as `a` at t = i, for every i < n at once -- so that a decode that starts at
 * position n reads the caches as if it had stepped through the prefix.
 * qkv: rows q | k | v of the stacked GEMM output, element (r, j) at qkv[r * q_rs + j], r < 3 D.  out: element (c, j) at
 * out[c * o_rs + j]; it may be NULL: then only the caches are filled (the last layer's case: nothing reads the last
 * layer's outputs at prefix positions), with the same bits as a call with out.  k_cache / v_cache: THIS ROW's slice,
 * element (c, j) at base[c * cs + j]: row b of a [D, B, Tp] buffer is base + b * Tp with cs = B * Tp.
 * Columns >= n of the caches, of out and of qkv are never read or written (they may hold NaN); every cache and out
 * element with j < n is written exactly once; qkv is not written.  No dense mask: one workgroup per (tile of 16 queries,
 * head) walks 64-key blocks up to its diagonal and no further, with a running maximum and sum per query; scores and
 * probabilities never reach global memory.  No atomics and every sum in a fixed order: column i of out depends on
 * columns 0 .. i of the head's q / k / v alone -- not on n, not on anything beside the row.  One launch, no allocation,
 * no host synchronisation, no global state; heads of more than 87 channels need more than 32 KB of LDS, and the first
 * such call on a device raises the kernel's limit, which is not legal inside a stream capture.
 * hsp_plm_prefill_attn_supported(D, H): 1 when a kernel exists: H dividing D, D / H <= 128, D <= 8192 (the PLM's
 * 276 / 4 and 64 / 8 among them).
 * HSP_EINVAL, decided before any HIP call, nothing launched: NULL a, qkv, k_cache or v_cache; n < 1; n > q_rs; out given
 * and n > o_rs; n > cs; a negative stride; D % H != 0 or a geometry without a kernel; a non-zero debug;
 * n > HSP_PLM_PREFILL_MAX_N = 65 536 keys (the bound the 32-bit column indices and the grid are checked for; the PLM's
 * position table ends at 4 000). */
#define HSP_PLM_PREFILL_MAX_N 65536
typedef struct hsp_plm_prefill_attn_args {
  const float* qkv;
  int64_t q_rs;
  float* out; /* may be NULL */
  int64_t o_rs;
  float *k_cache, *v_cache;
  int64_t cs; /* both caches: channel stride; the time stride is 1 */
  int32_t n, D, H;
  int32_t debug; /* must be 0 (as hsp_conv1d_args.debug) */
} hsp_plm_prefill_attn_args;
int hsp_plm_prefill_attn_supported(int32_t D, int32_t H);
int hsp_plm_prefill_attn_f32(const hsp_plm_prefill_attn_args* a, void* stream);
/* y[b, c, t] (contiguous) = x[b * s_bs + c * s_cs + t * s_ts] : strided gather, e.g. the last
 * position of every utterance (`[:, -1:, :]`, ttv_v1/t2w2v_transformer.py:716) */
int hsp_copy_strided_f32(const float* x, int64_t s_bs, int64_t s_cs, int64_t s_ts, float* y, int32_t B,
                         int32_t C, int32_t T, void* stream);


/* ---------------------------------------------- t2w2v front-end */
/* out[b, c, t] = sum_k tab_k[id_k[b, t], c] * scale over up to three tables (tab1 / tab2 may be
 * NULL), channel-major output with strides (o_bs, o_cs, 1) : TextEncoder.forward
 * (ttv_v1/t2w2v_transformer.py:127-131); one table with scale 1 = the RVQ codebook lookup of
 * quantizer.decode (ttv_v1/core_vq.py:188-190,380-386). */
int hsp_embedding_sum_f32(const int64_t* id0, const int64_t* id1, const int64_t* id2, const float* tab0,
                          const float* tab1, const float* tab2, int32_t n0, int32_t n1, int32_t n2, float scale,
                          float* out, int64_t o_bs, int64_t o_cs, int32_t B, int32_t C, int32_t T, void* stream);
/* One bidirectional torch.nn.LSTM layer (gate order i, f, g, o; zero initial state), the recurrence
 * only: xproj[b][dir][4H][N] = x W_ih^T + b_ih (a 1x1 GEMM), whh_t[dir][H][4H] = W_hh^T,
 * bhh[dir][4H]; utterance b runs lengths[b] steps (the reverse direction from its own last step, as a
 * packed sequence does) and writes zeros after; out[b, dir*H + j, t] with strides (o_bs, o_cs, 1).
 * nn.LSTM of DurationPredictor (ttv_v1/vits_models.py:101,125) and RangePredictor (ttv_v1/Gaussian.py:100-110). */
/* Limit: H <= 256 (4 H gate rows = the threads of one workgroup); larger returns HSP_EINVAL. */
int hsp_lstm_bidir_f32(const float* xproj, int64_t xp_bs, const float* whh_t, const float* bhh,
                       const int64_t* lengths, float* out, int64_t o_bs, int64_t o_cs, int32_t B, int32_t H,
                       int32_t N, void* stream);
/* dur[b, n] = n < lengths[b] ? ceil(exp(logw[b, n]) * length_scale) : 0, frames[b] = sum_n dur[b, n]
 * (ttv_v1/t2w2v_transformer.py:955-957,972-975).  logw == NULL keeps caller-supplied durations and only
 * zeroes the padding / sums. */
int hsp_duration_f32(const float* logw, int64_t lw_bs, const int64_t* lengths, float length_scale, float* dur,
                     int64_t d_bs, float* frames, int32_t B, int32_t N, void* stream);
/* hsp_duration_f32 with a scale per phone (additive: HSP_VERSION unchanged), scale fp32 [B, N] of row stride sc_bs:
 *   dur[b, n] = ceilf((expf(logw[b, n]) * length_scale) * scale[b, n]) for n < lengths[b], from predicted log-durations;
 *   dur[b, n] = ceilf(dur[b, n] * scale[b, n]) for caller-supplied durations (logw == NULL);
 * zeros from lengths[b] on, frames[b] = sum_n dur[b, n].  Every product is a rounded fp32 product, formed in the order
 * written.  With every scale equal to 1 the result is bit-identical to hsp_duration_f32 (x * 1.0f is x; supplied
 * durations are whole frame counts, which ceilf leaves alone).  HSP_EINVAL: NULL lengths, dur, frames or scale, B < 1,
 * N < 1, sc_bs < N. */
int hsp_duration_scaled_f32(const float* logw, int64_t lw_bs, const int64_t* lengths, float length_scale, float* dur,
                            int64_t d_bs, float* frames, int32_t B, int32_t N, const float* scale, int64_t sc_bs,
                            void* stream);
/* y[b, c, t] = max_{j < k} x[b, c, k t + j], t < L / k : nn.MaxPool1d(kernel_size = 8, stride = 8) of the legacy
 * prosody path (ttv_v1/t2w2v_transformer.py:795,1046).  y contiguous [B, C, L / k]. */
int hsp_maxpool1d_f32(const float* x, int64_t x_bs, int64_t x_cs, float* y, int32_t B, int32_t C, int32_t L,
                      int32_t k, void* stream);
/* codes[b, rep t + r] = argmax_e -(|x_t|^2 - 2 x_t . embed[e] + |embed[e]|^2) for r < rep and rep t + r < Tout:
 * EuclideanCodebook.quantize (ttv_v1/core_vq.py:175-183; first maximum on ties) followed by the "repeat every
 * pooled frame `stride` times, cut to the mel length" of ttv_v1/t2w2v_transformer.py:1051-1052.
 * x [B, D, T] with strides (x_bs, x_cs, 1), embed [bins, D], codes int64 rows of stride c_bs. */
int hsp_vq_nearest_f32(const float* x, int64_t x_bs, int64_t x_cs, const float* embed, int64_t* codes, int64_t c_bs,
                       int32_t B, int32_t D, int32_t T, int32_t bins, int32_t rep, int32_t Tout, void* stream);
/* Prosody codes of a mel in ONE launch (additive: HSP_VERSION unchanged; csrc/hsp_prosody.hip): the arithmetic of
 * SynthesizerTrn.extract_tc_latent_code (ttv_v1/t2w2v_transformer.py:912-929) -- first D mel bins -> PLMConv ->
 * MaxPool1d(8, 8) -> PLMConv -> nearest code, every code held for 8 frames -- for a ragged batch.
 *   x        [B, D, T], strides (x_bs, x_cs, 1): the [:, :D] view of a mel, read in place.  T >= 1, any value.
 *   lengths  device int64 [B], clamped to [0, T]; n below is a row's clamped length.
 *   w1a b1a w1b b1b  conv1 / conv2 of the first PLMConv, w2a b2a w2b b2b of the second: taps [k][D][w_ld] (the packed
 *            layout of hsp_conv1d_args.w with M = w_ld >= D), biases [D] or NULL.  k must be 5 (padding 2).
 *   embed    [bins, D].
 * Per row:  m(t) = t < n;  h = conv2(conv1(x m) m) m, zero padding outside [0, T);
 *           p[c, j] = max_{r < 8} h[c, 8 j + r] for j < ceil(T / 8), frames >= T counting as zeros (the row is as if
 *           zero-padded to a multiple of 8; a window that straddles the row's end takes its maximum over the masked
 *           zeros too);  mp(j) = j < ceil(n / 8);  q = conv2'(conv1'(p mp) mp) mp;
 *           code[j] = first maximum over e of -((|q_j|^2 - 2 q_j . embed[e]) + |embed[e]|^2).
 * Masked values are zeros that the next conv reads, never skipped taps (conv(0) is its bias, hence the mask after
 * every conv).  Every sum has a fixed order (taps ascending, input channels ascending inside a tap, bias last); the
 * distance is the device function hsp_vq_nearest_f32 uses, so both choose the same code for the same q.  A row does not
 * depend on the other rows nor on T beyond its own length.
 * Outputs (either may be NULL, not both):
 *   codes   int64 [B, T], row stride c_bs:            codes[b, t] = t < n ? code[t / 8] : 0   (the reference's lr_codes)
 *   pooled  int64 [B, ceil(T / 8)], row stride p_bs:  pooled[b, j] = j < ceil(n / 8) ? code[j] : 0
 * HSP_EINVAL before any HIP call: NULL a / x / lengths / embed / any of the four tap pointers, both outputs NULL,
 * B <= 0 or > 65535, T <= 0, D <= 0 or > 32, bins <= 0 or > 1024, k != 5, w_ld < D. */
typedef struct {
  const float* x;
  int64_t x_bs, x_cs;
  const int64_t* lengths;
  int32_t B, D, T, k, w_ld, bins;
  const float *w1a, *b1a, *w1b, *b1b, *w2a, *b2a, *w2b, *b2b;
  const float* embed;
  int64_t* codes;
  int64_t c_bs;
  int64_t* pooled;
  int64_t p_bs;
} hsp_prosody_args;
int hsp_prosody_encode_f32(const hsp_prosody_args* a, void* stream);
/* GaussianUpsampling.forward (ttv_v1/Gaussian.py:35-69) with the range clamp
 * min(range, 2 dur), max(., 1e-5) of ttv_v1/t2w2v_transformer.py:961-963: x [B, C, N] (strides x_bs, x_cs, 1)
 * -> out [B, C, T] contiguous, frames t >= frames[b] zero. */
int hsp_gaussian_upsample_f32(const float* x, int64_t x_bs, int64_t x_cs, const float* dur, int64_t d_bs,
                              const float* rng, int64_t r_bs, const int64_t* lengths, const float* frames,
                              float* out, int32_t B, int32_t C, int32_t N, int32_t T, void* stream);
/* y[b, c, t] (contiguous) = x[b, c, t] + cb[b, c] : `x + self.cond(g)` with a per-utterance vector
 * (ttv_v1/vits_models.py:119, ttv_v1/t2w2v_transformer.py:222) */
int hsp_add_cbias_f32(const float* x, int64_t x_bs, int64_t x_cs, const float* cb, int64_t cb_bs, float* y,
                      int32_t B, int32_t C, int32_t T, void* stream);

/* ------------------------------------------------ inference_plm.py:tts post-steps (row A19) */
/* y[i] = x[i] < thr ? 0 : x[i] : pitch clipping `pitch[pitch < log(55)] = 0` (inference_plm.py:166) */
int hsp_zero_below_f32(const float* x, float thr, float* y, int64_t n, void* stream);
/* out[b, i] = (int16) (x[b, i] / max_j |x[b, j]| * 32767 * gain) over the first lengths[b] samples
 * (NULL = all n), zeros after : `audio / max(abs(audio)) * 32767.0 * 0.999` then numpy
 * astype('int16') (inference_plm.py:183-190).  A row whose peak is 0 (all its lengths[b] samples are zero) is
 * written as zeros, which is what the reference's NaN -> astype('int16') gives; values beyond the int16 range
 * (a gain above 1) saturate.  hsp_peak_int16_gains (above) shares the row function and both rules. */
int hsp_peak_int16(const float* x, int64_t x_bs, const int64_t* lengths, float gain, int16_t* out, int64_t o_bs,
                   int32_t B, int64_t n, void* stream);

/* ------------------------------------------------ pitch edit of a log-F0 track (additive: HSP_VERSION unchanged;
 * csrc/hsp_f0_edit.hip).  Neither harness of the reference can move the pitch of a take: the track the
 * vocoder is given -- l = log(f0 + 1), fp32, 0 = unvoiced, 200 frames a second -- is shifted, widened or flattened
 * about its own mean, moved to a target register and drawn over, per row, in ONE launch of one workgroup per row.
 *
 * Per row b: n_b = lengths[b] clamped into [0, n] (device int64 [B]; NULL = all n).  Frame i is voiced when i < n_b and
 * l[b, i] > 0.  Frames at and after n_b are never read.  All arithmetic below is double.
 *   p_i   = log(expm1(l_i))                                  ln Hz of a voiced frame
 *   m_b   = mean of p_i over the voiced frames: each of the 256 threads sums its frames i = t, t + 256, ... in
 *           ascending order, then a halving tree over the threads (128, 64, ..., 1); the voiced count likewise.  The
 *           order depends on the row alone, so row b of a batch is bit-identical to the call on row b alone.
 *   c_b   = log(target_hz[b]) where target_hz[b] > 0, else m_b
 *   p'_i  = c_b + range[b] (p_i - m_b) + (shift[b] + offsets[b, i]) ln2 / 12, clamped into [log f_min, log f_max]
 *   out[b, i] = (float) log1p(exp(p'_i)) for a voiced frame, 0 for an unvoiced one, 0 for n_b <= i < n
 *   mean_hz[b] (may be NULL) = (float) exp(m_b): the geometric mean of the voiced frames in Hz; 0 for a row without one.
 * shift (semitones), range, target_hz: device fp32 [B], each may be NULL = 0, 1, no target.  offsets (semitones): device
 * fp32 [B, n] of row stride off_bs, may be NULL.
 * Identity rule: a row with shift == 0, range == 1, no target (target_hz NULL or not > 0) and offsets == NULL is copied
 * bit for bit over [0, n_b) -- no clamp, whatever the values -- so it takes part in a mixed batch without changing.
 * offsets != NULL is NOT an identity row even where every offset is zero: its voiced frames go through the arithmetic
 * above (and the clamp), and come back within one fp32 ulp, not bit for bit.
 * out may be lf0 (same pointer and row stride).
 * HSP_EINVAL before any HIP call: NULL a, lf0 or out, B < 1 or > 65535, n < 1, a row stride (lf0_bs, out_bs, off_bs
 * with offsets) below n, f_min or f_max not finite, f_min <= 0, f_min >= f_max. */
typedef struct {
  const float* lf0;
  int64_t lf0_bs;
  const int64_t* lengths;
  int32_t B;
  int64_t n;
  const float* shift;
  const float* range;
  const float* target_hz;
  const float* offsets;
  int64_t off_bs;
  float f_min, f_max;
  float* out;
  int64_t out_bs;
  float* mean_hz;
} hsp_f0_edit_args;
int hsp_f0_edit_rows_f32(const hsp_f0_edit_args* a, void* stream);

/* ------------------------------------------------ loudness-normalised output (additive: HSP_VERSION unchanged;
 * csrc/hsp_loudness.hip).  Neither harness of the reference has a loudness rule: scale_norm="lufs" of
 * inference_plm / inference_vc / inference_speechsr replaces the gain of the int16 conversion above by one that
 * brings every row to a target loudness.  Nothing here reads back: meter -> gains -> hsp_peak_int16_gains is three
 * calls on one stream and can be captured in a hipGraph.
 *
 * The meter: ITU-R BS.1770-4 integrated loudness of B mono rows.  K-weighting = the standard's high shelf and
 * high-pass biquads, designed on the host in double from the sample rate (at 48 kHz the standard's own table);
 * 400 ms blocks every 100 ms that lie wholly inside the row; absolute gate at -70 LUFS, relative gate 10 LU below the
 * loudness of the absolute-gated blocks; lufs[b] = -0.691 + 10 log10(mean power of the gated blocks).  A row shorter
 * than 400 ms has no block: its loudness is that of its whole length taken as one block, ungated.  A row with no
 * block above -70 LUFS (and an empty row) reports -inf.  peak[b] = max |x[b, i]| over the row, as
 * hsp_abs_max_rows_f32 gives it.  Row b covers x[b * x_bs + i], i < lengths[b] (device int64 [B], clamped into [0, n];
 * NULL = all n): samples at and after the length are never read, and row b of a batch is bit-identical to the call
 * on row b alone.  The filter recurrence and every sum run in fp64 in a fixed order; lufs and peak are fp32 [B].
 * sample_rate: a multiple of 8000 from 8000 to 48000.  `workspace`: 8-B aligned device memory of at least the byte
 * count the size query returns for (B, n), contents irrelevant; it must stay alive until the call has run.
 * HSP_EINVAL: a null pointer (lengths excepted), B < 1 or > 65535, n < 1, x_bs < n, an unsupported rate, a workspace
 * that is too small or misaligned.
 * The size query returns the byte count, or HSP_EINVAL for B / n outside the ranges above.
 * The coefficient query writes the 10 doubles (b0, b1, b2, a1, a2; a0 = 1) of the shelf, then of the high-pass, as the
 * meter uses them at that rate, into host memory (HSP_EINVAL: NULL or an unsupported rate). */
int64_t hsp_loudness_workspace_bytes(int32_t B, int64_t n);
int hsp_loudness_coefs_f64(int32_t sample_rate, double* coefs);
int hsp_loudness_f32(const float* x, int64_t x_bs, const int64_t* lengths, int32_t B, int64_t n, int32_t sample_rate,
                     void* workspace, int64_t workspace_bytes, float* lufs, float* peak, void* stream);
/* gains[b] = min(10^((target_lufs - lufs[b]) / 20) * peak[b], ceiling): the peak fraction hsp_peak_int16_gains takes as
 * row b's gain, so that the int16 row comes out at target_lufs; limited[b] (int32) = 1 where the ceiling was taken,
 * else 0.  A row whose loudness is not finite (-inf: silence) takes the ceiling -- the 'max' rule -- with limited = 1;
 * its int16 row is zeros either way.  Formed in double, rounded once.  HSP_EINVAL: a null pointer, B < 1, a target
 * that is not finite, a ceiling that is not finite and positive. */
int hsp_loudness_gains_f32(const float* lufs, const float* peak, float target_lufs, float ceiling, float* gains,
                           int32_t* limited, int32_t B, void* stream);

/* ------------------------------------------------ true-peak meter and look-ahead limiter (additive: HSP_VERSION
 * unchanged; csrc/hsp_limiter.hip).  The gain above caps a whole row where its sample peak would pass
 * the ceiling, and the row then comes out under the target.  The limiter pulls down the peaks alone, so that the row
 * can take the gain its loudness asks for, and the ceiling it keeps is a true-peak ceiling.  Launches only, no
 * read-back: the chain meter -> gain -> limiter -> meter -> ... -> int16 (functional.lufs_limit_int16) can be captured.
 *
 * Per row b: n_b = lengths[b] clamped into [0, n] (device int64 [B]; NULL = all n), G_b = gains[b] (device fp32 [B];
 * NULL = 1), y[i] = fl(G_b x[b, i]) for 0 <= i < n_b and y = 0 elsewhere.  Samples at and after n_b are never read.
 *
 * Interpolator.  F = 192000 / rate phases (12, 8, 4 at 16, 24, 48 kHz: the standard's 4x at 48 kHz, held at 192 kHz
 * for the lower rates), Z = 6, 2Z taps per phase: h_p[d] = sinc(d - p/F) kaiser_8(|d - p/F| / Z), d = -(Z-1) ... Z,
 * kaiser_beta(u) = I0(beta sqrt(1 - u^2)) / I0(beta).  The bank is built by the caller in double and passed as device
 * fp32 [F][2Z] (tap d at index d + Z - 1); phase 0 must be the unit impulse exactly, so that a true peak is never
 * below the sample peak.  u[i, p] = sum_d h_p[d] y[i + d] (taps ascending, one fma chain from 0),
 * P[i] = max_p |u[i, p]| for 0 <= i < n_b.
 * True peak: tp[b] = max_i P[i], 0 for an empty row.
 *
 * Limiter.  Ceiling c > 0 (linear, 1 = full scale), look-ahead W samples, 1 <= W <= 480.
 *   p2[i] = max(P[i-1], P[i]), P[-1] = 0
 *   r[i]  = min(1, c / p2[i]), 1 where p2[i] = 0, and r = 1 outside [0, n_b).  The fp32 quotient is stepped down by
 *           one float where fl(r p2) > c: rounding is monotone, so fl(s |y[i]|) <= c for every s <= r[i].
 *   m[k]  = min_{|j| <= W} r[k + j] for every integer k (not only inside the row: padding m with ones at the row ends
 *           would let the mean below rise above r over the last W samples)
 *   s[i]  = min(r[i], 1 - sum_{|j| <= W} w[j] (1 - m[i + j])), w[j] = (1 + cos(pi j / (W + 1))) / (2 W + 2): the
 *           weights sum to 1, so this is the weighted mean of m, formed from 1 - m so that it is exactly 1 where the
 *           limiter is idle (w formed in double and rounded to fp32; the sum runs j ascending in one fma chain from 0)
 *   z[i]  = fl(s[i] y[i]) for i < n_b, 0 for n_b <= i < n;  min_gain[b] = min_i s[i], 1 for an empty row.
 * Every m[i + j] with |j| <= W contains r[i], so the weighted mean is at most r[i] in exact arithmetic; the outer min
 * makes |z[i]| <= c hold in fp32 on every sample.  All windows are finite: one workgroup per (row, tile of 2048
 * samples, origin at the row start) computes its tile from the samples around it.  tp and min_gain are a max and a
 * min, folded over the tiles with integer atomics on the floats' bit patterns into outputs preset on the same stream:
 * bit-reproducible, and row b of a batch is bit-identical to the call on row b alone.
 * hsp_limiter_args.tp (may be NULL): the true peak of y, the limiter's input, from the P it computes anyway.
 * HSP_EINVAL before any HIP call: a null pointer (lengths, gains and hsp_limiter_args.tp excepted), B < 1 or > 65535,
 * n < 1, a row stride below n, F not in {4, 8, 12}, Z != 6, W < 1 or > 480, a ceiling that is not finite and positive. */
typedef struct {
  const float* x;
  int64_t x_bs;
  const int64_t* lengths;
  const float* gains;
  int32_t B;
  int64_t n;
  const float* bank;
  int32_t F, Z, W;
  float ceiling;
  float* y; /* z of the text above: [B, n], row stride y_bs */
  int64_t y_bs;
  float* min_gain;
  float* tp;
} hsp_limiter_args;
int hsp_true_peak_f32(const float* x, int64_t x_bs, const int64_t* lengths, const float* gains, int32_t B, int64_t n,
                      const float* bank, int32_t F, int32_t Z, float* tp, void* stream);
int hsp_limiter_f32(const hsp_limiter_args* a, void* stream);
/* gains_out[b] = gains_in[b] 10^((target_lufs - lufs[b]) / 20), formed in double, rounded once; a loudness that is not
 * finite leaves the gain unchanged.  gains_in NULL: the first gain of a row, from 1 -- and 0 for a row without a
 * loudness (-inf: silence), which is then written as zeros.  gains_out may be gains_in.  HSP_EINVAL: NULL lufs or
 * gains_out, B < 1, a target that is not finite. */
int hsp_gain_update_f32(const float* gains_in, const float* lufs, float target_lufs, float* gains_out, int32_t B,
                        void* stream);
/* The safety scale that ends the chain, and the stats it reports: q[b] = min(1, ceiling / tp[b]) (1 where tp = 0;
 * stepped down like r above, so fl(q tp) <= ceiling), achieved_lufs[b] = lufs[b] + 20 log10 q[b] (in double),
 * true_peak[b] = fl(tp[b] q[b]).  HSP_EINVAL: a null pointer, B < 1, a ceiling that is not finite and positive. */
int hsp_limiter_stats_f32(const float* lufs, const float* tp, float ceiling, float* q, float* achieved_lufs,
                          float* true_peak, int32_t B, void* stream);
/* out[b, i] = (int16) fl(fl(x[b, i] gains[b]) 32767) over the first lengths[b] samples (NULL = all n), zeros after:
 * truncated toward zero and saturating, as hsp_peak_int16 converts.  HSP_EINVAL: NULL x, gains or out, B < 1 or
 * > 65535, n < 1, x_bs < n, o_bs < n. */
int hsp_gain_int16_f32(const float* x, int64_t x_bs, const int64_t* lengths, const float* gains, int16_t* out,
                       int64_t o_bs, int32_t B, int64_t n, void* stream);

/* ------------------------------------------------ prompt ingest: sinc resampling to 16 kHz
 * torchaudio.functional.resample (0.13.1: _get_sinc_resample_kernel + _apply_sinc_resample_kernel) of the reference
 * harnesses (inference_plm.py:124-126, inference.py:122-124, inference_vc.py:76-78,101-103, inference_speechsr.py:32-34):
 *   y[b][i n + p] = sum_{j < n_taps} bank[p * n_taps + j] * xz[b][i o + tap0[p] + j - width],  i n + p < T_b,
 *   xz[b] = x[b] on [0, len_b), zero elsewhere; T_b = ceil(n len_b / o); y[b][t] = 0 for T_b <= t < T_out.
 * o / n = the two rates divided by their gcd; width and the compacted bank (per phase p the n_taps coefficients from
 * tap k = tap0[p] of torchaudio's [n][K = 2 width + o] bank, zero-padded) come from the host builder
 * (functional.sinc_resample_bank).  x rows of stride x_bs >= L, y rows of stride y_bs >= T_out (contiguous in time);
 * lengths int64 [B] (device; NULL = all L): lengths[b] <= L is the caller's contract (values are clamped to [0, L]),
 * as is 0 <= tap0[p] <= K - n_taps (clamped into that range).
 * HSP_EINVAL: o, n < 1, gcd(o, n) != 1, n_taps < 1 or > K, T_out < ceil(n L / o), x_bs < L, y_bs < T_out, B > 65535,
 * or a bank + tap0 + one frame's K input samples above 64 KB of LDS (n n_taps + n + K <= 16384 words; every rate pair
 * of the reference's prompts -- 8 ... 96 kHz -- is far below). */
int hsp_resample_f32(const float* x, int64_t x_bs, const int64_t* lengths, int32_t B, int32_t L, const float* bank,
                     const int32_t* tap0, int32_t n_taps, int32_t o, int32_t n, int32_t width, float* y, int64_t y_bs,
                     int32_t T_out, void* stream);

/* ------------------------------------------------ prompt front-end */
/* torchaudio MelSpectrogram as wrapped by MelSpectrogramFixed (Mels_preprocess.py:8-18; built with the
 * kwargs of inference_plm.py:204-213, applied at :134,150).  Three steps: these two kernels around one
 * hsp_conv1d_mfma_f32 launch (K = 1, Cin = n_fft) against the host-built DFT matrix.
 * frames[b][n][t] = window[n] * x[b][reflect(t * hop + n - n_fft / 2)], t < T = 1 + L / hop
 *   (torch.stft center=True, pad_mode="reflect": index i < 0 -> -i, i >= L -> 2 (L - 1) - i; needs
 *   L > n_fft / 2); x [B, L] contiguous, frames [B, n_fft, f_ld] with row pitch f_ld >= T. */
int hsp_stft_frames_f32(const float* x, const float* window, float* frames, int32_t B, int32_t L, int32_t n_fft,
                        int32_t hop, int32_t T, int32_t f_ld, void* stream);
/* out[b][m][t] = log(sum_f fb[f][m] * (re[b][f][t]^2 + im[b][f][t]^2) + eps), t < T_out :
 *   Spectrogram(power=2) -> MelScale -> log(. + 0.001)[..., :-1].  spec[b] holds rows 0 .. n_freqs-1 (real)
 *   and n_freqs .. 2 n_freqs - 1 (imaginary) with row pitch s_ld and batch stride s_bs; fb [n_freqs, n_mels]
 *   row-major; filter m is non-zero only on bins [f_lo[m], f_hi[m]); out [B, n_mels, T_out] contiguous. */
int hsp_power_mel_log_f32(const float* spec, int64_t s_bs, int32_t s_ld, const float* fb, const int32_t* f_lo,
                          const int32_t* f_hi, float* out, int32_t B, int32_t n_freqs, int32_t n_mels,
                          int32_t T_out, float eps, void* stream);

/* ------------------------------------------------ frequency-domain form of a long dilated Conv1d (round 4)
 * The same-length, stride-1 Conv1d(C -> C, k taps, dilation d, zero padding `pad`) of an AMP block
 * (hierspeechpp_speechsynthesizer.py:340-392) as overlap-save with a 128-point real DFT (csrc/hsp_dftseg.hip):
 *   hsp_dftseg_fwd_f32   x [B][C][L] -> xf [64 bins][2 C][Np]: row part * C + c of bin j holds Re (part 0) / Im (part 1)
 *                        of bin j of channel c (bin 0: DC in part 0, Nyquist in part 1); column n = (b * d + p) * nseg + s
 *                        is segment s of phase p (the samples xpad[p + d i]) of utterance b;
 *                        nseg = ceil(ceil(L / d) / (129 - k)), Np >= B d nseg (a multiple of 4); the transforms write (read) the columns
 *                        [0, B d nseg) only: the padding columns up to Np and a bin plane beyond 2 C Np keep their contents
 *   the channel product  ONE launch over the 64 bins, either of
 *     hsp_cprod3_f32       (round 5, below; the forward transform then runs with prod3 = 1) three real C x C products per bin, or
 *     hsp_conv1d_mfma_f32  B = 64 (the bins), Cin = M = 2 C, K = 1, Lin = Np, w_bs = 4 C^2 -- per bin the real block matrix
 *                          [[Wr, Wi], [-Wi, Wr]] of conj(rfft(w, 128)) (bin 0: [[W_dc, 0], [0, W_nyquist]]); prod3 = 0
 *   hsp_dftseg_inv_f32   yf [64][2 C][Np] -> y [B][C][L] = ((corr + bias[c] + res) [+ y]) * post_scale
 * `dft` = the transform's constant table in device memory (HSP_DFTSEG_TABLE_FLOATS floats; hsp_dftseg_tables_f32 fills
 * the forward and the inverse one into host buffers): the 64 x 64 matrix of the radix-2 half-length real transform in
 * the row order the kernel's accumulator layout wants, then (cos, sin)(2 pi k / 128), k < 32.  fp32 arithmetic on the
 * fp32 MFMA; against float64 as close as the direct fp32 sum (tools/fft_conv_err.py). */
#define HSP_DFTSEG_TABLE_FLOATS 4160
typedef struct hsp_dftseg_args {
  const float* x;   /* forward: input [B][C][L], unit time stride */
  int64_t x_bs, x_cs;
  float* y;         /* inverse: output */
  int64_t y_bs, y_cs;
  int32_t B, C, L;
  int32_t k, dil, pad, nseg, Np;
  float* xf;        /* forward: written; inverse: read */
  int64_t xf_bs;    /* plane (bin) stride >= 2 C Np, and xf_bs * 256 <= 0xffffffff: the kernels address the spectrum with
                       32-bit byte offsets, every hsp_dftseg_* entry point refuses a larger stride */
  const float* dft;
  const float* bias; /* inverse epilogue: optional */
  const float* res;
  int64_t res_bs, res_cs;
  int32_t accumulate;
  float post_scale;
  /* forward, optional: the anti-aliased SnakeBeta in front of the conv (Activation1d; the arguments of
   * hsp_act1d_snakebeta_f32) applied while the input is staged -- the transform of act(x) without act(x) ever being
   * written.  NULL act_alpha_exp = none.  Needs 16-B addressable rows (L, x_bs, x_cs multiples of 4, x 16-B aligned). */
  const float* act_alpha_exp;
  const float* act_beta_inv;
  const float* act_filt;
  /* forward (and the forward half of the pair launch): non-zero = the spectrum feeds hsp_cprod3_f32, whose three-product
   * form cannot keep the two real bins of slot 0 apart by its matrices alone: slot 0 then holds (-E0, -O0) -- the 64-point
   * transforms of the even / odd samples at bin 0 -- instead of (DC, Nyquist) = (E0 + O0, E0 - O0).  0 = the layout above
   * (the [2C x 2C] block product on hsp_conv1d_mfma_f32). */
  int32_t prod3;
  /* forward with act_* (and the forward half of the pair launch): device int64 [B] valid lengths, or NULL.  Row b's
   * activation clamps its reads at act_len[b] - 1 and the transformed input is zero from act_len[b] on: the forward of
   * the row cut to that length (the ragged activation of hsp_act1d_snakebeta_ragged_f32). */
  const int64_t* act_len;
} hsp_dftseg_args;
int hsp_dftseg_fwd_f32(const hsp_dftseg_args* a, void* stream);
int hsp_dftseg_inv_f32(const hsp_dftseg_args* a, void* stream);
int hsp_dftseg_tables_f32(float* fwd, float* inv); /* host buffers of HSP_DFTSEG_TABLE_FLOATS floats each */
/* The two convs of an AMP pair (hierspeechpp_speechsynthesizer.py:380-384: xt = c1(a1(x)); xt = c2(a2(xt))) met in ONE
 * launch: `inv` describes the inverse transform of c1's product (xf = c1's product output, dft = the inverse table, bias;
 * no residual / running sum / post_scale), `fwd` the forward transform of c2's input (xf = c2's spectrum to write, dft =
 * the forward table, act_* = a2, required); same B, C, L.  y / res of `inv` are not used (refused) and x of `fwd` is not
 * read: the tensor between the convs exists in LDS only.  hsp_dftseg_pair_supported: 1 if the pair fits (both unchunked,
 * two row stretches in one CU's LDS, each spectrum below 4 GiB), else 0 and the caller runs hsp_dftseg_inv_f32 +
 * hsp_dftseg_fwd_f32. */
int hsp_dftseg_pair_supported(const hsp_dftseg_args* inv, const hsp_dftseg_args* fwd);
int hsp_dftseg_pair_f32(const hsp_dftseg_args* inv, const hsp_dftseg_args* fwd, void* stream);

/* Is the frequency-domain form available for this geometry?  1 when hsp_dftseg_fwd_f32 / hsp_dftseg_inv_f32 accept the
 * arguments' B, C, L, k, dil, pad, nseg, Np, xf_bs (pointers are not read): dilation <= 8, the spectrum of one launch
 * below 4 GiB (the kernels address it with 32-bit byte offsets: xf_bs * 256 <= 0xffffffff), item counts within int, the
 * LDS stretch of one row chunk within a CU's 160 KB.  0 = the caller keeps the direct conv (hsp_conv1d_mfma_f32), which
 * has no such limit (hierspeechpp_speechsynthesizer.py:377-386,635-651: the reference has no batch or length limit). */
int hsp_dftseg_supported(const hsp_dftseg_args* a);

/* ------------------------------------------------ channel product in three real products per bin (round 5)
 * yf[bin] = conj(rfft(w, 128))[bin] xf[bin] for every bin of a spectrum written by hsp_dftseg_fwd_f32 with prod3 = 1
 * (csrc/hsp_cprod3.hip): with conj(W) = a + i b and X = Xr + i Xi (rows [0, C) / [C, 2C) of a bin's [2C][Np] matrix)
 *     k1 = (a + b) Xr,  k2 = a (Xi - Xr),  k3 = b (Xr + Xi);   Yr = k1 - k3,  Yi = k1 + k2
 * -- 6 C^2 instead of 8 C^2 flops per column and 3 C^2 instead of 4 C^2 weights per bin.  w: [bins][3][C][C], the matrices
 * (a + b), a, b of every bin stored [input channel][output row] (hsp_dftseg_weight_spectrum_f32 writes them; bin 0:
 * (0, W_nyquist, W_dc)).  C a multiple of 64, Np a multiple of 4, xf / w 16-B aligned, xf_bs / yf_bs multiples of 4;
 * `zeros`: >= 16 B of zeros in device memory (the source of DMA lanes past Np).  Replaces the one launch of
 * hsp_conv1d_mfma_f32 with w_bs != 0 between the two transforms (reference: the C x C channel mix of the k = 7 / 11
 * convs of AMPBlock1, hierspeechpp_speechsynthesizer.py:349-364). */
typedef struct hsp_cprod3_args {
  const float* xf;
  float* yf;
  const float* w;
  const float* zeros;
  int64_t xf_bs, yf_bs; /* floats between bins, >= 2 C Np */
  int32_t bins, C, Np;
  int32_t debug;        /* must be 0 (kernel decomposition switches of the tuning build, libhsp_tune.so) */
} hsp_cprod3_args;
int hsp_cprod3_f32(const hsp_cprod3_args* a, void* stream);
int hsp_cprod3_supported(const hsp_cprod3_args* a);
/* The per-bin matrices of a conv from its packed taps w[k][C][w_ld] (hsp_conv1d_args.w of a C -> C conv, row m of input
 * channel ci and tap j at w[(j * C + ci) * w_ld + m]), on the device: 128-point DFT of the k <= 64 taps of every (ci, m)
 * pair in float64 with the twiddles of `tw` (256 doubles in device memory: cos(2 pi n / 128), n < 128, then sin),
 * conjugated and rounded once to fp32.  form HSP_WSPEC_THREE: out [64][3][C][C] for hsp_cprod3_f32; HSP_WSPEC_BLOCK: out
 * [64][2C][2C], the block matrices of the hsp_conv1d_mfma_f32 form (w_bs = 4 C^2).  Every rank of a multi-GPU job derives
 * them from the broadcast taps (the broadcast carries the folded weights only). */
#define HSP_WSPEC_BLOCK 0
#define HSP_WSPEC_THREE 1
int hsp_dftseg_weight_spectrum_f32(const float* w, int32_t k, int32_t C, int32_t w_ld, const double* tw, float* out,
                                   int32_t form, void* stream);

/* ------------------------------------------------ SURVEY.md §8(b) names (dispatching entry points) */
/* The minimum export set of SURVEY.md §8(b) under its own names; each forwards to the entry points above.
 * hsp_conv1d_f32: any weight-normed / plain Conv1d or Linear of the path with its fused prologue / epilogue
 *   (PLAIN or GATE rows); picks the MFMA or the VALU kernel by shape exactly as the host mirror does
 *   (stride != 1, Cin / Cout / Lout < 8 or the SiLU prologue -> hsp_conv1d_direct_f32).
 * hsp_convtr1d_f32: ConvTranspose1d as its polyphase conv (rows == HSP_ROWS_SHUFFLE, weights packed with
 *   hip_layers.convtr_pack_map): hierspeechpp_speechsynthesizer.py:292-300,430-436.
 * hsp_wn_layer_f32: one layer of modules.WN (modules.py:156-175): `in_layer` (HSP_ROWS_GATE_WN: conv + g_l +
 *   tanh*sigmoid), then the residual half `res` (x = (x + rs[:H]) * mask) and the skip half `skip`
 *   (out += rs[H:]) of res_skip_layers; either of the two may be NULL (last layer: skip only).  `res` and `skip`
 *   read in_layer->y.  Issued layer by layer (round 2's one-launch kernel was retired in round 4: it lost to the
 *   separate launches at every batch grouping of the step, profiles/r04_stage_split_policies.txt).
 * hsp_ffn_conv_f32: modules.FFN_Conv (modules.py:382-388) = `fc1` (conv k + bias + pointwise function) then `fc2`
 *   (1x1 conv reading fc1->y, with its mask / per-channel gate / residual epilogue); two launches.
 * hsp_layernorm_modulate_f32: LayerNorm (no affine) + mask + modulate of the DiT blocks (modules.py:346-347,
 *   409-410) = hsp_layernorm_mod_f32 without gamma / beta. */
int hsp_conv1d_f32(const hsp_conv1d_args* a, void* stream);
int hsp_convtr1d_f32(const hsp_conv1d_args* a, void* stream);
int hsp_wn_layer_f32(const hsp_conv1d_args* in_layer, const hsp_conv1d_args* res, const hsp_conv1d_args* skip,
                     void* stream);
int hsp_ffn_conv_f32(const hsp_conv1d_args* fc1, const hsp_conv1d_args* fc2, void* stream);
int hsp_layernorm_modulate_f32(const float* x, float* y, int32_t B, int32_t C, int32_t T, float eps,
                               const float* mask, const float* shift, const float* scale, int64_t mod_bs,
                               void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* HSP_H_ */
