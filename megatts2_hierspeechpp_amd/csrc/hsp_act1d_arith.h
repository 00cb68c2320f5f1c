// The arithmetic of the wave-per-segment Activation1d (act1d_seg_kernel, hsp_pointwise.hip), stated once for the two
// kernels that run it: the stand-alone launch and the conv kernel's activation epilogue (HSP_EPI_ACT,
// hsp_conv1d_epilogue.h).  Same taps, same FMA order, same hsp_snake_hw: equal inputs give equal bits in both.
//   raw[j] = x[clamp(p0 - 8 + j)]                  the raw window of a segment that starts at output p0
//   a2[j]  = a[clamp(2 p0 - 5 + j, 0, 2L - 1)]     the 2x-rate snake signal; slot 4 l of lane l is the first tap of
//                                                  outputs (p0 + 2 l, p0 + 2 l + 1)
#pragma once
#include "hsp_device.h"

typedef float act_f32x2 __attribute__((ext_vector_type(2)));

// the up filter with its x2 gain folded in (exact) and the down filter, as the pairs the packed FMAs take
#define HSP_ACT2_TAPS(filt, hu, hd)                                              \
  _Pragma("unroll") for (int i = 0; i < 6; ++i) {                                \
    (hu)[i] = act_f32x2{2.0f * (filt)[10 - 2 * i], 2.0f * (filt)[11 - 2 * i]};   \
    (hd)[i] = act_f32x2{(filt)[12 + 2 * i], (filt)[13 + 2 * i]};                 \
  }

// Phases B and C are MACROS: as __forceinline__ functions the stand-alone kernel compiles to another instruction
// schedule (the scalar tap loads move, registers are renumbered); expanded in place its ISA is what it was.
//
// phase B: lane pair pi owns a[2q+1 .. 2q+4], q = p0 - 3 + 2 pi (odd(q), even(q+1), odd(q+1), even(q+2)) -- slots
// 4 pi .. 4 pi + 3 of a2, one b128 write; its inputs x[q-2 .. q+4] sit in four aligned b64 reads of the raw window
#define HSP_ACT2_UP(a2, raw, pi, hu, kf, kb)                                                                         \
  {                                                                                                                  \
    const act_f32x2* rp = reinterpret_cast<const act_f32x2*>((raw) + 2 * (pi) + 2);                                  \
    const act_f32x2 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];                                                  \
    const float xv[7] = {r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y}; /* x[q-2 .. q+4] */                              \
    act_f32x2 u0 = {0.0f, 0.0f}, u1 = {0.0f, 0.0f};                                                                  \
    _Pragma("unroll") for (int i = 0; i < 6; ++i) {                                                                  \
      u0 = __builtin_elementwise_fma(act_f32x2{xv[i], xv[i]}, (hu)[i], u0);         /* a[2q+1], a[2q+2] */           \
      u1 = __builtin_elementwise_fma(act_f32x2{xv[i + 1], xv[i + 1]}, (hu)[i], u1); /* a[2q+3], a[2q+4] */           \
    }                                                                                                                \
    *reinterpret_cast<float4*>((a2) + 4 * (pi)) = make_float4(hsp_snake_hw(u0.x, kf, kb), hsp_snake_hw(u0.y, kf, kb), \
                                                              hsp_snake_hw(u1.x, kf, kb), hsp_snake_hw(u1.y, kf, kb)); \
  }

// phase C: yo = outputs (p0 + 2 l2, p0 + 2 l2 + 1): y[p0 + s] = sum_k hd[k] * a2[2 s + k]
#define HSP_ACT2_DOWN(yo, a2, l2, hd)                                                                                \
  {                                                                                                                  \
    const float4* ap = reinterpret_cast<const float4*>((a2) + 4 * (l2));                                             \
    const float4 q0 = ap[0], q1 = ap[1], q2 = ap[2];                                                                 \
    const act_f32x2 q3 = *reinterpret_cast<const act_f32x2*>((a2) + 4 * (l2) + 12);                                  \
    const act_f32x2 aw[7] = {{q0.x, q0.y}, {q0.z, q0.w}, {q1.x, q1.y}, {q1.z, q1.w}, {q2.x, q2.y}, {q2.z, q2.w}, q3}; \
    act_f32x2 s0 = {0.0f, 0.0f}, s1 = {0.0f, 0.0f};                                                                  \
    _Pragma("unroll") for (int k = 0; k < 6; ++k) {                                                                  \
      s0 = __builtin_elementwise_fma(aw[k], (hd)[k], s0);                                                            \
      s1 = __builtin_elementwise_fma(aw[k + 1], (hd)[k], s1);                                                        \
    }                                                                                                                \
    (yo) = make_float2(s0.x + s0.y, s1.x + s1.y);                                                                    \
  }
