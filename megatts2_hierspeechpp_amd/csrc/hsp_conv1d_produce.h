// The PRODUCER side of the fused conv kernel (part of hsp_conv1d_mfma_kernel.h, which includes it behind Cfg / LdsPlan
// and the barriers): the LDS-DMA staging routines of one chunk (Prod<C>).  The kernel's producer role calls them from
// the chunk loop of each staging form -- folded columns, fast, plain, ACT1D.
#pragma once

namespace hspconv {

// Only the fields the producers touch, held by value (a reference to the by-value kernel
// argument inside an aggregate makes the compiler spill the whole struct to scratch).
struct ProdArgs {
  const float* w;
  const float* zeros;      // >= 16 B of zeros: source of every out-of-range DMA lane
  const float* alpha_exp;
  const float* beta_inv;
  const float* filt;
  int K, Cin, Lin, M, w_ld, x_cs, x_ts, prologue;
  float slope;
};

// LDS-DMA (global_load_lds): each lane supplies a global address, the data lands at
// lds_base + lane * BYTES with no register staging; counted in vmcnt like a load.
#define HSP_GPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define HSP_LPTR(p) ((__attribute__((address_space(3))) void*)(p))
__device__ __forceinline__ void dma16(const float* g, float* l) {
  __builtin_amdgcn_global_load_lds(HSP_GPTR(g), HSP_LPTR(l), 16, 0, 0);
}
__device__ __forceinline__ void dma4(const float* g, float* l) {
  __builtin_amdgcn_global_load_lds(HSP_GPTR(g), HSP_LPTR(l), 4, 0, 0);
}
__device__ __forceinline__ void wait_vm0() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <class C>
struct Prod {
  static constexpr int CPR = C::BM / 4;                       // float4 columns per slab row
  static constexpr int RPI = (64 / CPR) > 0 ? (64 / CPR) : 1;  // slab rows per DMA instruction

  // ---- weight slab of chunk c0 -> Ws[j][kc][BM]: rows (j, c0+kc) of the packed matrix
  static __device__ __forceinline__ void dma_w(const ProdArgs& a, const LdsPlan& P, float* Ws, int c0, int m0, int pw,
                                               int lane) {
    const int r_in = lane / CPR, col = (lane % CPR) * 4;
    const int lipj = P.lkc - __builtin_ctz(RPI);  // log2(instructions per tap); KC >= RPI
    const int ninstr = a.K << lipj;
    const bool colok = m0 + col < a.M;
    const float* wcol = a.w + m0 + col;
    for (int q = pw; q < ninstr; q += C::NPW) {
      const int j = q >> lipj, g = q & ((1 << lipj) - 1);
      const int ci = c0 + g * RPI + r_in;
      const float* src = (colok && ci < a.Cin) ? wcol + (j * a.Cin + ci) * a.w_ld : a.zeros;
      dma16(src, Ws + ((j << P.lkc) + g * RPI) * C::BM);
    }
  }

  // ---- plain window rows -> Xa[kc][xwp] (zero outside [0, Lin) and beyond Cin)
  static __device__ __forceinline__ void dma_x(const ProdArgs& a, const LdsPlan& P, float* Xa, const float* xb, int c0,
                                               int p0, int pw, int lane) {
    const int npr = P.xwp >> 6;
    for (int kc = pw; kc < P.kc; kc += C::NPW) {
      const int ci = c0 + kc;
      const float* xc = xb + ci * a.x_cs;
      for (int i = 0; i < npr; ++i) {
        const int p = p0 + lane + 64 * i;
        const float* src = (ci < a.Cin && p >= 0 && p < a.Lin) ? xc + p * a.x_ts : a.zeros;
        dma4(src, Xa + kc * P.xwp + 64 * i);
      }
    }
  }
  // same with 16-B lanes: the window starts at p0a = p0 rounded down to a multiple of 4 and the
  // tensor is 16-B addressable with Lin % 4 == 0, so every 4-group is fully inside or outside
  static __device__ __forceinline__ void dma_x16(const ProdArgs& a, const LdsPlan& P, float* Xa, const float* xb,
                                                 int c0, int p0a, int pw, int lane) {
    const int ngrp = (P.xw + 3 + 3) >> 2;
    for (int kc = pw; kc < P.kc; kc += C::NPW) {
      const int ci = c0 + kc;
      const float* xc = xb + ci * a.x_cs;
      for (int g0 = 0; g0 < ngrp; g0 += 64) {
        const int g = g0 + lane, p = p0a + 4 * g;
        if (g < ngrp) {
          const float* src = (ci < a.Cin && p >= 0 && p < a.Lin) ? xc + p : a.zeros;
          dma16(src, Xa + kc * P.xwp + 4 * g0);
        }
      }
    }
  }
  // ---- folded columns: one 16-B group per lane (`on`: the lane has one), `xl` = its source in channel 0 and `xs` its
  // channel stride -- the zero buffer and 0 for a group of zeros
  static __device__ __forceinline__ void dma_x_fold(const float* xl, int xs, const float* zeros, int Cin, const LdsPlan& P,
                                                    float* Xa, int c0, int pw, bool on) {
    if (on) {
      for (int kc = pw; kc < P.kc; kc += C::NPW) {
        const int ci = c0 + kc;
        dma16(ci < Cin ? xl + (int64_t)ci * xs : zeros, Xa + kc * P.xwp);
      }
    }
  }
  // ---- fast staging: no per-instruction vector arithmetic.  The fp32 MFMAs of the consumer wave on the same
  // SIMD run on the VALU's own FMA lanes, so every address computation above (a 32-bit multiply, 64-bit adds,
  // selects: ~10 VALU instructions per DMA) is paid in matrix time (measured: 12 % of a k = 3 launch).  Here a
  // lane's byte offset is computed ONCE per tile and each instruction adds it to a wave-uniform base that the
  // scalar unit walks.  Preconditions (wave-uniform, checked by the kernel): the row tile lies inside [0, M),
  // Cin % KC == 0 (no channel tail), 16-B addressable window.
  static __device__ __forceinline__ unsigned w_lane_ofs(int lane, int w_ld) {   // a lane's byte offset within a DMA instruction's rows
    return 4u * (unsigned)((lane / CPR) * w_ld + (lane % CPR) * 4);
  }
  static __device__ __forceinline__ void dma_w_fast(const float* wtile, int w_ld, int Cin, int K, const LdsPlan& P,
                                                    float* Ws, int c0, int pw, unsigned wofs) {
    const int lipj = P.lkc - __builtin_ctz(RPI);
    const int ninstr = K << lipj;
    for (int q = pw; q < ninstr; q += C::NPW) {
      const int j = q >> lipj, g = q & ((1 << lipj) - 1);
      const char* base = reinterpret_cast<const char*>(wtile + (size_t)(j * Cin + c0 + g * RPI) * (size_t)w_ld);  // uniform
      dma16(reinterpret_cast<const float*>(base + wofs), Ws + ((j << P.lkc) + g * RPI) * C::BM);
    }
  }
  // window rows: `xtile` = row 0 of the utterance + p0a (may point before the row: such lanes are masked).
  // Lanes whose 4-group lies outside [0, Lin) take no part (EXEC-masked DMA lanes write nothing); the kernel
  // zero-fills those LDS positions once per tile (zero_x_rows).
  static __device__ __forceinline__ void dma_x16_fast(const float* xtile, int x_cs, int Lin, const LdsPlan& P, float* Xa,
                                                      int c0, int p0a, int pw, int lane) {
    const int ngrp = (P.xw + 3 + 3) >> 2;
    for (int g0 = 0; g0 < ngrp; g0 += 64) {
      const int g = g0 + lane, p = p0a + 4 * g;
      if (g < ngrp && p >= 0 && p < Lin) {
        const unsigned xofs = 16u * (unsigned)lane;
        for (int kc = pw; kc < P.kc; kc += C::NPW) {
          const char* base = reinterpret_cast<const char*>(xtile + (size_t)(c0 + kc) * (size_t)x_cs + 4 * g0);  // uniform
          dma16(reinterpret_cast<const float*>(base + xofs), Xa + kc * P.xwp + 4 * g0);
        }
      }
    }
  }
  // rows this wave stages (kc = pw, pw + NPW, ...) of BOTH window buffers <- 0 (edge tiles only)
  static __device__ __forceinline__ void zero_x_rows(const LdsPlan& P, float* Xa0, int pw, int lane) {
    for (int bsel = 0; bsel < 2; ++bsel)
      for (int kc = pw; kc < P.kc; kc += C::NPW)
        for (int s = lane; s < P.xwp; s += 64) Xa0[bsel * P.xa_sz + kc * P.xwp + s] = 0.0f;
    wave_lds_fence();  // the zeros have landed before this wave's DMA may write the same rows
  }
  static __device__ __forceinline__ void lrelu_x(const ProdArgs& a, const LdsPlan& P, float* Xa, int pw, int lane) {
    for (int kc = pw; kc < P.kc; kc += C::NPW)
      for (int s = lane; s < P.xwp; s += 64) {
        const float v = Xa[kc * P.xwp + s];
        Xa[kc * P.xwp + s] = v > 0.0f ? v : v * a.slope;
      }
  }

  // ---- ACT1D: raw rows (replicate padding = index clamp) -> this wave's scratch
  static __device__ __forceinline__ void dma_raw(const ProdArgs& a, const LdsPlan& P, float* rawbuf, const float* xb,
                                                 int c0, int p0, int pw, int lane) {
    const int npr = P.xrwp >> 6;
    for (int rs = 0; rs < P.rpw; ++rs) {
      const int ci = c0 + pw + rs * C::NPW;
      const float* xc = xb + ci * a.x_cs;
      for (int i = 0; i < npr; ++i) {
        const float* src = ci < a.Cin ? xc + hsp_clampi(p0 - 5 + lane + 64 * i, 0, a.Lin - 1) : a.zeros;
        dma4(src, rawbuf + rs * P.xrwp + 64 * i);
      }
    }
  }

  // one channel row: raw (LDS) -> 2x-rate snake signal (LDS) -> activated window row.
  // VALU cycles here are stolen from the fp32 MFMAs of the consumer wave on the same SIMD
  // (they share the fp32 datapath), so the arithmetic is kept minimal: packed fp32 FMAs
  // (v_pk_fma_f32: an even and an odd output sample per lane) and hardware cosine.
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ void act_row(const ProdArgs& a, const LdsPlan& P, const float* raw, float* a2,
                                                 float* xa, int ci, int p0, int lane) {
    const int L = a.Lin;
    const int mlo = 2 * p0 - 5;
    const bool interior = mlo >= 0 && mlo + P.a2w <= 2 * L;  // no index clamp needed at the 2x rate
    const float* hu = a.filt;
    const float* hd = a.filt + 12;
    const int cic = ci < a.Cin ? ci : a.Cin - 1;
    const float kf = a.alpha_exp[cic] * 0.318309886183790672f, kb = 0.5f * a.beta_inv[cic];
    // phase B: a[m] = snake(2 * up[m]);  up[2q]   = sum_i x[q-3+i] * hu[11-2i],
    //                                    up[2q+1] = sum_i x[q-2+i] * hu[10-2i]   (i = 0..5)
    if (interior) {
      // slot 2i+1 <-> m = 2q (q = p0-2+i), slot 2i+2 <-> m = 2q+1: both read raw[i .. i+6]
      const int npair = (P.a2w - 1) >> 1;
      for (int i = lane; i < npair; i += 64) {
        float xv[7];
#pragma unroll
        for (int t = 0; t < 7; ++t) xv[t] = raw[i + t];
        f32x2 u = {0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 6; ++t) {
          const f32x2 xx = {xv[t], xv[t + 1]};
          const f32x2 hh = {hu[11 - 2 * t], hu[10 - 2 * t]};
          u = __builtin_elementwise_fma(xx, hh, u);
        }
        u = u * 2.0f;
        a2[2 * i + 1] = hsp_snake_hw(u.x, kf, kb);
        a2[2 * i + 2] = hsp_snake_hw(u.y, kf, kb);
      }
      if (lane < 2) {  // slot 0 (odd m, q = p0-3, raw[0..5]) and the last slot (even m, raw[xw+4..xw+9])
        const float* xr_ = lane ? raw + P.xw + 4 : raw;
        float uu = 0.0f;
#pragma unroll
        for (int t = 0; t < 6; ++t) uu = fmaf(xr_[t], lane ? hu[11 - 2 * t] : hu[10 - 2 * t], uu);
        a2[lane ? P.a2w - 1 : 0] = hsp_snake_hw(2.0f * uu, kf, kb);
      }
    } else {
      for (int s = lane; s < P.a2w; s += 64) {
        const int m = hsp_clampi(mlo + s, 0, 2 * L - 1);
        const int q = m >> 1, odd = m & 1;
        const float* xr_ = raw + (q - 3 + odd) - (p0 - 5);
        float u = 0.0f;
#pragma unroll
        for (int t = 0; t < 6; ++t) u = fmaf(xr_[t], odd ? hu[10 - 2 * t] : hu[11 - 2 * t], u);
        a2[s] = hsp_snake_hw(2.0f * u, kf, kb);
      }
    }
    wave_lds_fence();
    // phase C: y[p] = sum_k hd[k] * a[clamp(2p+k-5)], zero outside [0, L) (conv zero padding)
    for (int s = lane; s < P.xwp; s += 64) {
      const int p = p0 + s;
      f32x2 v = {0.0f, 0.0f};
      if (p >= 0 && p < L && s < P.xw) {
        const f32x2* ar = reinterpret_cast<const f32x2*>(a2 + 2 * s);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const f32x2 hh = {hd[2 * k], hd[2 * k + 1]};
          v = __builtin_elementwise_fma(ar[k], hh, v);
        }
      }
      xa[s] = v.x + v.y;
    }
    wave_lds_fence();  // a2 is reused by the next row
  }

  static __device__ __forceinline__ void act_rows(const ProdArgs& a, const LdsPlan& P, const float* rawbuf, float* a2,
                                                  float* Xa, int c0, int p0, int pw, int lane) {
    for (int rs = 0; rs < P.rpw; ++rs) {
      const int row = pw + rs * C::NPW;
      if (row < P.kc) act_row(a, P, rawbuf + rs * P.xrwp, a2, Xa + row * P.xwp, c0 + row, p0, lane);
    }
  }
};

}  // namespace hspconv
