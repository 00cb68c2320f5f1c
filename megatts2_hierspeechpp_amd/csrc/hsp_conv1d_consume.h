// The CONSUMER role of a wave of the fused conv kernel (part of hsp_conv1d_mfma_kernel.h, behind
// hsp_conv1d_epilogue.h): the hand-placed fragment reads and conv_consume -- the accumulator start, the hand-scheduled
// MFMA loop with its chunk handover, the K-split reduction, the epilogue by EPI.  The two halves of HSP_EPI_INIT (the
// accumulator preload and its stores) are written out inside conv_consume, on plain locals and explicit static_for nests:
// as functions of their own, or on the for_* helpers, the 128 x 128 INIT kernels compile to other register / scratch counts.
#pragma once

namespace hspconv {

// 32-bit LDS byte address of a pointer into the workgroup's dynamic shared memory
__device__ __forceinline__ unsigned lds_addr(const float* p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) float*)p;
}

// N fragment registers from consecutive 32-float blocks: f[i] = lds[addr + i * 128 B]
template <int N, int I = 0>
__device__ __forceinline__ void ds_read_frags(float (&f)[N], unsigned addr) {
  if constexpr (I < N) {
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(f[I]) : "v"(addr), "n"(I * 128));
    ds_read_frags<N, I + 1>(f, addr);
  }
}

// the same from a compile-time byte offset: f[i] = lds[addr + OFF + i * 128 B]
template <int N, int OFF, int I = 0>
__device__ __forceinline__ void ds_read_frags_at(float (&f)[N], unsigned addr) {
  if constexpr (I < N) {
    static_assert(OFF + I * 128 < 65536, "ds_read immediate offsets are 16 bits");
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(f[I]) : "v"(addr), "n"(OFF + I * 128));
    ds_read_frags_at<N, OFF, I + 1>(f, addr);
  }
}

// The fragment registers written by the asynchronous inline-asm ds_reads above become valid at an s_waitcnt.  The
// compiler does not know that: nothing but scheduling barriers kept it from moving an MFMA that reads them above a
// bare `asm volatile("s_waitcnt")` (hsp_bgemm.hip met the failure: stale fragments in some waves).  Here every
// fragment register is re-defined by an (empty) asm statement right behind the wait -- volatile asm statements keep
// their order -- so each consumer of a fragment carries a DATA dependency on the wait.  No instruction is emitted
// for the re-definitions: the ISA of the consumer loop is unchanged.
template <int N, int I = 0>
__device__ __forceinline__ void bind_frags(float (&f)[N]) {
  if constexpr (I < N) {
    asm volatile("" : "+v"(f[I]));
    bind_frags<N, I + 1>(f);
  }
}
template <int NA, int NB>
__device__ __forceinline__ void wait_frags(float (&fa)[NA], float (&fb)[NB]) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  bind_frags<NA>(fa);
  bind_frags<NB>(fb);
}

// The consumer role of one wave: a (TM x TN) grid of 32 x 32 MFMA blocks at rows m0 + wm * TM * 32, columns
// t0 + wn * TN * 32 of the tile.  TM / TN are the shape's own (C::kTM, C::kTN) except in a narrow tail tile
// (has_tail_path): the slab and window layouts in LDS belong to the SHAPE (C::BM, C::XWP), only the part of the
// tile a wave multiplies changes.
// FOLD (folded columns): t0 is the tile's first VIRTUAL column, in utterance b at time ts0; every lane takes the utterance
// and time of its own column (TN == 1), and the epilogues read each per-utterance operand there.
template <class C, int EPI, bool ACT, int TM, int TN, bool FOLD = false>
__device__ __forceinline__ void conv_consume(const hsp_conv1d_args& a, const LdsPlan& P, float* const lds, const int b,
                                             const int m0, const int t0, const int p0, const int wm, const int wn,
                                             const int lane, const int nchunks, const int lkc, const int xvec,
                                             const int ks = 0, const int ts0 = 0) {
  static_assert(!FOLD || (TN == 1 && C::kKS == 1 && EPI != HSP_EPI_SHUF && !ACT), "folded columns: one column per lane, plain kernels");
  // validate() refuses Cin < 1.  Said to the compiler as well: without it the "no chunk at all" exit it generates runs the
  // epilogue on registers that the first fragment reads -- issued before the loop -- are still going to write
  // (tools/check_isa.py reports exactly that path).
  __builtin_assume(nchunks > 0);
  ConsLane L;
  L.lane = lane, L.l32 = lane & 31, L.half = lane >> 5;
  L.slot = wm * C::kWN + wn;
  L.mw = m0 + wm * (TM * 32), L.wcol = wn * (TN * 32);
  L.b = b, L.t0 = t0, L.ts0 = ts0;
  L.bl = b, L.tw = t0 + L.wcol + L.l32;
  int piece;
  fold_lane<FOLD>(a, b, ts0, L.wcol + L.l32, L.bl, L.tw, piece);
  L.xfold = 8 * piece + 4 - a.pad;

  f32x16 acc[TM][TN];
  {  // ---- the accumulators before the main loop: zero, or the HSP_EPI_INIT preload
  const int mw = L.mw, half = L.half, tw = L.tw, bl = L.bl;
  static_assert(C::kKS == 1 || EPI != HSP_EPI_INIT, "a K split with the accumulator-init epilogue would add the residual once per group");
  if constexpr (EPI == HSP_EPI_INIT) {
    // The accumulators START at bias + cbias + residual (+ the running sum of `accumulate`), loaded in
    // the MFMA C layout while the producers' first chunk is still in flight: the loads' latency hides
    // under the staging latency every tile pays anyway, and the epilogue has no loads left -- nothing
    // there ever waits on vmcnt.  (Each load instruction covers two rows x 128 B.)  Out-of-range rows /
    // columns read a clamped address and are never stored.
    // Whole passes sit under ONE wave-uniform branch each, so that the loads of a pass issue back to back
    // (a branch per load makes hipcc wait on vmcnt(0) after every one of them).  In a wave whose rows all lie
    // inside [0, Cout) an address is a uniform (scalar) per-register row pointer plus one per-lane offset per
    // column block; otherwise (Cout % 32 != 0) the row is clamped per lane.  Lanes past the last column read a
    // clamped column.  A wave wholly past Cout starts from zero and stores nothing.
    const int rcs = (int)a.res_cs, ycs = (int)a.y_cs;
    const int lrow = mw + 4 * half;                // this lane's row for register 0 of block i = 0
    int tcl[TN];
#pragma unroll
    for (int n = 0; n < TN; ++n) tcl[n] = min(tw + n * 32, a.ncols - 1);
    auto init = [&](auto full_tag) __attribute__((always_inline)) {
      constexpr bool FULL = decltype(full_tag)::value;
      // element offset of (row of register r in block i, column block n) for a tensor with channel stride cs
      auto vec1 = [&](const float* p, int c) __attribute__((always_inline)) -> float {
        if constexpr (FULL) return (p + c)[lrow];
        else return p[min(lrow + c, a.Cout - 1)];
      };
      auto mat = [&](const float* p, int c, int cs, int n) __attribute__((always_inline)) -> float {
        if constexpr (FULL) return (p + c * cs)[lrow * cs + tcl[n]];
        else return p[min(lrow + c, a.Cout - 1) * cs + tcl[n]];
      };
      float add[TM][16];
      if (a.bias) {
        static_for<TM>([&](auto ii) __attribute__((always_inline)) {
          constexpr int i = decltype(ii)::value;
          static_for<16>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            add[i][r] = vec1(a.bias, i * 32 + HSP_ACC_ROW(r, 0));
          });
        });
      } else {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) add[i][r] = 0.0f;
      }
      if (a.res) {
        const float* const rb = a.res + (int64_t)bl * a.res_bs;
        static_for<TM>([&](auto ii) __attribute__((always_inline)) {
          constexpr int i = decltype(ii)::value;
          static_for<16>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            static_for<TN>([&](auto nn) __attribute__((always_inline)) {
              constexpr int n = decltype(nn)::value;
              acc[i][n][r] = mat(rb, i * 32 + HSP_ACC_ROW(r, 0), rcs, n);
            });
          });
        });
      } else {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int n = 0; n < TN; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][n][r] = 0.0f;
      }
      static_for<TM>([&](auto ii) __attribute__((always_inline)) {
        constexpr int i = decltype(ii)::value;
        static_for<TN>([&](auto nn) __attribute__((always_inline)) {
          constexpr int n = decltype(nn)::value;
          static_for<16>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            acc[i][n][r] += add[i][r];
          });
        });
      });
      if (a.cbias) {
        const float* const cb = a.cbias + (int64_t)bl * a.cbias_bs;
        static_for<TM>([&](auto ii) __attribute__((always_inline)) {
          constexpr int i = decltype(ii)::value;
          static_for<16>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            const float c = vec1(cb, i * 32 + HSP_ACC_ROW(r, 0));
            static_for<TN>([&](auto nn) __attribute__((always_inline)) {
              constexpr int n = decltype(nn)::value;
              acc[i][n][r] += c;
            });
          });
        });
      }
      if (a.accumulate) {
        // one 32 x 32 block at a time: its 16 loads issue together into temporaries, then one wait
        const float* const yb = a.y + (int64_t)bl * a.y_bs;
        static_for<TM>([&](auto ii) __attribute__((always_inline)) {
          constexpr int i = decltype(ii)::value;
          static_for<TN>([&](auto nn) __attribute__((always_inline)) {
            constexpr int n = decltype(nn)::value;
            float tmp[16];
            static_for<16>([&](auto rr) __attribute__((always_inline)) {
              constexpr int r = decltype(rr)::value;
              tmp[r] = mat(yb, i * 32 + HSP_ACC_ROW(r, 0), ycs, n);
            });
            __builtin_amdgcn_sched_barrier(0);
            static_for<16>([&](auto rr) __attribute__((always_inline)) {
              constexpr int r = decltype(rr)::value;
              acc[i][n][r] += tmp[r];
            });
            __builtin_amdgcn_sched_barrier(0);
          });
        });
      }
    };
    if (mw + TM * 32 <= a.Cout) {
      init(std::true_type{});
    } else if (mw < a.Cout) {
      init(std::false_type{});
    } else {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int n = 0; n < TN; ++n)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][n][r] = 0.0f;
    }
  } else if constexpr (EPI == HSP_EPI_ACT) {
    // 0 + bias, what HSP_EPI_INIT's preload makes of a launch without residual: the same start of the same chain
    static_for<TM>([&](auto ii) __attribute__((always_inline)) {
      constexpr int i = decltype(ii)::value;
      static_for<16>([&](auto rr) __attribute__((always_inline)) {
        constexpr int r = decltype(rr)::value;
        const float bz = 0.0f + (a.bias ? a.bias[min(mw + i * 32 + HSP_ACC_ROW(r, half), a.Cout - 1)] : 0.0f);
        static_for<TN>([&](auto nn) __attribute__((always_inline)) {
          constexpr int n = decltype(nn)::value;
          acc[i][n][r] = bz;
        });
      });
    });
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  }
  }
  const int wlane = L.half * C::BM + wm * (TM * 32) + L.l32;
  const int xlane = L.half * P.xwp + L.wcol + L.l32 + (FOLD ? L.xfold : (xvec ? (p0 & 3) : 0));

  // ---- the main loop: every chunk's k-steps on this wave's blocks, fragments from wlane (weight slab) and xlane (window),
  // in floats from the start of the chunk buffers.  (Here and not in a function of its own: that compiles to another
  // loop-exit branch.)
  // k-steps ordered tap outer, channel pair inner.  The weight slab is [tap][channel][row], so the A side is
  // one linear walk (1 KB per step for BM = 128); the B side moves one pair (2 window rows) per step and one tap
  // (dil columns) per KC / 2 steps.  A trip is two steps of the same tap: the second step's addresses are the
  // first's plus compile-time immediates (Cfg::XWP is a constant of the shape), so a trip costs two VALU adds and
  // six scalar instructions, no branch.  With fp32
  // MFMAs sharing the VALU datapath that matters: tools/micro/mfma_loop_bench.hip loses 5 % of the matrix pipe to
  // two VALU adds per step and 11 % more to a branchy tap wrap (what this loop looked like in round 1).
  // Fragment reads are hand-placed (inline asm + explicit lgkmcnt): the reads of step s+1 are issued right
  // after the wait that retires the reads of step s and BEFORE the MFMAs of step s, so an LDS round trip never
  // sits between two MFMA groups (left to itself hipcc sinks the prefetch under the MFMAs and waits at once).
  {
    constexpr int BM = C::BM;
    const int KC = P.kc;
    // steps of a chunk (even: KC >= 4, so a tap has an even number of channel pairs); with a K split this group's share,
    // [ks * nsteps, (ks + 1) * nsteps) of them (pick_lkc: the share is even, so a trip never straddles a tap)
    const int nsteps = ((a.K * KC) >> 1) / C::kKS;

    HSP_BARRIER(a);  // chunk 0 staged
    constexpr int kStepA = 2 * BM * 4;     // bytes: next channel pair in the weight slab
    constexpr int rowB = 2 * C::XWP * 4;   // bytes: next channel pair in the window
    const int spanB = (KC >> 1) * rowB;    // all pairs of one tap
    const int tapB = 4 * a.dil;
    float fa0[TM], fb0[TN], fa1[TM], fb1[TN];
    auto mma_set = [&](const float (&fa)[TM], const float (&fb)[TN]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int n = 0; n < TN; ++n)
          acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[n], acc[i][n], 0, 0, 0);
    };
    // The fragment pipeline runs ACROSS chunks: the barrier that hands over chunk c+1 sits between the last two
    // MFMA groups of chunk c (all LDS reads of chunk c are retired by then - its last fragments are in registers),
    // and the first fragments of chunk c+1 are requested right behind it, under the last MFMA group of chunk c.
    // With the barrier after the last group the first reads of every chunk were exposed (~3 % at 22-28 steps per
    // chunk).  Barrier count is unchanged: one before the loop, one per chunk.
    unsigned aA = lds_addr(lds + wlane);                 // per-lane LDS byte addresses of the chunk's buffers
    unsigned aB = lds_addr(lds + P.xa_off + xlane);
    // where this K group's share of a chunk starts: step s0 = tap s0 / (KC / 2), channel pair s0 % (KC / 2)
    int offA0 = 0, pairB0 = 0, tapoff0 = 0;
    if constexpr (C::kKS > 1) {
      const int s0 = ks * nsteps;
      offA0 = s0 * kStepA;
      pairB0 = (s0 & ((KC >> 1) - 1)) * rowB;
      tapoff0 = (s0 >> (lkc - 1)) * tapB;
    }
    unsigned va = aA + (unsigned)offA0, vb = aB + (unsigned)(pairB0 + tapoff0);
    const bool run = !HSP_DBG(a, HSP_CV_NO_MFMA);
    if (run) {
      ds_read_frags<TM>(fa0, va);
      ds_read_frags<TN>(fb0, vb);
    }
    for (int c = 0; c < nchunks; ++c) {
      if (!run) {
        HSP_BARRIER(a);
        continue;
      }
      int offA = offA0, pairB = pairB0, tapoff = tapoff0;  // scalar byte offsets of the current trip
      // The hazard recogniser wants one COUNTED instruction between the re-definition of the fragments in wait_frags
      // and the first MFMA that reads them, and it does not count inline asm.  So the scalar walk of a trip sits in its
      // first slot, followed by the one scalar add hipcc emits itself (window offset = pair + tap), and the two VALU
      // address adds sit in the second slot behind its wait: no s_nop, and as many instructions per trip as before.
      int offB = 0;
      auto advance = [&]() __attribute__((always_inline)) {
        int t;
        asm volatile(
            "s_add_i32 %[oa], %[oa], %[sa]\n\t"
            "s_add_i32 %[pb], %[pb], %[sb]\n\t"
            "s_cmp_eq_u32 %[pb], %[span]\n\t"
            "s_cselect_b32 %[pb], 0, %[pb]\n\t"
            "s_cselect_b32 %[t], %[tap], 0\n\t"
            "s_add_i32 %[to], %[to], %[t]"
            : [oa] "+s"(offA), [pb] "+s"(pairB), [to] "+s"(tapoff), [t] "=&s"(t)
            : [sa] "n"(2 * kStepA), [sb] "n"(2 * rowB), [span] "s"(spanB), [tap] "s"(tapB)
            : "scc");
        offB = pairB + tapoff;
      };
      // first slot of a trip: the second step of the same tap, through immediates (+ the scalar walk to the next trip)
      auto slot_a = [&](bool walk) __attribute__((always_inline)) {
        wait_frags(fa0, fb0);               // the first step's fragments have landed (and only now are they valid)
        __builtin_amdgcn_sched_barrier(0);
        if (walk) advance();
        ds_read_frags_at<TM, kStepA>(fa1, va);
        ds_read_frags_at<TN, rowB>(fb1, vb);
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the MFMAs (true double buffer)
        mma_set(fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);  // or the MFMAs sink below the next wait, which then follows its reads at once
      };
      for (int s = 0; s + 2 < nsteps; s += 2) {   // every trip but the last
        slot_a(true);
        wait_frags(fa1, fb1);               // the second step's fragments have landed
        __builtin_amdgcn_sched_barrier(0);
        va = aA + (unsigned)offA;           // two VALU adds behind the wait: counted instructions before the MFMAs
        vb = aB + (unsigned)offB;
        ds_read_frags<TM>(fa0, va);
        ds_read_frags<TN>(fb0, vb);
        __builtin_amdgcn_sched_barrier(0);
        mma_set(fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
      }
      slot_a(false);                               // last trip, first step
      HSP_BARRIER(a);                              // (waits lgkmcnt(0) first) chunk c+1 is staged, chunk c's buffer is free
      bind_frags<TM>(fa1);                         // the barrier's wait is what makes the last step's fragments valid
      bind_frags<TN>(fb1);
      if (c + 1 < nchunks) {
        const int nb = (c + 1) & 1;
        aA = lds_addr(lds + nb * P.ws_sz + wlane);
        aB = lds_addr(lds + P.xa_off + nb * P.xa_sz + xlane);
        va = aA + (unsigned)offA0;
        vb = aB + (unsigned)(pairB0 + tapoff0);
        __builtin_amdgcn_sched_barrier(0);
        ds_read_frags<TM>(fa0, va);                // chunk c+1, step 0
        ds_read_frags<TN>(fb0, vb);
      }
      __builtin_amdgcn_sched_barrier(0);
      mma_set(fa1, fb1);                           // last step of chunk c, over the barrier's wake-up and the new reads
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  if constexpr (C::kKS > 1) {
    // The K groups' partial sums meet in LDS: the chunk buffers are free behind the loop's last barrier (every consumer
    // retired its fragment reads there), the producers have left, so the barrier below counts the consumer waves only.
    // (Inline here: as a function of its own the reduction compiles to another register count.)
    static_assert(C::kKS == 2, "one partner group per wave");
    // (behind the VEC epilogue's per-wave staging slots: a group-0 wave that has finished adding may already be
    // transposing its tile there while its neighbour still reads its partner's partial sums)
    float* const red = lds + C::kWM * C::kWN * (32 * 36) + (wm * C::kWN + wn) * (TM * TN * 16 * 64) + lane;
    if (ks > 0) {
      for_acc<TM, TN>([&](auto ii, auto nn, auto rr) __attribute__((always_inline)) {
        constexpr int i = ii, n = nn, r = rr;
        red[((i * TN + n) * 16 + r) * 64] = acc[i][n][r];
      });
    }
    lds_barrier();
    if (ks > 0) return;
    for_acc<TM, TN>([&](auto ii, auto nn, auto rr) __attribute__((always_inline)) {
      constexpr int i = ii, n = nn, r = rr;
      acc[i][n][r] += red[((i * TN + n) * 16 + r) * 64];
    });
  }
  if (HSP_DBG(a, HSP_CV_NO_EPILOGUE) && EPI != HSP_EPI_ACT) return;   // (HSP_EPI_ACT: the producers wait at its barriers)
  if constexpr (EPI == HSP_EPI_INIT) {  // ---- HSP_EPI_INIT: stores only (see the top of this file)
    const int mw = L.mw, half = L.half, tw = L.tw, bl = L.bl;
    // stores only, straight from the accumulator layout: one instruction = two rows x 128 B
    float* const yb = a.y + (int64_t)bl * a.y_bs;
    const int ycs = (int)a.y_cs;
    const bool full = mw + TM * 32 <= a.Cout &&
                      t0 + wn * (TN * 32) + TN * 32 <= (FOLD ? a.B * a.ncols : a.ncols);  // wave-uniform
    const float ps = a.post_scale;
    if (full) {
      const int lrow = mw + 4 * half;
      int voff[TN];
#pragma unroll
      for (int n = 0; n < TN; ++n) voff[n] = lrow * ycs + tw + n * 32;
      static_for<TM>([&](auto ii) __attribute__((always_inline)) {
        constexpr int i = decltype(ii)::value;
        static_for<16>([&](auto rr) __attribute__((always_inline)) {
          constexpr int r = decltype(rr)::value;
          float* const yp = yb + (i * 32 + HSP_ACC_ROW(r, 0)) * ycs;  // uniform
          static_for<TN>([&](auto nn) __attribute__((always_inline)) {
            constexpr int n = decltype(nn)::value;
            // tuning bit 65536: non-temporal stores -- measured: k = 3 launches +2-4 % in isolation, step unchanged
            if (HSP_DBG(a, HSP_CV_NT_STORES)) __builtin_nontemporal_store(acc[i][n][r] * ps, yp + voff[n]);
            else yp[voff[n]] = acc[i][n][r] * ps;
          });
        });
      });
    } else {
      static_for<TM>([&](auto ii) __attribute__((always_inline)) {
        constexpr int i = decltype(ii)::value;
        static_for<TN>([&](auto nn) __attribute__((always_inline)) {
          constexpr int n = decltype(nn)::value;
          const int t = tw + n * 32;
          static_for<16>([&](auto rr) __attribute__((always_inline)) {
            constexpr int r = decltype(rr)::value;
            const int row = mw + i * 32 + HSP_ACC_ROW(r, half);
            if (row < a.Cout && t < a.ncols) yb[row * ycs + t] = acc[i][n][r] * ps;
          });
        });
      });
    }
  }
  else if constexpr (EPI == HSP_EPI_VEC) epi_vec<FOLD>(a, L, lds, acc);
  else if constexpr (EPI == HSP_EPI_GATE) epi_gate(a, L, acc);
  else if constexpr (EPI == HSP_EPI_SHUF) epi_shuf(a, L, acc);
  else if constexpr (EPI == HSP_EPI_ACT) EpiAct<C>::consumer(a, L, lds, m0, wm * C::kWN + wn, acc);
  else epi_gen(a, L, acc);
}

}  // namespace hspconv
