// Row helpers of the pointwise, framing and row-glue kernels: what "row b of a ragged or packed batch" means, stated
// once for hsp_pointwise.hip, hsp_mel.hip, hsp_vcbatch.hip, hsp_denoiser.hip, hsp_frontend.hip, hsp_loudness.hip and
// hsp_f0_edit.hip.
// The block sums of those files (dn_block_sum, block_sum_256, the reductions inside hsp_f0_convert_row and f0_edit_rows_kernel) are NOT here: they
// add in different orders, so one shared sum would change result bits.
#pragma once
#include "hsp_device.h"

// A row length clamped into [lo, cap], the buffer it indexes: THE statement of the clamp (lo = 1 where the row's last
// valid sample is read).  hsp_row_len is the same for row b of device lengths; NULL lengths = every row is `cap` long.
__device__ __forceinline__ int64_t hsp_clamp_len(int64_t len, int64_t cap, int64_t lo = 0) { return min(max(len, lo), cap); }
__device__ __forceinline__ int64_t hsp_row_len(const int64_t* len, int64_t b, int64_t cap, int64_t lo = 0) {
  return len ? hsp_clamp_len(len[b], cap, lo) : cap;
}

// Sample i of a row of n >= 1 samples under reflect padding (torch's "reflect": the edge sample is not repeated), exact
// for -n < i < 2 n - 1.  The clamp acts only outside that range, which every launcher's contract excludes (pad < n,
// n > n_fft / 2); it keeps the read inside the row when device lengths break the contract.
template <class I>
__device__ __forceinline__ I hsp_reflect(I i, I n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, (I)0), n - 1);
}

// One thread per element on a flat grid: blocks of `threads` that cover n elements, at most `cap`.  A kernel with a
// grid-stride loop passes its own cap; one without is launched only when hsp_grid_fits (the x dimension of a grid holds
// 2^31 - 1 blocks), else the launcher refuses.
constexpr int64_t HSP_GRID_MAX = 0x7fffffff;
inline unsigned hsp_flat_grid(int64_t n, int threads, int64_t cap = HSP_GRID_MAX) {
  int64_t b = (n + threads - 1) / threads;
  if (b < 1) b = 1;
  return (unsigned)(b > cap ? cap : b);
}
inline bool hsp_grid_fits(int64_t n, int threads) { return (n + threads - 1) / threads <= HSP_GRID_MAX; }

// Segment table of a packed batch: B utterances laid end to end along T with zero gap rows between them;
// one prompt is the table with one row.  seg = device int32 [B][2] = (first row, T_b), ascending and disjoint (dn_seg_ok
// checks the host copy).  B is a handful of prompts: the table is scanned linearly, with addresses every lane shares.
// Returns the segment that holds row t (and its first row and length), or -1 on a gap row.
__device__ __forceinline__ int dn_seg_of(const int32_t* __restrict__ seg, int B, int t, int& t0, int& Tb) {
  for (int b = 0; b < B; ++b) {
    const int s = seg[2 * b], n = seg[2 * b + 1];
    if (t < s) break;
    if (t < s + n) {
      t0 = s;
      Tb = n;
      return b;
    }
  }
  return -1;
}

// the host copy of a segment table: B >= 1 segments (first row >= 0, T_b >= 1), ascending, disjoint, inside T_tot
// (defined in hsp_denoiser.hip)
bool dn_seg_ok(const int32_t* seg, const int32_t* seg_host, int32_t B, int64_t T_tot);
