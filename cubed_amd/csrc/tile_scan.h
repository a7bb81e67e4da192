// tile_scan.h -- the per-task scan of tile counts that the compaction kernels
// (unique.hip, select.hip) run between their count and their pack launch.
#pragma once
#include "common.h"

namespace cubed {

// One workgroup of kBlock threads: the exclusive prefix of the ntiles int64
// counts at sc, in place (wave scan with __shfl_up, wave totals through LDS,
// a running carry), the total into sc[ntiles] and, if count_out is not null,
// there as well.
CUBED_DEV void scan_tile_counts(CUBED_G int64_t* __restrict__ sc, int64_t ntiles,
                                CUBED_G int64_t* __restrict__ count_out) {
  constexpr int kWaves = kBlock / 64;
  __shared__ int64_t wtot[kWaves];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  int64_t carry = 0;  // the same in every thread
  for (int64_t base = 0; base < ntiles; base += kBlock) {
    const int64_t i = base + tid;
    const int64_t c = i < ntiles ? sc[i] : 0;
    int64_t s = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = __shfl_up(s, d);
      if (lane >= d) s += up;
    }
    if (lane == 63) wtot[w] = s;
    __syncthreads();
    int64_t before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      if (k < w) before += wtot[k];
      total += wtot[k];
    }
    if (i < ntiles) sc[i] = carry + before + s - c;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) {
    sc[ntiles] = carry;
    if (count_out) *count_out = carry;
  }
}

}  // namespace cubed
