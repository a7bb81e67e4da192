// select.hip -- the elements of a chunk that a one-element predicate selects:
// count them, or pack their positions or the values at their places densely
// (stream compaction; nonzero and boolean-mask indexing).
//
// A task has a 1-d run of n elements of ES bytes (1, 2, 4 or 8).  Element j is
// selected iff (bits & m) != 0, m all ones or, for floats, all ones but the
// sign bit: -0.0 is zero, NaNs, infinities, denormals and the most negative
// integer are not.  The kernels are templated on the element size, not on the
// dtype, and there is no float compare.
//
// Every lane loads 16 bytes per round, V = 16 / ES consecutive elements, so a
// wave covers 1 KiB with one load instruction.  A workgroup owns a tile of
// CUBED_SELECT_TILE_BYTES of the run and each of its four waves a quarter of
// it, kRounds consecutive KiB.  lane_flags turns a lane's vector into V flag
// bits (bit e: element e of the vector); wave_flags, and wave_count, which
// keeps no flags, load and mask off the elements at or past n.  A vector that
// starts at or past n is never loaded; the last one loaded may reach up to 15
// bytes past element n - 1 (the host interface requires that storage).
//
//   k_select_count  a tile's selected elements: the lanes' counts, a wave sum,
//                   the four waves' sums through LDS, one int64 per tile into
//                   the task's scratch.
//   k_select_scan   one workgroup per task: scan_tile_counts of tile_scan.h
//                   (shared with unique.hip), the total behind the prefixes and,
//                   for CUBED_SELECT_COUNT, into dst.
//   k_select_pack   the flags again, from vectors kept in registers.  A lane's
//                   start in round r is the tile's offset + the selected of the
//                   earlier waves + those of the wave's earlier rounds + an
//                   exclusive scan of the 64 lane counts (__shfl_up; the four
//                   rounds' counts scanned together, packed 16 bits each); the
//                   lane writes its selected elements from there in element
//                   order, so the order is memory order.  The workgroup then
//                   zeroes its share of dst[total, n).
//
// The three run as separate launches on one stream: no workgroup waits for,
// signals or spins on another one, and there are no atomics, so reruns are
// bit-identical.  Pack reads the run twice (count pass and pack pass).
#include <cstdlib>
#include <stdio.h>
#include "common.h"
#include "tile_scan.h"

namespace cubed {
extern thread_local char g_err[512];
}
using namespace cubed;

static int fail(const char* m) { snprintf(g_err, sizeof(g_err), "%s", m); return CUBED_E_ARG; }

namespace {

constexpr int kTileBytes = CUBED_SELECT_TILE_BYTES;
constexpr int kWaves = kBlock / 64;
constexpr int kSegBytes = kTileBytes / kWaves;  // consecutive bytes of one wave
constexpr int kRounds = kSegBytes / 1024;       // rounds of 64 lanes x 16 bytes
static_assert(kTileBytes % (kWaves * 1024) == 0, "a tile is whole rounds of every wave");
static_assert(kRounds == 4, "k_select_pack scans the lane counts of four rounds as two packed words");

template <int N> struct uint_of;
template <> struct uint_of<1> { using type = uint8_t; };
template <> struct uint_of<2> { using type = uint16_t; };
template <> struct uint_of<4> { using type = uint32_t; };
template <> struct uint_of<8> { using type = uint64_t; };

// The mask of one 32-bit word of the run: the element mask m repeated for 1-
// and 2-byte elements; for 8-byte elements the mask of the high word.
uint32_t word_mask(int esize, int ignore_sign) {
  if (!ignore_sign) return 0xffffffffu;
  return esize == 1 ? 0x7f7f7f7fu : esize == 2 ? 0x7fff7fffu : 0x7fffffffu;
}

// One word of 1- or 2-byte elements, masked: the top bit of every element that
// is not zero (an element's low bits plus all ones carry into its top bit, and
// never out of it).
template <int ES>
CUBED_DEV uint32_t word_marks(const uint32_t x) {
  constexpr uint32_t low = ES == 2 ? 0x7fff7fffu : 0x7f7f7f7fu;
  return (((x & low) + low) | x) & ~low;
}

// The V = 16 / ES flags of a 16-byte vector, bit e for its element e.
template <int ES>
CUBED_DEV uint32_t lane_flags(const u32x4 w, const uint32_t m) {
  uint32_t f = 0;
  if constexpr (ES == 8) {
    f = (uint32_t)((w.x | (w.y & m)) != 0) | ((uint32_t)((w.z | (w.w & m)) != 0) << 1);
  } else if constexpr (ES == 4) {
    f = (uint32_t)((w.x & m) != 0) | ((uint32_t)((w.y & m) != 0) << 1) | ((uint32_t)((w.z & m) != 0) << 2) |
        ((uint32_t)((w.w & m) != 0) << 3);
  } else {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const uint32_t t = word_marks<ES>(w[d] & m);
      if constexpr (ES == 2) {
        f |= ((t >> 15) | ((t >> 30) & 2u)) << (2 * d);
      } else {
        // the multiply gathers bits 0, 8, 16 and 24 into bits 21..24 (no two
        // partial products meet, so nothing carries)
        f |= ((((t >> 7) * 0x00204081u) >> 21) & 0xfu) << (4 * d);
      }
    }
  }
  return f;
}

// The number of selected elements of a whole 16-byte vector: the popcount of
// lane_flags, without gathering the flags of narrow elements.
template <int ES>
CUBED_DEV int lane_count(const u32x4 w, const uint32_t m) {
  if constexpr (ES >= 4) {
    return __popc(lane_flags<ES>(w, m));
  } else {
    int c = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) c += __popc(word_marks<ES>(w[d] & m));
    return c;
  }
}

// The flags f[r] of the V elements s0 + (r * 64 + lane) * V + e of the task;
// elements at or past n are not selected.  Returns the lane's number of
// selected elements.  A vector is loaded only if its first element is below n.
template <int ES>
CUBED_DEV int wave_flags(const cubed_select_task_t* __restrict__ K, int64_t s0, int lane, uint32_t m,
                         uint32_t (&f)[kRounds]) {
  constexpr int V = 16 / ES;
  const CUBED_G u32x4* __restrict__ src = (const CUBED_G u32x4*)(uintptr_t)K->src_base;
  const int64_t n = K->n;
  u32x4 w[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t j0 = s0 + (int64_t)(r * 64 + lane) * V;
    w[r] = j0 < n ? src[j0 / V] : (u32x4)(0u);
  }
  int count = 0;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t j0 = s0 + (int64_t)(r * 64 + lane) * V;
    const int64_t left = n - j0;  // elements of the vector below n, if in [0, V)
    const uint32_t keep = left >= V ? (1u << V) - 1u : left > 0 ? (1u << (int)left) - 1u : 0u;
    f[r] = lane_flags<ES>(w[r], m) & keep;
    count += __popc(f[r]);
  }
  return count;
}

// The lane's number of selected elements among those wave_flags looks at,
// without keeping the flags: whole vectors are counted by lane_count, the one
// vector that n cuts by its masked flags.
template <int ES>
CUBED_DEV int wave_count(const cubed_select_task_t* __restrict__ K, int64_t s0, int lane, uint32_t m) {
  constexpr int V = 16 / ES;
  const CUBED_G u32x4* __restrict__ src = (const CUBED_G u32x4*)(uintptr_t)K->src_base;
  const int64_t n = K->n;
  u32x4 w[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t j0 = s0 + (int64_t)(r * 64 + lane) * V;
    w[r] = j0 < n ? src[j0 / V] : (u32x4)(0u);
  }
  int count = 0;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t left = n - (s0 + (int64_t)(r * 64 + lane) * V);
    if (left >= V) count += lane_count<ES>(w[r], m);
    else if (left > 0) count += __popc(lane_flags<ES>(w[r], m) & ((1u << (int)left) - 1u));
  }
  return count;
}

// Grid: 1-d, block g -> (task g / work, tile g % work).
template <int ES>
__global__ __launch_bounds__(kBlock) void k_select_count(const cubed_select_task_t* __restrict__ tasks,
                                                         int64_t ntasks, int64_t work, uint32_t m) {
  constexpr int64_t kTile = kTileBytes / ES;
  __shared__ int wsum[kWaves];
  const int64_t g = blockIdx.x;
  const int64_t ti = g / work, tw = g - ti * work;
  if (ti >= ntasks) return;
  const cubed_select_task_t* __restrict__ K = tasks + ti;
  if (tw * kTile >= K->n) return;  // workgroup-uniform
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  int c = wave_count<ES>(K, tw * kTile + (int64_t)w * (kSegBytes / ES), lane, m);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
  if (lane == 0) wsum[w] = c;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) total += wsum[k];
    ((CUBED_G int64_t*)(uintptr_t)K->scratch_base)[tw] = total;
  }
}

// Grid: one workgroup per task.
__global__ __launch_bounds__(kBlock) void k_select_scan(const cubed_select_task_t* __restrict__ tasks,
                                                        int64_t ntasks, int64_t tile, int32_t write_count) {
  const int64_t ti = blockIdx.x;
  if (ti >= ntasks) return;
  const cubed_select_task_t* __restrict__ K = tasks + ti;
  scan_tile_counts((CUBED_G int64_t*)(uintptr_t)K->scratch_base, (K->n + tile - 1) / tile,
                   write_count ? (CUBED_G int64_t*)(uintptr_t)K->dst_base : nullptr);
}

// Grid: as k_select_count.  VS: 0 packs positions (int64), else the values of
// VS bytes at the selected places.
template <int ES, int VS>
__global__ __launch_bounds__(kBlock) void k_select_pack(const cubed_select_task_t* __restrict__ tasks,
                                                        int64_t ntasks, int64_t work, uint32_t m) {
  constexpr int V = 16 / ES;
  constexpr int64_t kTile = kTileBytes / ES;
  using D = typename uint_of<VS == 0 ? 8 : VS>::type;
  __shared__ int wsum[kWaves];
  const int64_t g = blockIdx.x;
  const int64_t ti = g / work, tw = g - ti * work;
  if (ti >= ntasks) return;
  const cubed_select_task_t* __restrict__ K = tasks + ti;
  const int64_t n = K->n;
  if (tw * kTile >= n) return;  // workgroup-uniform
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int64_t s0 = tw * kTile + (int64_t)w * (kSegBytes / ES);
  uint32_t f[kRounds];
  wave_flags<ES>(K, s0, lane, m, f);
  // a lane's counts are at most 16 and a wave's at most 1024 per round: two
  // rounds share a word, 16 bits each
  const uint32_t c01 = __popc(f[0]) | (__popc(f[1]) << 16), c23 = __popc(f[2]) | (__popc(f[3]) << 16);
  uint32_t i01 = c01, i23 = c23;  // inclusive scans over the lanes
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u01 = __shfl_up(i01, d), u23 = __shfl_up(i23, d);
    if (lane >= d) { i01 += u01; i23 += u23; }
  }
  const uint32_t t01 = __shfl(i01, 63), t23 = __shfl(i23, 63);  // the wave's totals per round
  const int tot[kRounds] = {(int)(t01 & 0xffffu), (int)(t01 >> 16), (int)(t23 & 0xffffu), (int)(t23 >> 16)};
  const uint32_t e01 = i01 - c01, e23 = i23 - c23;
  const int excl[kRounds] = {(int)(e01 & 0xffffu), (int)(e01 >> 16), (int)(e23 & 0xffffu), (int)(e23 >> 16)};
  if (lane == 0) wsum[w] = tot[0] + tot[1] + tot[2] + tot[3];
  __syncthreads();
  const CUBED_G int64_t* __restrict__ sc = (const CUBED_G int64_t*)(uintptr_t)K->scratch_base;
  const CUBED_G D* __restrict__ val = (const CUBED_G D*)(uintptr_t)K->val_base;
  CUBED_G D* __restrict__ dst = (CUBED_G D*)(uintptr_t)K->dst_base;
  // selected before this wave's: at most total - the wave's, so every store below is in [0, total)
  int64_t off = sc[tw];
#pragma unroll
  for (int k = 0; k < kWaves; ++k)
    if (k < w) off += wsum[k];
  const int64_t offset = K->offset;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t j0 = s0 + (int64_t)(r * 64 + lane) * V;
    int64_t p = off + excl[r];
    uint32_t bits = f[r];
    while (bits) {
      const int64_t j = j0 + __builtin_ctz(bits);  // < n: wave_flags masked the rest off
      bits &= bits - 1;
      if constexpr (VS == 0) dst[p] = (D)(offset + j);
      else dst[p] = val[j];
      ++p;
    }
    off += tot[r];
  }
  // the tail behind the packed elements: this tile's share of [total, n)
  const int64_t total = sc[(n + kTile - 1) / kTile];
  const int64_t end = (tw + 1) * kTile < n ? (tw + 1) * kTile : n;
  for (int64_t p = tw * kTile + tid; p < end; p += kBlock)
    if (p >= total) dst[p] = (D)0;
}

bool size_ok(int32_t s) { return s == 1 || s == 2 || s == 4 || s == 8; }

bool bad_kind(int32_t kind, int32_t vsize, int32_t ignore_sign) {
  if (kind != CUBED_SELECT_COUNT && kind != CUBED_SELECT_PACK) return true;
  if (ignore_sign != 0 && ignore_sign != 1) return true;
  if (vsize != 0 && !size_ok(vsize)) return true;
  return kind == CUBED_SELECT_COUNT && vsize != 0;
}

template <int ES, int VS>
void launch_pack(const cubed_select_task_t* d_tasks, int64_t ntasks, int64_t work, uint32_t m, hipStream_t st) {
  hipLaunchKernelGGL((k_select_pack<ES, VS>), dim3((unsigned)(ntasks * work)), dim3(kBlock), 0, st, d_tasks,
                     ntasks, work, m);
}

template <int ES>
void launch(const cubed_select_task_t* d_tasks, int64_t ntasks, int kind, int vsize, int64_t work, uint32_t m,
            hipStream_t st) {
  const dim3 grid((unsigned)(ntasks * work)), block(kBlock);
  hipLaunchKernelGGL((k_select_count<ES>), grid, block, 0, st, d_tasks, ntasks, work, m);
  hipLaunchKernelGGL(k_select_scan, dim3((unsigned)ntasks), block, 0, st, d_tasks, ntasks,
                     (int64_t)(kTileBytes / ES), (int32_t)(kind == CUBED_SELECT_COUNT));
  if (kind != CUBED_SELECT_PACK) return;
  switch (vsize) {
    case 0: launch_pack<ES, 0>(d_tasks, ntasks, work, m, st); break;
    case 1: launch_pack<ES, 1>(d_tasks, ntasks, work, m, st); break;
    case 2: launch_pack<ES, 2>(d_tasks, ntasks, work, m, st); break;
    case 4: launch_pack<ES, 4>(d_tasks, ntasks, work, m, st); break;
    default: launch_pack<ES, 8>(d_tasks, ntasks, work, m, st); break;
  }
}

}  // namespace

extern "C" int64_t cubed_select_tile_bytes(void) { return kTileBytes; }

extern "C" int64_t cubed_select_work(const cubed_select_task_t* tasks, int64_t ntasks, int32_t esize,
                                     int32_t ignore_sign, int32_t kind, int32_t vsize) {
  if (ntasks < 0 || (ntasks > 0 && !tasks)) return fail("cubed_select_work: null task table");
  if (!size_ok(esize)) return fail("cubed_select_work: bad element size");
  if (bad_kind(kind, vsize, ignore_sign)) return fail("cubed_select_work: bad kind, value size or sign flag");
  const int64_t dsize = kind == CUBED_SELECT_COUNT || vsize == 0 ? 8 : vsize;
  int64_t work = 0;
  for (int64_t i = 0; i < ntasks; ++i) {
    const cubed_select_task_t& t = tasks[i];
    if (t.n < 0) return fail("cubed_select_work: negative extent");
    if (t.n > (int64_t)1 << 40) return fail("cubed_select_work: chunk too large");
    if (!t.scratch_base || t.scratch_base % 8) return fail("cubed_select_work: scratch missing or misaligned");
    if (!t.dst_base) return fail("cubed_select_work: null destination");
    if (t.n > 0 && !t.src_base) return fail("cubed_select_work: null chunk address");
    if (t.src_base % 16) return fail("cubed_select_work: the run is not aligned to 16 bytes");
    if (t.dst_base % dsize || (vsize && t.val_base % vsize))
      return fail("cubed_select_work: address not aligned to its element");
    if (vsize == 0 && t.val_base) return fail("cubed_select_work: values without a value size");
    if (vsize != 0 && t.n > 0 && !t.val_base) return fail("cubed_select_work: null values");
    if (t.n > 0 && (t.dst_base == t.src_base || t.dst_base == t.val_base))
      return fail("cubed_select_work: select in place");
    const int64_t tiles = (t.n * esize + kTileBytes - 1) / kTileBytes;
    if (tiles > work) work = tiles;
  }
  return work;
}

extern "C" int cubed_select_chunks(const cubed_select_task_t* d_tasks, int64_t ntasks, int32_t esize,
                                   int32_t ignore_sign, int32_t kind, int32_t vsize, int64_t work,
                                   void* stream) {
  if (ntasks == 0) return 0;
  if (!d_tasks || ntasks < 0 || work < 0) return fail("cubed_select_chunks: bad task table");
  if (!size_ok(esize)) return fail("cubed_select_chunks: bad element size");
  if (bad_kind(kind, vsize, ignore_sign)) return fail("cubed_select_chunks: bad kind, value size or sign flag");
  if (ntasks > 0x7fffffff || (work > 0 && work > 0x7fffffff / ntasks))
    return fail("cubed_select_chunks: more than 2^31 - 1 workgroups");
  if (work == 0) work = 1;  // empty chunks only: the scan still writes their zero counts
  hipStream_t st = (hipStream_t)stream;
  const uint32_t m = word_mask(esize, ignore_sign);
  switch (esize) {
    case 1: launch<1>(d_tasks, ntasks, kind, vsize, work, m, st); break;
    case 2: launch<2>(d_tasks, ntasks, kind, vsize, work, m, st); break;
    case 4: launch<4>(d_tasks, ntasks, kind, vsize, work, m, st); break;
    default: launch<8>(d_tasks, ntasks, kind, vsize, work, m, st); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s", hipGetErrorString(e)); return (int)e; }
  return 0;
}
