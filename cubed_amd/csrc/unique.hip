// unique.hip -- run heads of a sorted chunk: count them, or pack them densely
// (stream compaction; the unique_* set functions).
//
// A task has a sorted 1-d run of n keys (plain, or the key field of a pairs
// chunk whose int64 index field sits in a slab of its own), the run of the
// chunk before it (none for block 0) and the global position of its first
// element.  Element j is a head if it is the first element of block 0, else iff
// key_lt(predecessor, element) in the order of sort_keys.h; the predecessor of
// a chunk's first element is the last element of the chunk before.  NaNs tie
// and -0.0 ties 0.0 there, so a run of either has one head.
//
// A workgroup owns one tile of kTile consecutive elements and each of its four
// waves kTile / 4 consecutive ones, 64 per round.  wave_heads is the one place
// that decides heads: a lane takes its left neighbour's key with __shfl_up
// (lane 0 loads it), and __ballot gives the round's 64 flags to every lane.
//
//   k_unique_count  a tile's heads: popcounts of the ballots, the four waves'
//                   sums through LDS, one int64 per tile into the task's scratch.
//   k_unique_scan   one workgroup per task: the exclusive prefix of the tile
//                   counts in place (scan_tile_counts of tile_scan.h, shared
//                   with select.hip), the total behind them and, for
//                   CUBED_UNIQUE_COUNT, into dst.
//   k_unique_pack   the flags again, from keys kept in registers; a head goes to
//                   dst[tile offset + heads of the earlier waves + heads of the
//                   earlier rounds + popcount(ballot below the lane)], so the
//                   heads of a tile land on consecutive addresses in order.  The
//                   workgroup then zeroes its share of dst[total, n).
//
// The three run as separate launches on one stream: no workgroup waits for,
// signals or spins on another one, and there are no atomics, so reruns are
// bit-identical.  Pack reads the keys twice (count pass and pack pass).
#include <cstdlib>
#include <stdio.h>
#include "common.h"
#include "sort_keys.h"
#include "tile_scan.h"

namespace cubed {
extern thread_local char g_err[512];
}
using namespace cubed;

static int fail(const char* m) { snprintf(g_err, sizeof(g_err), "%s", m); return CUBED_E_ARG; }

namespace {

constexpr int kTile = CUBED_UNIQUE_TILE;
constexpr int kWaves = kBlock / 64;
constexpr int kSeg = kTile / kWaves;  // consecutive elements of one wave
constexpr int kRounds = kSeg / 64;    // rounds of 64 elements
static_assert(kTile % (kWaves * 64) == 0, "a tile is whole rounds of every wave");

// The keys v[r] and head flags heads[r] (one bit per lane, the same in every
// lane) of the elements s0 + r * 64 + lane of the task; elements at or past n
// are no heads.  Returns the number of heads.  Every index read is in [0, n),
// or n_prev - 1 of the previous run.
template <typename T>
CUBED_DEV int wave_heads(const cubed_unique_task_t* __restrict__ K, int64_t s0, int lane, T (&v)[kRounds],
                         uint64_t (&heads)[kRounds]) {
  const CUBED_G T* __restrict__ src = (const CUBED_G T*)(uintptr_t)K->src_base;
  const CUBED_G T* __restrict__ prev = (const CUBED_G T*)(uintptr_t)K->prev_base;
  const int64_t n = K->n;
  const bool has_prev = K->prev_base != 0 && K->n_prev > 0;
  int count = 0;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int64_t j = s0 + r * 64 + lane;
    const bool in = j < n;
    const T cur = in ? src[j] : (T)0;
    T left = __shfl_up(cur, 1);
    if (lane == 0 && in) {
      if (j > 0) left = src[j - 1];
      else if (has_prev) left = prev[K->n_prev - 1];
    }
    const bool head = in && ((j == 0 && !has_prev) || key_lt(left, cur));
    v[r] = cur;
    heads[r] = __ballot(head);
    count += __popcll(heads[r]);
  }
  return count;
}

// Grid: 1-d, block g -> (task g / work, tile g % work).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_unique_count(const cubed_unique_task_t* __restrict__ tasks,
                                                         int64_t ntasks, int64_t work) {
  __shared__ int wsum[kWaves];
  const int64_t g = blockIdx.x;
  const int64_t ti = g / work, tw = g - ti * work;
  if (ti >= ntasks) return;
  const cubed_unique_task_t* __restrict__ K = tasks + ti;
  if (tw * kTile >= K->n) return;  // workgroup-uniform
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  T v[kRounds];
  uint64_t heads[kRounds];
  const int c = wave_heads<T>(K, tw * kTile + (int64_t)w * kSeg, lane, v, heads);
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
__global__ __launch_bounds__(kBlock) void k_unique_scan(const cubed_unique_task_t* __restrict__ tasks,
                                                        int64_t ntasks, int32_t write_count) {
  const int64_t ti = blockIdx.x;
  if (ti >= ntasks) return;
  const cubed_unique_task_t* __restrict__ K = tasks + ti;
  scan_tile_counts((CUBED_G int64_t*)(uintptr_t)K->scratch_base, (K->n + kTile - 1) / kTile,
                   write_count ? (CUBED_G int64_t*)(uintptr_t)K->dst_base : nullptr);
}

// Grid: as k_unique_count.  PAYLOAD: CUBED_UNIQUE_KEYS, _POSITION or _INDEX.
template <typename T, int PAYLOAD>
__global__ __launch_bounds__(kBlock) void k_unique_pack(const cubed_unique_task_t* __restrict__ tasks,
                                                        int64_t ntasks, int64_t work) {
  __shared__ int wsum[kWaves];
  const int64_t g = blockIdx.x;
  const int64_t ti = g / work, tw = g - ti * work;
  if (ti >= ntasks) return;
  const cubed_unique_task_t* __restrict__ K = tasks + ti;
  const int64_t n = K->n;
  if (tw * kTile >= n) return;  // workgroup-uniform
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int64_t s0 = tw * kTile + (int64_t)w * kSeg;
  T v[kRounds];
  uint64_t heads[kRounds];
  const int c = wave_heads<T>(K, s0, lane, v, heads);
  if (lane == 0) wsum[w] = c;
  __syncthreads();
  const CUBED_G int64_t* __restrict__ sc = (const CUBED_G int64_t*)(uintptr_t)K->scratch_base;
  const CUBED_G int64_t* __restrict__ srci = (const CUBED_G int64_t*)(uintptr_t)K->src_idx_base;
  CUBED_G T* __restrict__ dst = (CUBED_G T*)(uintptr_t)K->dst_base;
  CUBED_G int64_t* __restrict__ dsti = (CUBED_G int64_t*)(uintptr_t)K->dst_idx_base;
  // heads before this wave's: at most total - c, so every store below is in [0, total)
  int64_t off = sc[tw];
#pragma unroll
  for (int k = 0; k < kWaves; ++k)
    if (k < w) off += wsum[k];
  const uint64_t below = ((uint64_t)1 << lane) - 1;
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    if ((heads[r] >> lane) & 1) {
      const int64_t p = off + __popcll(heads[r] & below);
      const int64_t j = s0 + r * 64 + lane;
      dst[p] = v[r];
      if constexpr (PAYLOAD == CUBED_UNIQUE_POSITION) dsti[p] = K->offset + j;
      if constexpr (PAYLOAD == CUBED_UNIQUE_INDEX) dsti[p] = srci[j];
    }
    off += __popcll(heads[r]);
  }
  // the tail behind the packed heads: this tile's share of [total, n)
  const int64_t total = sc[(n + kTile - 1) / kTile];
  const int64_t end = (tw + 1) * kTile < n ? (tw + 1) * kTile : n;
  for (int64_t p = tw * kTile + tid; p < end; p += kBlock) {
    if (p >= total) {
      dst[p] = (T)0;
      if constexpr (PAYLOAD != CUBED_UNIQUE_KEYS) dsti[p] = 0;
    }
  }
}

int key_size(int32_t ktype) {
  switch (ktype) {
    case CUBED_F32: case CUBED_I32: case CUBED_U32: return 4;
    case CUBED_F64: case CUBED_I64: case CUBED_U64: return 8;
  }
  return 0;
}

template <typename T>
void launch(const cubed_unique_task_t* d_tasks, int64_t ntasks, int kind, int payload, int64_t work,
            hipStream_t st) {
  const dim3 grid((unsigned)(ntasks * work)), block(kBlock);
  hipLaunchKernelGGL((k_unique_count<T>), grid, block, 0, st, d_tasks, ntasks, work);
  hipLaunchKernelGGL(k_unique_scan, dim3((unsigned)ntasks), block, 0, st, d_tasks, ntasks,
                     (int32_t)(kind == CUBED_UNIQUE_COUNT));
  if (kind != CUBED_UNIQUE_PACK) return;
  if (payload == CUBED_UNIQUE_KEYS)
    hipLaunchKernelGGL((k_unique_pack<T, CUBED_UNIQUE_KEYS>), grid, block, 0, st, d_tasks, ntasks, work);
  else if (payload == CUBED_UNIQUE_POSITION)
    hipLaunchKernelGGL((k_unique_pack<T, CUBED_UNIQUE_POSITION>), grid, block, 0, st, d_tasks, ntasks, work);
  else
    hipLaunchKernelGGL((k_unique_pack<T, CUBED_UNIQUE_INDEX>), grid, block, 0, st, d_tasks, ntasks, work);
}

bool bad_kind(int32_t kind, int32_t payload) {
  if (kind != CUBED_UNIQUE_COUNT && kind != CUBED_UNIQUE_PACK) return true;
  if (payload != CUBED_UNIQUE_KEYS && payload != CUBED_UNIQUE_POSITION && payload != CUBED_UNIQUE_INDEX) return true;
  return kind == CUBED_UNIQUE_COUNT && payload != CUBED_UNIQUE_KEYS;
}

}  // namespace

extern "C" int64_t cubed_unique_tile(void) { return kTile; }

extern "C" int64_t cubed_unique_work(const cubed_unique_task_t* tasks, int64_t ntasks, int32_t ktype,
                                     int32_t kind, int32_t payload) {
  if (ntasks < 0 || (ntasks > 0 && !tasks)) return fail("cubed_unique_work: null task table");
  const int64_t isz = key_size(ktype);
  if (!isz) return fail("cubed_unique_work: bad key type");
  if (bad_kind(kind, payload)) return fail("cubed_unique_work: bad kind or payload");
  int64_t work = 0;
  for (int64_t i = 0; i < ntasks; ++i) {
    const cubed_unique_task_t& t = tasks[i];
    if (t.n < 0 || t.n_prev < 0) return fail("cubed_unique_work: negative extent");
    if (t.n > (int64_t)1 << 40) return fail("cubed_unique_work: chunk too large");
    if (!t.scratch_base || t.scratch_base % 8) return fail("cubed_unique_work: scratch missing or misaligned");
    if (!t.dst_base) return fail("cubed_unique_work: null destination");
    if (t.n > 0 && !t.src_base) return fail("cubed_unique_work: null chunk address");
    if (t.prev_base && t.n_prev == 0) return fail("cubed_unique_work: an empty previous chunk");
    if ((t.src_base | t.prev_base) % isz || t.src_idx_base % 8 || t.dst_idx_base % 8 ||
        t.dst_base % (kind == CUBED_UNIQUE_COUNT ? 8 : isz))
      return fail("cubed_unique_work: address not aligned to its element");
    if (kind == CUBED_UNIQUE_PACK) {
      if ((payload != CUBED_UNIQUE_KEYS) != (t.dst_idx_base != 0))
        return fail("cubed_unique_work: the payload and the destination's index field do not match");
      if (payload == CUBED_UNIQUE_INDEX && t.n > 0 && !t.src_idx_base)
        return fail("cubed_unique_work: the index payload needs a pairs chunk");
      if (t.n > 0 && (t.dst_base == t.src_base || (t.dst_idx_base && t.dst_idx_base == t.src_idx_base)))
        return fail("cubed_unique_work: pack in place");
    }
    const int64_t tiles = (t.n + kTile - 1) / kTile;
    if (tiles > work) work = tiles;
  }
  return work;
}

extern "C" int cubed_unique_chunks(const cubed_unique_task_t* d_tasks, int64_t ntasks, int32_t ktype,
                                   int32_t kind, int32_t payload, int64_t work, void* stream) {
  if (ntasks == 0) return 0;
  if (!d_tasks || ntasks < 0 || work < 0) return fail("cubed_unique_chunks: bad task table");
  if (!key_size(ktype)) return fail("cubed_unique_chunks: bad key type");
  if (bad_kind(kind, payload)) return fail("cubed_unique_chunks: bad kind or payload");
  if (ntasks > 0x7fffffff || (work > 0 && work > 0x7fffffff / ntasks))
    return fail("cubed_unique_chunks: more than 2^31 - 1 workgroups");
  if (work == 0) work = 1;  // empty chunks only: the scan still writes their zero counts
  hipStream_t st = (hipStream_t)stream;
  switch (ktype) {
    case CUBED_F32: launch<float>(d_tasks, ntasks, kind, payload, work, st); break;
    case CUBED_F64: launch<double>(d_tasks, ntasks, kind, payload, work, st); break;
    case CUBED_I32: launch<int32_t>(d_tasks, ntasks, kind, payload, work, st); break;
    case CUBED_I64: launch<int64_t>(d_tasks, ntasks, kind, payload, work, st); break;
    case CUBED_U32: launch<uint32_t>(d_tasks, ntasks, kind, payload, work, st); break;
    default: launch<uint64_t>(d_tasks, ntasks, kind, payload, work, st); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s", hipGetErrorString(e)); return (int)e; }
  return 0;
}
