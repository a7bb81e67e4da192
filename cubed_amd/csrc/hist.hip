// hist.hip -- bin counts of one chunk over given edges (histogram).
//
// A task has a flat run of n_values values, nbins + 1 non-decreasing edges e of
// the same type and its own row of nbins int64 counts.  A value v is counted in
// bin i when e[i] <= v < e[i+1]; the last bin also takes v == e[nbins].  NaN
// and values outside [e[0], e[nbins]] are dropped before any bin is looked for.
// For a kept value the bin is min(c - 1, nbins - 1) with c the number of edges
// that are <= v, which only comparisons with the edges decide.
//
//   k_hist<T, CUBED_HIST_UNIFORM>  edges and 32-bit counters in LDS.  The bin
//       is guessed as (v - e[0]) * nbins / (e[nbins] - e[0]) and then walked
//       down while v < e[i] and up while e[i+1] <= v, so the arithmetic only
//       chooses where the walk starts.
//   k_hist<T, CUBED_HIST_SEARCH>   the same LDS layout, c by a binary search in
//       descending power-of-two steps (the order of sort_keys.h).
//   k_hist<T, CUBED_HIST_WIDE>     any nbins: the same binary search over the
//       edges in global memory, counts added straight to the task's row.
//
// A workgroup owns `per` consecutive values of one task (per = ceil(n_values /
// work) rounded up to kStep, below 2^32 by the host's choice of work, so a
// 32-bit counter cannot wrap).  A lane loads 4 consecutive values with 16-byte
// accesses; a ragged end or a misaligned chunk goes element by element.
//
// Contention: lanes of a wave that hold equal bins side by side are merged
// before the add -- a lane adds only if the lane before it has another bin,
// and then adds the length of its run (one ballot and one lane shift per
// value).  Constant input costs one add per wave and step where it would cost
// 64 on one LDS word.
//
// At its end a workgroup adds its nonzero counters to the task's row with
// 64-bit integer atomics; k_hist_zero clears the rows on the same stream
// before.  All atomics are integer adds, so every run gives the same bits.
#include <cstdlib>
#include <stdio.h>
#include "common.h"
#include "sort_keys.h"

namespace cubed {
extern thread_local char g_err[512];
}
using namespace cubed;

static int fail(const char* m) { snprintf(g_err, sizeof(g_err), "%s", m); return CUBED_E_ARG; }

namespace {

constexpr int kBinsLds = CUBED_HIST_BINS_LDS;
constexpr int kPer = 4;               // consecutive values of one lane per step
constexpr int kStep = kBlock * kPer;  // values of one workgroup per step
constexpr int kZeroGroups = 64;       // most workgroups that clear one row
static_assert((kBinsLds + 1) * 8 + 8 + kBinsLds * 4 <= 80 * 1024, "two workgroups fit 160 KiB of LDS");

// bytes of the staged edges, rounded so that the counters start 16-byte aligned
__host__ __device__ constexpr size_t edges_bytes(int nbins, size_t isz) { return ((size_t)(nbins + 1) * isz + 15) & ~(size_t)15; }

// the largest power of two <= n (0 for n <= 0)
CUBED_DEV int pow2_floor(int n) { return n <= 0 ? 0 : 1 << (31 - __builtin_clz((unsigned)n)); }

// The number of the m edges that are <= v (every index read is in [0, m)).
template <typename T, typename E>
CUBED_DEV int edges_le(E e, int m, int p2, T v) {
  int pos = 0;
  for (int step = p2; step > 0; step >>= 1) {
    const int next = pos + step;
    const T s = e[(next < m ? next : m) - 1];
    if (next <= m && !key_lt(v, s)) pos = next;
  }
  return pos;
}

// The bin of v, e[0] <= v <= e[nbins], from a guess (every index read is in [0, nbins]).
template <typename T>
CUBED_DEV int bin_walk(const T* e, int nbins, T lo, T scale, T v) {
  const T t = (v - lo) * scale;
  int i = t > (T)0 ? (t < (T)(nbins - 1) ? (int)t : nbins - 1) : 0;
  while (i > 0 && v < e[i]) --i;
  while (i < nbins - 1 && !(v < e[i + 1])) ++i;
  return i;
}

// The lanes of the wave (all of them call) each bring a bin, or -1 for nothing.
// A lane whose left neighbour brings another bin adds the length of its run.
template <typename C, typename N>
CUBED_DEV void add_runs(C* counts, int key) {
  const int lane = (int)__lane_id();
  const int left = __shfl_up(key, 1);
  const bool head = lane == 0 || left != key;
  const uint64_t heads = __ballot(head);
  if (head && key >= 0) {
    const uint64_t above = lane == 63 ? 0 : heads >> (lane + 1);
    const int run = above ? __ffsll((unsigned long long)above) : 64 - lane;
    atomicAdd(counts + key, (N)run);
  }
}

// Grid: 1-d, block g -> (task g / work, values (g % work) * per .. + per).
// Dynamic LDS: none (WIDE), else edges_bytes + nbins * 4.
template <typename T, int PATH>
__global__ __launch_bounds__(kBlock) void k_hist(const cubed_hist_task_t* __restrict__ tasks, int64_t ntasks,
                                                 int64_t work, int nbins) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int64_t g = blockIdx.x;
  const int64_t ti = g / work, tw = g - ti * work;
  if (ti >= ntasks) return;
  const cubed_hist_task_t* __restrict__ K = tasks + ti;
  const int64_t nv = K->n_values;
  int64_t per = (nv + work - 1) / work;
  per = (per + kStep - 1) / kStep * kStep;
  const int64_t v0 = tw * per;
  if (v0 >= nv || nbins < 1) return;  // workgroup-uniform
  const int64_t v1 = nv - v0 < per ? nv : v0 + per;
  const int tid = threadIdx.x;
  const int m = nbins + 1;
  const CUBED_G T* __restrict__ ge = (const CUBED_G T*)(uintptr_t)K->edges_base;
  const CUBED_G T* __restrict__ x = (const CUBED_G T*)(uintptr_t)K->x_base;
  unsigned long long* dst = (unsigned long long*)(uintptr_t)K->dst_base;
  T* se = (T*)smem;
  uint32_t* cnt = (uint32_t*)(smem + edges_bytes(nbins, sizeof(T)));

  if constexpr (PATH != CUBED_HIST_WIDE) {
    for (int i = tid; i < m; i += kBlock) se[i] = ge[i];
    for (int i = tid; i < nbins; i += kBlock) cnt[i] = 0;
    __syncthreads();
  }
  const T lo = ge[0], hi = ge[nbins];
  const T scale = (T)nbins / (hi - lo);
  const int p2 = pow2_floor(m);
  const bool aligned = (K->x_base & 15) == 0;

  // every lane of the workgroup takes every step (add_runs is a wave operation)
  for (int64_t s0 = v0; s0 < v1; s0 += kStep) {
    const int64_t e0 = s0 + (int64_t)tid * kPer;
    T v[kPer];
    bool have[kPer];
    if (aligned && e0 + kPer <= v1) {
      u32x4 w[kPer * sizeof(T) / 16];
#pragma unroll
      for (int i = 0; i < (int)(kPer * sizeof(T) / 16); ++i) w[i] = *((const CUBED_G u32x4*)(x + e0) + i);
      __builtin_memcpy(&v[0], &w[0], sizeof(w));
#pragma unroll
      for (int q = 0; q < kPer; ++q) have[q] = true;
    } else {
#pragma unroll
      for (int q = 0; q < kPer; ++q) {
        have[q] = e0 + q < v1;
        v[q] = have[q] ? x[e0 + q] : (T)0;
      }
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      int key = -1;
      if (have[q] && v[q] >= lo && v[q] <= hi) {  // false for NaN
        if constexpr (PATH == CUBED_HIST_UNIFORM) {
          key = bin_walk<T>(se, nbins, lo, scale, v[q]);
        } else {
          int c;
          if constexpr (PATH == CUBED_HIST_SEARCH) c = edges_le<T>((const T*)se, m, p2, v[q]);
          else c = edges_le<T>(ge, m, p2, v[q]);
          key = c - 1 < nbins - 1 ? c - 1 : nbins - 1;  // c >= 1: e[0] <= v
        }
      }
      if constexpr (PATH == CUBED_HIST_WIDE) add_runs<unsigned long long, unsigned long long>(dst, key);
      else add_runs<uint32_t, uint32_t>(cnt, key);
    }
  }

  if constexpr (PATH != CUBED_HIST_WIDE) {
    __syncthreads();
    for (int i = tid; i < nbins; i += kBlock) {
      const uint32_t c = cnt[i];
      if (c) atomicAdd(dst + i, (unsigned long long)c);
    }
  }
}

// Grid: 1-d, block g -> (task g / zwork, bins (g % zwork) * kBlock + tid, stride zwork * kBlock).
__global__ __launch_bounds__(kBlock) void k_hist_zero(const cubed_hist_task_t* __restrict__ tasks, int64_t ntasks,
                                                      int64_t zwork, int nbins) {
  const int64_t g = blockIdx.x;
  const int64_t ti = g / zwork, tw = g - ti * zwork;
  if (ti >= ntasks) return;
  CUBED_G int64_t* __restrict__ dst = (CUBED_G int64_t*)(uintptr_t)tasks[ti].dst_base;
  for (int64_t i = tw * kBlock + threadIdx.x; i < nbins; i += zwork * kBlock) dst[i] = 0;
}

template <typename T>
void launch(const cubed_hist_task_t* d_tasks, int64_t ntasks, int nbins, int path, int64_t work, hipStream_t st) {
  const dim3 grid((unsigned)(ntasks * work)), block(kBlock);
  const size_t lds = edges_bytes(nbins, sizeof(T)) + (size_t)nbins * 4;
  if (path == CUBED_HIST_UNIFORM)
    hipLaunchKernelGGL((k_hist<T, CUBED_HIST_UNIFORM>), grid, block, lds, st, d_tasks, ntasks, work, nbins);
  else if (path == CUBED_HIST_SEARCH)
    hipLaunchKernelGGL((k_hist<T, CUBED_HIST_SEARCH>), grid, block, lds, st, d_tasks, ntasks, work, nbins);
  else
    hipLaunchKernelGGL((k_hist<T, CUBED_HIST_WIDE>), grid, block, 0, st, d_tasks, ntasks, work, nbins);
}

}  // namespace

extern "C" int64_t cubed_hist_bins_lds(void) { return kBinsLds; }

extern "C" int cubed_hist_path(const cubed_hist_task_t* tasks, int64_t ntasks, int32_t ktype, int64_t nbins,
                               int32_t uniform) {
  if (ntasks < 0 || (ntasks > 0 && !tasks)) return fail("cubed_hist_path: null task table");
  if (ktype != CUBED_F32 && ktype != CUBED_F64) return fail("cubed_hist_path: bad key type");
  if (nbins < 1 || nbins > (int64_t)1 << 30) return fail("cubed_hist_path: nbins out of range");
  const int64_t isz = ktype == CUBED_F32 ? 4 : 8;
  for (int64_t i = 0; i < ntasks; ++i) {
    const cubed_hist_task_t& t = tasks[i];
    if (t.n_values < 0) return fail("cubed_hist_path: negative extent");
    if (t.n_values > (int64_t)1 << 40) return fail("cubed_hist_path: chunk too large");
    if (!t.dst_base || !t.edges_base || (t.n_values > 0 && !t.x_base))
      return fail("cubed_hist_path: null chunk address");
    if ((t.x_base | t.edges_base) % isz || t.dst_base % 8)
      return fail("cubed_hist_path: address not aligned to its element");
  }
  if (nbins > kBinsLds) return CUBED_HIST_WIDE;
  return uniform ? CUBED_HIST_UNIFORM : CUBED_HIST_SEARCH;
}

extern "C" int cubed_hist_chunks(const cubed_hist_task_t* d_tasks, int64_t ntasks, int32_t ktype, int64_t nbins,
                                 int32_t path, int64_t work, void* stream) {
  if (ntasks == 0) return 0;
  if (!d_tasks || ntasks < 0 || ntasks > 0x7fffffff || work < 0) return fail("cubed_hist_chunks: bad task table");
  if (ktype != CUBED_F32 && ktype != CUBED_F64) return fail("cubed_hist_chunks: bad key type");
  if (nbins < 1 || nbins > (int64_t)1 << 30) return fail("cubed_hist_chunks: nbins out of range");
  if (path != CUBED_HIST_UNIFORM && path != CUBED_HIST_SEARCH && path != CUBED_HIST_WIDE)
    return fail("cubed_hist_chunks: bad path");
  if (path != CUBED_HIST_WIDE && nbins > kBinsLds) return fail("cubed_hist_chunks: too many bins for an LDS path");
  if (work > 0x7fffffff / ntasks) return fail("cubed_hist_chunks: more than 2^31 - 1 workgroups");
  hipStream_t st = (hipStream_t)stream;
  int64_t zwork = (nbins + kBlock - 1) / kBlock;
  if (zwork > kZeroGroups) zwork = kZeroGroups;
  if (zwork > 0x7fffffff / ntasks) zwork = 0x7fffffff / ntasks;  // >= 1: ntasks <= 2^31 - 1
  hipLaunchKernelGGL(k_hist_zero, dim3((unsigned)(ntasks * zwork)), dim3(kBlock), 0, st, d_tasks, ntasks, zwork,
                     (int)nbins);
  if (work > 0) {
    if (ktype == CUBED_F32) launch<float>(d_tasks, ntasks, (int)nbins, path, work, st);
    else launch<double>(d_tasks, ntasks, (int)nbins, path, work, st);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s", hipGetErrorString(e)); return (int)e; }
  return 0;
}
