// search.hip -- many independent binary searches against one sorted chunk
// (searchsorted).
//
// A task has a sorted run of n_sorted keys and a flat run of n_values values of
// the same type.  For every value v it counts the keys that sort before v
// (CUBED_SEARCH_RIGHT: before or tied with v) in the order of sort_keys.h, adds
// the count of the earlier blocks of the sorted array (acc, if any) and writes
// int64.  The predicate "key goes before v" is true on a prefix of the sorted
// run and false on the rest, so the count is the length of that prefix.
//
//   k_search<T, RIGHT, false>  CUBED_SEARCH_LDS: n_sorted <= kTile.  The
//       workgroup stages the whole sorted run into LDS with 16-byte loads and
//       every lane searches it for its own values.
//   k_search<T, RIGHT, true>   CUBED_SEARCH_SPLIT: any n_sorted.  With
//       stride = ceil(n_sorted / kTile) the workgroup stages the splitters
//       sorted[min(n, (k + 1) * stride) - 1], the last keys of the buckets
//       [k * stride, min(n, (k + 1) * stride)).  The splitters that go before v
//       are a prefix too; their count c names the one bucket that holds the end
//       of the prefix of the whole run (splitter c - 1 goes before v, splitter c
//       does not), and c == buckets means every key goes before v.  The lane
//       finishes with a binary search of bucket c in global memory.
//
// Both searches take descending power-of-two steps from the largest one that
// fits, the same number for every lane, with the four values of a lane
// interleaved.  A workgroup owns kVals consecutive values of one task: a lane
// loads 4 consecutive values and, with an acc, 4 counts with 16-byte accesses
// and stores 4 counts with two of them; a ragged end or a misaligned chunk goes
// element by element.
//
// No workgroup waits for, signals or reads the output of another one, and there
// are no atomics.
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

constexpr int kTile = CUBED_SEARCH_TILE;
constexpr int kVals = CUBED_SEARCH_VALUES;
constexpr int kPer = 4;               // consecutive values of one lane per step
constexpr int kStep = kBlock * kPer;  // values of one workgroup per step
static_assert(kVals % kStep == 0, "a workgroup's values are whole steps");
static_assert((kTile & (kTile - 1)) == 0 && kTile * 8 <= 64 * 1024, "kTile: a power of two, at most 64 KiB of keys");

// key s counts for value v
template <typename T, bool RIGHT>
CUBED_DEV bool goes_before(T s, T v) { return RIGHT ? !key_lt(v, s) : key_lt(s, v); }

// the largest power of two <= n (0 for n <= 0)
CUBED_DEV int64_t pow2_floor(int64_t n) { return n <= 0 ? 0 : (int64_t)1 << (63 - __builtin_clzll((uint64_t)n)); }

// Grid: 1-d, block g -> (task g / work, values (g % work) * kVals .. + kVals).
template <typename T, bool RIGHT, bool SPLIT>
__global__ __launch_bounds__(kBlock) void k_search(const cubed_search_task_t* __restrict__ tasks, int64_t ntasks,
                                                   int64_t work) {
  __shared__ __attribute__((aligned(16))) T sk[kTile];
  constexpr int EP = 16 / sizeof(T);  // keys of one 16-byte access
  const int64_t g = blockIdx.x;
  const int64_t ti = g / work, tw = g - ti * work;
  if (ti >= ntasks) return;
  const cubed_search_task_t* __restrict__ K = tasks + ti;
  const int64_t n = K->n_sorted, nv = K->n_values;
  const int64_t v0 = tw * kVals;
  if (v0 >= nv || n < 0) return;  // workgroup-uniform
  const int64_t v1 = nv - v0 < kVals ? nv : v0 + kVals;
  const int tid = threadIdx.x;
  const CUBED_G T* __restrict__ src = (const CUBED_G T*)(uintptr_t)K->sorted_base;

  // ---- stage the sorted run, or its splitters: m keys in sk
  int m;
  int64_t stride = 1;
  if constexpr (SPLIT) {
    stride = (n + kTile - 1) / kTile;
    if (stride < 1) stride = 1;
    m = (int)((n + stride - 1) / stride);  // buckets, <= kTile
  } else {
    m = (int)(n < kTile ? n : kTile);  // the host sends n <= kTile only
  }
  if (!SPLIT || stride == 1) {
    if ((K->sorted_base & 15) == 0) {
      for (int i = tid * EP; i < m; i += kBlock * EP) {
        if (i + EP <= m) {
          *(u32x4*)(sk + i) = *(const CUBED_G u32x4*)(src + i);
        } else {
          for (int e = i; e < m; ++e) sk[e] = src[e];
        }
      }
    } else {
      for (int i = tid; i < m; i += kBlock) sk[i] = src[i];
    }
  } else {
    for (int k = tid; k < m; k += kBlock) {
      const int64_t end = (k + 1) * stride;
      sk[k] = src[(end < n ? end : n) - 1];
    }
  }
  __syncthreads();

  const int p2 = (int)pow2_floor(m);
  const int64_t bp2 = pow2_floor(stride);
  const CUBED_G T* __restrict__ vals = (const CUBED_G T*)(uintptr_t)K->values_base;
  const CUBED_G int64_t* __restrict__ acc = (const CUBED_G int64_t*)(uintptr_t)K->acc_base;
  CUBED_G int64_t* __restrict__ dst = (CUBED_G int64_t*)(uintptr_t)K->dst_base;
  const bool aligned = ((K->values_base | K->acc_base | K->dst_base) & 15) == 0;

  for (int64_t e0 = v0 + (int64_t)tid * kPer; e0 < v1; e0 += kStep) {
    const bool wide = aligned && e0 + kPer <= v1;
    T v[kPer];
    int64_t a[kPer];
    if (wide) {
      u32x4 w[kPer * sizeof(T) / 16];
#pragma unroll
      for (int i = 0; i < (int)(kPer * sizeof(T) / 16); ++i) w[i] = *((const CUBED_G u32x4*)(vals + e0) + i);
      __builtin_memcpy(&v[0], &w[0], sizeof(w));
    } else {
#pragma unroll
      for (int q = 0; q < kPer; ++q) v[q] = e0 + q < v1 ? vals[e0 + q] : (T)0;
    }
    if (!acc) {
#pragma unroll
      for (int q = 0; q < kPer; ++q) a[q] = 0;
    } else if (wide) {
      u32x4 w[kPer * 8 / 16];
#pragma unroll
      for (int i = 0; i < kPer * 8 / 16; ++i) w[i] = *((const CUBED_G u32x4*)(acc + e0) + i);
      __builtin_memcpy(&a[0], &w[0], sizeof(w));
    } else {
#pragma unroll
      for (int q = 0; q < kPer; ++q) a[q] = e0 + q < v1 ? acc[e0 + q] : 0;
    }

    // the keys of sk that go before each value (every index read is in [0, m))
    int pos[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) pos[q] = 0;
    for (int step = p2; step > 0; step >>= 1) {
#pragma unroll
      for (int q = 0; q < kPer; ++q) {
        const int next = pos[q] + step;
        const T s = sk[(next < m ? next : m) - 1];
        if (next <= m && goes_before<T, RIGHT>(s, v[q])) pos[q] = next;
      }
    }
    int64_t count[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) count[q] = pos[q];
    if (SPLIT && stride > 1) {
      // bucket pos[q] of the sorted run, in global memory (every index read is
      // in [0, n): an empty range, past the last bucket, reads key n - 1)
      int64_t base[kPer], len[kPer], off[kPer];
#pragma unroll
      for (int q = 0; q < kPer; ++q) {
        base[q] = pos[q] == m ? n : pos[q] * stride;
        const int64_t end = base[q] + stride < n ? base[q] + stride : n;
        len[q] = end - base[q];
        off[q] = 0;
      }
      for (int64_t step = bp2; step > 0; step >>= 1) {
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
          const int64_t next = off[q] + step;
          const T s = src[base[q] + (next < len[q] ? next : len[q]) - 1];
          if (next <= len[q] && goes_before<T, RIGHT>(s, v[q])) off[q] = next;
        }
      }
#pragma unroll
      for (int q = 0; q < kPer; ++q) count[q] = base[q] + off[q];
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) a[q] += count[q];

    if (wide) {
      u32x4 w[kPer * 8 / 16];
      __builtin_memcpy(&w[0], &a[0], sizeof(w));
#pragma unroll
      for (int i = 0; i < kPer * 8 / 16; ++i) *((CUBED_G u32x4*)(dst + e0) + i) = w[i];
    } else {
#pragma unroll
      for (int q = 0; q < kPer; ++q)
        if (e0 + q < v1) dst[e0 + q] = a[q];
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
void launch(const cubed_search_task_t* d_tasks, int64_t ntasks, bool right, int path, int64_t work,
            hipStream_t st) {
  const dim3 grid((unsigned)(ntasks * work)), block(kBlock);
  if (path == CUBED_SEARCH_LDS) {
    if (right) hipLaunchKernelGGL((k_search<T, true, false>), grid, block, 0, st, d_tasks, ntasks, work);
    else hipLaunchKernelGGL((k_search<T, false, false>), grid, block, 0, st, d_tasks, ntasks, work);
  } else {
    if (right) hipLaunchKernelGGL((k_search<T, true, true>), grid, block, 0, st, d_tasks, ntasks, work);
    else hipLaunchKernelGGL((k_search<T, false, true>), grid, block, 0, st, d_tasks, ntasks, work);
  }
}

}  // namespace

extern "C" int64_t cubed_search_tile(void) { return kTile; }

extern "C" int cubed_search_path(const cubed_search_task_t* tasks, int64_t ntasks, int32_t ktype) {
  if (ntasks < 0 || (ntasks > 0 && !tasks)) return fail("cubed_search_path: null task table");
  const int64_t isz = key_size(ktype);
  if (!isz) return fail("cubed_search_path: bad key type");
  int path = CUBED_SEARCH_LDS;
  for (int64_t i = 0; i < ntasks; ++i) {
    const cubed_search_task_t& t = tasks[i];
    if (t.n_sorted < 0 || t.n_values < 0) return fail("cubed_search_path: negative extent");
    if (t.n_sorted > (int64_t)1 << 40 || t.n_values > (int64_t)1 << 40)
      return fail("cubed_search_path: chunk too large");
    if (t.n_sorted > kTile) path = CUBED_SEARCH_SPLIT;
    if (t.n_values == 0) continue;  // nothing to read or write
    if (!t.values_base || !t.dst_base || (t.n_sorted > 0 && !t.sorted_base))
      return fail("cubed_search_path: null chunk address");
    if ((t.sorted_base | t.values_base) % isz || (t.acc_base | t.dst_base) % 8)
      return fail("cubed_search_path: address not aligned to its element");
  }
  return path;
}

extern "C" int cubed_search_chunks(const cubed_search_task_t* d_tasks, int64_t ntasks, int32_t ktype,
                                   int32_t flags, int32_t path, int64_t work, void* stream) {
  if (ntasks == 0 || work == 0) return 0;
  if (!d_tasks || ntasks < 0 || work < 0) return fail("cubed_search_chunks: bad task table");
  if (!key_size(ktype)) return fail("cubed_search_chunks: bad key type");
  if (flags & ~CUBED_SEARCH_RIGHT) return fail("cubed_search_chunks: bad flags");
  if (path != CUBED_SEARCH_LDS && path != CUBED_SEARCH_SPLIT) return fail("cubed_search_chunks: bad path");
  if (work > 0x7fffffff / ntasks) return fail("cubed_search_chunks: more than 2^31 - 1 workgroups");
  hipStream_t st = (hipStream_t)stream;
  const bool right = (flags & CUBED_SEARCH_RIGHT) != 0;
  switch (ktype) {
    case CUBED_F32: launch<float>(d_tasks, ntasks, right, path, work, st); break;
    case CUBED_F64: launch<double>(d_tasks, ntasks, right, path, work, st); break;
    case CUBED_I32: launch<int32_t>(d_tasks, ntasks, right, path, work, st); break;
    case CUBED_I64: launch<int64_t>(d_tasks, ntasks, right, path, work, st); break;
    case CUBED_U32: launch<uint32_t>(d_tasks, ntasks, right, path, work, st); break;
    default: launch<uint64_t>(d_tasks, ntasks, right, path, work, st); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s", hipGetErrorString(e)); return (int)e; }
  return 0;
}
