// gather.hip -- an index chunk applied to one block of an axis
// (take_along_axis).
//
// A task has an int64 index chunk seen as (outer, n_idx, inner), a source chunk
// (outer, n_src, inner) that holds the places [lo, lo + n_src) of an axis of
// n_total places, and a destination of the index chunk's extent.  For every
// output element (o, j, k), with i = idx[o][j][k] wrapped once (i + n_total if
// i < 0):
//
//   dst[o][j][k] = src[o][i - lo][k]              if lo <= i < lo + n_src
//                = prev ? prev[o][j][k] : 0       otherwise
//
// The guard is the algorithm: the blocks of the axis are gathered in chained
// passes and it decides which pass owns an element.  It is also the only way to
// a read of src, so an index out of [-n_total, n_total) reads nothing.
//
//   k_gather<ES, false>  CUBED_GATHER_DIRECT: any extents.  A workgroup owns
//       kElems consecutive outputs of the flattened chunk and every lane reads
//       its elements of src from global memory (ordinary cached loads: the
//       gather is uncoalesced by nature and lives on L2 and the Infinity Cache).
//       With inner > 1 the lanes of a wave run along k, so their reads fall in
//       different rows but in adjacent columns.
//   k_gather<ES, true>   CUBED_GATHER_LDS: inner == 1 and n_src * ES <=
//       kTileBytes.  A workgroup owns up to kLdsElems consecutive outputs of ONE
//       row o; it streams that source row into LDS with 16-byte loads and
//       serves the random reads from there.
//
// Elements are moved as bits (ES = 1, 2, 4 or 8 bytes).  A lane owns 4
// consecutive outputs whose flat position is a multiple of 4: where the chunks
// start on 16 bytes (4 * ES bytes for ES < 4) it loads its 4 indices with two
// 16-byte non-temporal loads (they are read once) and loads the earlier result
// and stores its outputs with one access of 4 * ES bytes (two 16-byte ones for
// ES = 8); the ragged ends of a workgroup's run and misaligned chunks go element
// by element.
//
// No workgroup waits for, signals or reads the output of another one, and there
// are no atomics.
#include <cstdlib>
#include <stdio.h>
#include "common.h"

namespace cubed {
extern thread_local char g_err[512];
}
using namespace cubed;

static int fail(const char* m) { snprintf(g_err, sizeof(g_err), "%s", m); return CUBED_E_ARG; }

namespace {

constexpr int kTileBytes = CUBED_GATHER_TILE_BYTES;
constexpr int kElems = CUBED_GATHER_ELEMS;
constexpr int kLdsElems = CUBED_GATHER_LDS_ELEMS;
constexpr int kPer = 4;               // consecutive outputs of one lane per step
constexpr int kStep = kBlock * kPer;  // outputs of one workgroup per step
static_assert(kElems % kStep == 0 && kLdsElems % kStep == 0, "a workgroup's outputs are whole steps");
static_assert(kTileBytes % 16 == 0 && 2 * kTileBytes <= 160 * 1024, "two workgroups fit a CU's LDS");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <int N> struct uint_of;
template <> struct uint_of<1> { using type = uint8_t; };
template <> struct uint_of<2> { using type = uint16_t; };
template <> struct uint_of<4> { using type = uint32_t; };
template <> struct uint_of<8> { using type = uint64_t; };

// the 4 elements at p, which is aligned to min(16, 4 * ES) bytes
template <int ES, typename D>
CUBED_DEV void load4(const CUBED_G D* p, D (&v)[kPer]) {
  if constexpr (ES == 1) {
    const uint32_t w = *(const CUBED_G uint32_t*)p;
    __builtin_memcpy(&v[0], &w, 4);
  } else if constexpr (ES == 2) {
    const u32x2 w = *(const CUBED_G u32x2*)p;
    __builtin_memcpy(&v[0], &w, 8);
  } else if constexpr (ES == 4) {
    const u32x4 w = *(const CUBED_G u32x4*)p;
    __builtin_memcpy(&v[0], &w, 16);
  } else {
    u32x4 w[2];
    w[0] = *(const CUBED_G u32x4*)p;
    w[1] = *((const CUBED_G u32x4*)p + 1);
    __builtin_memcpy(&v[0], &w[0], 32);
  }
}

template <int ES, typename D>
CUBED_DEV void store4(CUBED_G D* p, const D (&v)[kPer]) {
  if constexpr (ES == 1) {
    uint32_t w;
    __builtin_memcpy(&w, &v[0], 4);
    *(CUBED_G uint32_t*)p = w;
  } else if constexpr (ES == 2) {
    u32x2 w;
    __builtin_memcpy(&w, &v[0], 8);
    *(CUBED_G u32x2*)p = w;
  } else if constexpr (ES == 4) {
    u32x4 w;
    __builtin_memcpy(&w, &v[0], 16);
    *(CUBED_G u32x4*)p = w;
  } else {
    u32x4 w[2];
    __builtin_memcpy(&w[0], &v[0], 32);
    *(CUBED_G u32x4*)p = w[0];
    *((CUBED_G u32x4*)p + 1) = w[1];
  }
}

// a / b for a >= 0, b > 0; the 32-bit divide when both fit
CUBED_DEV int64_t udiv(int64_t a, int64_t b) {
  return ((uint64_t)(a | b) >> 32) == 0 ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

// Grid: 1-d, block g -> (task g / work, work item g % work).  Direct form: work
// item w owns the flat outputs [w * kElems, + kElems).  LDS form: with segs =
// ceil(n_idx / kLdsElems), work item w owns the outputs [s * kLdsElems,
// + kLdsElems) of row w / segs, s = w % segs.
template <int ES, bool LDS>
__global__ __launch_bounds__(kBlock) void k_gather(const cubed_gather_task_t* __restrict__ tasks, int64_t ntasks,
                                                   int64_t work) {
  using D = typename uint_of<ES>::type;
  __shared__ __attribute__((aligned(16))) D sk[LDS ? kTileBytes / ES : kPer];  // referenced by the LDS form only
  const int64_t g = blockIdx.x;
  const int64_t ti = g / work, tw = g - ti * work;
  if (ti >= ntasks) return;
  const cubed_gather_task_t* __restrict__ K = tasks + ti;
  const int64_t outer = K->outer, n_idx = K->n_idx, n_src = K->n_src, inner = LDS ? 1 : K->inner;
  const int64_t lo = K->lo, n_total = K->n_total;
  if (outer <= 0 || n_idx <= 0 || inner <= 0 || n_src < 0) return;  // workgroup-uniform
  const int tid = threadIdx.x;
  const CUBED_G D* __restrict__ src = (const CUBED_G D*)(uintptr_t)K->src_base;
  const int64_t rowlen = n_idx * inner;

  // ---- the run [p0, p1) of flat outputs of this workgroup
  int64_t p0, p1, row = 0;
  int64_t m = n_src;  // source places a read may name
  if constexpr (LDS) {
    const int64_t segs = (n_idx + kLdsElems - 1) / kLdsElems;
    row = tw / segs;
    if (row >= outer) return;  // workgroup-uniform
    const int64_t s0 = (tw - row * segs) * kLdsElems;
    p0 = row * n_idx + s0;
    p1 = row * n_idx + (n_idx - s0 < kLdsElems ? n_idx : s0 + kLdsElems);
    // stage source row `row` (the host sends n_src * ES <= kTileBytes only)
    if (m > kTileBytes / ES) m = kTileBytes / ES;
    constexpr int EP = 16 / ES;  // elements of one 16-byte access
    const CUBED_G D* __restrict__ srow = src + row * n_src;
    const int mi = (int)m;
    if (((K->src_base + row * n_src * ES) & 15) == 0) {
      for (int i = tid * EP; i < mi; i += kBlock * EP) {
        if (i + EP <= mi) {
          *(u32x4*)(sk + i) = *(const CUBED_G u32x4*)(srow + i);
        } else {
          for (int e = i; e < mi; ++e) sk[e] = srow[e];
        }
      }
    } else {
      for (int i = tid; i < mi; i += kBlock) sk[i] = srow[i];
    }
    __syncthreads();
  } else {
    const int64_t total = outer * rowlen;
    p0 = tw * kElems;
    if (p0 >= total) return;  // workgroup-uniform
    p1 = total - p0 < kElems ? total : p0 + kElems;
  }

  const CUBED_G int64_t* __restrict__ idx = (const CUBED_G int64_t*)(uintptr_t)K->idx_base;
  const CUBED_G D* __restrict__ prev = (const CUBED_G D*)(uintptr_t)K->prev_base;
  CUBED_G D* __restrict__ dst = (CUBED_G D*)(uintptr_t)K->dst_base;
  constexpr int kAlign = kPer * ES < 16 ? kPer * ES : 16;
  const bool aligned = (K->idx_base & 15) == 0 && ((K->dst_base | K->prev_base) & (kAlign - 1)) == 0;

  // a lane's 4 outputs start at a multiple of 4 of the flat position, so the
  // run's ragged head and tail are the only partial lanes
  for (int64_t e0 = (p0 & ~(int64_t)(kPer - 1)) + (int64_t)tid * kPer; e0 < p1; e0 += kStep) {
    const bool wide = aligned && e0 >= p0 && e0 + kPer <= p1;
    int64_t ix[kPer];
    D v[kPer];
    bool in[kPer];
    if (wide) {
      const i64x2 a = __builtin_nontemporal_load((const CUBED_G i64x2*)(idx + e0));
      const i64x2 b = __builtin_nontemporal_load((const CUBED_G i64x2*)(idx + e0) + 1);
      ix[0] = a.x; ix[1] = a.y; ix[2] = b.x; ix[3] = b.y;
      if (prev) {
        load4<ES, D>(prev + e0, v);
      } else {
#pragma unroll
        for (int q = 0; q < kPer; ++q) v[q] = (D)0;
      }
#pragma unroll
      for (int q = 0; q < kPer; ++q) in[q] = true;
    } else {
#pragma unroll
      for (int q = 0; q < kPer; ++q) {
        const int64_t p = e0 + q;
        in[q] = p >= p0 && p < p1;
        ix[q] = in[q] ? __builtin_nontemporal_load(idx + p) : 0;
        v[q] = in[q] && prev ? prev[p] : (D)0;
      }
    }

    // (o, k) of flat position e0; rem = its offset in row o
    int64_t o = row, rem = 0, k = 0;
    if constexpr (!LDS) {
      o = udiv(e0, rowlen);
      rem = e0 - o * rowlen;
      if (inner > 1) k = rem - udiv(rem, inner) * inner;
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      int64_t i = ix[q];
      if (i < 0) i += n_total;
      const int64_t r = i - lo;
      // every read of the source: lo <= i < lo + n_src
      if (in[q] && (uint64_t)r < (uint64_t)m) {
        if constexpr (LDS) v[q] = sk[r];
        else v[q] = src[(o * n_src + r) * inner + k];
      }
      if constexpr (!LDS) {
        if (++k == inner) k = 0;
        if (++rem == rowlen) { rem = 0; ++o; }
      }
    }

    if (wide) {
      store4<ES, D>(dst + e0, v);
    } else {
#pragma unroll
      for (int q = 0; q < kPer; ++q)
        if (in[q]) dst[e0 + q] = v[q];
    }
  }
}

bool size_ok(int32_t s) { return s == 1 || s == 2 || s == 4 || s == 8; }

template <int ES>
void launch(const cubed_gather_task_t* d_tasks, int64_t ntasks, int path, int64_t work, hipStream_t st) {
  const dim3 grid((unsigned)(ntasks * work)), block(kBlock);
  if (path == CUBED_GATHER_LDS) hipLaunchKernelGGL((k_gather<ES, true>), grid, block, 0, st, d_tasks, ntasks, work);
  else hipLaunchKernelGGL((k_gather<ES, false>), grid, block, 0, st, d_tasks, ntasks, work);
}

}  // namespace

extern "C" int64_t cubed_gather_tile_bytes(void) { return kTileBytes; }

extern "C" int cubed_gather_path(const cubed_gather_task_t* tasks, int64_t ntasks, int32_t esize) {
  if (ntasks < 0 || (ntasks > 0 && !tasks)) return fail("cubed_gather_path: null task table");
  if (!size_ok(esize)) return fail("cubed_gather_path: bad element size");
  const int64_t big = (int64_t)1 << 40;
  bool lds = true, any = false;
  for (int64_t i = 0; i < ntasks; ++i) {
    const cubed_gather_task_t& t = tasks[i];
    if (t.outer < 0 || t.n_idx < 0 || t.n_src < 0 || t.inner < 0) return fail("cubed_gather_path: negative extent");
    if (t.outer > big || t.n_idx > big || t.n_src > big || t.inner > big ||
        (t.n_idx && t.inner && t.outer > big / t.n_idx / t.inner) ||
        (t.n_src && t.inner && t.outer > big / t.n_src / t.inner))
      return fail("cubed_gather_path: chunk too large");
    if (t.lo < 0 || t.n_total < 0 || t.n_src > t.n_total || t.lo > t.n_total - t.n_src)
      return fail("cubed_gather_path: the source block is not inside the axis");
    if (t.outer == 0 || t.n_idx == 0 || t.inner == 0) continue;  // nothing to read or write
    if (!t.idx_base || !t.dst_base || (t.n_src > 0 && !t.src_base))
      return fail("cubed_gather_path: null chunk address");
    if ((t.src_base | t.dst_base | t.prev_base) % esize || t.idx_base % 8)
      return fail("cubed_gather_path: address not aligned to its element");
    if (t.dst_base == t.src_base || t.dst_base == t.idx_base || t.dst_base == t.prev_base)
      return fail("cubed_gather_path: gather in place");
    any = true;
    if (t.inner != 1 || t.n_src * esize > kTileBytes || t.n_idx < t.n_src) lds = false;
  }
  return any && lds ? CUBED_GATHER_LDS : CUBED_GATHER_DIRECT;
}

extern "C" int cubed_gather_chunks(const cubed_gather_task_t* d_tasks, int64_t ntasks, int32_t esize, int32_t path,
                                   int64_t work, void* stream) {
  if (ntasks == 0 || work == 0) return 0;
  if (!d_tasks || ntasks < 0 || work < 0) return fail("cubed_gather_chunks: bad task table");
  if (!size_ok(esize)) return fail("cubed_gather_chunks: bad element size");
  if (path != CUBED_GATHER_DIRECT && path != CUBED_GATHER_LDS) return fail("cubed_gather_chunks: bad path");
  if (work > 0x7fffffff / ntasks) return fail("cubed_gather_chunks: more than 2^31 - 1 workgroups");
  hipStream_t st = (hipStream_t)stream;
  switch (esize) {
    case 1: launch<1>(d_tasks, ntasks, path, work, st); break;
    case 2: launch<2>(d_tasks, ntasks, path, work, st); break;
    case 4: launch<4>(d_tasks, ntasks, path, work, st); break;
    default: launch<8>(d_tasks, ntasks, path, work, st); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s", hipGetErrorString(e)); return (int)e; }
  return 0;
}
