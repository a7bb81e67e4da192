// scan.hip -- prefix sums along one axis of a chunk (cumulative_sum).
//
// A task is one chunk seen as (outer, n, inner): the dims before the scanned
// axis coalesced into outer, the dims after it into inner.  The accumulator is
// f64 (f32 and f64 values) or wrapping int64 (int64 / uint64 bits); it starts
// from the task's carry plane -- the exclusive prefix of the totals of the
// chunks before this one along the axis, computed by an earlier launch of the
// same kernels -- or from zero.  Chunks are therefore independent: no
// workgroup waits for, signals or reads the output of another one, so a launch
// is deterministic and cannot hang.
//
//   k_scan_cols<T, A, VEC>  inner > 1 (or a strided n): one lane owns VEC
//       consecutive inner elements of one outer index and walks n with U rows
//       of non-temporal loads in flight; lanes of a wave read consecutive
//       addresses of each row.
//   k_scan_rows<T, A>       inner == 1 and n contiguous: one wave per row, in
//       tiles of 64 lanes x 4 elements: a serial prefix inside each lane, a
//       wave scan of the lane totals (6 __shfl_up steps), the running total of
//       the earlier tiles carried in a register.
//
// Both read every element once and write it once.
#include <cstdlib>
#include <stdio.h>
#include "common.h"

namespace cubed {
extern thread_local char g_err[512];
}
using namespace cubed;

static int fail(const char* m) { snprintf(g_err, sizeof(g_err), "%s", m); return CUBED_E_ARG; }

namespace {

constexpr int kRowsInFlight = 4;  // rows of loads issued before the first add
constexpr int kTile = 256;        // elements of one wave tile (64 lanes x 4)

template <typename T, int VEC>
struct Pack { T v[VEC]; };

// VEC consecutive elements at p (aligned to min(16, VEC * sizeof(T)) bytes
// when VEC == 4: the host checks before it chooses the width)
template <typename T, int VEC>
CUBED_DEV Pack<T, VEC> load_nt(const CUBED_G T* p) {
  Pack<T, VEC> r;
  if constexpr (VEC == 1) {
    r.v[0] = __builtin_nontemporal_load(p);
  } else if constexpr (sizeof(T) == 4) {
    u32x4 w = __builtin_nontemporal_load((const CUBED_G u32x4*)p);
    __builtin_memcpy(&r, &w, 16);
  } else {
    u32x4 w0 = __builtin_nontemporal_load((const CUBED_G u32x4*)p);
    u32x4 w1 = __builtin_nontemporal_load((const CUBED_G u32x4*)p + 1);
    __builtin_memcpy(&r.v[0], &w0, 16);
    __builtin_memcpy(&r.v[2], &w1, 16);
  }
  return r;
}

template <typename T, int VEC>
CUBED_DEV void store_nt(CUBED_G T* p, const Pack<T, VEC>& r) {
  if constexpr (VEC == 1) {
    __builtin_nontemporal_store(r.v[0], p);
  } else if constexpr (sizeof(T) == 4) {
    u32x4 w;
    __builtin_memcpy(&w, &r, 16);
    __builtin_nontemporal_store(w, (CUBED_G u32x4*)p);
  } else {
    u32x4 w0, w1;
    __builtin_memcpy(&w0, &r.v[0], 16);
    __builtin_memcpy(&w1, &r.v[2], 16);
    __builtin_nontemporal_store(w0, (CUBED_G u32x4*)p);
    __builtin_nontemporal_store(w1, (CUBED_G u32x4*)p + 1);
  }
}

// ---------------------------------------------------------------- columns
// Grid: 1-d, block g -> (task g / bpt, column block g % bpt); the columns of a
// task are its (outer, inner / VEC) pairs, flattened, 256 per block.
template <typename T, typename A, int VEC>
__global__ __launch_bounds__(kBlock) void k_scan_cols(const cubed_scan_task_t* __restrict__ tasks,
                                                      int64_t ntasks, int64_t bpt, int exclusive) {
  const int64_t g = blockIdx.x;
  const int64_t ti = g / bpt, cb = g - ti * bpt;
  if (ti >= ntasks) return;
  const cubed_scan_task_t* __restrict__ K = tasks + ti;
  const int64_t n = K->n, inner = K->inner;
  const int64_t ivec = inner / VEC;
  const int64_t col = cb * kBlock + threadIdx.x;
  if (col >= K->outer * ivec) return;
  const int64_t o = col / ivec, j = (col - o * ivec) * VEC;
  const CUBED_G T* __restrict__ src =
      (const CUBED_G T*)(uintptr_t)K->src_base + (o * K->src_outer_stride + j);
  CUBED_G T* __restrict__ dst = (CUBED_G T*)(uintptr_t)K->dst_base + (o * K->dst_outer_stride + j);
  const int64_t sn = K->src_n_stride, dn = K->dst_n_stride;
  A acc[VEC];
  if (K->carry_base) {
    const CUBED_G A* c = (const CUBED_G A*)(uintptr_t)K->carry_base + (o * K->carry_outer_stride + j);
    Pack<A, VEC> cv = load_nt<A, VEC>(c);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = cv.v[e];
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = (A)0;
  }
  for (int64_t i0 = 0; i0 < n; i0 += kRowsInFlight) {
    Pack<T, VEC> v[kRowsInFlight];
#pragma unroll
    for (int k = 0; k < kRowsInFlight; ++k)
      if (i0 + k < n) v[k] = load_nt<T, VEC>(src + (i0 + k) * sn);
#pragma unroll
    for (int k = 0; k < kRowsInFlight; ++k) {
      if (i0 + k < n) {
        Pack<T, VEC> out;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const A before = acc[e];
          acc[e] = before + (A)v[k].v[e];
          out.v[e] = (T)(exclusive ? before : acc[e]);
        }
        store_nt<T, VEC>(dst + (i0 + k) * dn, out);
      }
    }
  }
}

// ---------------------------------------------------------------- rows
// One wave per row (4 rows per block); block g -> (task g / bpt, rows
// (g % bpt) * 4 .. + 4).
template <typename T, typename A>
__global__ __launch_bounds__(kBlock) void k_scan_rows(const cubed_scan_task_t* __restrict__ tasks,
                                                      int64_t ntasks, int64_t bpt, int exclusive) {
  const int64_t g = blockIdx.x;
  const int64_t ti = g / bpt, rb = g - ti * bpt;
  if (ti >= ntasks) return;
  const cubed_scan_task_t* __restrict__ K = tasks + ti;
  const int lane = threadIdx.x & 63;
  const int64_t row = rb * (kBlock / 64) + (threadIdx.x >> 6);
  if (row >= K->outer) return;  // wave-uniform
  const int64_t n = K->n;
  const CUBED_G T* __restrict__ src = (const CUBED_G T*)(uintptr_t)K->src_base + row * K->src_outer_stride;
  CUBED_G T* __restrict__ dst = (CUBED_G T*)(uintptr_t)K->dst_base + row * K->dst_outer_stride;
  A run = (A)0;  // total of everything before the current tile, the same in every lane
  if (K->carry_base)
    run = *((const CUBED_G A*)(uintptr_t)K->carry_base + row * K->carry_outer_stride);
  const bool aligned = ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
  for (int64_t t0 = 0; t0 < n; t0 += kTile) {
    const int64_t e0 = t0 + lane * 4;
    const bool wide = aligned && t0 + kTile <= n;  // wave-uniform
    Pack<T, 4> v;
    if (wide) {
      v = load_nt<T, 4>(src + e0);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v.v[e] = e0 + e < n ? __builtin_nontemporal_load(src + e0 + e) : (T)0;
    }
    // serial prefix inside the lane
    A p[4];
    p[0] = (A)v.v[0];
#pragma unroll
    for (int e = 1; e < 4; ++e) p[e] = p[e - 1] + (A)v.v[e];
    // inclusive wave scan of the lane totals
    A s = p[3];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const A up = __shfl_up(s, d, 64);
      if (lane >= d) s += up;
    }
    A before = __shfl_up(s, 1, 64);  // total of the lanes below this one
    if (lane == 0) before = (A)0;
    const A total = __shfl(s, 63, 64);
    const A base = run + before;
    Pack<T, 4> out;
    if (exclusive) {
      out.v[0] = (T)base;
#pragma unroll
      for (int e = 1; e < 4; ++e) out.v[e] = (T)(base + p[e - 1]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) out.v[e] = (T)(base + p[e]);
    }
    if (wide) {
      store_nt<T, 4>(dst + e0, out);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e0 + e < n) __builtin_nontemporal_store(out.v[e], dst + e0 + e);
    }
    run += total;
  }
}

bool vtype_ok(int32_t vtype) { return vtype == CUBED_V_F32 || vtype == CUBED_V_F64 || vtype == CUBED_V_I64; }

template <typename T, typename A>
void launch(const cubed_scan_task_t* d_tasks, int64_t ntasks, int exclusive, int path, int64_t bpt,
            hipStream_t st) {
  const dim3 grid((unsigned)(ntasks * bpt));
  if (path == CUBED_SCAN_ROWS)
    hipLaunchKernelGGL((k_scan_rows<T, A>), grid, dim3(kBlock), 0, st, d_tasks, ntasks, bpt, exclusive);
  else if (path == CUBED_SCAN_COLS_V4)
    hipLaunchKernelGGL((k_scan_cols<T, A, 4>), grid, dim3(kBlock), 0, st, d_tasks, ntasks, bpt, exclusive);
  else
    hipLaunchKernelGGL((k_scan_cols<T, A, 1>), grid, dim3(kBlock), 0, st, d_tasks, ntasks, bpt, exclusive);
}

}  // namespace

extern "C" int cubed_scan_path(const cubed_scan_task_t* tasks, int64_t ntasks, int32_t vtype) {
  if (ntasks < 0 || (ntasks > 0 && !tasks)) return fail("cubed_scan_path: null task table");
  if (!vtype_ok(vtype)) return fail("cubed_scan_path: bad value type");
  const int64_t isz = vtype == CUBED_V_F32 ? 4 : 8;
  const int64_t vbytes = 4 * isz;  // 16 (f32) or 32 (f64, i64): the bytes of one lane's 4 elements
  bool rows = true, v4 = true;
  for (int64_t i = 0; i < ntasks; ++i) {
    const cubed_scan_task_t& t = tasks[i];
    if (t.outer < 0 || t.n < 0 || t.inner < 0) return fail("cubed_scan_path: negative extent");
    if (t.outer == 0 || t.n == 0 || t.inner == 0) continue;  // nothing to read or write
    if (!t.src_base || !t.dst_base) return fail("cubed_scan_path: null chunk address");
    if ((t.src_base | t.dst_base) % isz || t.carry_base % 8)
      return fail("cubed_scan_path: address not aligned to its element");
    if (!(t.inner == 1 && t.src_n_stride == 1 && t.dst_n_stride == 1)) rows = false;
    int64_t bits = t.inner * isz | t.src_base | t.dst_base | t.src_n_stride * isz | t.dst_n_stride * isz;
    if (t.outer > 1) bits |= t.src_outer_stride * isz | t.dst_outer_stride * isz;
    if (bits % vbytes) v4 = false;
    if (t.carry_base) {
      int64_t cbits = t.carry_base | t.inner * 8;
      if (t.outer > 1) cbits |= t.carry_outer_stride * 8;
      if (cbits % 32) v4 = false;
    }
  }
  if (rows) return CUBED_SCAN_ROWS;
  return v4 ? CUBED_SCAN_COLS_V4 : CUBED_SCAN_COLS;
}

extern "C" int cubed_scan_chunks(const cubed_scan_task_t* d_tasks, int64_t ntasks, int32_t vtype,
                                 int32_t exclusive, int32_t path, int64_t work, void* stream) {
  if (ntasks == 0 || work == 0) return 0;
  if (!d_tasks || ntasks < 0 || work < 0) return fail("cubed_scan_chunks: bad task table");
  if (!vtype_ok(vtype)) return fail("cubed_scan_chunks: bad value type");
  if (path != CUBED_SCAN_ROWS && path != CUBED_SCAN_COLS && path != CUBED_SCAN_COLS_V4)
    return fail("cubed_scan_chunks: bad path");
  // work: the most rows (rows path) or elements of one (outer, inner) plane
  // (cols paths) of any task
  const int64_t per_block = path == CUBED_SCAN_ROWS ? kBlock / 64
                            : (int64_t)kBlock * (path == CUBED_SCAN_COLS_V4 ? 4 : 1);
  const int64_t bpt = (work + per_block - 1) / per_block;
  if (bpt > 0x7fffffff / ntasks) return fail("cubed_scan_chunks: more than 2^31 - 1 workgroups");
  hipStream_t st = (hipStream_t)stream;
  const int ex = exclusive != 0;
  if (vtype == CUBED_V_F32) launch<float, double>(d_tasks, ntasks, ex, path, bpt, st);
  else if (vtype == CUBED_V_F64) launch<double, double>(d_tasks, ntasks, ex, path, bpt, st);
  else launch<uint64_t, uint64_t>(d_tasks, ntasks, ex, path, bpt, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s", hipGetErrorString(e)); return (int)e; }
  return 0;
}
