// sort.hip -- sorting along the last axis of a chunk (sort / argsort).
//
// A task is one chunk seen as (rows, n), rows contiguous.  Keys are f32, f64,
// i32, i64, u32 or u64; keys-only mode (sort) moves keys, pairs mode (argsort)
// moves (key, int64 index) and orders by (key, index), so it has no ties.
// Order of the keys: ascending with every NaN above every number and all NaNs
// tied, -0.0 == 0.0; descending reverses the key order only.
//
//   k_sort_tile<T, PAIRS>     sorts every aligned tile of kTile elements of
//       every row in LDS: a bitonic network in its normalised form (every
//       comparator ascending), a lane owning 8 consecutive elements so that
//       the steps of distance 4, 2, 1 run in registers.  A row shorter than a
//       tile is padded to npad, the next power of two, kTile / npad rows share
//       a workgroup and the network stops at runs of npad.  Pads sort after
//       every real element, so they never reach the first n places.
//   k_merge_pass<T, PAIRS>    inside a chunk: runs of L become runs of 2L.
//   k_merge_split<T, PAIRS>   across chunks: the first na or the last nb
//       elements of the merge of a lower and an upper chunk, or a copy.
//   Both merges call merge_pick: a lane finds the co-rank of its output
//   element by binary search on its diagonal (ties to the lower run) and
//   writes that one element.
//
// No workgroup waits for, signals or reads what another one writes in the same
// launch; the passes are ordered by the stream.
#include <cstdlib>
#include <limits>
#include <stdio.h>
#include "common.h"
#include "sort_keys.h"

namespace cubed {
extern thread_local char g_err[512];
}
using namespace cubed;

static int fail(const char* m) { snprintf(g_err, sizeof(g_err), "%s", m); return CUBED_E_ARG; }

namespace {

constexpr int kTile = CUBED_SORT_TILE;
constexpr int kPer = kTile / kBlock;  // consecutive elements of one lane
static_assert(kPer == 8, "the register steps are written for 8 elements per lane");

// key_lt, is_float_key: sort_keys.h
template <typename T>
CUBED_DEV bool key_before(T a, T b, bool desc) { return desc ? key_lt(b, a) : key_lt(a, b); }

// the key that sorts after every other one
template <typename T>
CUBED_DEV T pad_key(bool desc) {
  if constexpr (is_float_key<T>) return desc ? -std::numeric_limits<T>::infinity() : std::numeric_limits<T>::quiet_NaN();
  else return desc ? std::numeric_limits<T>::lowest() : std::numeric_limits<T>::max();
}

// kPer consecutive elements at p with 16-byte accesses (p 16-byte aligned)
template <typename T>
CUBED_DEV void load_wide(T (&v)[kPer], const CUBED_G T* p) {
  constexpr int W = kPer * sizeof(T) / 16;
  u32x4 w[W];
#pragma unroll
  for (int i = 0; i < W; ++i) w[i] = *((const CUBED_G u32x4*)p + i);
  __builtin_memcpy(&v[0], &w[0], sizeof(w));
}
template <typename T>
CUBED_DEV void store_wide(CUBED_G T* p, const T (&v)[kPer]) {
  constexpr int W = kPer * sizeof(T) / 16;
  u32x4 w[W];
  __builtin_memcpy(&w[0], &v[0], sizeof(w));
#pragma unroll
  for (int i = 0; i < W; ++i) *((CUBED_G u32x4*)p + i) = w[i];
}

// ---------------------------------------------------------------- tile sort
template <typename T, bool PAIRS>
struct Regs {
  T k[kPer];
  uint32_t i[PAIRS ? kPer : 1];  // position inside the tile when loaded

  // compare-exchange of places a < b: the smaller one goes to a
  CUBED_DEV void cx(int a, int b, bool desc) {
    bool swap = key_before(k[b], k[a], desc);
    if constexpr (PAIRS) swap = swap || (!key_before(k[a], k[b], desc) && i[b] < i[a]);
    if (swap) {
      const T t = k[a]; k[a] = k[b]; k[b] = t;
      if constexpr (PAIRS) { const uint32_t u = i[a]; i[a] = i[b]; i[b] = u; }
    }
  }
  template <int K>
  CUBED_DEV void flip(bool desc) {
#pragma unroll
    for (int a = 0; a < kPer; ++a)
      if ((a ^ (K - 1)) > a) cx(a, a ^ (K - 1), desc);
  }
  template <int J>
  CUBED_DEV void half(bool desc) {
#pragma unroll
    for (int a = 0; a < kPer; ++a)
      if ((a ^ J) > a) cx(a, a ^ J, desc);
  }
};

template <typename T, bool PAIRS>
CUBED_DEV void lds_cx(T* sk, uint32_t* si, int a, int b, bool desc) {
  const T ka = sk[a], kb = sk[b];
  bool swap = key_before(kb, ka, desc);
  if constexpr (PAIRS) {
    const uint32_t ia = si[a], ib = si[b];
    swap = swap || (!key_before(ka, kb, desc) && ib < ia);
    if (swap) { si[a] = ib; si[b] = ia; }
  }
  if (swap) { sk[a] = kb; sk[b] = ka; }
}

// Grid: 1-d, block g -> (task g / work, workgroup g % work of the task).
// to_scratch: the sorted tiles go to the scratch buffers (an odd number of
// merge passes follows).
template <typename T, bool PAIRS>
__global__ __launch_bounds__(kBlock) void k_sort_tile(const cubed_sort_task_t* __restrict__ tasks,
                                                      int64_t ntasks, int64_t work, int to_scratch,
                                                      int descending) {
  __shared__ T sk[kTile];
  __shared__ uint32_t si[PAIRS ? kTile : 1];
  const int64_t g = blockIdx.x;
  const int64_t ti = g / work, tw = g - ti * work;
  if (ti >= ntasks) return;
  const cubed_sort_task_t* __restrict__ K = tasks + ti;
  const int64_t n = K->n, rows = K->rows;
  if (n <= 0 || rows <= 0) return;
  const bool desc = descending != 0;
  // lg: log2 of the run the network sorts (npad); a tile holds kTile >> lg rows
  int lg = 11;
  int64_t row0, col0;
  if (n <= kTile) {
    lg = n <= 1 ? 0 : 32 - __builtin_clz((unsigned)(n - 1));
    row0 = tw << (11 - lg);
    col0 = 0;
  } else {
    const int64_t tpr = (n + kTile - 1) / kTile;
    row0 = tw / tpr;
    col0 = (tw - row0 * tpr) * kTile;
  }
  static_assert(kTile == 2048, "lg assumes tiles of 2^11 elements");
  if (row0 >= rows) return;  // workgroup-uniform
  const int npad = 1 << lg;
  const int e0 = threadIdx.x * kPer;
  const CUBED_G T* __restrict__ src = (const CUBED_G T*)(uintptr_t)K->src_base;
  const int64_t sstride = K->src_row_stride, dstride = K->dst_row_stride;

  Regs<T, PAIRS> r;
  // the lane's first element: row and column (its 8 elements lie in one row
  // when npad >= 8)
  const int64_t lrow = row0 + (e0 >> lg), lcol = col0 + (e0 & (npad - 1));
  const bool one_row = lg >= 3 && lrow < rows && lcol + kPer <= n;
  {
    const CUBED_G T* p = src + (lrow * sstride + lcol);
    if (one_row && (((uintptr_t)p) & 15) == 0) {
      load_wide<T>(r.k, p);
    } else {
#pragma unroll
      for (int q = 0; q < kPer; ++q) {
        const int e = e0 + q;
        const int64_t row = row0 + (e >> lg), col = col0 + (e & (npad - 1));
        r.k[q] = (row < rows && col < n) ? src[row * sstride + col] : pad_key<T>(desc);
      }
    }
    if constexpr (PAIRS) {
#pragma unroll
      for (int q = 0; q < kPer; ++q) r.i[q] = (uint32_t)(e0 + q);
    }
  }
  // runs of up to 8 in registers
  if (lg >= 1) r.template flip<2>(desc);
  if (lg >= 2) { r.template flip<4>(desc); r.template half<1>(desc); }
  if (lg >= 3) { r.template flip<8>(desc); r.template half<2>(desc); r.template half<1>(desc); }
  // runs of 16 .. npad: the flip and the steps of distance >= 8 in LDS
  for (int k = 16; k <= npad; k <<= 1) {
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      sk[e0 + q] = r.k[q];
      if constexpr (PAIRS) si[e0 + q] = r.i[q];
    }
    __syncthreads();
    const int hk = k >> 1;
#pragma unroll
    for (int q = 0; q < kPer / 2; ++q) {
      const int p = q * kBlock + threadIdx.x;  // comparator 0 .. kTile / 2
      const int blk = p / hk, off = p - blk * hk;
      lds_cx<T, PAIRS>(sk, si, blk * k + off, blk * k + k - 1 - off, desc);
    }
    __syncthreads();
    for (int j = k >> 2; j >= kPer; j >>= 1) {
#pragma unroll
      for (int q = 0; q < kPer / 2; ++q) {
        const int p = q * kBlock + threadIdx.x;
        const int a = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        lds_cx<T, PAIRS>(sk, si, a, a + j, desc);
      }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      r.k[q] = sk[e0 + q];
      if constexpr (PAIRS) r.i[q] = si[e0 + q];
    }
    r.template half<4>(desc); r.template half<2>(desc); r.template half<1>(desc);
  }
  // the lane's 8 places of the sorted tile
  CUBED_G T* __restrict__ dst = (CUBED_G T*)(uintptr_t)(to_scratch ? K->scratch_base : K->dst_base);
  CUBED_G T* p = dst + (lrow * dstride + lcol);
  if (one_row && (((uintptr_t)p) & 15) == 0) {
    store_wide<T>(p, r.k);
  } else {
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int e = e0 + q;
      const int64_t row = row0 + (e >> lg), col = col0 + (e & (npad - 1));
      if (row < rows && col < n) dst[row * dstride + col] = r.k[q];
    }
  }
  if constexpr (PAIRS) {
    CUBED_G int64_t* __restrict__ di =
        (CUBED_G int64_t*)(uintptr_t)(to_scratch ? K->scratch_idx_base : K->dst_idx_base);
    const int64_t ib = K->index_base + col0;
    int64_t idx[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) idx[q] = ib + (int64_t)(r.i[q] & (uint32_t)(npad - 1));
    CUBED_G int64_t* pi = di + (lrow * dstride + lcol);
    if (one_row && (((uintptr_t)pi) & 15) == 0) {
      store_wide<int64_t>(pi, idx);
    } else {
#pragma unroll
      for (int q = 0; q < kPer; ++q) {
        const int e = e0 + q;
        const int64_t row = row0 + (e >> lg), col = col0 + (e & (npad - 1));
        if (row < rows && col < n) di[row * dstride + col] = idx[q];
      }
    }
  }
}

// ---------------------------------------------------------------- merges
// Element d of the stable merge of the sorted runs A[0:na] and B[0:nb] (ties
// to A): the co-rank i of d -- how many of the first d elements come from A --
// by binary search on the diagonal i + j = d, then the smaller head.
template <typename T, bool PAIRS>
CUBED_DEV void merge_pick(const CUBED_G T* __restrict__ Ak, const CUBED_G int64_t* __restrict__ Ai, int64_t na,
                          const CUBED_G T* __restrict__ Bk, const CUBED_G int64_t* __restrict__ Bi, int64_t nb,
                          int64_t d, bool desc, T* outk, int64_t* outi) {
  int64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const T a = Ak[mid], b = Bk[d - 1 - mid];
    bool b_first = key_before(b, a, desc);
    if constexpr (PAIRS) {
      if (!b_first && !key_before(a, b, desc)) b_first = Bi[d - 1 - mid] < Ai[mid];
    }
    if (b_first) hi = mid; else lo = mid + 1;
  }
  const int64_t i = lo, j = d - lo;
  bool take_a = i < na;
  if (take_a && j < nb) {
    const T a = Ak[i], b = Bk[j];
    bool b_first = key_before(b, a, desc);
    if constexpr (PAIRS) {
      if (!b_first && !key_before(a, b, desc)) b_first = Bi[j] < Ai[i];
    }
    take_a = !b_first;
  }
  *outk = take_a ? Ak[i] : Bk[j];
  if constexpr (PAIRS) *outi = take_a ? Ai[i] : Bi[j];
}

// flat element f of a (rows, width) task -> (row, column)
CUBED_DEV void row_col(int64_t f, int64_t width, bool small, int64_t* row, int64_t* col) {
  if (small) {
    const uint32_t r = (uint32_t)f / (uint32_t)width;
    *row = r;
    *col = (uint32_t)f - r * (uint32_t)width;
  } else {
    *row = f / width;
    *col = f - *row * width;
  }
}

// One pass inside a chunk: every pair of runs of L elements of a row becomes
// one run of 2L (a short last run is merged as it is, an unpaired one copied;
// a row of n <= L is copied).  Block g -> (task g / work, elements
// (g % work) * kTile .. + kTile of the task's rows * n, flattened).
template <typename T, bool PAIRS>
__global__ __launch_bounds__(kBlock) void k_merge_pass(const cubed_sort_task_t* __restrict__ tasks,
                                                       int64_t ntasks, int64_t work, int64_t L,
                                                       int from_scratch, int descending) {
  const int64_t g = blockIdx.x;
  const int64_t ti = g / work, tw = g - ti * work;
  if (ti >= ntasks) return;
  const cubed_sort_task_t* __restrict__ K = tasks + ti;
  const int64_t n = K->n, rows = K->rows;
  if (n <= 0 || rows <= 0) return;
  const int64_t total = rows * n;
  if (tw * kTile >= total) return;
  const bool small = total <= 0xffffffffll, desc = descending != 0;
  const CUBED_G T* __restrict__ sk = (const CUBED_G T*)(uintptr_t)(from_scratch ? K->scratch_base : K->dst_base);
  CUBED_G T* __restrict__ dk = (CUBED_G T*)(uintptr_t)(from_scratch ? K->dst_base : K->scratch_base);
  const CUBED_G int64_t* __restrict__ sidx =
      (const CUBED_G int64_t*)(uintptr_t)(from_scratch ? K->scratch_idx_base : K->dst_idx_base);
  CUBED_G int64_t* __restrict__ didx =
      (CUBED_G int64_t*)(uintptr_t)(from_scratch ? K->dst_idx_base : K->scratch_idx_base);
  const int64_t stride = K->dst_row_stride;
#pragma unroll 2
  for (int q = 0; q < kPer; ++q) {
    const int64_t f = tw * kTile + q * kBlock + threadIdx.x;
    if (f >= total) break;
    int64_t row, col;
    row_col(f, n, small, &row, &col);
    const int64_t a0 = col & ~(2 * L - 1);  // L is a power of two
    const int64_t na = n - a0 < L ? n - a0 : L;
    const int64_t nb = n - a0 - na < L ? n - a0 - na : L;
    const int64_t base = row * stride + a0;
    T k;
    int64_t ix = 0;
    merge_pick<T, PAIRS>(sk + base, sidx + base, na, sk + base + na, sidx + base + na, nb, col - a0, desc,
                         &k, &ix);
    dk[row * stride + col] = k;
    if constexpr (PAIRS) didx[row * stride + col] = ix;
  }
}

// Across chunks.  Block g -> (task g / work, elements (g % work) * kTile ..
// of the task's rows * count output elements, flattened).
template <typename T, bool PAIRS>
__global__ __launch_bounds__(kBlock) void k_merge_split(const cubed_merge_task_t* __restrict__ tasks,
                                                        int64_t ntasks, int64_t work, int descending) {
  const int64_t g = blockIdx.x;
  const int64_t ti = g / work, tw = g - ti * work;
  if (ti >= ntasks) return;
  const cubed_merge_task_t* __restrict__ K = tasks + ti;
  const int64_t role = K->role, rows = K->rows, na = K->na;
  const int64_t nb = role == CUBED_MERGE_COPY ? 0 : K->nb;
  const int64_t count = role == CUBED_MERGE_HIGH ? nb : na;
  const int64_t first = role == CUBED_MERGE_HIGH ? na : 0;
  if (count <= 0 || rows <= 0) return;
  const int64_t total = rows * count;
  if (tw * kTile >= total) return;
  const bool small = total <= 0xffffffffll, desc = descending != 0;
  const CUBED_G T* __restrict__ ak = (const CUBED_G T*)(uintptr_t)K->lo_base;
  const CUBED_G T* __restrict__ bk = (const CUBED_G T*)(uintptr_t)K->hi_base;
  const CUBED_G int64_t* __restrict__ ai = (const CUBED_G int64_t*)(uintptr_t)K->lo_idx_base;
  const CUBED_G int64_t* __restrict__ bi = (const CUBED_G int64_t*)(uintptr_t)K->hi_idx_base;
  CUBED_G T* __restrict__ dk = (CUBED_G T*)(uintptr_t)K->dst_base;
  CUBED_G int64_t* __restrict__ di = (CUBED_G int64_t*)(uintptr_t)K->dst_idx_base;
  const int64_t as = K->lo_row_stride, bs = K->hi_row_stride, ds = K->dst_row_stride;
#pragma unroll 2
  for (int q = 0; q < kPer; ++q) {
    const int64_t f = tw * kTile + q * kBlock + threadIdx.x;
    if (f >= total) break;
    int64_t row, col;
    row_col(f, count, small, &row, &col);
    T k;
    int64_t ix = 0;
    merge_pick<T, PAIRS>(ak + row * as, ai + row * as, na, bk + row * bs, bi + row * bs, nb, first + col, desc,
                         &k, &ix);
    dk[row * ds + col] = k;
    if constexpr (PAIRS) di[row * ds + col] = ix;
  }
}

// ---------------------------------------------------------------- host
int key_size(int32_t ktype) {
  switch (ktype) {
    case CUBED_F32: case CUBED_I32: case CUBED_U32: return 4;
    case CUBED_F64: case CUBED_I64: case CUBED_U64: return 8;
  }
  return 0;
}

int64_t round256(int64_t b) { return (b + 255) / 256 * 256; }

int passes_for(int64_t n) {
  int p = 0;
  for (int64_t runs = (n + kTile - 1) / kTile; runs > 1; runs = (runs + 1) / 2) ++p;
  return p;
}

template <typename T, bool PAIRS>
void launch_sort(const cubed_sort_task_t* d_tasks, int64_t ntasks, int desc, int passes, int64_t work,
                 hipStream_t st) {
  const dim3 grid((unsigned)(ntasks * work));
  int in_scratch = passes & 1;
  hipLaunchKernelGGL((k_sort_tile<T, PAIRS>), grid, dim3(kBlock), 0, st, d_tasks, ntasks, work, in_scratch, desc);
  int64_t L = kTile;
  for (int p = 0; p < passes; ++p, L *= 2, in_scratch ^= 1)
    hipLaunchKernelGGL((k_merge_pass<T, PAIRS>), grid, dim3(kBlock), 0, st, d_tasks, ntasks, work, L,
                       in_scratch, desc);
}

template <typename T, bool PAIRS>
void launch_merge(const cubed_merge_task_t* d_tasks, int64_t ntasks, int desc, int64_t work, hipStream_t st) {
  hipLaunchKernelGGL((k_merge_split<T, PAIRS>), dim3((unsigned)(ntasks * work)), dim3(kBlock), 0, st, d_tasks,
                     ntasks, work, desc);
}

int last_hip_error() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s", hipGetErrorString(e)); return (int)e; }
  return 0;
}

}  // namespace

#define CUBED_SORT_DISPATCH(FN, ...)                                                        \
  switch (ktype) {                                                                          \
    case CUBED_F32: if (pairs) FN<float, true>(__VA_ARGS__); else FN<float, false>(__VA_ARGS__); break;       \
    case CUBED_F64: if (pairs) FN<double, true>(__VA_ARGS__); else FN<double, false>(__VA_ARGS__); break;     \
    case CUBED_I32: if (pairs) FN<int32_t, true>(__VA_ARGS__); else FN<int32_t, false>(__VA_ARGS__); break;   \
    case CUBED_I64: if (pairs) FN<int64_t, true>(__VA_ARGS__); else FN<int64_t, false>(__VA_ARGS__); break;   \
    case CUBED_U32: if (pairs) FN<uint32_t, true>(__VA_ARGS__); else FN<uint32_t, false>(__VA_ARGS__); break; \
    default: if (pairs) FN<uint64_t, true>(__VA_ARGS__); else FN<uint64_t, false>(__VA_ARGS__); break;        \
  }

extern "C" int64_t cubed_sort_tile(void) { return kTile; }

extern "C" int cubed_sort_plan(const cubed_sort_task_t* tasks, int64_t ntasks, int32_t ktype, int32_t pairs,
                               int32_t* passes, int64_t* scratch_bytes) {
  if (ntasks < 0 || (ntasks > 0 && !tasks)) return fail("cubed_sort_plan: null task table");
  if (!passes || !scratch_bytes) return fail("cubed_sort_plan: null result address");
  const int64_t isz = key_size(ktype);
  if (!isz) return fail("cubed_sort_plan: bad key type");
  int most = 0;
  int64_t bytes = 0;
  for (int64_t i = 0; i < ntasks; ++i) {
    const cubed_sort_task_t& t = tasks[i];
    if (t.rows < 0 || t.n < 0) return fail("cubed_sort_plan: negative extent");
    if (t.rows == 0 || t.n == 0) continue;  // nothing to read or write
    if (!t.src_base || !t.dst_base || (pairs && !t.dst_idx_base))
      return fail("cubed_sort_plan: null chunk address");
    if ((t.src_base | t.dst_base) % isz || t.dst_idx_base % 8)
      return fail("cubed_sort_plan: address not aligned to its element");
    if (t.src_row_stride < t.n || t.dst_row_stride < t.n)
      return fail("cubed_sort_plan: row stride shorter than the row");
    if (t.n > (int64_t)1 << 40 || t.rows > (int64_t)1 << 40 || t.rows * t.dst_row_stride > (int64_t)1 << 44)
      return fail("cubed_sort_plan: chunk too large");
    if (t.index_base < 0) return fail("cubed_sort_plan: negative index base");
    const int p = passes_for(t.n);
    if (p > most) most = p;
    const int64_t elems = t.rows * t.dst_row_stride;
    bytes += round256(elems * isz) + (pairs ? round256(elems * 8) : 0);
  }
  *passes = most;
  *scratch_bytes = most ? bytes : 0;
  return 0;
}

extern "C" int cubed_sort_chunks(const cubed_sort_task_t* d_tasks, int64_t ntasks, int32_t ktype, int32_t flags,
                                 int32_t passes, int64_t work, void* stream) {
  if (ntasks == 0 || work == 0) return 0;
  if (!d_tasks || ntasks < 0 || work < 0) return fail("cubed_sort_chunks: bad task table");
  if (!key_size(ktype)) return fail("cubed_sort_chunks: bad key type");
  if (flags & ~(CUBED_SORT_DESCENDING | CUBED_SORT_PAIRS)) return fail("cubed_sort_chunks: bad flags");
  if (passes < 0 || passes > 40) return fail("cubed_sort_chunks: bad pass count");
  if (work > 0x7fffffff / ntasks) return fail("cubed_sort_chunks: more than 2^31 - 1 workgroups");
  hipStream_t st = (hipStream_t)stream;
  const int desc = (flags & CUBED_SORT_DESCENDING) != 0;
  const bool pairs = (flags & CUBED_SORT_PAIRS) != 0;
  CUBED_SORT_DISPATCH(launch_sort, d_tasks, ntasks, desc, passes, work, st)
  return last_hip_error();
}

extern "C" int cubed_merge_split(const cubed_merge_task_t* d_tasks, int64_t ntasks, int32_t ktype, int32_t flags,
                                 int64_t work, void* stream) {
  if (ntasks == 0 || work == 0) return 0;
  if (!d_tasks || ntasks < 0 || work < 0) return fail("cubed_merge_split: bad task table");
  if (!key_size(ktype)) return fail("cubed_merge_split: bad key type");
  if (flags & ~(CUBED_SORT_DESCENDING | CUBED_SORT_PAIRS)) return fail("cubed_merge_split: bad flags");
  if (work > 0x7fffffff / ntasks) return fail("cubed_merge_split: more than 2^31 - 1 workgroups");
  hipStream_t st = (hipStream_t)stream;
  const int desc = (flags & CUBED_SORT_DESCENDING) != 0;
  const bool pairs = (flags & CUBED_SORT_PAIRS) != 0;
  CUBED_SORT_DISPATCH(launch_merge, d_tasks, ntasks, desc, work, st)
  return last_hip_error();
}
