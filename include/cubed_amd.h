/*
 * cubed_amd.h -- C ABI of the MI355X execution path for Cubed's blockwise /
 * reduction / rechunk primitives (libcubed_amd.so).
 *
 * Plain C: fixed-size structs, raw device pointers, element counts and a
 * hipStream_t passed as void*.  No torch or C++ types cross this boundary.
 * The caller owns every buffer (arrays, task tables, workspace); the library
 * never allocates or frees persistent memory and never synchronises the
 * device.  Every entry point returns 0 on success, a positive hipError_t
 * value on a HIP failure, or a negative CUBED_E_* code on a bad argument;
 * cubed_last_error() gives a message for the calling thread.
 *
 * Which reference interface each entry point replaces (paths relative to the
 * reference tree, rsignell/cubed v0.12.0):
 *
 *   cubed_fused_chunks   -> apply_blockwise(out_key, config=BlockwiseSpec)
 *                           cubed/primitive/blockwise.py:61-84, running the
 *                           fused chunk function built by fuse/fuse_multiple
 *                           (:368-508): elementwise chains (array_object.py
 *                           :121-348, elementwise_functions.py), per-chunk
 *                           reductions (_mean_func/_mean_combine/
 *                           _mean_aggregate statistical_functions.py:54-100,
 *                           nan_functions.py:37-59, sum/max/min/prod) and the
 *                           merge_chunks+combine rounds of core/ops.py:849-889.
 *   cubed_random_chunks  -> _random(x, numblocks, root_seed, block_id)
 *                           cubed/random.py:31-36 (numpy Philox4x64-10 +
 *                           Generator.random), bit-exact.
 *   cubed_copy_boxes     -> copy_read_to_write(chunk_key, config=CubedCopySpec)
 *                           cubed/primitive/rechunk.py:187-192, and the
 *                           map_direct region reads _copy_chunk
 *                           (core/ops.py:784-787) / _read_index_chunk
 *                           (core/ops.py:481-486).
 *   cubed_gemm_chain     -> _matmul / _tensordot chunk products together
 *                           with the _sum_wo_cat k-sum
 *                           cubed/array_api/linear_algebra_functions.py
 *                           :35-78, :139-149 (numpy BLAS sgemm/dgemm per task
 *                           + a reduction over k).
 *   cubed_scan_chunks    -> no reference interface: Array API cumulative_sum
 *                           (2023.12) is not in v0.12.0; the semantics are
 *                           numpy's cumsum along one axis of a chunk.
 *   cubed_sort_chunks,
 *   cubed_merge_split    -> no reference interface: sort / argsort are listed
 *                           as missing in the reference's api_status.md; the
 *                           semantics are numpy's stable sort along one axis.
 *   cubed_search_chunks  -> no reference interface: searchsorted is not in the
 *                           reference either; the semantics are numpy's
 *                           searchsorted of a chunk of values in a sorted chunk.
 *   cubed_hist_chunks    -> no reference interface: histogram is not in the
 *                           reference either; the semantics are numpy's
 *                           histogram of a chunk of values over given edges.
 *   cubed_unique_chunks  -> no reference interface: the unique_* set functions
 *                           are not in the reference either; the semantics are
 *                           numpy's unique (equal_nan) of a sorted chunk.
 *   cubed_select_chunks  -> no reference interface: nonzero and boolean-mask
 *                           indexing are not in the reference either; the
 *                           semantics are numpy's flatnonzero and a[mask].
 *   cubed_gather_chunks  -> no reference interface: the reference notes that
 *                           the Array API lacked take_along_axis
 *                           (cubed/core/ops.py:1124,1145); the semantics are
 *                           numpy's take_along_axis of one block of the axis.
 */
#ifndef CUBED_AMD_H
#define CUBED_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUBED_ABI_VERSION 19

#define CUBED_MAX_DIMS 6   /* iteration dims of one task after coalescing   */
#define CUBED_MAX_LEAVES 4 /* array/philox/const-array inputs of a program  */
#define CUBED_MAX_FIELDS 3 /* reduced fields (mean: n, total; var: n, mu, M2) */
#define CUBED_MAX_OUTS 3   /* output arrays written per task (var: n, mu, M2) */
#define CUBED_MAX_INSNS 48 /* VM instructions in the prologue program       */
#define CUBED_MAX_EPI 16   /* VM instructions in the epilogue program       */
#define CUBED_MAX_CONSTS 16
#define CUBED_NREGS 6      /* VM registers; leaf i is preloaded into reg i  */

/* error codes (negative); positive values are hipError_t */
#define CUBED_MODE_STREAM 8
#define CUBED_MODE_PARTIALS 16
#define CUBED_MODE_STREAM_W2 32
#define CUBED_MODE_STREAM_W4 64
#define CUBED_MODE_HOST_COUNT 128 /* partials: COUNT fields are left to the host */
#define CUBED_MODE_STREAM_EVEN 256 /* stream: every task the same reduced extent */
/* stream + partials, multi-GPU reduce-scatter (ABI 16): the ONE stored field's
 * partial of SoA element i (group g = i / mko) is written to owner-major slot
 * ((g % W) * L + g / W) * mko + i % mko of the SoA region, with mko, W, L in
 * consts[CUBED_MAX_CONSTS - 3 .. - 1] (host-checked: block-cyclic owners, one
 * summed field, every other field host-counted) */
#define CUBED_MODE_OWNER_MAJOR 512

#define CUBED_E_ARG (-1)
#define CUBED_E_DTYPE (-2)
#define CUBED_E_LAYOUT (-3)
#define CUBED_E_WORKSPACE (-4)
#define CUBED_E_JIT (-5)
#define CUBED_E_CODEC (-6)       /* malformed compressed chunk */
#define CUBED_E_UNSUPPORTED (-7) /* codec / shuffle this build does not decode */

/* element dtypes (numpy kinds); bool is 1 byte 0/1 */
enum cubed_dtype {
  CUBED_BOOL = 0, CUBED_I8, CUBED_I16, CUBED_I32, CUBED_I64,
  CUBED_U8, CUBED_U16, CUBED_U32, CUBED_U64,
  CUBED_F32, CUBED_F64, CUBED_F16, CUBED_BF16
};

/* register value type of a program (all arithmetic happens in it; narrower
 * node dtypes are re-rounded by CAST instructions) */
enum cubed_vtype { CUBED_V_F32 = 0, CUBED_V_F64 = 1, CUBED_V_I64 = 2 };

/* leaf kinds */
enum cubed_leaf_kind {
  CUBED_LEAF_ARRAY = 0,  /* strided view of a chunk (or of merged chunks)  */
  CUBED_LEAF_PHILOX = 1, /* numpy Generator(Philox(key)).random() stream,  */
                         /* element = C-order position in the task's box   */
  CUBED_LEAF_OFFSET = 2, /* the task's block offset (int64), for block_id  */
  CUBED_LEAF_IOTA = 3    /* int64 value leaf_base + sum(coord*stride): the  */
                         /* global index along an axis (arange/eye/tril)    */
};

/* reduction ops of a field; accumulators are f64 or i64 (acc_type).  The
 * pair ops couple field 0 (the lead, one of ARGMAX/ARGMIN/CPROD) with field 1
 * (its partner, PAIR_INDEX / PAIR_IMAG): argmax/argmin reduce {value, index}
 * pairs (core/ops.py:1093-1153 _arg_func/_arg_combine), cprod the {re, im}
 * parts of a complex product (np.prod of complex chunks).  A program holding
 * a pair has exactly these two fields.
 * var triples couple field 0 (n, int64: VAR or VARC) with field 1 (mu,
 * VAR_MEAN) and field 2 (M2, VAR_M2), f64: the count, mean and sum of
 * squared deviations of Chan, Golub & LeVeque's pairwise update.  VAR folds
 * element VALUES (field 0's source) by Welford's update; VARC folds partial
 * {n, mu, M2} triples (the three fields' sources) -- the combine rounds of
 * var's reduction; accumulators always combine by Chan's update.  A program
 * holding a triple has exactly these three fields. */
enum cubed_rop {
  CUBED_R_NONE = 0, CUBED_R_SUM, CUBED_R_NANSUM, CUBED_R_COUNT,
  CUBED_R_COUNT_NONNAN, CUBED_R_MAX, CUBED_R_MIN, CUBED_R_PROD,
  CUBED_R_NANMAX, CUBED_R_NANMIN, CUBED_R_ANY, CUBED_R_ALL, CUBED_R_NANPROD,
  CUBED_R_ARGMAX, CUBED_R_ARGMIN, CUBED_R_CPROD, CUBED_R_PAIR_INDEX, CUBED_R_PAIR_IMAG,
  CUBED_R_VAR, CUBED_R_VARC, CUBED_R_VAR_MEAN, CUBED_R_VAR_M2
};

/* VM opcodes (two-address: r[a] = op(r[a], r[b]); where: r[a] = r[c] ? r[a] : r[b]) */
enum cubed_op {
  CUBED_OP_NOP = 0,
  CUBED_OP_CONST,   /* r[a] = consts[imm]                                  */
  CUBED_OP_MOV,     /* r[a] = r[b]                                         */
  CUBED_OP_CAST,    /* r[a] = round r[a] to dtype t (from dtype imm)       */
  CUBED_OP_WHERE,   /* r[a] = r[c] ? r[a] : r[b]                           */
  /* unary */
  CUBED_OP_NEG = 16, CUBED_OP_ABS, CUBED_OP_SQRT, CUBED_OP_EXP, CUBED_OP_LOG,
  CUBED_OP_SIN, CUBED_OP_COS, CUBED_OP_TAN, CUBED_OP_TANH, CUBED_OP_FLOOR,
  CUBED_OP_CEIL, CUBED_OP_TRUNC, CUBED_OP_RINT, CUBED_OP_ISNAN, CUBED_OP_ISINF,
  CUBED_OP_ISFINITE, CUBED_OP_LNOT, CUBED_OP_BNOT, CUBED_OP_SIGN,
  CUBED_OP_SQUARE, CUBED_OP_RECIP, CUBED_OP_LOG1P, CUBED_OP_EXPM1,
  CUBED_OP_LOG2, CUBED_OP_LOG10, CUBED_OP_SINH, CUBED_OP_COSH, CUBED_OP_ASIN,
  CUBED_OP_ACOS, CUBED_OP_ATAN, CUBED_OP_ASINH, CUBED_OP_ACOSH,
  CUBED_OP_ATANH, CUBED_OP_EXP2, CUBED_OP_SIGNBIT,
  /* binary */
  CUBED_OP_ADD = 64, CUBED_OP_SUB, CUBED_OP_MUL, CUBED_OP_DIV,
  CUBED_OP_FLOORDIV, CUBED_OP_MOD, CUBED_OP_POW, CUBED_OP_MAX, CUBED_OP_MIN,
  CUBED_OP_EQ, CUBED_OP_NE, CUBED_OP_LT, CUBED_OP_LE, CUBED_OP_GT,
  CUBED_OP_GE, CUBED_OP_LAND, CUBED_OP_LOR, CUBED_OP_LXOR, CUBED_OP_BAND,
  CUBED_OP_BOR, CUBED_OP_BXOR, CUBED_OP_SHL, CUBED_OP_SHR, CUBED_OP_ATAN2,
  CUBED_OP_HYPOT, CUBED_OP_LOGADDEXP, CUBED_OP_COPYSIGN, CUBED_OP_FMAX,
  CUBED_OP_FMIN, CUBED_OP_LOGADDEXP2,
  /* uint64 operands in int64 registers (ABI 17): the register holds the bit
   * pattern, these read it as unsigned */
  CUBED_OP_UFLOORDIV, CUBED_OP_UMOD, CUBED_OP_UMAX, CUBED_OP_UMIN, CUBED_OP_ULT,
  CUBED_OP_ULE, CUBED_OP_UGT, CUBED_OP_UGE, CUBED_OP_USHR
};

typedef struct {
  uint8_t op, a, b, c; /* opcode and register operands                      */
  uint8_t t;           /* CAST target dtype                                 */
  uint8_t pad;
  uint16_t imm;        /* CONST index / CAST source dtype                   */
} cubed_insn_t;

/* A fused chunk program: leaves -> prologue -> (per-field reduce) ->
 * epilogue -> outputs.  Passed by value as the kernel argument. */
typedef struct {
  int32_t vtype;                 /* enum cubed_vtype                        */
  int32_t ndim;                  /* iteration dims (<= CUBED_MAX_DIMS)      */
  int32_t nred;                  /* dims [0,nred) are reduced (kernel A) or */
                                 /* dims [ndim-nred,ndim) (kernel B)        */
  int32_t mode;                  /* kernel shape: 0 = A (reduced dims first,*/
                                 /* or a map), 1 = B (reduced dims last);   */
                                 /* +4 when the innermost dim is packed     */
                                 /* (VEC=4 loads/stores; host-checked)      */
                                 /* +8 (CUBED_MODE_STREAM): streaming fast  */
                                 /* path, host-checked: kernel A, VEC=4,    */
                                 /* ndim == nred + 1, nred <= 2, every leaf */
                                 /* an ARRAY in the vtype's own dtype       */
                                 /* (f32/f64/i64) with packed kept dim and  */
                                 /* reduced strides that are multiples of 4 */
                                 /* +16 (CUBED_MODE_PARTIALS): reductions   */
                                 /* stop before the epilogue and leave the  */
                                 /* per-field accumulators as SoA partials  */
                                 /* at the start of the workspace (see      */
                                 /* cubed_fused_finish)                     */
                                 /* +32 / +64 (CUBED_MODE_STREAM_W2 / _W4): */
                                 /* streaming JIT kernels give each thread  */
                                 /* 2 / 4 groups of 4 kept elements         */
                                 /* (interpreted kernels ignore the bits)   */
                                 /* +128 (CUBED_MODE_HOST_COUNT): partials  */
                                 /* mode leaves plain COUNT fields unwritten*/
                                 /* in the SoA block -- the host fills them */
                                 /* with the (geometry-known) global count  */
                                 /* +256 (CUBED_MODE_STREAM_EVEN), +512     */
                                 /* (CUBED_MODE_OWNER_MAJOR): see above     */
  int32_t nleaves;
  uint8_t leaf_kind[CUBED_MAX_LEAVES];
  uint8_t leaf_dtype[CUBED_MAX_LEAVES];
  int32_t nfields;               /* 0 = map (no reduction)                  */
  uint8_t field_rop[CUBED_MAX_FIELDS];
  uint8_t field_acc[CUBED_MAX_FIELDS]; /* 0 = f64 accumulator, 1 = i64,     */
                                       /* 2 = i64 bits of a uint64 (ABI 17: */
                                       /* max / min order it as unsigned)   */
  uint8_t field_src[CUBED_MAX_FIELDS]; /* register holding the field value  */
  uint8_t pad0[3];
  int32_t nouts;
  uint8_t out_dtype[CUBED_MAX_OUTS];
  uint8_t out_src[CUBED_MAX_OUTS]; /* register (or field when no epilogue)  */
  uint8_t pad1[2];
  int32_t ninsns;
  int32_t nepi;                  /* -1 = store fields directly              */
  cubed_insn_t insns[CUBED_MAX_INSNS];
  cubed_insn_t epi[CUBED_MAX_EPI];
  union { double f; int64_t i; } consts[CUBED_MAX_CONSTS];
} cubed_program_t;

/* One task (= one output chunk of the pipeline, or one sub-box of it).
 * Strides are in elements; a broadcast dim has stride 0; an output has
 * stride 0 on reduced dims.  Bases are device byte addresses. */
typedef struct {
  int64_t extent[CUBED_MAX_DIMS];
  int64_t leaf_base[CUBED_MAX_LEAVES];
  int64_t leaf_stride[CUBED_MAX_LEAVES][CUBED_MAX_DIMS];
  int64_t out_base[CUBED_MAX_OUTS];
  int64_t out_stride[CUBED_MAX_OUTS][CUBED_MAX_DIMS];
  uint64_t key_lo, key_hi; /* Philox key of this task's random leaf          */
  int64_t block_offset;    /* C-order block offset (block_id_to_offset)      */
  int64_t pad;
} cubed_task_t;

/* Run a fused chunk program over ntasks tasks (task table in device memory).
 * All tasks share the dim structure of `prog` (ndim, nred) but may differ in
 * extents (edge chunks).  max_kept / max_red bound the per-task kept and
 * reduced element counts (the library sizes its grid from them).
 * `prog` is read on the host (launch shape, argument checks); `d_prog` is a
 * byte-identical copy in device memory that the kernels read through the
 * scalar cache (a by-value kernel argument indexed by the interpreter loop
 * would be demoted to scratch).
 * workspace may be NULL when cubed_fused_workspace_bytes() returns 0. */
int cubed_fused_chunks(const cubed_program_t* prog, const cubed_program_t* d_prog,
                       const cubed_task_t* d_tasks,
                       int64_t ntasks, int64_t max_kept, int64_t max_red,
                       void* d_workspace, int64_t workspace_bytes, void* stream);

/* Runtime-specialised form of cubed_fused_chunks (same semantics, same task
 * table): cubed_fused_compile() generates a kernel for *prog with the program
 * baked in as compile-time constants (straight-line code, no interpreter
 * dispatch), compiles it for gfx950 with hipRTC and caches the code object
 * per program for the life of the process.  `include_dirs` is a ';'-separated
 * list holding kernels.h/vm.h/common.h and cubed_amd.h.  Needs no GPU; the
 * code object is loaded on the current device at first launch.
 * Replaces the same reference interface as cubed_fused_chunks, plus the
 * plan-time composition of the chunk function (fuse / fuse_multiple,
 * cubed/primitive/blockwise.py:368-508). */
int cubed_fused_compile(const cubed_program_t* prog, const char* include_dirs, void** handle);
int cubed_fused_chunks_compiled(void* handle, const cubed_program_t* prog,
                                const cubed_program_t* d_prog, const cubed_task_t* d_tasks,
                                int64_t ntasks, int64_t max_kept, int64_t max_red,
                                void* d_workspace, int64_t workspace_bytes, void* stream);
/* The generated source / code object size of a compiled program (diagnostics). */
const char* cubed_fused_source(const void* handle);
int64_t cubed_fused_code_bytes(const void* handle);

/* Split target of streaming reductions: a grid too small to cover HBM
 * latency unsplit is split toward this many workgroups (default 256, one per
 * CU).  Process-wide tuning hook for probes (tools/); workgroups <= 0 only
 * queries.  Returns the previous value. */
int64_t cubed_stream_split_target(int64_t workgroups);
/* Probe hook: split streaming reductions whose grid already fills the chip
 * into nsplit row ranges too (0 = off, the default; < 0 queries). */
int64_t cubed_stream_force_split(int64_t nsplit);

/* Workspace the call above needs (split reductions keep partial
 * accumulators there).  Pure host function. */
int64_t cubed_fused_workspace_bytes(const cubed_program_t* prog, int64_t ntasks,
                                    int64_t max_kept, int64_t max_red);

/* Multi-GPU reductions (partials mode, CUBED_MODE_PARTIALS in prog->mode).
 * cubed_fused_chunks / _compiled then stop before the epilogue: the first
 * nfields*ntasks*max_kept*8 bytes of the workspace receive the per-field
 * accumulators as SoA, partials[f][t][k] (f64 or i64 per field_acc, the
 * reduction identity for k past an edge task's extent), identical in layout
 * on every rank so they can be combined with RCCL.  Replaces the last
 * combine round + aggregate of reduction (cubed/core/ops.py:849-892,
 * _mean_combine/_mean_aggregate statistical_functions.py:61-100) when the
 * round's inputs live on different GPUs.
 * cubed_fused_finish runs the epilogue + stores of the same program from
 * combined SoA partials (same task table, ntasks, max_kept).
 * cubed_combine_partials folds nparts SoA blocks (nfields*n accumulators
 * each, n = ntasks*max_kept, block r at r*nfields*n) in block order into
 * d_out with the fields' own combine ops (used for max/min/prod/any/all,
 * whose NaN semantics RCCL's reductions do not follow). */
int cubed_fused_finish(const cubed_program_t* prog, const cubed_program_t* d_prog,
                       const cubed_task_t* d_tasks, int64_t ntasks, int64_t max_kept,
                       const void* d_partials, void* stream);
/* The same finish, specialised: the JIT module of `handle` (cubed_fused_compile
 * of a CUBED_MODE_PARTIALS program) carries it; CUBED_E_JIT if it does not. */
int cubed_fused_finish_compiled(void* handle, const cubed_program_t* prog, const cubed_task_t* d_tasks,
                                int64_t ntasks, int64_t max_kept, const void* d_partials, void* stream);
/* Grouped finish (partials mode): tasks [group_start[g], group_start[g+1]) are
 * pieces of ONE output box -- a task split where its inputs straddle source
 * chunks along a reduced dim (e.g. the a[1:] regions of index/map_direct,
 * core/ops.py:374-486, feeding a reduction) -- whose partials are combined in
 * piece order; the first piece's output views get the epilogue.
 * d_group_start: ngroups + 1 int64 in device memory. */
int cubed_fused_finish_groups(const cubed_program_t* prog, const cubed_program_t* d_prog,
                              const cubed_task_t* d_tasks, int64_t ntasks, int64_t max_kept,
                              const void* d_partials, const int64_t* d_group_start,
                              int64_t ngroups, void* stream);
/* Multi-GPU form of the grouped finish: fold each group's rows into
 * d_group_partials[f][g][k] (max_kept_out per group, identity past a group's
 * kept extent) WITHOUT the epilogue, so the per-rank group partials -- pieces
 * of one output box run on the GPUs that hold their source chunks -- can be
 * combined over RCCL and finished by cubed_fused_finish on the owner. */
int cubed_combine_groups(const cubed_program_t* prog, const cubed_program_t* d_prog,
                         const cubed_task_t* d_tasks, int64_t ntasks, int64_t max_kept,
                         const void* d_row_partials, const int64_t* d_group_start,
                         int64_t ngroups, int64_t max_kept_out, void* d_group_partials,
                         void* stream);
/* Fold each group's rows AND their kept elements into one accumulator per
 * field: d_group_partials[f][g].  For full reductions run "lifted" (the
 * innermost reduced dims walked as kept dims so every lane streams, e.g.
 * mean(a[1:] * x + b[1:] * y) of the vorticity example).  With an epilogue
 * program (fin / d_fin: the same program with nred = ndim) the kernel also
 * finishes each group into d_fin_tasks[g] (one launch); without it the caller
 * runs cubed_fused_finish over d_group_partials.  ABI 13. */
int cubed_fold_groups(const cubed_program_t* prog, const cubed_program_t* d_prog,
                      const cubed_task_t* d_tasks, int64_t ntasks, int64_t max_kept,
                      const void* d_row_partials, const int64_t* d_group_start,
                      int64_t ngroups, void* d_group_partials, int64_t nsplit,
                      void* d_split_ws, const cubed_program_t* fin, const cubed_program_t* d_fin,
                      const cubed_task_t* d_fin_tasks, void* stream);
/* Splits per group cubed_fold_groups should use (few groups of many
 * elements: each group's rows x max_kept SoA entries cut into nsplit equal
 * runs, the last run to finish folds them); d_split_ws then holds
 * nfields x ngroups x nsplit 8-byte accumulators followed by ngroups uint32
 * arrival counters -- zero it once, the kernel leaves the counters at zero. */
int64_t cubed_fold_groups_splits(int64_t ngroups, int64_t max_rows_per_group, int64_t max_kept);
/* The same fold + finish from the JIT module of a CUBED_MODE_PARTIALS program
 * (cubed_fused_compile): combine and epilogue specialised, the epilogue the
 * program's own (its outputs through d_fin_tasks[g]); CUBED_E_JIT if the
 * module has no fold kernel. */
int cubed_fold_groups_compiled(void* handle, const cubed_program_t* prog, const cubed_task_t* d_tasks,
                               int64_t ntasks, int64_t max_kept, const void* d_row_partials,
                               const int64_t* d_group_start, int64_t ngroups, void* d_group_partials,
                               int64_t nsplit, void* d_split_ws, const cubed_task_t* d_fin_tasks, void* stream);
int cubed_combine_partials(const cubed_program_t* prog, const cubed_program_t* d_prog,
                           const void* d_parts, int32_t nparts, int64_t n, void* d_out,
                           void* stream);
/* Fill ntasks chunks with numpy Generator(Philox(key)).random() doubles:
 * d_out[i] (device pointers) gets counts[i] doubles from key (lo,hi)[i].
 * All three tables are device arrays of ntasks entries. */
int cubed_random_chunks(const int64_t* d_out_ptrs, const int64_t* d_counts,
                        const uint64_t* d_keys /* 2*ntasks: lo,hi */,
                        int64_t ntasks, int64_t max_count, void* stream);

/* Strided N-d box copies (rechunk, merge_chunks, index).  Each box moves
 * extent[0..ndim) elements of `itemsize` bytes from src to dst views. */
typedef struct {
  int64_t src_base, dst_base;      /* device byte addresses                 */
  int64_t extent[CUBED_MAX_DIMS];  /* innermost last; unused dims = 1       */
  int64_t src_stride[CUBED_MAX_DIMS];
  int64_t dst_stride[CUBED_MAX_DIMS];
} cubed_box_t;

/* path: CUBED_COPY_ROWS   -- innermost dim contiguous on both sides; rows are
 *                            moved with lane_bytes-wide lanes (16/8/4/1, must
 *                            divide every row's byte count and offset);
 *                            work = max rows per box, row_bytes = max row size
 *       CUBED_COPY_ELEMS  -- any strides, element at a time; work = max elems
 *       CUBED_COPY_TILE   -- 2-d boxes, src contiguous along dim 1 and dst
 *                            along dim 0 (64x64 LDS tile); work = tiles/box
 *       CUBED_COPY_FLAT   -- 2-d boxes, innermost dim contiguous on both sides
 *                            and dst packed (dst_stride[0] == extent[1]): the
 *                            box is written as one run of lane_bytes words;
 *                            work = max words per box (< 2^31) */
#define CUBED_COPY_ROWS 0
#define CUBED_COPY_ELEMS 1
#define CUBED_COPY_TILE 2
#define CUBED_COPY_FLAT 3
int cubed_copy_boxes(const cubed_box_t* d_boxes, int64_t nboxes, int32_t ndim,
                     int32_t itemsize, int32_t path, int32_t lane_bytes,
                     int64_t work, int64_t row_bytes, void* stream);

/* Prefix sums along one axis of a chunk (cumulative_sum, ABI 18).  A task is
 * one chunk seen as (outer, n, inner) -- the dims before the scanned axis
 * coalesced into outer, those after it into inner, whose stride is 1 -- and
 * writes dst[o, i, j] = carry[o, j] + sum of src[o, 0..i, j] (exclusive:
 * 0..i-1).  Values are f32, f64 or int64 (uint64 has the same bits under a
 * wrapping add); the sum runs in f64 for both float types and in wrapping
 * 64-bit integers otherwise, and the carry plane holds that accumulator type
 * (f64 for f32 values).  carry_base 0 = start from zero.  Tasks are
 * independent: no workgroup communicates with another one, so results are
 * bit-identical from run to run. */
typedef struct {
  int64_t src_base, dst_base, carry_base;      /* device byte addresses; carry_base 0 = none */
  int64_t outer, n, inner;                     /* elements */
  int64_t src_outer_stride, src_n_stride;      /* elements; the inner stride is 1 */
  int64_t dst_outer_stride, dst_n_stride;
  int64_t carry_outer_stride;                  /* elements of the accumulator type */
} cubed_scan_task_t;

/* path: CUBED_SCAN_ROWS    -- every task has inner == 1 and n contiguous: one
 *                             wave per row, tiles of 64 lanes x 4 elements;
 *                             work = max rows (outer) of a task
 *       CUBED_SCAN_COLS    -- one lane per (outer, inner) column walking n;
 *                             work = max outer * inner of a task
 *       CUBED_SCAN_COLS_V4 -- the same with 4 consecutive inner elements per
 *                             lane: inner, every base and every stride of
 *                             every task keep 16-byte (f32) / 32-byte (f64,
 *                             int64) alignment */
#define CUBED_SCAN_ROWS 0
#define CUBED_SCAN_COLS 1
#define CUBED_SCAN_COLS_V4 2
/* Host only (no device call): the path a HOST copy of a task table takes, or a
 * negative CUBED_E_* code for a malformed table. */
int cubed_scan_path(const cubed_scan_task_t* tasks, int64_t ntasks, int32_t vtype);
/* One launch over a DEVICE task table, with the path cubed_scan_path gave for
 * its host copy. */
int cubed_scan_chunks(const cubed_scan_task_t* d_tasks, int64_t ntasks, int32_t vtype,
                      int32_t exclusive, int32_t path, int64_t work, void* stream);

/* Sorting along the last (contiguous) axis of a chunk (sort / argsort, ABI 19).
 * A task is one chunk seen as (rows, n).  Keys are f32, f64, i32, i64, u32 or
 * u64 (ktype: the cubed_dtype code).  Order: values ascend, every NaN is
 * greater than every number and all NaNs tie, -0.0 and 0.0 tie; descending
 * reverses the value order.  Pairs mode sorts (key, int64 index) with ties
 * going to the smaller index in both directions, so its order is total and the
 * result stable; keys-only mode leaves equal keys interchangeable.  No
 * workgroup waits for, signals or reads the output of another one inside a
 * launch; passes are ordered by the stream only. */
#define CUBED_SORT_TILE 2048      /* elements one workgroup sorts in LDS */
#define CUBED_SORT_DESCENDING 1   /* flags */
#define CUBED_SORT_PAIRS 2

/* cubed_sort_chunks task.  The tile sort reads src (keys only: in pairs mode
 * element i of a row gets index index_base + i) and the merge passes ping-pong
 * between dst and scratch, ending in dst.  Scratch buffers have dst's layout
 * (rows * dst_row_stride elements); they may be 0 when the launch has no merge
 * pass.  The idx addresses are used in pairs mode only. */
typedef struct {
  int64_t src_base;                        /* device byte addresses */
  int64_t dst_base, dst_idx_base;
  int64_t scratch_base, scratch_idx_base;
  int64_t rows, n;                         /* elements */
  int64_t src_row_stride, dst_row_stride;  /* elements */
  int64_t index_base;
} cubed_sort_task_t;

/* cubed_merge_split task: the rows of a lower chunk (rows x na) and an upper
 * chunk (rows x nb), each row sorted, are merged row by row (ties go to the
 * lower chunk) and dst receives the first na (CUBED_MERGE_LOW) or the last nb
 * (CUBED_MERGE_HIGH) elements of every merged row.  CUBED_MERGE_COPY: no
 * partner, dst = the lower chunk (hi_* unused). */
#define CUBED_MERGE_LOW 0
#define CUBED_MERGE_HIGH 1
#define CUBED_MERGE_COPY 2
typedef struct {
  int64_t lo_base, lo_idx_base;
  int64_t hi_base, hi_idx_base;
  int64_t dst_base, dst_idx_base;
  int64_t rows, na, nb;
  int64_t lo_row_stride, hi_row_stride, dst_row_stride;  /* elements */
  int64_t role;
} cubed_merge_task_t;

/* Host only: CUBED_SORT_TILE of the loaded library. */
int64_t cubed_sort_tile(void);
/* Host only (no device call): validates a HOST copy of a sort task table
 * (scratch addresses are not looked at) and reports what its launch needs:
 * *passes = merge passes = ceil(log2(ceil(n / TILE))) of the largest n, and
 * *scratch_bytes = 0 without a pass, else the sum over the tasks of their key
 * (and, pairs, index) scratch, each rounded up to 256 bytes.  Returns 0 or a
 * negative CUBED_E_* code. */
int cubed_sort_plan(const cubed_sort_task_t* tasks, int64_t ntasks, int32_t ktype,
                    int32_t pairs, int32_t* passes, int64_t* scratch_bytes);
/* 1 + passes launches over a DEVICE task table.  work = the most workgroups
 * any task needs: ceil(rows * npad / TILE) with npad the next power of two at
 * or above n when n <= TILE, else rows * ceil(n / TILE).  Neither synchronises
 * nor allocates. */
int cubed_sort_chunks(const cubed_sort_task_t* d_tasks, int64_t ntasks, int32_t ktype,
                      int32_t flags, int32_t passes, int64_t work, void* stream);
/* One launch over a DEVICE table of merge tasks.  work = the most
 * ceil(rows * count / TILE) of any task, count the elements per row it writes. */
int cubed_merge_split(const cubed_merge_task_t* d_tasks, int64_t ntasks, int32_t ktype,
                      int32_t flags, int64_t work, void* stream);

/* Searching a sorted chunk (searchsorted; new symbols only, the ABI version is
 * unchanged).  A task counts, for every element v of a flat run of n_values
 * values, the elements of a sorted run of n_sorted keys that sort before v
 * (before or tied with v: CUBED_SEARCH_RIGHT) in the order of the sort
 * entries: values ascend, every NaN is greater than every number and all NaNs
 * tie, -0.0 and 0.0 tie.  dst[i] = (acc_base ? acc[i] : 0) + count(values[i]),
 * int64; acc and dst are flat runs of n_values int64.  Keys and values have
 * the same type (ktype: the cubed_dtype code of f32, f64, i32, i64, u32 or
 * u64).  No workgroup waits for, signals or reads the output of another one
 * and there are no atomics: results are bit-identical run to run. */
#define CUBED_SEARCH_TILE 4096    /* most sorted elements one workgroup stages whole in
                                     LDS (32 KiB at 8-byte keys); splitters of the other path */
#define CUBED_SEARCH_VALUES 16384 /* values one workgroup searches */
#define CUBED_SEARCH_RIGHT 1      /* flags */
#define CUBED_SEARCH_LDS 0        /* paths: every n_sorted <= TILE, the sorted chunk in LDS */
#define CUBED_SEARCH_SPLIT 1      /* up to TILE splitters in LDS, then one bucket in global memory */

typedef struct {
  int64_t sorted_base, values_base;  /* device byte addresses */
  int64_t acc_base;                  /* 0 = none */
  int64_t dst_base;
  int64_t n_sorted, n_values;        /* elements */
} cubed_search_task_t;

/* Host only: CUBED_SEARCH_TILE of the loaded library. */
int64_t cubed_search_tile(void);
/* Host only (no device call): validates a HOST copy of a search task table and
 * returns the path of its launch: CUBED_SEARCH_LDS when every task has
 * n_sorted <= CUBED_SEARCH_TILE, else CUBED_SEARCH_SPLIT; a negative CUBED_E_*
 * code for a malformed table. */
int cubed_search_path(const cubed_search_task_t* tasks, int64_t ntasks, int32_t ktype);
/* One launch over a DEVICE task table.  work = the most workgroups any task
 * needs = ceil(n_values / CUBED_SEARCH_VALUES) of the largest n_values.
 * CUBED_SEARCH_SPLIT is correct for every n_sorted, CUBED_SEARCH_LDS only for
 * the tables cubed_search_path gives it to.  Neither synchronises nor allocates. */
int cubed_search_chunks(const cubed_search_task_t* d_tasks, int64_t ntasks, int32_t ktype,
                        int32_t flags, int32_t path, int64_t work, void* stream);

/* Histogram of a chunk (histogram; new symbols only, the ABI version is
 * unchanged).  A task counts a flat run of n_values values v into the nbins
 * bins of nbins + 1 non-decreasing edges e, numpy's definition: bin i holds
 * e[i] <= v < e[i+1], the last bin also v == e[nbins]; NaN and values outside
 * [e[0], e[nbins]] are counted nowhere, -0.0 == 0.0, and a zero-width bin gets
 * nothing unless it is the last.  Only comparisons with the edges decide a
 * bin.  dst is the task's own row of nbins int64 counts; the entry zeroes every
 * row on the stream before it counts.  Values and edges have the same type
 * (ktype: CUBED_F32 or CUBED_F64).  A workgroup counts its share of a task,
 * ceil(n_values / work) rounded up to 1024 values, in 32-bit LDS counters (or
 * not at all: CUBED_HIST_WIDE) and adds them to dst with 64-bit integer
 * atomics, so the share must stay below 2^32; integer sums do not depend on
 * their order and results are bit-identical run to run. */
#define CUBED_HIST_BINS_LDS 4096 /* most bins whose edges and counters one workgroup keeps in
                                    LDS: 48 KiB at 8-byte edges, three workgroups per CU */
#define CUBED_HIST_VALUES 16384  /* least values of a workgroup's share the host plans with */
#define CUBED_HIST_UNIFORM 0     /* paths: nbins <= BINS_LDS, evenly spaced edges: a guessed
                                    bin corrected against the edges in LDS */
#define CUBED_HIST_SEARCH 1      /* nbins <= BINS_LDS: binary search of the edges in LDS */
#define CUBED_HIST_WIDE 2        /* any nbins: binary search of the edges in global memory, one
                                    64-bit atomic per run of equal bins of a wave */

typedef struct {
  int64_t x_base, edges_base, dst_base; /* device byte addresses */
  int64_t n_values;                     /* elements of x */
} cubed_hist_task_t;

/* Host only: CUBED_HIST_BINS_LDS of the loaded library. */
int64_t cubed_hist_bins_lds(void);
/* Host only (no device call): validates a HOST copy of a histogram task table
 * and returns the path of its launch: CUBED_HIST_WIDE when nbins >
 * CUBED_HIST_BINS_LDS, else CUBED_HIST_UNIFORM if uniform (the edges are evenly
 * spaced) and CUBED_HIST_SEARCH if not; a negative CUBED_E_* code for a
 * malformed table. */
int cubed_hist_path(const cubed_hist_task_t* tasks, int64_t ntasks, int32_t ktype, int64_t nbins,
                    int32_t uniform);
/* One zeroing launch and one counting launch over a DEVICE task table, grid
 * ntasks x work workgroups.  CUBED_HIST_WIDE and CUBED_HIST_SEARCH are correct
 * for every set of edges (the latter for nbins <= CUBED_HIST_BINS_LDS),
 * CUBED_HIST_UNIFORM is as well but slow for edges far from evenly spaced.
 * Neither synchronises nor allocates. */
int cubed_hist_chunks(const cubed_hist_task_t* d_tasks, int64_t ntasks, int32_t ktype, int64_t nbins,
                      int32_t path, int64_t work, void* stream);

/* Run heads of a sorted chunk (the unique_* set functions; new symbols only,
 * the ABI version is unchanged).  A task has a sorted 1-d run of n keys of the
 * type ktype (one of the six sort key types), in the order of the sort:
 * ascending, every NaN last and all NaNs tied, -0.0 tied with 0.0.  Element j
 * is a head if it is the first element of the whole sorted array (j == 0 and
 * prev_base == 0), else iff its predecessor sorts strictly before it; the
 * predecessor of element 0 is element n_prev - 1 of the run at prev_base, the
 * chunk before this one.
 *   CUBED_UNIQUE_COUNT: dst_base gets the int64 number of heads.
 *   CUBED_UNIQUE_PACK: dst_base, a run of n keys, gets the heads in order at
 *     its front and zeros behind them.  With a payload dst_idx_base, a run of n
 *     int64, gets next to every head offset + j (CUBED_UNIQUE_POSITION, its
 *     global position in the sorted array) or element j of the int64 run at
 *     src_idx_base (CUBED_UNIQUE_INDEX, the index field of a pairs chunk), and
 *     zeros behind them.  The destination is never the source.
 * scratch_base is the task's own ceil(n / CUBED_UNIQUE_TILE) + 1 int64.  No
 * workgroup waits for another one and there are no atomics: results are
 * bit-identical run to run. */
#define CUBED_UNIQUE_TILE 4096   /* elements of one workgroup */
#define CUBED_UNIQUE_COUNT 0     /* kinds */
#define CUBED_UNIQUE_PACK 1
#define CUBED_UNIQUE_KEYS 0      /* payloads: none, the packed elements are plain keys */
#define CUBED_UNIQUE_POSITION 1
#define CUBED_UNIQUE_INDEX 2

typedef struct {
  int64_t src_base, src_idx_base; /* device byte addresses; src_idx_base 0: plain keys */
  int64_t prev_base;              /* the chunk before this one; 0: block 0 */
  int64_t dst_base, dst_idx_base; /* dst_idx_base 0: no payload */
  int64_t scratch_base;
  int64_t n, n_prev;              /* elements of this chunk and of the one before */
  int64_t offset;                 /* global position of element 0 in the sorted array */
} cubed_unique_task_t;

/* Host only: CUBED_UNIQUE_TILE of the loaded library. */
int64_t cubed_unique_tile(void);
/* Host only (no device call): validates a HOST copy of a task table and
 * returns the workgroups per task of its launch, ceil(max n / tile); a
 * negative CUBED_E_* code for a malformed table. */
int64_t cubed_unique_work(const cubed_unique_task_t* tasks, int64_t ntasks, int32_t ktype, int32_t kind,
                          int32_t payload);
/* Over a DEVICE task table: one launch that counts the heads of every tile
 * (ntasks x work workgroups), one that scans the tile counts of every task
 * (ntasks workgroups) and, for CUBED_UNIQUE_PACK, one that packs (ntasks x
 * work).  Neither synchronises nor allocates. */
int cubed_unique_chunks(const cubed_unique_task_t* d_tasks, int64_t ntasks, int32_t ktype, int32_t kind,
                        int32_t payload, int64_t work, void* stream);

/* Selection by a one-element predicate (nonzero, x[mask]; new symbols only,
 * the ABI version is unchanged).  A task has a 1-d run of n elements of esize
 * bytes (1, 2, 4 or 8) at src_base.  Element j is selected iff
 * (bits & m) != 0, where m is all ones, or with ignore_sign all ones but the
 * top bit of the element: -0.0 is not selected, NaNs, infinities, denormals
 * and the most negative integer are.
 *   CUBED_SELECT_COUNT: dst_base gets the int64 number of selected elements;
 *     vsize and every val_base are 0.
 *   CUBED_SELECT_PACK, vsize 0: dst_base, a run of n int64, gets offset + j of
 *     every selected element in order at its front and zeros behind them;
 *     every val_base is 0.
 *   CUBED_SELECT_PACK, vsize 1, 2, 4 or 8: dst_base, a run of n elements of
 *     vsize bytes, gets element j of the run at val_base for every selected j
 *     in order at its front and zeros behind them.
 * src_base is a multiple of 16 and the storage behind the run extends to the
 * next multiple of 16 bytes: the kernels load whole 16-byte vectors, never one
 * that starts at or past element n, and mask off the elements at or past n.
 * The destination is never the source or the values.  scratch_base is the
 * task's own ceil(n * esize / tile bytes) + 1 int64.  No workgroup waits for
 * another one and there are no atomics: results are bit-identical run to
 * run. */
#define CUBED_SELECT_TILE_BYTES 16384 /* bytes of src one workgroup owns */
#define CUBED_SELECT_COUNT 0          /* kinds */
#define CUBED_SELECT_PACK 1

typedef struct {
  int64_t src_base;      /* the run the predicate reads: n elements of esize bytes */
  int64_t val_base;      /* 0: pack positions; else n elements of vsize bytes to pack */
  int64_t dst_base, scratch_base;
  int64_t n, offset;     /* offset: global flat position of element 0 */
} cubed_select_task_t;

/* Host only: CUBED_SELECT_TILE_BYTES of the loaded library. */
int64_t cubed_select_tile_bytes(void);
/* Host only (no device call): validates a HOST copy of a task table and
 * returns the workgroups per task of its launch, ceil(max n * esize / tile
 * bytes); a negative CUBED_E_* code for a malformed table. */
int64_t cubed_select_work(const cubed_select_task_t* tasks, int64_t ntasks, int32_t esize,
                          int32_t ignore_sign, int32_t kind, int32_t vsize);
/* Over a DEVICE task table: one launch that counts the selected elements of
 * every tile (ntasks x work workgroups), one that scans the tile counts of
 * every task (ntasks workgroups) and, for CUBED_SELECT_PACK, one that packs
 * (ntasks x work).  Neither synchronises nor allocates. */
int cubed_select_chunks(const cubed_select_task_t* d_tasks, int64_t ntasks, int32_t esize,
                        int32_t ignore_sign, int32_t kind, int32_t vsize, int64_t work, void* stream);

/* Gathering along one axis (take_along_axis; new symbols only, the ABI version
 * is unchanged).  A task has an int64 index chunk seen as (outer, n_idx, inner),
 * a source chunk (outer, n_src, inner) of elements of esize bytes (1, 2, 4 or
 * 8) that holds the places [lo, lo + n_src) of an axis of n_total places, a
 * destination chunk and, if prev_base is not 0, an earlier result, both of the
 * index chunk's extent and of esize bytes.  All four are compact and C-ordered.
 * For every (o, j, k), with i = idx[o][j][k], plus n_total if i < 0:
 *   dst[o][j][k] = src[o][i - lo][k]                 if lo <= i < lo + n_src
 *                = prev_base ? prev[o][j][k] : 0     otherwise.
 * That guard is on every read of src, so no index, however far out of range,
 * reaches memory outside the source chunk.  Elements move as bits.  The
 * destination is never one of the inputs.  No workgroup waits for, signals or
 * reads the output of another one and there are no atomics: results are
 * bit-identical run to run. */
#define CUBED_GATHER_TILE_BYTES 32768 /* most bytes of a source row the LDS form stages */
#define CUBED_GATHER_ELEMS 4096       /* outputs of one workgroup, direct form */
#define CUBED_GATHER_LDS_ELEMS 16384  /* most outputs of one workgroup, LDS form (one row) */
#define CUBED_GATHER_DIRECT 0         /* paths: every read of src goes to global memory */
#define CUBED_GATHER_LDS 1            /* inner == 1: the source row is staged in LDS */

typedef struct {
  int64_t src_base, idx_base, dst_base;  /* device byte addresses */
  int64_t prev_base;                     /* 0 = none */
  int64_t outer, n_idx, n_src, inner;    /* elements */
  int64_t lo, n_total;                   /* the source chunk's start on the axis; the axis */
} cubed_gather_task_t;

/* Host only: CUBED_GATHER_TILE_BYTES of the loaded library. */
int64_t cubed_gather_tile_bytes(void);
/* Host only (no device call): validates a HOST copy of a gather task table and
 * returns the path of its launch: CUBED_GATHER_LDS when every task that writes
 * anything has inner == 1, n_src * esize <= CUBED_GATHER_TILE_BYTES and
 * n_idx >= n_src, else CUBED_GATHER_DIRECT; a negative CUBED_E_* code for a
 * malformed table. */
int cubed_gather_path(const cubed_gather_task_t* tasks, int64_t ntasks, int32_t esize);
/* One launch over a DEVICE task table.  work = the most workgroups any task
 * needs: ceil(outer * n_idx * inner / CUBED_GATHER_ELEMS) in the direct form,
 * outer * ceil(n_idx / CUBED_GATHER_LDS_ELEMS) in the LDS form.
 * CUBED_GATHER_DIRECT is correct for every table, CUBED_GATHER_LDS only for
 * the tables cubed_gather_path gives it to; both write the same bytes there.
 * Neither synchronises nor allocates. */
int cubed_gather_chunks(const cubed_gather_task_t* d_tasks, int64_t ntasks, int32_t esize, int32_t path,
                        int64_t work, void* stream);

/* Chained chunk GEMMs (blockwise matmul / tensordot with the k-sum fused):
 * task t computes C_t (=|+=) sum over its segments s of A_s @ B_s, row-major
 * views, every A_s m x k_s, every B_s k_s x n, accumulated in one continuous
 * K loop (f32 for f32/bf16 inputs, f64 / wrapping int64 otherwise) and
 * rounded to out_dtype once.  Replaces, per OUTPUT chunk, the (i, k, j)
 * tasks of _matmul (cubed/array_api/linear_algebra_functions.py:35-52,62-64:
 * one numpy BLAS call per chunk pair) together with the _sum_wo_cat
 * reduction over k (:52,67-78) that reads their partial products back; a
 * per-chunk product is a chain of one segment.  Host copies of both tables
 * (tasks, segs) are validated and pick the kernel; the device copies are
 * what the kernels read.  d_zero: >= 64 zero bytes of device memory (the
 * bf16 path reads k past the chain's end from it).  path: CUBED_GEMM_AUTO,
 * or CUBED_GEMM_ANY to force the element-wise kernel (tests). */
typedef struct {
  int64_t c;            /* output chunk base (device byte address)           */
  int64_t m, n, ldc;    /* output extents and row pitch (elements)           */
  int64_t seg0, nseg;   /* segments [seg0, seg0 + nseg) of the segment table  */
  int64_t ktot;         /* sum of the segments' k                            */
  int64_t accumulate;   /* 1: C += ..., 0: C = ...                           */
} cubed_gemm_chain_t;

typedef struct {
  int64_t a, b;         /* device byte addresses of A_s (m x k) and B_s (k x n) */
  int64_t k;            /* contracted extent of this pair                      */
  int64_t lda, ldb;     /* row pitches in elements                             */
  int64_t pad;
} cubed_gemm_seg_t;

#define CUBED_GEMM_AUTO (-1)
#define CUBED_GEMM_ANY 0   /* element-wise tiles, any dtype and shape          */
#define CUBED_GEMM_MFMA 1  /* bf16 (16x16x32) / f32 (32x32x2) MFMA tiles       */

/* Kernel the chain set would run on (CUBED_GEMM_MFMA or CUBED_GEMM_ANY). */
int cubed_gemm_chain_path(const cubed_gemm_chain_t* tasks, int64_t ntasks,
                          const cubed_gemm_seg_t* segs, int32_t in_dtype, int32_t out_dtype);
int cubed_gemm_chain(const cubed_gemm_chain_t* tasks, const cubed_gemm_chain_t* d_tasks,
                     int64_t ntasks, const cubed_gemm_seg_t* segs, const cubed_gemm_seg_t* d_segs,
                     int64_t nsegs, int32_t in_dtype, int32_t out_dtype, const void* d_zero,
                     int32_t path, void* stream);

/* Grid tiling (f32 / bf16 MFMA): the ti x tj tasks are the C-order chunk grid
 * of ONE (M, N) output (task I*tj + J = chunk (I, J); chunks cm x cn with cm,
 * cn >= 256 and cn % 4 (f32) / 8 (bf16) == 0 except the last row / column; every task the
 * same k segmentation).  256 x 256 tiles then cover the whole matrix --
 * a tile straddling chunk boundaries reads each row / column from its own
 * chunk -- instead of padding every chunk to whole tiles.  Same results
 * contract as cubed_gemm_chain (each element one f32 accumulation chain over
 * K in the same order).  cubed_gemm_grid_check (host only): 0 when the
 * tables fit, CUBED_E_LAYOUT (message set) otherwise. */
int cubed_gemm_grid_check(const cubed_gemm_chain_t* tasks, int64_t ti, int64_t tj,
                          const cubed_gemm_seg_t* segs, int64_t nsegs, int32_t in_dtype, int32_t out_dtype);
int cubed_gemm_chain_grid(const cubed_gemm_chain_t* tasks, const cubed_gemm_chain_t* d_tasks, int64_t ti,
                          int64_t tj, const cubed_gemm_seg_t* segs, const cubed_gemm_seg_t* d_segs,
                          int64_t nsegs, int32_t in_dtype, int32_t out_dtype, const void* d_zero,
                          void* stream);

/* Packed operands (bf16 in, f32 / bf16 out; f32 in, f32 out): the same chain
 * set as cubed_gemm_chain_grid, additionally ONE chunked product (segment s of
 * every task in chunk row I reads the same A chunk, in chunk column J the same
 * B chunk).  Both operands are first rewritten into the workspace as blocks
 * that are the GEMM's LDS image (bf16: 32 KiB per 256-row A panel / 256-column
 * B^T panel and 64-k tile; f32: 16 KiB per 256-row A panel / 256-column B
 * panel and 16-k step; K segments concatenated, pads zero), then one launch
 * tiles the whole output.  Same results contract as cubed_gemm_chain
 * (bit-identical to its MFMA paths).
 * cubed_gemm_pack_bytes (host only): workspace bytes the set needs, or a
 * negative CUBED_E_* with the message set when it does not pack.
 * cubed_gemm_chain_packed: d_ws 256-B aligned, ws_bytes >= that size
 * (else CUBED_E_WORKSPACE); stream-ordered, the workspace is free again once
 * the launches have run. */
int64_t cubed_gemm_pack_bytes(const cubed_gemm_chain_t* tasks, int64_t ti, int64_t tj,
                              const cubed_gemm_seg_t* segs, int64_t nsegs, int32_t in_dtype, int32_t out_dtype);
int cubed_gemm_chain_packed(const cubed_gemm_chain_t* tasks, const cubed_gemm_chain_t* d_tasks, int64_t ti,
                            int64_t tj, const cubed_gemm_seg_t* segs, const cubed_gemm_seg_t* d_segs,
                            int64_t nsegs, int32_t in_dtype, int32_t out_dtype, void* d_ws, int64_t ws_bytes,
                            void* stream);

/* Multi-GPU matmul on packed operands (ABI 15).  Replaces, on W ranks, the
 * same _matmul chunk products + _sum_wo_cat k-sum
 * (cubed/array_api/linear_algebra_functions.py:35-78) when the block-cyclic
 * ownership gives every k chunk of A one rank and every chunk column of C
 * (and of B) one rank.  A is packed into ONE k-major image of the whole A
 * (block (mt, kt) at (kt * TM + mt) * block bytes; bf16: 32 KiB blocks of 256
 * rows x 64 k, f32: 16 KiB of 256 rows x 16 k, the single-GPU packed blocks),
 * so the k blocks a rank packs are one contiguous byte run it sends whole to
 * every peer; the block straddling two k chunks is packed by the owner of
 * the first one from a received halo of the next chunk's first columns.
 * Every element stays the single-GPU packed path's f32 chain over K.
 * cubed_gemm_dist_image_bytes (host only): the image's size.
 * cubed_gemm_dist_pack_a: a_tasks = one task per A chunk row (m rows,
 *   segments = its k chunks: a = the chunk, a halo buffer (lda = its width)
 *   or 0 where the rank has neither); packs k blocks [kt0, kt1), which must
 *   read only present segments (else CUBED_E_LAYOUT, nothing launched).
 * cubed_gemm_dist_b_bytes / cubed_gemm_dist_pack_b: B (B^T for bf16) of the
 *   rank's own C chunk grid (ti x tj tasks, as cubed_gemm_chain_packed; the
 *   A addresses are not read) packed into d_ws.
 * cubed_gemm_dist_gemm: the rank's C chunks from the filled image and d_ws. */
int64_t cubed_gemm_dist_image_bytes(int64_t M, int64_t K, int32_t in_dtype);
int cubed_gemm_dist_pack_a(const cubed_gemm_chain_t* a_tasks, const cubed_gemm_chain_t* d_a_tasks, int64_t ti,
                           const cubed_gemm_seg_t* a_segs, const cubed_gemm_seg_t* d_a_segs, int64_t nsegs,
                           int32_t in_dtype, int64_t kt0, int64_t kt1, void* d_image, int64_t image_bytes,
                           void* stream);
int64_t cubed_gemm_dist_b_bytes(const cubed_gemm_chain_t* tasks, int64_t ti, int64_t tj,
                                const cubed_gemm_seg_t* segs, int64_t nsegs, int32_t in_dtype, int32_t out_dtype);
int cubed_gemm_dist_pack_b(const cubed_gemm_chain_t* tasks, const cubed_gemm_chain_t* d_tasks, int64_t ti,
                           int64_t tj, const cubed_gemm_seg_t* segs, const cubed_gemm_seg_t* d_segs, int64_t nsegs,
                           int32_t in_dtype, int32_t out_dtype, void* d_ws, int64_t ws_bytes, void* stream);
int cubed_gemm_dist_gemm(const cubed_gemm_chain_t* tasks, const cubed_gemm_chain_t* d_tasks, int64_t ti, int64_t tj,
                         const cubed_gemm_seg_t* segs, int64_t nsegs, int32_t in_dtype, int32_t out_dtype,
                         const void* d_image, int64_t image_bytes, const void* d_ws, int64_t ws_bytes,
                         void* stream);

/* ---- Zarr v2 chunk codecs (host only; cubed_amd/csrc/codec.cpp) --------
 * Replace numcodecs.Blosc's decode/encode behind zarr's chunk reads and
 * writes (storage/zarr.py:8-103 LazyZarrArray.create/open; the chunk I/O of
 * core/ops.py:88-182 from_zarr / store / to_zarr).  Reentrant, no GPU calls.
 * cubed_blosc_decompress: dst must hold exactly the frame's nbytes.
 * cubed_blosc_compress: lz4 + byte shuffle (shuffle != 0), unsplit blocks;
 * dst must hold cubed_blosc_max_compressed(nbytes); returns the frame size
 * or a negative error. */
int cubed_blosc_header(const void* src, int64_t srclen, int64_t* nbytes, int64_t* cbytes,
                       int* typesize, int* flags);
int cubed_blosc_decompress(const void* src, int64_t srclen, void* dst, int64_t dstlen);
int64_t cubed_blosc_max_compressed(int64_t nbytes);
/* Standalone numcodecs chunk codecs (zarr compressor ids "zstd" and "lz4"):
 * one zstd frame (decoded by the system libzstd, loaded on first use;
 * CUBED_E_UNSUPPORTED when it is absent) / a little-endian int32 size + one
 * LZ4 block.  dst must hold exactly the decoded size. */
int cubed_zstd_decompress(const void* src, int64_t srclen, void* dst, int64_t dstlen);
int cubed_lz4_chunk_decompress(const void* src, int64_t srclen, void* dst, int64_t dstlen);
int64_t cubed_blosc_compress(const void* src, int64_t nbytes, int typesize, int shuffle, void* dst,
                             int64_t dstcap);

/* library info */
int cubed_abi_version(void);
const char* cubed_last_error(void);
int cubed_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* CUBED_AMD_H */
