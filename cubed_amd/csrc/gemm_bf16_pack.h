// gemm_bf16_pack.h -- PackPlan (the geometry of a packed chain set, bf16 and
// f32) and the bf16 pack kernels (round 5; included by gemm_chain.hip before
// gemm_bf16_8p.h and gemm_f32_w4p.h; launched by cubed_gemm_chain_packed and
// cubed_gemm_dist_pack_a / _b).
//
// The one-wave kernel of gemm_bf16_w4l.h stages A from the chunks as stored:
// every 64-k tile is 256 scattered 128-B row lines, and B is read with
// ds_read_b64_tr_b16.  tools/mfma_gap_probe.hip (profiles/r05_mfma_flow.log)
// holds 2.0 GHz with 16 ds_read_b128 per step against 1.72 GHz for w4l's
// read mix, and w4l's stamped main loop put ~5 cycles per MFMA into fills that
// miss L2.
// Here both operands are first rewritten, in one HBM pass each, into the LDS
// image itself: per 256-row panel of A (256-column panel of B^T) and 64-deep k
// tile one 32 KiB block, row r at r * 128 and 16-B slot s holding k chunk
// s ^ ((r >> 1) & 7) (the w4l A swizzle), the chain's K segments concatenated,
// every pad (rows past M, columns past N, k past K) zero.  The GEMM then
// stages each piece as 1 KiB of consecutive bytes from one uniform base, reads
// A and B fragments alike with ds_read_b128, and its K loop has no segment or
// edge logic -- which also makes 256 x 256 tiles over the WHOLE output (157^2
// instead of 8^2 x 20^2 padded per chunk on config 5) free: chunk boundaries
// matter only in the epilogue.
//
// Config 5 (profiles/r05_gemm_bf16_w4p.log): the first GEMM on this image
// (k_gemm_bf16_w4p, one wave per SIMD; replaced by k_gemm_bf16_8p in round 6)
// 1330 TF vs 1214 for w4l on one box, bit-identical; pack A 1.37 ms + B^T
// 1.26 ms (~5 TB/s each, 3.3 GB written per operand).  Pack variants measured
// and dropped (non-temporal loads / stores, grids of 4096 / 65536 blocks): all
// ~5 TB/s (profiles/r06_pack_variants.log).
//
// Same results contract as k_gemm_bf16_w4l: every element one f32 chain over K
// in k order (zero pads add exact zeros; the K loop stops at ceil(K / 32)
// steps like w4l's).
#pragma once

// geometry of one packed chain set (host-validated, see cubed_gemm_pack_bytes)
struct PackPlan {
  int64_t ti, tj, cm, cn, M, N, K;
  int64_t TM, TN, KTL;  // 256-row / 256-column panels over M / N, k blocks over K
  int64_t pstride;      // bytes from one panel's first block to the next panel's (B / B^T)
  // the A image: block (mt, kt) at mt * apstride + kt * akstride (one GPU:
  // panel-major, apstride = pstride; the multi-GPU image is k-major so every
  // k chunk's tile range is one contiguous run, cubed_gemm_dist_*)
  int64_t apstride, akstride;
  int64_t kt0, kt1;     // k blocks [kt0, kt1) the A pack writes
};

// segment containing k (start ks), walking from (s, ks): every task has the
// same k segmentation (cubed_gemm_grid_check), read from task 0's list
__device__ __forceinline__ void seg_at(const cubed_gemm_seg_t* __restrict__ sg, int64_t k, int64_t& s, int64_t& ks) {
  int64_t ke = ks + sg[s].k;
  while (k >= ke) {
    ks = ke;
    ++s;
    ke += sg[s].k;
  }
}

// A -> PA: block (mt, kt) = rows 256 mt .. +255 of the whole A, k 64 kt .. +63
__global__ __launch_bounds__(256) void k_pack_a(const cubed_gemm_chain_t* __restrict__ tasks,
                                                const cubed_gemm_seg_t* __restrict__ segs, PackPlan pp,
                                                char* __restrict__ PA) {
  const int64_t nkt = pp.kt1 - pp.kt0, nblk = pp.TM * nkt;
  const cubed_gemm_seg_t* __restrict__ sg0 = segs + tasks[0].seg0;
  const int sl = threadIdx.x & 7;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t mt = blk / nkt, kt = pp.kt0 + (blk - mt * nkt);
    // the panel's first chunk row (rows of a panel lie in at most two: cm >= 256)
    const int64_t I0 = (mt * 256) / pp.cm, mb = (I0 + 1) * pp.cm;
    int64_t s0 = 0, ks0 = 0;
    if (kt * 64 < pp.K) seg_at(sg0, kt * 64, s0, ks0);
    char* dst = PA + mt * pp.apstride + kt * pp.akstride;
#pragma unroll 2
    for (int j = 0; j < 8; ++j) {
      const int r = (threadIdx.x >> 3) + 32 * j, c = sl ^ ((r >> 1) & 7);
      const int64_t gm = mt * 256 + r, k = kt * 64 + c * 8;
      uint4 v = {0, 0, 0, 0};
      if (gm < pp.M && k < pp.K) {
        int64_t s = s0, ks = ks0;
        seg_at(sg0, k, s, ks);
        const bool hi = gm >= mb;
        const int64_t I = hi ? I0 + 1 : I0, lm = gm - I * pp.cm;
        const cubed_gemm_seg_t& S = segs[tasks[I * pp.tj].seg0 + s];
        v = *(const uint4*)((const char*)(uintptr_t)S.a + (lm * S.lda + (k - ks)) * 2);
      }
      *(uint4*)(dst + r * 128 + sl * 16) = v;
    }
  }
}

// B -> PB as B^T: block (nt, kt) = columns 256 nt .. +255 as rows.  Thread t
// takes k chunk c = t & 7 and columns 8 (t >> 3) .. +7: eight 16-B row reads,
// an 8 x 8 transpose in registers, eight 16-B writes (8 consecutive threads
// fill one 128-B row of the block).  cn % 8 == 0: a column group never
// straddles chunk columns; k_s % 8 == 0: a k chunk never straddles segments.
__global__ __launch_bounds__(256) void k_pack_bt(const cubed_gemm_chain_t* __restrict__ tasks,
                                                 const cubed_gemm_seg_t* __restrict__ segs, PackPlan pp,
                                                 char* __restrict__ PB) {
  const int64_t nblk = pp.TN * pp.KTL;
  const cubed_gemm_seg_t* __restrict__ sg0 = segs + tasks[0].seg0;
  const int c = threadIdx.x & 7, n8 = threadIdx.x >> 3;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t nt = blk / pp.KTL, kt = blk - nt * pp.KTL;
    const int64_t J0 = (nt * 256) / pp.cn, nb = (J0 + 1) * pp.cn;
    const int64_t gn = nt * 256 + n8 * 8, k0 = kt * 64 + c * 8;
    uint4 in[8];
    if (gn < pp.N && k0 < pp.K) {
      int64_t s = 0, ks = 0;
      seg_at(sg0, k0, s, ks);
      const bool hi = gn >= nb;
      const int64_t J = hi ? J0 + 1 : J0, ln = gn - J * pp.cn;
      const cubed_gemm_seg_t& S = segs[tasks[J].seg0 + s];
      const char* src = (const char*)(uintptr_t)S.b + ((k0 - ks) * S.ldb + ln) * 2;
#pragma unroll
      for (int e = 0; e < 8; ++e) in[e] = k0 + e < pp.K ? *(const uint4*)(src + e * S.ldb * 2) : uint4{0, 0, 0, 0};
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) in[e] = uint4{0, 0, 0, 0};
    }
    char* dst = PB + nt * pp.pstride + kt * 32768;
    const uint16_t(*w)[8] = (const uint16_t(*)[8])in;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = n8 * 8 + j, sl = c ^ ((r >> 1) & 7);
      uint16_t o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = w[e][j];
      *(uint4*)(dst + r * 128 + sl * 16) = *(const uint4*)o;
    }
  }
}
