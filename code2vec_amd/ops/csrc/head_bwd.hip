// Fused output-head + loss backward (recompute-G): dW, dbias, dcv straight
// from (logits, lse) — the [B, L] softmax gradient ("dlogits") is NEVER
// materialized.  Replaces the unfused chain lsm_nll_bwd (61 MB write) +
// colsum (61 MB read) + rocBLAS dW GEMM (61 MB read) + head_dgrad (61 MB
// read) with two kernels that each read logits once and recompute
//   G[b,l] = coef_b * (exp(logit[b,l] - lse_b) - [l == y_b]),
//   coef_b = gscale * weight[y_b] / sum_b weight[y_b]
// in registers (reference math: main.py:251-264 chained through
// model/model.py:83; G is the gradient of the weighted-NLL log-softmax
// composed with the linear head).
//
// A tiny prep kernel packs per-row (coef_b, lse_b, y_b) into one f32x4 so
// the G recompute costs ONE 16-B load per staged logits chunk instead of
// three scattered scalar loads (label i64 + weight gather + lse) per
// thread per stage.  y is carried as a float: exact for L < 2^24.
//
// Kernel 1 (label-major): dW[L, EP] = G^T @ cv and dbias[L] = colsum(G).
//   Block = 64 labels x EP(=128), K-loop over ALL batch rows in 64-row
//   stages.  G tiles are computed at stage time from coalesced logits row
//   chunks and written TRANSPOSED into LDS MFMA A-fragment images (the
//   wgrad.hip padded-image recipe — G^T fragment k-runs walk the batch
//   dim, which is logits' slow axis).  cv is pre-transposed once
//   ([EP, B], 256 KB — L2-resident) so B-fragment k-runs are contiguous
//   global loads.  All staging values live in named vector registers —
//   NO lambdas, NO address-taken arrays (hipcc demotes those to scratch
//   inside K-loops; PERF.md pathology #0 — the first version of this
//   kernel measured 81 us instead of ~25 for exactly that reason).
//   dbias falls out of the same pass: each thread keeps 8 label-column
//   partial sums of its staged G values, LDS-reduced at the end; every
//   label belongs to exactly ONE block, so the store is a plain f32 write.
//
// Kernel 2 (batch-major): dcv[B, EP] = G @ W — head_dgrad.hip's proven
//   split-K structure with the A fragment recomputed from contiguous
//   logits row chunks instead of read from dlogits.  The label chunk per
//   block is a runtime parameter: 1024 up to L = 131072 (71 slabs at
//   top11), 4096 above (java-large) so the fp32 partial-slab traffic stays
//   ~33 MB instead of 268 MB.

#include <cstdlib>

#include "common.h"

#define HB_LB 64    // labels per dW block
#define HB_ROWS 64  // batch rows staged per K-iteration
#define HB_NSTR (64 * 8 + 8)  // padded A-image stride (wgrad recipe)
#define HB_DW_DEPTH 2   // shipped sub-stages per stage of head_bwd_dw_pipe
#define HB_DCV_DBUF 1   // W-image buffering of head_bwd_dcv_pipe_kernel

// coef_lse[b] = (coef_b, lse_b, (float)y_b, 0)
__global__ __launch_bounds__(256) void head_bwd_prep_kernel(
    const long* __restrict__ label, const float* __restrict__ weight,
    const float* __restrict__ acc_ws, const float* __restrict__ gscale,
    const float* __restrict__ lse, float* __restrict__ coef_lse, long B) {
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const long y = label[b];
  const float coef = gscale[0] * (weight ? weight[y] : 1.f) / acc_ws[1];
  f32x4 v = {coef, lse[b], (float)y, 0.f};
  *(f32x4*)(coef_lse + 4 * b) = v;
}

// variant: phase-isolation bitmask (C2V_HBDW_VARIANT, perf diagnosis):
//   1 = skip dW/dbias global stores, 2 = skip cv (B-operand) staging loads,
//   4 = skip logits staging loads, 8 = replace expf with identity,
//   16 = replace the MFMA chain with a cheap accumulate
//
// The B operand (cv) is PRE-SWIZZLED ONCE into MFMA fragment-image
// layout in global memory (swizzle_cv_kernel, 256 KB at B=1024): each
// B-fragment read is then a fully contiguous 1-KB wave read that streams
// from L2.  Two rejected designs, both variant-isolated on hardware:
// (a) per-lane loads from a pre-transposed cvT — 16 lanes hit
// 2-KB-strided addresses, camping on a few memory channels (~37 of
// 69 us); (b) staging cv rows through LDS fragment images per stage —
// 16 extra ds_write_b16 per thread per stage on the CU-shared LDS pipe
// (~33 us of skeleton).
// MINW: forced min waves/SIMD (C2V_HBDW_OCC env A/B; 512-thread blocks
// make 6 the next level above the default 4 — costs 136 B/lane scratch)
template <int MINW = 1>
__global__ __launch_bounds__(512, MINW) void head_bwd_dw_kernel(
    const bf16* __restrict__ logits, const bf16* __restrict__ cvimg,
    const float* __restrict__ coef_lse, bf16* __restrict__ dw,
    float* __restrict__ dbias, long B, long L, int variant) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const long l0 = (long)blockIdx.x * HB_LB;
  // staging role A (logits->G): one bf16x8 chunk per thread per stage
  const int krow = threadIdx.x >> 3;        // 0..63: batch row within stage
  const int col8 = (threadIdx.x & 7) * 8;   // 0..56: label chunk start

  // A-fragment images (double-buffered) reused as the dbias reduction
  // scratch after the K-loop (lives separated by barriers)
  __shared__ union {
    bf16 img[2][2][4][HB_NSTR];  // [buf][ksub][label tile][image]
    float red[HB_ROWS][HB_LB + 1];
  } sm;
  __shared__ float red2[8][HB_LB + 1];

  const int n = col8 >> 4;          // this thread's label tile
  const int base_l = col8 & 15;     // label offset within the tile
  const int ksub = krow >> 5;       // which 32-k MFMA step of the stage
  const int kgrp = (krow >> 3) & 3; // 16-lane fragment group
  const int jslot = krow & 7;
  const long lc = l0 + col8;
  const bool lok = lc < L;          // L % 8 == 0: chunk fully in bounds

  f32x4 db0 = {0.f, 0.f, 0.f, 0.f};
  f32x4 db1 = {0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero8 = {};

  // named staging registers (macro-expanded; no address-taken arrays)
  bf16x8 lv;          // staged logits chunk
  f32x4 meta;         // (coef, lse, yf, -)
  bool rok;

#define DW_LOAD(mb)                                                        \
  do {                                                                     \
    const long row_ = (mb) + krow;                                         \
    rok = row_ < B && lok && !(variant & 4);                               \
    if (rok) {                                                             \
      meta = *(const f32x4*)(coef_lse + 4 * row_);                         \
      lv = *(const bf16x8*)(logits + row_ * L + lc);                       \
    }                                                                      \
  } while (0)

#define DW_WRITE(buf)                                                      \
  do {                                                                     \
    bf16x8 gv = zero8;                                                     \
    if (rok) {                                                             \
      const float coef_ = meta[0];                                         \
      const float lse_ = meta[1];                                          \
      const long y_ = (long)meta[2];                                       \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) {                      \
        const float x_ = bf2f(lv[j]) - lse_;                               \
        float g_ = coef_ * ((variant & 8) ? x_ : __expf(x_));              \
        if (lc + j == y_) g_ -= coef_;                                     \
        const bf16 gb_ = f2bf(g_);                                         \
        gv[j] = gb_;                                                       \
        if (j < 4) db0[j & 3] += bf2f(gb_);                                \
        else db1[j & 3] += bf2f(gb_);                                      \
      }                                                                    \
    }                                                                      \
    bf16* dst_ = sm.img[buf][ksub][n];                                     \
    _Pragma("unroll") for (int j = 0; j < 8; ++j)                          \
        dst_[(base_l + j + kgrp * 16) * 8 + jslot] = gv[j];                \
  } while (0)

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc1 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc3 = {0.f, 0.f, 0.f, 0.f};

  const int lt = wave >> 1;          // this wave's label tile
  const int nh = (wave & 1) * 64;    // this wave's EP half
  const int ng = (wave & 1) * 4;     // first B-image tile of this wave
  // cvimg layout: [k-chunk][8 nt][64 lanes][8] — per-fragment reads are
  // contiguous 1-KB wave reads
  const bf16* cbase = cvimg + (long)lane * 8;

  DW_LOAD(0);
  DW_WRITE(0);
  __syncthreads();
  int buf = 0;
  for (long mb = 0; mb < B; mb += HB_ROWS) {
    const bool more = mb + HB_ROWS < B;
    if (more) DW_LOAD(mb + HB_ROWS);
    // B fragments stream from the global cv image (contiguous per wave);
    // A fragments from the LDS G image
    const bool bl = !(variant & 2);
    const long kc0 = (mb >> 5) * 8 * 512;       // this stage's first chunk
    const bf16x8 b00 = bl ? *(const bf16x8*)(cbase + kc0 + (ng + 0) * 512) : zero8;
    const bf16x8 b01 = bl ? *(const bf16x8*)(cbase + kc0 + (ng + 1) * 512) : zero8;
    const bf16x8 b02 = bl ? *(const bf16x8*)(cbase + kc0 + (ng + 2) * 512) : zero8;
    const bf16x8 b03 = bl ? *(const bf16x8*)(cbase + kc0 + (ng + 3) * 512) : zero8;
    const bf16x8 b10 = bl ? *(const bf16x8*)(cbase + kc0 + (8 + ng + 0) * 512) : zero8;
    const bf16x8 b11 = bl ? *(const bf16x8*)(cbase + kc0 + (8 + ng + 1) * 512) : zero8;
    const bf16x8 b12 = bl ? *(const bf16x8*)(cbase + kc0 + (8 + ng + 2) * 512) : zero8;
    const bf16x8 b13 = bl ? *(const bf16x8*)(cbase + kc0 + (8 + ng + 3) * 512) : zero8;
    const bf16x8 a0 = *(const bf16x8*)&sm.img[buf][0][lt][lane * 8];
    const bf16x8 a1 = *(const bf16x8*)&sm.img[buf][1][lt][lane * 8];
    if (!(variant & 16)) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b00, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b01, acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b02, acc2, 0, 0, 0);
      acc3 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b03, acc3, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b10, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b11, acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b12, acc2, 0, 0, 0);
      acc3 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b13, acc3, 0, 0, 0);
    } else {
      acc0[0] += bf2f(b00[0]) + bf2f(a0[0]);
      acc1[0] += bf2f(b01[0]) + bf2f(a1[0]);
      acc2[0] += bf2f(b02[0]) + bf2f(b12[0]);
      acc3[0] += bf2f(b03[0]) + bf2f(b10[0]) + bf2f(b11[0]) + bf2f(b13[0]);
    }
    if (more) DW_WRITE(buf ^ 1);
    buf ^= 1;
    __syncthreads();
  }
#undef DW_LOAD
#undef DW_WRITE

  // dW: each wave owns [16 labels x 64 EP] of the block's [64, 128] tile
#define DW_STORE(nt, accv)                                                 \
  _Pragma("unroll") for (int r = 0; r < 4; ++r) {                          \
    const long lrow_ = l0 + lt * 16 + (lane >> 4) * 4 + r;                 \
    if (lrow_ < L && !(variant & 1))                                       \
      dw[lrow_ * 128 + nh + nt * 16 + (lane & 15)] = f2bf(accv[r]);        \
  }
  DW_STORE(0, acc0)
  DW_STORE(1, acc1)
  DW_STORE(2, acc2)
  DW_STORE(3, acc3)
#undef DW_STORE

  // dbias: reduce the per-thread 8-label partials.  Write layout
  // red[krow][label]: bank-conflict-free both ways (stride 65).
#pragma unroll
  for (int j = 0; j < 4; ++j) sm.red[krow][col8 + j] = db0[j];
#pragma unroll
  for (int j = 0; j < 4; ++j) sm.red[krow][col8 + 4 + j] = db1[j];
  __syncthreads();
  {
    const int lbl = threadIdx.x & 63;
    const int kg0 = (threadIdx.x >> 6) * 8;
    float p = 0.f;
#pragma unroll
    for (int kg = 0; kg < 8; ++kg) p += sm.red[kg0 + kg][lbl];
    red2[threadIdx.x >> 6][lbl] = p;
  }
  __syncthreads();
  if (threadIdx.x < 64 && l0 + threadIdx.x < L && !(variant & 1)) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) s += red2[q][threadIdx.x];
    dbias[l0 + threadIdx.x] = s;
  }
}

// three live floats of a coef_lse row: a 12-byte load leaves no dead
// destination register for the allocator to reuse while the load is in
// flight (reuse forces a full vmcnt drain)
struct __attribute__((aligned(16))) hb_meta3 {
  float coef, lse, yf;
};

// PIPELINED head_bwd_dw: same arithmetic, same G image, same dbias
// ownership and tree as head_bwd_dw_kernel — bit-identical outputs — with
// the loads arranged so that HBM requests stay in flight across the MFMAs:
//   * a K-loop stage is D 64-row sub-stages (D * 8 KB of logits per
//     block); the logits chunks and (coef, lse, y) rows of the next TWO
//     stages are in registers or in flight: stage S+2 is issued before
//     stage S's MFMAs and consumed after stage S+1's, so the loads also
//     cover the G arithmetic and the barrier.
//   * wave -> tile map is [64 labels x 16 EP] (was [16 labels x 64 EP]).
//     Per accumulator the MFMA sequence is unchanged (k ascending: a0*b0
//     then a1*b1 per 64-row sub-stage), but a wave needs only TWO global B
//     fragments per sub-stage instead of eight, so a whole stage's B
//     fragments fit in registers and the cv image is read once per block
//     instead of four times (L2 traffic 1.16 GB -> 0.29 GB at top11); the
//     extra A-fragment reads come from LDS.
//   * issue order per stage: B fragments of THIS stage, then the logits
//     prefetch of stage S+2, then a counted wait for the B fragments only —
//     vmcnt counts in issue order, so the prefetch stays outstanding
//     through the MFMAs.
//   * every load is unconditional with the row / label chunk / image
//     sub-stage clamped into its tensor; the guard selects the result of
//     the arithmetic, so G of an invalid row or label chunk is exactly zero.
//     Sub-stages past B multiply an all-zero G image (acc unchanged).
//   * VAR (the C2V_HBDW_VARIANT phase-isolation bits) is a template
//     parameter: the production instantiation has no branch around a load.
// The staging registers are constant-indexed arrays under full unrolls
// (registers, not scratch: the resource report shows 0 scratch).
template <int D, int VAR>
__global__ __launch_bounds__(512, 4) void head_bwd_dw_pipe_kernel(
    const bf16* __restrict__ logits, const bf16* __restrict__ cvimg,
    const float* __restrict__ coef_lse, bf16* __restrict__ dw,
    float* __restrict__ dbias, long B, long L) {
  static_assert(D >= 1 && D <= 2, "sub-stages per stage (3 and 4 spill)");
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const long l0 = (long)blockIdx.x * HB_LB;
  const int krow = threadIdx.x >> 3;        // 0..63: batch row within sub-stage
  const int col8 = (threadIdx.x & 7) * 8;   // 0..56: label chunk start

  // dynamic LDS: G images [2 buf][D][2 ksub][4 label tiles][HB_NSTR] bf16,
  // reused as the dbias reduction scratch red[64][65] after the K-loop,
  // then red2[8][65] f32
  extern __shared__ __attribute__((aligned(16))) char hbp_smem[];
  bf16* img = (bf16*)hbp_smem;
  float* red = (float*)hbp_smem;
  constexpr int SUBSZ = 2 * 4 * HB_NSTR;  // one sub-stage image (elements)
  constexpr int IMGB = 2 * D * SUBSZ * 2;
  constexpr int REDB = HB_ROWS * (HB_LB + 1) * 4;
  float* red2 = (float*)(hbp_smem + (IMGB > REDB ? IMGB : REDB));

  const int n = col8 >> 4;
  const int base_l = col8 & 15;
  const int ksub = krow >> 5;
  const int kgrp = (krow >> 3) & 3;
  const int jslot = krow & 7;
  const long lc = l0 + col8;
  const bool lok = lc < L;             // L % 8 == 0: chunk fully in bounds
  const long lcc = lok ? lc : L - 8;   // clamped load address
  const long nsub = (B + HB_ROWS - 1) / HB_ROWS;
  const long nst = (nsub + D - 1) / D;

  f32x4 db0 = {0.f, 0.f, 0.f, 0.f};
  f32x4 db1 = {0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero8 = {};

  // two staging register sets: stage t's logits chunks and (coef, lse, y)
  // rows live in set t & 1 (named, swapped by unrolling the loop by two)
  bf16x8 lvA[D], lvB[D];
  hb_meta3 mtA[D], mtB[D];  // 12 of the row's 16 bytes
  // cvimg layout: [k-chunk][8 nt][64 lanes][8]; this wave's EP tile = wave
  const bf16* cbase = cvimg + (long)wave * 512 + (long)lane * 8;
  // this thread's slot in a sub-stage G image
  const int woff = (ksub * 4 + n) * HB_NSTR + (base_l + kgrp * 16) * 8 + jslot;

// the (coef, lse, y) rows first (L2 hits), then the logits chunks (HBM)
#define DWP_LOADL(lv, meta, S)                                             \
  _Pragma("unroll") for (int i = 0; i < D; ++i) {                          \
    if (VAR & 4) {                                                         \
      meta[i] = hb_meta3{0.f, 0.f, 0.f};                                   \
    } else {                                                               \
      const long row_ = min(((S) * D + i) * HB_ROWS + krow, B - 1);        \
      meta[i] = *(const hb_meta3*)(coef_lse + 4 * row_);                   \
    }                                                                      \
  }                                                                        \
  __builtin_amdgcn_sched_barrier(0);                                       \
  _Pragma("unroll") for (int i = 0; i < D; ++i) {                          \
    if (VAR & 4) {                                                         \
      lv[i] = zero8;                                                       \
    } else {                                                               \
      const long row_ = min(((S) * D + i) * HB_ROWS + krow, B - 1);        \
      lv[i] = *(const bf16x8*)(logits + row_ * L + lcc);                   \
    }                                                                      \
  }

// branch-free on purpose: the guard selects the result, so the arithmetic
// sits in the loop's one basic block and the loads cannot be sunk into it
#define DWP_WRITE(lv, meta, S, buf)                                        \
  _Pragma("unroll") for (int i = 0; i < D; ++i) {                          \
    const bool rok_ =                                                      \
        ((S) * D + i) * HB_ROWS + krow < B && lok && !(VAR & 4);           \
    bf16x8 gv;                                                             \
    const float coef_ = meta[i].coef;                                      \
    const float lse_ = meta[i].lse;                                        \
    const long y_ = (long)meta[i].yf;                                      \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) {                        \
      const float x_ = bf2f(lv[i][j]) - lse_;                              \
      float g_ = coef_ * ((VAR & 8) ? x_ : __expf(x_));                    \
      if (lc + j == y_) g_ -= coef_;                                       \
      const bf16 gb_ = rok_ ? f2bf(g_) : zero8[0];                         \
      gv[j] = gb_;                                                         \
      if (j < 4) db0[j & 3] += rok_ ? bf2f(gb_) : 0.f;                     \
      else db1[j & 3] += rok_ ? bf2f(gb_) : 0.f;                           \
    }                                                                      \
    bf16* dst_ = img + ((buf) * D + i) * SUBSZ + woff;                     \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) dst_[j * 8] = gv[j];     \
  }

  f32x4 acc[4];  // [label tile]
#pragma unroll
  for (int lt = 0; lt < 4; ++lt) acc[lt] = f32x4{0.f, 0.f, 0.f, 0.f};

#define DWP_LOADB(S)                                                       \
  bf16x8 bq0[D], bq1[D];                                                   \
  _Pragma("unroll") for (int i = 0; i < D; ++i) {                          \
    if (VAR & 2) {                                                         \
      bq0[i] = zero8;                                                      \
      bq1[i] = zero8;                                                      \
    } else {                                                               \
      const bf16* p_ = cbase + min((S) * D + i, nsub - 1) * (16 * 512);    \
      bq0[i] = *(const bf16x8*)(p_);                                       \
      bq1[i] = *(const bf16x8*)(p_ + 8 * 512);                             \
    }                                                                      \
  }

#define DWP_MMA(buf)                                                       \
  {                                                                        \
    const bf16* ib = img + (buf) * D * SUBSZ + lane * 8;                   \
    _Pragma("unroll") for (int i = 0; i < D; ++i) {                        \
      bf16x8 a0[4], a1[4];                                                 \
      _Pragma("unroll") for (int lt = 0; lt < 4; ++lt) {                   \
        a0[lt] = *(const bf16x8*)(ib + (i * 8 + lt) * HB_NSTR);            \
        a1[lt] = *(const bf16x8*)(ib + (i * 8 + 4 + lt) * HB_NSTR);        \
      }                                                                    \
      if (!(VAR & 16)) {                                                   \
        _Pragma("unroll") for (int lt = 0; lt < 4; ++lt)                   \
            acc[lt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(             \
                a0[lt], bq0[i], acc[lt], 0, 0, 0);                         \
        _Pragma("unroll") for (int lt = 0; lt < 4; ++lt)                   \
            acc[lt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(             \
                a1[lt], bq1[i], acc[lt], 0, 0, 0);                         \
      } else {                                                             \
        _Pragma("unroll") for (int lt = 0; lt < 4; ++lt)                   \
            acc[lt][0] += bf2f(a0[lt][0]) + bf2f(a1[lt][0]) +              \
                          bf2f(bq0[i][0]) + bf2f(bq1[i][0]);               \
      }                                                                    \
    }                                                                      \
  }

// one stage: this stage's B fragments first, then the logits of the stage
// after next (into the set the previous G write just freed); the wait in
// front of the MFMAs covers the B fragments (and the older, next-stage
// logits) only.  The next stage's G image is written from the other set.
#define DWP_BODY(S, lvN, mtN, lvW, mtW, bufc)                              \
  {                                                                        \
    DWP_LOADB(S)                                                           \
    __builtin_amdgcn_sched_barrier(0);                                     \
    DWP_LOADL(lvN, mtN, (S) + 2)                                           \
    __builtin_amdgcn_sched_barrier(0);                                     \
    DWP_MMA(bufc)                                                          \
    __builtin_amdgcn_sched_barrier(0);                                     \
    if ((S) + 1 < nst2) {                                                  \
      DWP_WRITE(lvW, mtW, (S) + 1, (bufc) ^ 1)                             \
    }                                                                      \
    __syncthreads();                                                       \
  }

  DWP_LOADL(lvA, mtA, 0L)
  DWP_LOADL(lvB, mtB, 1L)
  DWP_WRITE(lvA, mtA, 0L, 0)
  __syncthreads();

  // the loop body is two whole stages, straight-line (a conditional
  // second stage makes a join where the compiler drains every load); an
  // odd stage count runs one all-zero stage: zero G image, acc unchanged
  const long nst2 = (nst + 1) & ~1L;
  for (long S = 0; S < nst2; S += 2) {
    DWP_BODY(S, lvA, mtA, lvB, mtB, 0)
    DWP_BODY(S + 1, lvB, mtB, lvA, mtA, 1)
  }
#undef DWP_BODY
#undef DWP_LOADB
#undef DWP_MMA
#undef DWP_LOADL
#undef DWP_WRITE

  // dW: each wave owns [64 labels x 16 EP] of the block's [64, 128] tile
#pragma unroll
  for (int lt = 0; lt < 4; ++lt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long lrow_ = l0 + lt * 16 + (lane >> 4) * 4 + r;
      if (lrow_ < L && !(VAR & 1))
        dw[lrow_ * 128 + wave * 16 + (lane & 15)] = f2bf(acc[lt][r]);
    }

  // dbias: the head_bwd_dw_kernel tree, unchanged (red[krow][label],
  // stride 65)
#pragma unroll
  for (int j = 0; j < 4; ++j) red[krow * (HB_LB + 1) + col8 + j] = db0[j];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    red[krow * (HB_LB + 1) + col8 + 4 + j] = db1[j];
  __syncthreads();
  {
    const int lbl = threadIdx.x & 63;
    const int kg0 = (threadIdx.x >> 6) * 8;
    float p = 0.f;
#pragma unroll
    for (int kg = 0; kg < 8; ++kg) p += red[(kg0 + kg) * (HB_LB + 1) + lbl];
    red2[(threadIdx.x >> 6) * (HB_LB + 1) + lbl] = p;
  }
  __syncthreads();
  if (threadIdx.x < 64 && l0 + threadIdx.x < L && !(VAR & 1)) {
    float s2 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) s2 += red2[q * (HB_LB + 1) + threadIdx.x];
    dbias[l0 + threadIdx.x] = s2;
  }
}

// [N, 128] row-major -> MFMA B-fragment image [nchunk][8 nt][64 lanes][8]:
// entry [kc][nt][l][j] = x[kc*32 + (l>>4)*8 + j][nt*16 + (l&15)]
// (zero-padded past N).  One 32-row tile per block staged through LDS;
// output writes are contiguous 16 B per thread.  Used for BOTH operands
// that appear as MFMA B fragments with a row index as k: cv [B, 128] in
// head_bwd_dw and W [L, 128] in head_bwd_dcv.
__global__ __launch_bounds__(256) void swizzle_cv_kernel(
    const bf16* __restrict__ cv, bf16* __restrict__ cvimg, long B) {
  const long kc = blockIdx.x;
  __shared__ bf16 tile[32][132];
  const bf16x8 zero8 = {};
  for (int t = threadIdx.x; t < 32 * 16; t += 256) {
    const int r = t >> 4;
    const int c = t & 15;
    const long row = kc * 32 + r;
    const bf16x8 v =
        (row < B) ? *(const bf16x8*)(cv + row * 128 + c * 8) : zero8;
    *(bf16x8*)&tile[r][c * 8] = v;
  }
  __syncthreads();
  // 512 outputs of 16 B per tile: (nt, lane) pairs, 2 per thread
  for (int t = threadIdx.x; t < 512; t += 256) {
    const int nt = t >> 6;
    const int l = t & 63;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[(l >> 4) * 8 + j][nt * 16 + (l & 15)];
    *(bf16x8*)(cvimg + ((kc * 8 + nt) * 64 + (long)l) * 8) = v;
  }
}

// 128-label-tile variant of head_bwd_dw — MEASURED SLOWER and kept as an
// A/B reference (C2V_HBDW128=<threshold> to enable): 125 vs 88 us at
// L=72,416 and a wash (320 vs 326) at L=261k.  The hypothesis (halving
// the block count amortizes per-block skeleton cost and the 256-B logits
// row spans cut line amplification) loses to the doubled per-wave
// B-fragment read + MFMA chain per stage between the same barriers.
__global__ __launch_bounds__(512) void head_bwd_dw128_kernel(
    const bf16* __restrict__ logits, const bf16* __restrict__ cvimg,
    const float* __restrict__ coef_lse, bf16* __restrict__ dw,
    float* __restrict__ dbias, long B, long L) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const long l0 = (long)blockIdx.x * 128;
  const int krow = threadIdx.x >> 4;        // 0..31 (and +32: second chunk)
  const int col8 = (threadIdx.x & 15) * 8;  // 0..120: label chunk start

  __shared__ union {
    bf16 img[2][2][8][HB_NSTR];  // [buf][ksub][label tile][image]
    float red[32][129];
  } sm;
  __shared__ float red2[4][129];

  const int n = col8 >> 4;
  const int base_l = col8 & 15;
  const int kgrp = (krow >> 3) & 3;  // same for krow and krow+32
  const int jslot = krow & 7;
  const long lc = l0 + col8;
  const bool lok = lc < L;

  f32x4 db0 = {0.f, 0.f, 0.f, 0.f};
  f32x4 db1 = {0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero8 = {};

  bf16x8 lv0, lv1;
  f32x4 meta0, meta1;
  bool rok0, rok1;

#define DW1_LOAD(mb)                                                       \
  do {                                                                     \
    const long r0_ = (mb) + krow;                                          \
    const long r1_ = r0_ + 32;                                             \
    rok0 = r0_ < B && lok;                                                 \
    rok1 = r1_ < B && lok;                                                 \
    if (rok0) {                                                            \
      meta0 = *(const f32x4*)(coef_lse + 4 * r0_);                         \
      lv0 = *(const bf16x8*)(logits + r0_ * L + lc);                       \
    }                                                                      \
    if (rok1) {                                                            \
      meta1 = *(const f32x4*)(coef_lse + 4 * r1_);                         \
      lv1 = *(const bf16x8*)(logits + r1_ * L + lc);                       \
    }                                                                      \
  } while (0)

#define DW1_G(gv, rok, meta, lv)                                           \
  do {                                                                     \
    gv = zero8;                                                            \
    if (rok) {                                                             \
      const float coef_ = meta[0];                                         \
      const float lse_ = meta[1];                                          \
      const long y_ = (long)meta[2];                                       \
      _Pragma("unroll") for (int j = 0; j < 8; ++j) {                      \
        float g_ = coef_ * __expf(bf2f(lv[j]) - lse_);                     \
        if (lc + j == y_) g_ -= coef_;                                     \
        const bf16 gb_ = f2bf(g_);                                         \
        gv[j] = gb_;                                                       \
        if (j < 4) db0[j & 3] += bf2f(gb_);                                \
        else db1[j & 3] += bf2f(gb_);                                      \
      }                                                                    \
    }                                                                      \
  } while (0)

#define DW1_WRITE(buf)                                                     \
  do {                                                                     \
    bf16x8 g0, g1;                                                         \
    DW1_G(g0, rok0, meta0, lv0);                                           \
    DW1_G(g1, rok1, meta1, lv1);                                           \
    bf16* d0_ = sm.img[buf][0][n];                                         \
    bf16* d1_ = sm.img[buf][1][n];                                         \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) {                        \
      d0_[(base_l + j + kgrp * 16) * 8 + jslot] = g0[j];                   \
      d1_[(base_l + j + kgrp * 16) * 8 + jslot] = g1[j];                   \
    }                                                                      \
  } while (0)

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0,
        acc3 = acc0, acc4 = acc0, acc5 = acc0, acc6 = acc0, acc7 = acc0;

  const int lt = wave;               // this wave's label tile (16 labels)
  const bf16* cbase = cvimg + (long)lane * 8;

  DW1_LOAD(0);
  DW1_WRITE(0);
  __syncthreads();
  int buf = 0;
  for (long mb = 0; mb < B; mb += HB_ROWS) {
    const bool more = mb + HB_ROWS < B;
    if (more) DW1_LOAD(mb + HB_ROWS);
    const long kc0 = (mb >> 5) * 8 * 512;
    const bf16x8 a0 = *(const bf16x8*)&sm.img[buf][0][lt][lane * 8];
    const bf16x8 a1 = *(const bf16x8*)&sm.img[buf][1][lt][lane * 8];
#define DW1_MM(ks, nt, accv)                                               \
    {                                                                      \
      const bf16x8 b_ =                                                    \
          *(const bf16x8*)(cbase + kc0 + ((ks) * 8 + (nt)) * 512);         \
      accv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                      \
          (ks) ? a1 : a0, b_, accv, 0, 0, 0);                              \
    }
    DW1_MM(0, 0, acc0) DW1_MM(0, 1, acc1) DW1_MM(0, 2, acc2)
    DW1_MM(0, 3, acc3) DW1_MM(0, 4, acc4) DW1_MM(0, 5, acc5)
    DW1_MM(0, 6, acc6) DW1_MM(0, 7, acc7)
    DW1_MM(1, 0, acc0) DW1_MM(1, 1, acc1) DW1_MM(1, 2, acc2)
    DW1_MM(1, 3, acc3) DW1_MM(1, 4, acc4) DW1_MM(1, 5, acc5)
    DW1_MM(1, 6, acc6) DW1_MM(1, 7, acc7)
#undef DW1_MM
    if (more) DW1_WRITE(buf ^ 1);
    buf ^= 1;
    __syncthreads();
  }
#undef DW1_LOAD
#undef DW1_G
#undef DW1_WRITE

  // dW: wave owns [16 labels x 128 EP]
#define DW1_ST(nt, accv)                                                   \
  _Pragma("unroll") for (int r = 0; r < 4; ++r) {                          \
    const long lrow_ = l0 + lt * 16 + (lane >> 4) * 4 + r;                 \
    if (lrow_ < L)                                                         \
      dw[lrow_ * 128 + (nt) * 16 + (lane & 15)] = f2bf(accv[r]);           \
  }
  DW1_ST(0, acc0) DW1_ST(1, acc1) DW1_ST(2, acc2) DW1_ST(3, acc3)
  DW1_ST(4, acc4) DW1_ST(5, acc5) DW1_ST(6, acc6) DW1_ST(7, acc7)
#undef DW1_ST

  // dbias: red[krow(32)][label(128)] then 4-way fixed-order combine
#pragma unroll
  for (int j = 0; j < 4; ++j) sm.red[krow][col8 + j] = db0[j];
#pragma unroll
  for (int j = 0; j < 4; ++j) sm.red[krow][col8 + 4 + j] = db1[j];
  __syncthreads();
  {
    const int lbl = threadIdx.x & 127;
    const int kg0 = (threadIdx.x >> 7) * 8;
    float p = 0.f;
#pragma unroll
    for (int kg = 0; kg < 8; ++kg) p += sm.red[kg0 + kg][lbl];
    red2[threadIdx.x >> 7][lbl] = p;
  }
  __syncthreads();
  if (threadIdx.x < 128 && l0 + threadIdx.x < L) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) s += red2[q][threadIdx.x];
    dbias[l0 + threadIdx.x] = s;
  }
}

// dcv split-K partials: head_dgrad.hip's kernel with A = G recomputed.
// The W operand arrives as a pre-swizzled B-fragment image (swizzle_cv
// layout, 128-label-granular): per 128-label sub-stage the LDS staging is
// ONE contiguous 32-KB copy (replacing a transposed-W staging whose
// 256-B row reads at stride 2L were line-amplified, plus the per-step
// transpose_w kernel entirely).
__global__ __launch_bounds__(512) void head_bwd_dcv_kernel(
    const bf16* __restrict__ logits, const bf16* __restrict__ wimg,
    const float* __restrict__ coef_lse, float* __restrict__ partials, long B,
    long L, int chunk, int GYB) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int total = gridDim.x;
  const int lin = (total % 8 == 0)
      ? (int)(blockIdx.x % 8) * (total / 8) + (int)blockIdx.x / 8
      : (int)blockIdx.x;
  const int by = lin % GYB;
  const int sc = lin / GYB;
  const long bt0 = (long)by * 128;
  const int kj = (lane >> 4) * 8;

  const long row = bt0 + wave * 16 + (lane & 15);
  const bool aok = row < B;
  float coef = 0.f, lseb = 0.f;
  long y = -1;
  if (aok) {
    const f32x4 meta = *(const f32x4*)(coef_lse + 4 * row);
    coef = meta[0];
    lseb = meta[1];
    y = (long)meta[2];
  }
  const bf16* ap = logits + row * L + kj;

  // one 128-label sub-stage of the W image: [4 kc][8 nt][64 lanes][8]
  __shared__ bf16 wst[4 * 8 * 512];

  f32x4 acc[8];
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero8 = {};

  const int nsub = chunk / 128;
  for (int s = 0; s < nsub; ++s) {
    const long l0 = (long)sc * chunk + (long)s * 128;
    if (l0 >= L) break;
    // contiguous 32-KB image copy (image is zero-padded past L)
    const bf16* src = wimg + (l0 >> 5) * 4096;
    for (int t = threadIdx.x; t < 2048; t += 512)
      *(bf16x8*)&wst[t * 8] = *(const bf16x8*)(src + t * 8);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const long lc = l0 + kk * 32 + kj;
      bf16x8 a = zero8;
      if (aok && lc < L) {
        const bf16x8 v = *(const bf16x8*)(ap + l0 + kk * 32);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float gg = coef * __expf(bf2f(v[j]) - lseb);
          if (lc + j == y) gg -= coef;
          a[j] = f2bf(gg);
        }
      }
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        const bf16x8 b =
            *(const bf16x8*)&wst[(kk * 8 + nt) * 512 + lane * 8];
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt],
                                                          0, 0, 0);
      }
    }
    __syncthreads();
  }

  float* slab = partials + (long)sc * B * 128;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long grow = bt0 + wave * 16 + (lane >> 4) * 4 + r;
    if (grow < B) {
#pragma unroll
      for (int nt = 0; nt < 8; ++nt)
        slab[grow * 128 + nt * 16 + (lane & 15)] = acc[nt][r];
    }
  }
}

// PIPELINED head_bwd_dcv: same tiling, slabs, swizzle and per-accumulator
// MFMA order (sub-stage ascending, kk ascending) as head_bwd_dcv_kernel —
// bit-identical partials — with split staging: while sub-stage s runs its
// 32 MFMAs per wave, sub-stage s+1's four logits fragments and its four
// 16-B pieces of the W image are already in flight into registers, issued
// together.  Fragment loads are unconditional with row and label offset
// clamped into [0, B*L); the fragment is zeroed afterwards where the row
// or the label chunk is out of range.
// DBUF=1 double-buffers the W image in LDS (64 KB, one barrier per
// sub-stage); DBUF=0 keeps the single 32-KB buffer and the second barrier.
template <int DBUF>
__global__ __launch_bounds__(512, 4) void head_bwd_dcv_pipe_kernel(
    const bf16* __restrict__ logits, const bf16* __restrict__ wimg,
    const float* __restrict__ coef_lse, float* __restrict__ partials, long B,
    long L, int chunk, int GYB) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int total = gridDim.x;
  const int lin = (total % 8 == 0)
      ? (int)(blockIdx.x % 8) * (total / 8) + (int)blockIdx.x / 8
      : (int)blockIdx.x;
  const int by = lin % GYB;
  const int sc = lin / GYB;
  const long bt0 = (long)by * 128;
  const int kj = (lane >> 4) * 8;

  const long row = bt0 + wave * 16 + (lane & 15);
  const bool aok = row < B;
  float coef = 0.f, lseb = 0.f;
  long y = -1;
  if (aok) {
    const f32x4 meta = *(const f32x4*)(coef_lse + 4 * row);
    coef = meta[0];
    lseb = meta[1];
    y = (long)meta[2];
  }
  const bf16* ap = logits + min(row, B - 1) * L;  // clamped row

  // 128-label sub-stages of the W image: [4 kc][8 nt][64 lanes][8] each
  __shared__ bf16 wst[DBUF ? 2 : 1][4 * 8 * 512];

  f32x4 acc[8];
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero8 = {};

  // sub-stages of this block that start inside L (>= 1: sc * chunk < L)
  const long lbase = (long)sc * chunk;
  const int nv = (int)min((long)(chunk / 128), (L - lbase + 127) / 128);

  bf16x8 an[4];  // next sub-stage's logits fragments
  bf16x8 wr[4];  // next sub-stage's W image pieces

#define DCVP_LOAD(l0_)                                                     \
  do {                                                                     \
    _Pragma("unroll") for (int kk = 0; kk < 4; ++kk)                       \
        an[kk] = *(const bf16x8*)(ap +                                     \
                                  min((l0_) + kk * 32 + kj, L - 8));       \
    const bf16* src_ = wimg + ((l0_) >> 5) * 4096 + threadIdx.x * 8;       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                          \
        wr[i] = *(const bf16x8*)(src_ + i * 4096);                         \
  } while (0)

#define DCVP_STAGE(b)                                                      \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)                            \
      *(bf16x8*)&wst[b][(threadIdx.x + i * 512) * 8] = wr[i]

  DCVP_LOAD(lbase);
  DCVP_STAGE(0);
  __syncthreads();

  for (int s = 0; s < nv; ++s) {
    const long l0 = lbase + (long)s * 128;
    const int cur = DBUF ? (s & 1) : 0;
    const bool more = s + 1 < nv;  // block-uniform
    // the landed fragments move out of the prefetch registers so the next
    // sub-stage's loads are in flight before the G arithmetic starts
    bf16x8 ac[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) ac[kk] = an[kk];
    if (more) DCVP_LOAD(l0 + 128);
    bf16x8 a[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const long lc = l0 + kk * 32 + kj;
      a[kk] = zero8;
      if (aok && lc < L) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float gg = coef * __expf(bf2f(ac[kk][j]) - lseb);
          if (lc + j == y) gg -= coef;
          a[kk][j] = f2bf(gg);
        }
      }
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      bf16x8 b[8];
#pragma unroll
      for (int nt = 0; nt < 8; ++nt)
        b[nt] = *(const bf16x8*)&wst[cur][(kk * 8 + nt) * 512 + lane * 8];
#pragma unroll
      for (int nt = 0; nt < 8; ++nt)
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kk], b[nt],
                                                          acc[nt], 0, 0, 0);
    }
    if (!DBUF) __syncthreads();
    if (more) DCVP_STAGE(DBUF ? (cur ^ 1) : 0);
    __syncthreads();
  }
#undef DCVP_LOAD
#undef DCVP_STAGE

  float* slab = partials + (long)sc * B * 128;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long grow = bt0 + wave * 16 + (lane >> 4) * 4 + r;
    if (grow < B) {
#pragma unroll
      for (int nt = 0; nt < 8; ++nt)
        slab[grow * 128 + nt * 16 + (lane & 15)] = acc[nt][r];
    }
  }
}

// ---------------------------------------------------------------------------
// STREAMING variant of the dcv kernel: the logits tensor is never READ —
// each wave recomputes its [16 batch x 128 label] logits tile with a first
// MFMA pass (cv and W arrive as swizzle_a fragment images, so both operand
// streams are contiguous 1-KB wave reads), applies the softmax-gradient
// transform in registers, transposes G through a wave-PRIVATE LDS
// A-fragment image (producer wave == consumer wave, so no extra barriers),
// and runs the usual split-K accumulate against the staged W B-image.
// Removes the 2-B/elem logits read (534 MB at java-large) at the price of
// duplicating the forward GEMM's FLOPs (~68 GFLOP, ~3% of one MFMA-second)
// — the trade the MI355X's 2.5-PFLOP/s : 5.5-TB/s ratio is built for.
//
// The recomputed logits are the f32 MFMA accumulators plus the f32 bias,
// as in the forward's epilogue BEFORE its bf16 rounding.  The forward's
// online-softmax stats (and so lse) are taken from the bf16-ROUNDED value
// (head_fwd.hip, "stats from the bf16-rounded value"), so the exponent here,
// unrounded logit - lse, is one rounding FURTHER from lse than in the
// stored-logits kernel above: off by the logit's rounding error, up to
// 2^-9 |logit| (0.06 at a logit of 32).  G then differs from the
// stored-logits kernel's by that factor and sum_l p_l is not exactly 1.
__global__ __launch_bounds__(512) void head_bwd_dcv_rc_kernel(
    const bf16* __restrict__ cvimg_a, const bf16* __restrict__ wimg_a,
    const bf16* __restrict__ wimg, const float* __restrict__ bias,
    const float* __restrict__ coef_lse, float* __restrict__ partials, long B,
    long L, int chunk, int GYB) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int total = gridDim.x;
  const int lin = (total % 8 == 0)
      ? (int)(blockIdx.x % 8) * (total / 8) + (int)blockIdx.x / 8
      : (int)blockIdx.x;
  const int by = lin % GYB;
  const int sc = lin / GYB;
  const long bt0 = (long)by * 128;

  // per-lane meta for its 4 MFMA1 C rows (batch = bt0 + wave*16 + g4*4+r)
  float coef4[4], lse4[4], yf4[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long row = bt0 + wave * 16 + (lane >> 4) * 4 + r;
    if (row < B) {
      const f32x4 meta = *(const f32x4*)(coef_lse + 4 * row);
      coef4[r] = meta[0];
      lse4[r] = meta[1];
      yf4[r] = meta[2];
    } else {
      coef4[r] = 0.f;  // coef 0 => g == 0 for out-of-range rows
      lse4[r] = 0.f;
      yf4[r] = -1.f;
    }
  }
  // MFMA1 A operand: this wave's 16 cv rows, all 128 k — loaded ONCE
  // (cvimg_a rows past B are zero-padded by swizzle_a)
  const bf16* ca = cvimg_a + ((bt0 >> 4) + wave) * 4 * 512 + lane * 8;
  const bf16x8 acv0 = *(const bf16x8*)(ca);
  const bf16x8 acv1 = *(const bf16x8*)(ca + 512);
  const bf16x8 acv2 = *(const bf16x8*)(ca + 1024);
  const bf16x8 acv3 = *(const bf16x8*)(ca + 1536);

  __shared__ bf16 wst[4 * 8 * 512];       // MFMA2 W B-fragments (32 KB)
  __shared__ bf16 gst[8][4][512];         // per-wave G A-fragment image

  f32x4 acc[8];
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nsub = chunk / 128;
  for (int s = 0; s < nsub; ++s) {
    const long l0s = (long)sc * chunk + (long)s * 128;
    if (l0s >= L) break;
    // stage the MFMA2 W image (contiguous 32-KB copy, zero-padded past L)
    const bf16* src = wimg + (l0s >> 5) * 4096;
    for (int t = threadIdx.x; t < 2048; t += 512)
      *(bf16x8*)&wst[t * 8] = *(const bf16x8*)(src + t * 8);
    __syncthreads();

    // MFMA1: recompute the wave's [16 x 128] logits tile and emit G
    const bf16* wa = wimg_a + (l0s >> 4) * 4 * 512 + lane * 8;
#pragma unroll
    for (int nt2 = 0; nt2 < 8; ++nt2) {
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
      const bf16* wp = wa + (long)nt2 * 4 * 512;
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          acv0, *(const bf16x8*)(wp), c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          acv1, *(const bf16x8*)(wp + 512), c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          acv2, *(const bf16x8*)(wp + 1024), c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          acv3, *(const bf16x8*)(wp + 1536), c, 0, 0, 0);
      const long lab = l0s + nt2 * 16 + (lane & 15);
      const float bl = lab < L ? bias[lab] : 0.f;
      const int lab32 = (nt2 & 1) * 16 + (lane & 15);
      const int ebase = ((lab32 >> 3) * 16) * 8 + (lab32 & 7);
      bf16* gout = gst[wave][nt2 >> 1];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float g = 0.f;
        if (lab < L) {
          g = coef4[r] * __expf(c[r] + bl - lse4[r]);
          if ((float)lab == yf4[r]) g -= coef4[r];
        }
        gout[ebase + (((lane >> 4) * 4 + r)) * 8] = f2bf(g);
      }
    }
    // MFMA2: split-K accumulate (A = own-wave G image, B = staged W)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const bf16x8 a = *(const bf16x8*)&gst[wave][kk][lane * 8];
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        const bf16x8 b =
            *(const bf16x8*)&wst[(kk * 8 + nt) * 512 + lane * 8];
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[nt],
                                                          0, 0, 0);
      }
    }
    __syncthreads();
  }

  float* slab = partials + (long)sc * B * 128;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long grow = bt0 + wave * 16 + (lane >> 4) * 4 + r;
    if (grow < B) {
#pragma unroll
      for (int nt = 0; nt < 8; ++nt)
        slab[grow * 128 + nt * 16 + (lane & 15)] = acc[nt][r];
    }
  }
}

extern "C" {

void launch_head_bwd_prep(const long* label, const float* weight,
                          const float* acc_ws, const float* gscale,
                          const float* lse, float* coef_lse, long B,
                          hipStream_t stream) {
  head_bwd_prep_kernel<<<(B + 255) / 256, 256, 0, stream>>>(
      label, weight, acc_ws, gscale, lse, coef_lse, B);
}

void launch_swizzle_cv(const void* cv, void* cvimg, long B, long nchunk,
                       hipStream_t stream) {
  // nchunk is caller-chosen (rounded to the consumer's stage granularity:
  // 64 rows for head_bwd_dw's cv, 128 for head_bwd_dcv's W) so tail-stage
  // fragment reads always hit written (zero-padded) chunks
  swizzle_cv_kernel<<<(int)nchunk, 256, 0, stream>>>(
      (const bf16*)cv, (bf16*)cvimg, B);
}

void launch_head_bwd_dw(const void* logits, const void* cvimg,
                        const float* coef_lse, void* dw, float* dbias,
                        long B, long L, hipStream_t stream) {
  // 64-label tiles by default; the 128-tile variant measured slower at
  // both top11 and java-large shapes (see the kernel comment) and is
  // reachable for experiments via C2V_HBDW128=<L threshold>
  const char* te = getenv("C2V_HBDW128");
  const long thresh = te ? atol(te) : (1L << 60);
  if (L >= thresh) {
    const int grid = (int)((L + 127) / 128);
    head_bwd_dw128_kernel<<<grid, 512, 0, stream>>>(
        (const bf16*)logits, (const bf16*)cvimg, coef_lse, (bf16*)dw, dbias,
        B, L);
    return;
  }
  const int grid = (int)((L + HB_LB - 1) / HB_LB);
  const char* ve = getenv("C2V_HBDW_VARIANT");
  const int variant = ve ? atoi(ve) : 0;
  const char* occ_env = getenv("C2V_HBDW_OCC");
  if (occ_env && occ_env[0] == '6')
    head_bwd_dw_kernel<6><<<grid, 512, 0, stream>>>(
        (const bf16*)logits, (const bf16*)cvimg, coef_lse, (bf16*)dw, dbias,
        B, L, variant);
  else
    head_bwd_dw_kernel<<<grid, 512, 0, stream>>>(
        (const bf16*)logits, (const bf16*)cvimg, coef_lse, (bf16*)dw, dbias,
        B, L, variant);
}

void launch_head_bwd_dcv(const void* logits, const void* wimg,
                         const float* coef_lse, float* partials, long B,
                         long L, int chunk, hipStream_t stream) {
  const int GYB = (int)((B + 127) / 128);
  const int split = (int)((L + chunk - 1) / chunk);
  head_bwd_dcv_kernel<<<GYB * split, 512, 0, stream>>>(
      (const bf16*)logits, (const bf16*)wimg, coef_lse, partials, B, L,
      chunk, GYB);
}

// LDS bytes of head_bwd_dw_pipe_kernel<D>: G images (or the dbias scratch,
// whichever is larger) + red2
static int hbp_dw_smem(int D) {
  const int imgb = 2 * D * 2 * 4 * HB_NSTR * 2;
  const int redb = HB_ROWS * (HB_LB + 1) * 4;
  return (imgb > redb ? imgb : redb) + 8 * (HB_LB + 1) * 4;
}

// depth: 64-row sub-stages per stage D (1 or 2; two stages are prefetched,
// so 2 * D sub-stages of logits are in flight per thread); 0 =
// C2V_HB_DW_DEPTH or the shipped default.  Returns false for an
// unsupported depth / variant combination (the diagnostic variants exist
// at the shipped depth only, variant 16 at D = 1).
bool launch_head_bwd_dw_pipe(const void* logits, const void* cvimg,
                             const float* coef_lse, void* dw, float* dbias,
                             long B, long L, int depth, hipStream_t stream) {
  if (depth == 0) {
    const char* de = getenv("C2V_HB_DW_DEPTH");
    depth = de ? atoi(de) : HB_DW_DEPTH;
  }
  const char* ve = getenv("C2V_HBDW_VARIANT");
  const int variant = ve ? atoi(ve) : 0;
  const int grid = (int)((L + HB_LB - 1) / HB_LB);
#define DWP_CASE(d, v)                                                     \
  if (depth == d && variant == v) {                                        \
    head_bwd_dw_pipe_kernel<d, v><<<grid, 512, hbp_dw_smem(d), stream>>>(  \
        (const bf16*)logits, (const bf16*)cvimg, coef_lse, (bf16*)dw,      \
        dbias, B, L);                                                      \
    return true;                                                           \
  }
  DWP_CASE(1, 0) DWP_CASE(2, 0)
  // diagnostic instantiations (phase isolation) at the shipped depth
  DWP_CASE(HB_DW_DEPTH, 1) DWP_CASE(HB_DW_DEPTH, 2) DWP_CASE(HB_DW_DEPTH, 4)
  DWP_CASE(HB_DW_DEPTH, 6) DWP_CASE(HB_DW_DEPTH, 8)
  // the no-MFMA variant spills at D = 2 (the cheap accumulate keeps every
  // A fragment live at once); it exists at D = 1
  if (variant == 16) depth = 1;
  DWP_CASE(1, 16)
#undef DWP_CASE
  return false;
}

// dbuf: 1 = double-buffered W image, 0 = single buffer, -1 =
// C2V_HB_DCV_DBUF or the default
void launch_head_bwd_dcv_pipe(const void* logits, const void* wimg,
                              const float* coef_lse, float* partials, long B,
                              long L, int chunk, int dbuf,
                              hipStream_t stream) {
  if (dbuf < 0) {
    const char* de = getenv("C2V_HB_DCV_DBUF");
    dbuf = de ? atoi(de) : HB_DCV_DBUF;
  }
  const int GYB = (int)((B + 127) / 128);
  const int split = (int)((L + chunk - 1) / chunk);
  if (dbuf)
    head_bwd_dcv_pipe_kernel<1><<<GYB * split, 512, 0, stream>>>(
        (const bf16*)logits, (const bf16*)wimg, coef_lse, partials, B, L,
        chunk, GYB);
  else
    head_bwd_dcv_pipe_kernel<0><<<GYB * split, 512, 0, stream>>>(
        (const bf16*)logits, (const bf16*)wimg, coef_lse, partials, B, L,
        chunk, GYB);
}

void launch_head_bwd_dcv_rc(const void* cvimg_a, const void* wimg_a,
                            const void* wimg, const float* bias,
                            const float* coef_lse, float* partials, long B,
                            long L, int chunk, hipStream_t stream) {
  const int GYB = (int)((B + 127) / 128);
  const int split = (int)((L + chunk - 1) / chunk);
  head_bwd_dcv_rc_kernel<<<GYB * split, 512, 0, stream>>>(
      (const bf16*)cvimg_a, (const bf16*)wimg_a, (const bf16*)wimg, bias,
      coef_lse, partials, B, L, chunk, GYB);
}

}  // extern "C"
