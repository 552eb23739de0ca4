// K23: name prediction without the logits matrix.  For every query row of
// q [nq, EP] bf16 (a code vector), the k (<= 16) labels with the largest
//     z(i, l) = scale * sum_e q[i,e] * w[l,e] + bias[l]
// over w [L, EP] bf16, and the log-sum-exp of z(i, :) over ALL L labels,
// WITHOUT writing the [nq, L] matrix.  bias is fp32 [L] or null (0); an
// entry of -inf masks a label: it adds nothing to the lse and sorts below
// every finite logit.
//
// This is K20 (sim_topk.hip) with a head's epilogue; structure, layout and
// selection are K20's and live in sim_select.h.  w rows take the M position
// of mfma_f32_16x16x32_bf16, queries the N position; every fragment is one
// aligned 16-B global load; ONE fp32 chain per (i, l) over ascending K; by
// the C map lane l holds query l&15 against labels row0 .. row0+3,
// row0 = 16 t + 4 (l>>4).  z = fmaf(scale, acc, bias) in fp32, so a logit's
// bits depend on neither grid, tile position nor the number of slices, and
// neither do vals/idx.
//
// Bias: the lane's four consecutive floats are one 16-B load when the base
// is 16-B aligned and all four labels exist, else four loads with the index
// clamped to L-1 — no address past the end is formed.  They are issued with
// the next tile's fragments (EP = 128).  Labels >= L get key 0 and -inf.
//
// Log-sum-exp: every lane keeps an online (max, sumexp) over its own labels
// in ascending tile order (K19's update; all -inf so far stays (-inf, 0)).
// After the stream the four DPP rows that share a query merge by shfl_xor
// 16, 32, then the four waves through LDS in wave order.  nsplit == 1
// writes lse, otherwise pm/ps [nq, nsplit] and K19's stage 2 merges keys
// and pairs (slices in ascending order per thread, then its fixed tree).
// The lse's bits therefore depend on the slicing (tiles per slice) but not
// on nq, on the query's position or on its neighbours.
// No atomics, no host sync, bitwise reproducible, capturable.

#include "common.h"
#include "sim_select.h"

// bias[row0 .. row0+3]; row0 is a multiple of 4
__device__ __forceinline__ f32x4 head_bias4(const float* __restrict__ bias,
                                            long row0, long L, bool vec) {
  f32x4 b = {0.f, 0.f, 0.f, 0.f};
  if (!bias) return b;
  if (vec && row0 + 3 < L) return *(const f32x4*)(bias + row0);
#pragma unroll
  for (int j = 0; j < 4; ++j) b[j] = bias[min(row0 + j, L - 1)];
  return b;
}

// logits of the lane's four labels from the tile's accumulators; labels
// >= L come out as -inf.  Folds them into the lane's online (m, s).
__device__ __forceinline__ f32x4 head_logits(const f32x4& acc,
                                             const f32x4& b, float scale,
                                             long row0, long L, float& m,
                                             float& s) {
  f32x4 z;
  float mv = NEG_INF;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    z[j] = row0 + j < L ? __builtin_fmaf(scale, acc[j], b[j]) : NEG_INF;
    mv = fmaxf(mv, z[j]);
  }
  // online (max, sumexp); skipped while everything seen is -inf
  if (mv > m) {
    s *= __expf(m - mv);
    m = mv;
  }
  if (m > NEG_INF) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s += __expf(z[j] - m);
  }
  return z;
}

// EPT = 128: query fragments and a double-buffered label tile in registers.
// EPT = 0: generic EP (multiple of 32), fragments loaded per K-step.
// At least 4 waves per SIMD (K20's occupancy): without the bound the
// EP = 128 variant takes 126 VGPRs + 4 AGPRs and drops to 3; with it the
// accumulators stay in VGPRs and it fits 128 with no spill.
template <int EPT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
void head_topk_stage1_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ w,
    const float* __restrict__ bias, float scale, long nq, long L, int EPr,
    int nqt, int nsplit, long tiles_per_slice, int k, u64* __restrict__ part,
    float* __restrict__ pm, float* __restrict__ ps, float* __restrict__ vals,
    long* __restrict__ idx, float* __restrict__ lse) {
  const int EP = EPT ? EPT : EPr;
  const int slice = blockIdx.x / nqt;
  const int qt = blockIdx.x % nqt;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int kq = k - 1;
  const long ntile = (L + SIM_ROWS - 1) / SIM_ROWS;
  const long t0 = (long)slice * tiles_per_slice;
  const long t1 = min(ntile, t0 + tiles_per_slice);
  const bool bvec = ((unsigned long long)bias & 15ull) == 0;

  // this lane's query (C column / B column); clamped, never past q's end
  const long qrow = min((long)qt * SIM_QT + (lane & 15), nq - 1);
  const bf16* qp = q + qrow * EP + 8 * (lane >> 4);
  const int koff = 8 * (lane >> 4);
  const int lrow = 4 * (lane >> 4);

  u64 mine[4] = {0, 0, 0, 0};
  // a lane whose query is past nq (a clamped copy of the last one) starts
  // with an unbeatable threshold: it never offers a candidate
  const bool qvalid = (long)qt * SIM_QT + (lane & 15) < nq;
  u64 tau = qvalid ? 0ull : ~0ull;
  float tau_val = qvalid ? NEG_INF : __builtin_inff();
  float m = NEG_INF, s = 0.f;

  __shared__ volatile float s_tau[SIM_QT * 4];
  if (threadIdx.x < SIM_QT * 4) s_tau[threadIdx.x] = NEG_INF;
  __syncthreads();

  if constexpr (EPT == 128) {
    bf16x8 b[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) b[kk] = *(const bf16x8*)(qp + kk * 32);
    bf16x8 a[4];
    f32x4 bz;
    long t = t0 + wave;
    {
      // clamped row: a tile past the slice loads a valid row it never uses
      const long r = min(t * SIM_ROWS + (lane & 15), L - 1);
      const bf16* ap = w + r * 128 + koff;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) a[kk] = *(const bf16x8*)(ap + kk * 32);
      bz = head_bias4(bias, t * SIM_ROWS + lrow, L, bvec);
    }
    for (; t < t1; t += 4) {
      bf16x8 an[4];
      const long rn = min((t + 4) * SIM_ROWS + (lane & 15), L - 1);
      const bf16* ap = w + rn * 128 + koff;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) an[kk] = *(const bf16x8*)(ap + kk * 32);
      const f32x4 bn = head_bias4(bias, (t + 4) * SIM_ROWS + lrow, L, bvec);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kk], b[kk], acc, 0, 0,
                                                      0);
      const long row0 = t * SIM_ROWS + lrow;
      const f32x4 z = head_logits(acc, bz, scale, row0, L, m, s);
      sim_select(z, row0, L, -1, kq, mine, tau, tau_val, s_tau);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) a[kk] = an[kk];
      bz = bn;
    }
  } else {
    const int nk = EP / 32;
    for (long t = t0 + wave; t < t1; t += 4) {
      const long r = min(t * SIM_ROWS + (lane & 15), L - 1);
      const bf16* ap = w + r * EP + koff;
      const long row0 = t * SIM_ROWS + lrow;
      const f32x4 bz = head_bias4(bias, row0, L, bvec);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < nk; ++kk) {
        const bf16x8 av = *(const bf16x8*)(ap + kk * 32);
        const bf16x8 bv = *(const bf16x8*)(qp + kk * 32);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
      }
      const f32x4 z = head_logits(acc, bz, scale, row0, L, m, s);
      sim_select(z, row0, L, -1, kq, mine, tau, tau_val, s_tau);
    }
  }

  // the four DPP rows of a wave hold disjoint labels of the same query
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const float om = __shfl_xor(m, off);
    const float os = __shfl_xor(s, off);
    lse_merge(m, s, om, os);
  }

  // sk[query][wave][slot]: the 64 keys of one query are contiguous
  __shared__ u64 sk[SIM_QT * 4 * TOPK_SLOTS];
  __shared__ float sm[4 * SIM_QT], ss[4 * SIM_QT];
#pragma unroll
  for (int g = 0; g < 4; ++g)
    sk[((4 * g + (lane >> 4)) * 4 + wave) * TOPK_SLOTS + (lane & 15)] =
        mine[g];
  if (lane < SIM_QT) {
    sm[wave * SIM_QT + lane] = m;
    ss[wave * SIM_QT + lane] = s;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ql = 4 * wave + j;
    const long qg = (long)qt * SIM_QT + ql;
    u64 my;
    const int rank = block_rank(sk + ql * 4 * TOPK_SLOTS, my);
    if (qg >= nq) continue;
    if (nsplit == 1) {
      if (rank < k) {
        vals[qg * k + rank] = topk_key_val(my);
        idx[qg * k + rank] = topk_key_col(my);
      }
    } else if (rank < TOPK_SLOTS) {
      // only the slice's k best can matter; the rest go as empty slots,
      // which stage 2 skips without an insert
      part[(qg * nsplit + slice) * TOPK_SLOTS + rank] = rank < k ? my : 0ull;
    }
    if (lane == 0) {
      float bm = sm[ql], bs = ss[ql];
      for (int wv = 1; wv < 4; ++wv)
        lse_merge(bm, bs, sm[wv * SIM_QT + ql], ss[wv * SIM_QT + ql]);
      if (nsplit == 1) {
        lse[qg] = bm == NEG_INF ? NEG_INF : bm + logf(bs);
      } else {
        pm[qg * nsplit + slice] = bm;
        ps[qg * nsplit + slice] = bs;
      }
    }
  }
}

extern "C" {

void launch_row_topk_stage2(const void*, const float*, const float*, long,
                            int, int, float*, long*, float*, hipStream_t);

// q: [nq, EP] bf16, w: [L, EP] bf16, bias: [L] f32 or null.  The caller
// checks 1 <= k <= 16, k <= L < 2^31, EP % 32 == 0, nsplit >= 1,
// nsplit * ceil(nq/16) < 2^31, and part >= nq * nsplit * 16 keys and
// pm/ps >= nq * nsplit floats when nsplit > 1.  The tiles are K20's
// (sim_topk_query_tile / sim_topk_row_tile).
void launch_head_topk(const void* q, const void* w, const float* bias,
                      float scale, long nq, long L, int EP, int k, int nsplit,
                      void* part, float* pm, float* ps, float* vals,
                      long* idx, float* lse, hipStream_t stream) {
  if (nq == 0) return;
  const int nqt = (int)((nq + SIM_QT - 1) / SIM_QT);
  const long ntile = (L + SIM_ROWS - 1) / SIM_ROWS;
  const long tps = (ntile + nsplit - 1) / nsplit;
  const unsigned grid = (unsigned)((long)nsplit * nqt);
  u64* pp = (u64*)part;
  if (EP == 128)
    head_topk_stage1_kernel<128><<<grid, 256, 0, stream>>>(
        (const bf16*)q, (const bf16*)w, bias, scale, nq, L, EP, nqt, nsplit,
        tps, k, pp, pm, ps, vals, idx, lse);
  else
    head_topk_stage1_kernel<0><<<grid, 256, 0, stream>>>(
        (const bf16*)q, (const bf16*)w, bias, scale, nq, L, EP, nqt, nsplit,
        tps, k, pp, pm, ps, vals, idx, lse);
  if (nsplit > 1)
    launch_row_topk_stage2(pp, pm, ps, nq, nsplit, k, vals, idx, lse, stream);
}

}  // extern "C"
