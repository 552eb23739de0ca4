// K20: nearest-neighbour search over code vectors.  For every query row of
// q [nq, EP] bf16, the k (<= 16) index rows of db [N, EP] bf16 with the
// largest dot product, WITHOUT writing the [nq, N] score matrix.
//
// Score: score(i, j) = sum_e q[i,e] * db[j,e] by mfma_f32_16x16x32_bf16,
// ONE fp32 accumulator chain per (i, j) over the EP/32 K-steps in ascending
// order, so a score's bits depend on neither grid shape, tile position nor
// the number of index slices.  Order: K19's total order (topk_keys.h):
// descending score, ties to the smallest index row.  An excluded row and
// any row >= N get key 0, the empty slot.
//
// Layout.  Both operands are row-major with K contiguous, which is what the
// gfx950 lane maps want: lane l holds A[row l&15][k = 8(l>>4)+j] and
// B[k = 8(l>>4)+j][col l&15], each fragment ONE aligned 16-B global load —
// no LDS for layout.  Index rows take the M position, queries the N
// position, so by the C map (col = l&15, row = 4(l>>4)+reg) lane l ends up
// with the scores of query l&15 against 4 consecutive index rows.
//
// Stage 1: grid = nsplit * ceil(nq/16) blocks of 256 (slice-major, so the
//   blocks in flight together read the same slice).  A block owns 16
//   queries — their B fragments stay in registers for the whole kernel
//   (EP = 128) — and one contiguous slice of 16-row index tiles; wave w
//   streams tiles w, w+4, ... of the slice with the next tile's loads in
//   flight under the current MFMAs.  Tails are by construction: row and
//   query numbers are clamped to N-1 / nq-1 BEFORE an address is formed,
//   and the clamped duplicates are masked by key (rows) or never written
//   (queries).
//   Selection is threshold-first as in K19: each lane carries the value of
//   its query's current k-th best and does one float compare per score;
//   only when a ballot finds a candidate are keys built and inserted.  A
//   wave keeps 16 sorted lists in four 64-bit registers: list of query
//   4g+r lives in register g, DPP row r, slot = lane & 15, and an insert
//   is K19's  list[j] = max(list[j], min(key, list[j-1]))  on that row.
//   One insert step works on a whole register, so it serves four queries
//   at once, each DPP row fetching its own key by ds_bpermute; there is no
//   per-winner loop.
//   The waves publish their thresholds in LDS as a shared pre-filter (as in
//   K19), so a block inserts about k ln(n/k) keys per query in all, not
//   per wave.  The four waves' lists meet in LDS and are rank-merged per
//   query.
//   nsplit == 1 writes vals/idx directly, otherwise part[nq, nsplit, 16]
//   (a slice's k best keys, the other slots empty).
// Stage 2 (nsplit > 1): one block per query streams its nsplit*16 keys
//   through K19's wave lists and rank-merges the four.
// No atomics, no host sync, bitwise reproducible, capturable.

#include "common.h"
#include "sim_select.h"  // tiles, list inserts, sim_select (shared with K23)

// EPT = 128: query fragments and a double-buffered index tile in registers.
// EPT = 0: generic EP (multiple of 32), fragments loaded per K-step.
template <int EPT>
__global__ __launch_bounds__(256) void sim_topk_stage1_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ db,
    const long* __restrict__ exclude, long nq, long N, int EPr, int nqt,
    int nsplit, long tiles_per_slice, int k, u64* __restrict__ part,
    float* __restrict__ vals, long* __restrict__ idx) {
  const int EP = EPT ? EPT : EPr;
  const int slice = blockIdx.x / nqt;
  const int qt = blockIdx.x % nqt;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int kq = k - 1;
  const long ntile = (N + SIM_ROWS - 1) / SIM_ROWS;
  const long t0 = (long)slice * tiles_per_slice;
  const long t1 = min(ntile, t0 + tiles_per_slice);

  // this lane's query (C column / B column); clamped, never past q's end
  const long qrow = min((long)qt * SIM_QT + (lane & 15), nq - 1);
  const bf16* qp = q + qrow * EP + 8 * (lane >> 4);
  const long excl = exclude ? exclude[qrow] : -1;
  const int koff = 8 * (lane >> 4);

  u64 mine[4] = {0, 0, 0, 0};
  // a lane whose query is past nq (a clamped copy of the last one) starts
  // with an unbeatable threshold: it never offers a candidate
  const bool qvalid = (long)qt * SIM_QT + (lane & 15) < nq;
  u64 tau = qvalid ? 0ull : ~0ull;
  float tau_val = qvalid ? NEG_INF : __builtin_inff();

  __shared__ volatile float s_tau[SIM_QT * 4];
  if (threadIdx.x < SIM_QT * 4) s_tau[threadIdx.x] = NEG_INF;
  __syncthreads();

  if constexpr (EPT == 128) {
    bf16x8 b[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) b[kk] = *(const bf16x8*)(qp + kk * 32);
    bf16x8 a[4];
    long t = t0 + wave;
    {
      // clamped row: a tile past the slice loads a valid row it never uses
      const long r = min(t * SIM_ROWS + (lane & 15), N - 1);
      const bf16* ap = db + r * 128 + koff;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) a[kk] = *(const bf16x8*)(ap + kk * 32);
    }
    for (; t < t1; t += 4) {
      bf16x8 an[4];
      {
        const long r = min((t + 4) * SIM_ROWS + (lane & 15), N - 1);
        const bf16* ap = db + r * 128 + koff;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          an[kk] = *(const bf16x8*)(ap + kk * 32);
      }
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kk], b[kk], acc, 0, 0,
                                                      0);
      sim_select(acc, t * SIM_ROWS + 4 * (lane >> 4), N, excl, kq, mine, tau,
                 tau_val, s_tau);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) a[kk] = an[kk];
    }
  } else {
    const int nk = EP / 32;
    for (long t = t0 + wave; t < t1; t += 4) {
      const long r = min(t * SIM_ROWS + (lane & 15), N - 1);
      const bf16* ap = db + r * EP + koff;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < nk; ++kk) {
        const bf16x8 av = *(const bf16x8*)(ap + kk * 32);
        const bf16x8 bv = *(const bf16x8*)(qp + kk * 32);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
      }
      sim_select(acc, t * SIM_ROWS + 4 * (lane >> 4), N, excl, kq, mine, tau,
                 tau_val, s_tau);
    }
  }

  // sk[query][wave][slot]: the 64 keys of one query are contiguous
  __shared__ u64 sk[SIM_QT * 4 * TOPK_SLOTS];
#pragma unroll
  for (int g = 0; g < 4; ++g)
    sk[((4 * g + (lane >> 4)) * 4 + wave) * TOPK_SLOTS + (lane & 15)] =
        mine[g];
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
  }
}

// one block per query: K19's stage 2 without the log-sum-exp
__global__ __launch_bounds__(256) void sim_topk_stage2_kernel(
    const u64* __restrict__ part, int nsplit, int k,
    float* __restrict__ vals, long* __restrict__ idx) {
  const long row = blockIdx.x;
  const u64* pr = part + row * nsplit * TOPK_SLOTS;
  const long n = (long)nsplit * TOPK_SLOTS;
  const int kq = k - 1;
  u64 mine = 0, tau = 0;
  for (long p0 = 0; p0 < n; p0 += 256) {  // wave-uniform trip count
    const long p = p0 + threadIdx.x;
    const u64 key = p < n ? pr[p] : 0ull;
    wave_push(mine, tau, key, kq);
  }
  __shared__ u64 sk[4 * TOPK_SLOTS];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  if (lane < TOPK_SLOTS) sk[wave * TOPK_SLOTS + lane] = mine;
  __syncthreads();
  if (wave != 0) return;
  u64 my;
  const int rank = block_rank(sk, my);
  if (rank < k) {
    vals[row * k + rank] = topk_key_val(my);
    idx[row * k + rank] = topk_key_col(my);
  }
}

extern "C" {

int sim_topk_query_tile() { return SIM_QT; }
int sim_topk_row_tile() { return SIM_ROWS; }

// q: [nq, EP] bf16, db: [N, EP] bf16, exclude: [nq] i64 or null.  The
// caller checks 1 <= k <= 16, k <= N < 2^31, EP % 32 == 0, nsplit >= 1,
// nsplit * ceil(nq/16) < 2^31, and part >= nq * nsplit * 16 keys when
// nsplit > 1.
void launch_sim_topk(const void* q, const void* db, const long* exclude,
                     long nq, long N, int EP, int k, int nsplit, void* part,
                     float* vals, long* idx, hipStream_t stream) {
  if (nq == 0) return;
  const int nqt = (int)((nq + SIM_QT - 1) / SIM_QT);
  const long ntile = (N + SIM_ROWS - 1) / SIM_ROWS;
  const long tps = (ntile + nsplit - 1) / nsplit;
  const unsigned grid = (unsigned)((long)nsplit * nqt);
  u64* pp = (u64*)part;
  if (EP == 128)
    sim_topk_stage1_kernel<128><<<grid, 256, 0, stream>>>(
        (const bf16*)q, (const bf16*)db, exclude, nq, N, EP, nqt, nsplit, tps,
        k, pp, vals, idx);
  else
    sim_topk_stage1_kernel<0><<<grid, 256, 0, stream>>>(
        (const bf16*)q, (const bf16*)db, exclude, nq, N, EP, nqt, nsplit, tps,
        k, pp, vals, idx);
  if (nsplit > 1)
    sim_topk_stage2_kernel<<<(unsigned)nq, 256, 0, stream>>>(pp, nsplit, k,
                                                             vals, idx);
}

}  // extern "C"
