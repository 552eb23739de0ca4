// K24: similarity range search over code vectors.  For every query row of
// q [nq, EP] bf16, ALL index rows of db [N, EP] bf16 whose dot product is
// at least a threshold t, as a CSR (offsets, rows, scores) with the rows of
// a query strictly ascending, WITHOUT writing the [nq, N] score matrix.
//
// Score: K20's, bit for bit (sim_topk.hip): mfma_f32_16x16x32_bf16 with
// index rows in the M position and queries in the N position, ONE fp32
// accumulator chain per (i, j) over the EP/32 K-steps in ascending order,
// so a score depends on neither the grid, the tile nor the slicing, and a
// row reported here and by sim_topk carries the same float.
//
// Two passes of ONE kernel, sim_range_kernel<EPT, FILL>; the loads and the
// MFMA chain are the same source in both, only what is done with a hit
// differs, so the passes cannot decide differently.
//   grid = nsplit * ceil(nq/16) blocks of 256, slice-major as in K20.  A
//   block owns 16 queries and one contiguous slice of 16-row index tiles;
//   wave w owns the w-th CONTIGUOUS quarter of the slice (K20 interleaves
//   w, w+4, ...; ascending rows without a sort want runs), so the order
//   (query, slice, wave, tile, row) IS ascending row order per query.
//   FILL = false: counts[(query * nsplit + slice) * 4 + wave] = hits, i32.
//   The caller turns the counts into exclusive cursors cur[...] (i64, one
//   more entry than counts: the total) and reads the total back — the op's
//   one host sync — before it allocates rows/scores.
//   FILL = true: lane 16h + c holds query c against rows 4h + j of the
//   tile, so a hit's place among the tile's hits of its query is the
//   number of set bits below it, in (h, j) order, in the four per-j
//   ballots; the wave's cursor advances by the tile's hits.  Every store
//   is bounded by the end of its (query, slice, wave) segment, itself
//   clamped to nnz: passes that disagreed could corrupt a result, never
//   write outside the allocation.
// A hit: row < N, row != exclude[query], row > after[query], query < nq,
// score >= t.  Row and query numbers are clamped to N-1 / nq-1 BEFORE an
// address is formed (K20's tails); the clamped copies are masked.
// ``after`` skips work: tiles wholly at or below the smallest after of the
// block's queries are never loaded, and a block whose slice lies wholly
// there writes zero counts (count pass) or returns at once (fill pass) —
// which halves a self-join (after = own row).
// No atomics, bitwise reproducible, results independent of nsplit.  Not
// capturable: the total is read back between the passes.

#include "common.h"
#include "sim_select.h"  // SIM_QT, SIM_ROWS (K20's tiles)

#define SIM_RANGE_WAVES 4

// bit c of each 16-bit group: query c's lanes in a ballot
#define SIM_RANGE_QMASK 0x0001000100010001ull

template <bool FILL>
struct SimRangeOut {
  int* counts;        // count pass
  const long* cur;    // fill pass: exclusive cursors, numel = counts + 1
  long nnz;
  long* rows;
  float* scores;
};

// One tile's scores: count the hits (count pass) or write them (fill pass).
// row0: the lane's first index row.  cnt: this lane's hits so far (count
// pass); pos: the wave's cursor for the lane's query (fill pass, equal in
// the four lanes of a query).
template <bool FILL>
__device__ __forceinline__ void sim_range_tile(
    const f32x4& s, long row0, long N, long excl, long aft, bool qvalid,
    float thr, int& cnt, long& pos, long seg_end, long* __restrict__ rows,
    float* __restrict__ scores) {
  bool hit[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long r = row0 + j;
    hit[j] = qvalid && r < N && r != excl && r > aft && s[j] >= thr;
  }
  if constexpr (!FILL) {
#pragma unroll
    for (int j = 0; j < 4; ++j) cnt += hit[j] ? 1 : 0;
  } else {
    u64 m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = __ballot(hit[j]);
    if (!(m[0] | m[1] | m[2] | m[3])) return;  // wave-uniform
    const int lane = threadIdx.x & (WAVE - 1);
    const int c = lane & 15;
    const u64 below_h = (1ull << (16 * (lane >> 4))) - 1ull;
    int below = 0, total = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u64 mq = (m[j] >> c) & SIM_RANGE_QMASK;  // query c, bit 16h
      below += __popcll(mq & below_h);
      total += __popcll(mq);
    }
    long p = pos + below;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (hit[j]) {
        if (p >= 0 && p < seg_end) {
          rows[p] = row0 + j;
          scores[p] = s[j];
        }
        ++p;
      }
    }
    pos += total;
  }
}

// EPT = 128: query fragments and a double-buffered index tile in registers.
// EPT = 0: generic EP (multiple of 32), fragments loaded per K-step.
template <int EPT, bool FILL>
__global__ __launch_bounds__(256) void sim_range_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ db,
    const long* __restrict__ exclude, const long* __restrict__ after,
    float thr, long nq, long N, int EPr, int nqt, int nsplit,
    long tiles_per_slice, SimRangeOut<FILL> out) {
  const int EP = EPT ? EPT : EPr;
  const int slice = blockIdx.x / nqt;
  const int qt = blockIdx.x % nqt;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const long ntile = (N + SIM_ROWS - 1) / SIM_ROWS;
  const long t0 = (long)slice * tiles_per_slice;
  const long t1 = min(ntile, t0 + tiles_per_slice);
  const long tpw = (tiles_per_slice + SIM_RANGE_WAVES - 1) / SIM_RANGE_WAVES;

  // this lane's query (C column / B column); clamped, never past q's end
  const long qg = (long)qt * SIM_QT + (lane & 15);
  const bool qvalid = qg < nq;
  const long qrow = min(qg, nq - 1);
  const long excl = exclude ? exclude[qrow] : -1;
  const long aft = after ? after[qrow] : -1;
  // (query, slice, wave) of this lane in counts / cur
  const long seg = (qrow * nsplit + slice) * SIM_RANGE_WAVES + wave;

  // smallest ``after`` of the block's valid queries (a lane past nq holds
  // a copy of the last valid query's): rows <= amin are hits of nobody
  long amin = aft;
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) amin = min(amin, __shfl_xor(amin, off));
  if (t1 * SIM_ROWS - 1 <= amin) {  // block-uniform
    if constexpr (!FILL) {
      if (qvalid && lane < SIM_QT) out.counts[seg] = 0;
    }
    return;
  }
  // the wave's run of tiles, without the tiles wholly <= amin
  long wt0 = t0 + wave * tpw;
  const long wt1 = min(t1, wt0 + tpw);
  if (amin >= 0) wt0 = max(wt0, (amin + 1) / SIM_ROWS);

  const bf16* qp = q + qrow * EP + 8 * (lane >> 4);
  const int koff = 8 * (lane >> 4);
  int cnt = 0;
  long pos = 0, seg_end = 0;
  long* rows = nullptr;
  float* scores = nullptr;
  if constexpr (FILL) {
    pos = out.cur[seg];
    seg_end = min(out.cur[seg + 1], out.nnz);
    rows = out.rows;
    scores = out.scores;
  }

  if constexpr (EPT == 128) {
    if (wt0 < wt1) {
      bf16x8 b[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) b[kk] = *(const bf16x8*)(qp + kk * 32);
      bf16x8 a[4];
      {
        const long r = min(wt0 * SIM_ROWS + (lane & 15), N - 1);
        const bf16* ap = db + r * 128 + koff;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) a[kk] = *(const bf16x8*)(ap + kk * 32);
      }
      for (long t = wt0; t < wt1; ++t) {
        bf16x8 an[4];
        {
          // clamped row: the tile past the run loads a valid row never used
          const long r = min((t + 1) * SIM_ROWS + (lane & 15), N - 1);
          const bf16* ap = db + r * 128 + koff;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
            an[kk] = *(const bf16x8*)(ap + kk * 32);
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kk], b[kk], acc, 0,
                                                        0, 0);
        sim_range_tile<FILL>(acc, t * SIM_ROWS + 4 * (lane >> 4), N, excl,
                             aft, qvalid, thr, cnt, pos, seg_end, rows,
                             scores);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) a[kk] = an[kk];
      }
    }
  } else {
    const int nk = EP / 32;
    for (long t = wt0; t < wt1; ++t) {
      const long r = min(t * SIM_ROWS + (lane & 15), N - 1);
      const bf16* ap = db + r * EP + koff;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int kk = 0; kk < nk; ++kk) {
        const bf16x8 av = *(const bf16x8*)(ap + kk * 32);
        const bf16x8 bv = *(const bf16x8*)(qp + kk * 32);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, acc, 0, 0, 0);
      }
      sim_range_tile<FILL>(acc, t * SIM_ROWS + 4 * (lane >> 4), N, excl, aft,
                           qvalid, thr, cnt, pos, seg_end, rows, scores);
    }
  }

  if constexpr (!FILL) {
    // query c's hits sit in lanes c, c+16, c+32, c+48
    cnt += __shfl_xor(cnt, 16);
    cnt += __shfl_xor(cnt, 32);
    if (qvalid && lane < SIM_QT) out.counts[seg] = cnt;
  }
}

template <bool FILL>
static void sim_range_launch(const void* q, const void* db,
                             const long* exclude, const long* after,
                             float thr, long nq, long N, int EP, int nsplit,
                             SimRangeOut<FILL> out, hipStream_t stream) {
  const int nqt = (int)((nq + SIM_QT - 1) / SIM_QT);
  const long ntile = (N + SIM_ROWS - 1) / SIM_ROWS;
  const long tps = (ntile + nsplit - 1) / nsplit;
  const unsigned grid = (unsigned)((long)nsplit * nqt);
  if (EP == 128)
    sim_range_kernel<128, FILL><<<grid, 256, 0, stream>>>(
        (const bf16*)q, (const bf16*)db, exclude, after, thr, nq, N, EP, nqt,
        nsplit, tps, out);
  else
    sim_range_kernel<0, FILL><<<grid, 256, 0, stream>>>(
        (const bf16*)q, (const bf16*)db, exclude, after, thr, nq, N, EP, nqt,
        nsplit, tps, out);
}

extern "C" {

int sim_range_waves() { return SIM_RANGE_WAVES; }

// q: [nq, EP] bf16, db: [N, EP] bf16, exclude/after: [nq] i64 or null.  The
// caller checks 1 <= N < 2^31, EP % 32 == 0, nsplit >= 1, nsplit *
// ceil(nq/16) < 2^31 and counts = nq * nsplit * 4 i32.
void launch_sim_range_count(const void* q, const void* db,
                            const long* exclude, const long* after, float thr,
                            long nq, long N, int EP, int nsplit, int* counts,
                            hipStream_t stream) {
  if (nq == 0) return;
  SimRangeOut<false> out{counts, nullptr, 0, nullptr, nullptr};
  sim_range_launch<false>(q, db, exclude, after, thr, nq, N, EP, nsplit, out,
                          stream);
}

// cur: nq * nsplit * 4 + 1 exclusive cursors (i64) of the count pass run
// with the SAME arguments; rows/scores hold nnz entries.
void launch_sim_range_fill(const void* q, const void* db, const long* exclude,
                           const long* after, float thr, long nq, long N,
                           int EP, int nsplit, const long* cur, long nnz,
                           long* rows, float* scores, hipStream_t stream) {
  if (nq == 0 || nnz == 0) return;
  SimRangeOut<true> out{nullptr, cur, nnz, rows, scores};
  sim_range_launch<true>(q, db, exclude, after, thr, nq, N, EP, nsplit, out,
                         stream);
}

}  // extern "C"
