// Counting sort of BOTH embedding tables' index lists in one chain of four
// launches, plus the both-tables forms of the table Adam's heavy-row
// pre-pass and histogram clear.  Two chains build the same records: the
// two-level sort by LDS buckets (count, offsets, partition, finish: the
// default, second half of this file) and the global-atomic chain it
// replaced (count, scan partials, scan apply, group: C2V_GROUP_SORT=0).
//
// The term table's list is [starts | ends] (entry o < M is starts[o], else
// ends[o - M]: the numbering embed_scatter_* and adam_table_bf16 expect) and
// is read from the two tensors in place; the path table's list is paths.
// Every kernel covers the term table with its first blocks and the path
// table with the rest, so a wave never straddles the two and the ballot
// aggregation of indices 0 (<PAD/>) and 1 (@question) stays per table.
// Record contents equal two count/scan/scatter_group chains of
// gather_concat.hip; within-run order is decided by the cursor atomics and
// stays unspecified.

#include "common.h"
#include "scatter_heavy.h"

#define IG_BLOCK 256
#define IG_SCAN 1024  // histogram rows per scan block
// E (template parameter of the count and group kernels): entries per
// thread; a block covers IG_BLOCK * E consecutive entries.

struct GroupTable {
  const int* idx0;   // entries [0, split)
  const int* idx1;   // entries [split, N)
  long split, N;
  int rows;          // histogram length (table rows + 1)
  int* counts;
  int* cursor;
  int* sorted_idx;
  long* perm;
};

// A block's E x 256 entries, lane-consecutive per load so each of the E
// loads is coalesced; all are issued before the caller's first atomic.
// Entries past N, and indices outside the histogram, come back as -1.
template <int E>
__device__ __forceinline__ void load_entries(const GroupTable& t, long base,
                                             int (&v)[E]) {
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const long e = base + j * IG_BLOCK + threadIdx.x;
    int x = -1;
    if (e < t.N) x = e < t.split ? t.idx0[e] : t.idx1[e - t.split];
    v[j] = (unsigned)x < (unsigned)t.rows ? x : -1;
  }
}

template <int E>
__global__ __launch_bounds__(IG_BLOCK) void group_count_pair_kernel(
    GroupTable term, GroupTable path, int term_blocks) {
  const bool is_path = (int)blockIdx.x >= term_blocks;
  const GroupTable& t = is_path ? path : term;
  const long base =
      (long)((int)blockIdx.x - (is_path ? term_blocks : 0)) * (IG_BLOCK * E);
  const int lane = threadIdx.x & (WAVE - 1);
  int v[E];
  load_entries<E>(t, base, v);
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const unsigned long long m0 = __ballot(v[j] == 0);
    const unsigned long long m1 = __ballot(v[j] == 1);
    if (v[j] < 0) continue;
    if (v[j] <= 1) {
      const unsigned long long m = v[j] == 0 ? m0 : m1;
      if (lane == __ffsll((long long)m) - 1)
        atomicAdd(&t.counts[v[j]], __popcll(m));
    } else {
      atomicAdd(&t.counts[v[j]], 1);
    }
  }
}

template <int E>
__global__ __launch_bounds__(IG_BLOCK) void group_scatter_pair_kernel(
    GroupTable term, GroupTable path, int term_blocks) {
  const bool is_path = (int)blockIdx.x >= term_blocks;
  const GroupTable& t = is_path ? path : term;
  const long base =
      (long)((int)blockIdx.x - (is_path ? term_blocks : 0)) * (IG_BLOCK * E);
  const int lane = threadIdx.x & (WAVE - 1);
  int v[E];
  load_entries<E>(t, base, v);
  int pos[E];
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const unsigned long long m0 = __ballot(v[j] == 0);
    const unsigned long long m1 = __ballot(v[j] == 1);
    pos[j] = -1;
    if (v[j] >= 0 && v[j] <= 1) {
      const unsigned long long m = v[j] == 0 ? m0 : m1;
      const int leader = __ffsll((long long)m) - 1;
      const int rank = (int)__popcll(m & ((1ull << lane) - 1));
      int b = 0;
      if (lane == leader) b = atomicAdd(&t.cursor[v[j]], (int)__popcll(m));
      // every lane of the mask is active here, the leader among them
      pos[j] = __shfl(b, leader) + rank;
    } else if (v[j] > 1) {
      pos[j] = atomicAdd(&t.cursor[v[j]], 1);
    }
  }
#pragma unroll
  for (int j = 0; j < E; ++j) {
    // a position outside [0, N) can only come from a histogram that was
    // not all-zero going in: never follow it out of bounds
    if (v[j] >= 0 && (unsigned long)pos[j] < (unsigned long)t.N) {
      t.sorted_idx[pos[j]] = v[j];
      t.perm[pos[j]] = base + j * IG_BLOCK + threadIdx.x;
    }
  }
}

// ---------------------------------------------------------------------------
// Exclusive scan of the two histograms, two launches for both: per-block
// sums of IG_SCAN rows, then every block adds up the sums in front of it in
// its own segment (at most a few thousand L2-resident ints, cheaper than a
// spine launch in between) and scans its rows.
__device__ __forceinline__ int block_sum(int v, int* red) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();  // red may still be read from a previous call
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(IG_BLOCK) void group_scan_partials_kernel(
    const int* __restrict__ counts_t, int rows_t, const int* __restrict__ counts_p,
    int rows_p, int term_blocks, int* __restrict__ partial) {
  const bool is_path = (int)blockIdx.x >= term_blocks;
  const int* x = is_path ? counts_p : counts_t;
  const int n = is_path ? rows_p : rows_t;
  const int b0 = ((int)blockIdx.x - (is_path ? term_blocks : 0)) * IG_SCAN;
  int v = 0;
#pragma unroll
  for (int k = 0; k < IG_SCAN / IG_BLOCK; ++k) {
    const int i = b0 + k * IG_BLOCK + threadIdx.x;
    v += i < n ? x[i] : 0;
  }
  __shared__ int red[IG_BLOCK / WAVE];
  const int s = block_sum(v, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(IG_BLOCK) void group_scan_apply_kernel(
    const int* __restrict__ counts_t, int rows_t, const int* __restrict__ counts_p,
    int rows_p, int term_blocks, const int* __restrict__ partial,
    int* __restrict__ cursor_t, int* __restrict__ cursor_p) {
  const bool is_path = (int)blockIdx.x >= term_blocks;
  const int* x = is_path ? counts_p : counts_t;
  int* out = is_path ? cursor_p : cursor_t;
  const int n = is_path ? rows_p : rows_t;
  const int seg0 = is_path ? term_blocks : 0;
  const int lb = (int)blockIdx.x - seg0;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  __shared__ int red[IG_BLOCK / WAVE];
  // this thread's 4 consecutive rows (in flight while the prefix reduces)
  const int i0 = lb * IG_SCAN + threadIdx.x * 4;
  int c[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) c[k] = i0 + k < n ? x[i0 + k] : 0;
  int pre = 0;
  for (int i = threadIdx.x; i < lb; i += IG_BLOCK) pre += partial[seg0 + i];
  const int prefix = block_sum(pre, red);
  // inclusive scan of the thread sums across the wave, then across waves
  const int tsum = c[0] + c[1] + c[2] + c[3];
  int inc = tsum;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int up = __shfl_up(inc, off);
    if (lane >= off) inc += up;
  }
  __shared__ int wtot[IG_BLOCK / WAVE];
  if (lane == WAVE - 1) wtot[wave] = inc;
  __syncthreads();
  int run = prefix + inc - tsum;
  for (int w = 0; w < wave; ++w) run += wtot[w];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i0 + k < n) out[i0 + k] = run;
    run += c[k];
  }
}

// ---------------------------------------------------------------------------
// Two-level sort (the default chain): the same records with no global atomic
// and no scan over the histogram's rows.  Entries are first partitioned into
// buckets of R = 2^logr consecutive rows, then one block per bucket counts,
// scans and places its entries in LDS.
//
// Columns: 0 = row 0 (<PAD/>), 1 = row 1 (@question), 2 + k = bucket k
// without those two rows; in that order they tile [0, N) of the sorted
// arrays.  The two hot rows never reach a bucket, so a ragged batch does
// not pile half its entries into bucket 0.
//   count:     per block an LDS histogram over the columns of its tile,
//              stored as row `block` of mat[blocks][nbx]
//   offsets:   mat[b][c] <- start of block b's share of column c (block-
//              major within a column), bbase[c] <- start of column c,
//              bbase[nbx] <- number of kept entries
//   partition: re-reads the tile; columns 0/1 go to their final place,
//              the rest as (idx, entry) pairs to tmp[] at the same position
//   finish:    bucket k reads tmp[bbase[2+k] .. bbase[3+k]), writes counts
//              and cursor of its R rows and the final sorted_idx / perm
// Every position is checked against [0, N) (finish: against the bucket's
// clamped range) before it is used as an address, and every column against
// nbx: as in the chain above, a broken precondition may give a wrong
// grouping but no access out of range.
#define IG_MAXB 2048       // buckets per table the LDS images are sized for
#define IG_FIN_BLOCK 512   // threads of a finish block
#define IG_FIN_U 4         // pairs in flight per finish thread

__device__ __forceinline__ int group_column(int v, int logr, int nbx) {
  const int c = 2 + (v >> logr);
  return c < nbx ? c : nbx - 1;
}

template <int E>
__global__ __launch_bounds__(IG_BLOCK) void group_bucket_count_kernel(
    GroupTable term, GroupTable path, int term_blocks, int logr,
    int* __restrict__ mat_t, int nbx_t, int* __restrict__ mat_p, int nbx_p) {
  const bool is_path = (int)blockIdx.x >= term_blocks;
  const GroupTable& t = is_path ? path : term;
  const int lb = (int)blockIdx.x - (is_path ? term_blocks : 0);
  const int nbx = is_path ? nbx_p : nbx_t;
  int* row = (is_path ? mat_p : mat_t) + (long)lb * nbx;
  const int lane = threadIdx.x & (WAVE - 1);
  __shared__ int hist[IG_MAXB + 2];
  int v[E];
  load_entries<E>(t, (long)lb * (IG_BLOCK * E), v);
  for (int c = threadIdx.x; c < nbx; c += IG_BLOCK) hist[c] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const unsigned long long m0 = __ballot(v[j] == 0);
    const unsigned long long m1 = __ballot(v[j] == 1);
    if (v[j] > 1) {
      atomicAdd(&hist[group_column(v[j], logr, nbx)], 1);
    } else if (v[j] >= 0) {
      const unsigned long long m = v[j] == 0 ? m0 : m1;
      if (lane == __ffsll((long long)m) - 1)
        atomicAdd(&hist[v[j]], (int)__popcll(m));
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nbx; c += IG_BLOCK) row[c] = hist[c];
}

// One block per table.  Thread (g, cl) of 4 x 256 walks the rows of block
// group g in column cl, cl + 256, ...: every load of a walk is independent
// and coalesced across cl.
__global__ __launch_bounds__(1024) void group_bucket_offsets_kernel(
    int* __restrict__ mat_t, int blocks_t, int nbx_t, int* __restrict__ bbase_t,
    int* __restrict__ mat_p, int blocks_p, int nbx_p,
    int* __restrict__ bbase_p) {
  const bool is_path = blockIdx.x != 0;
  int* mat = is_path ? mat_p : mat_t;
  int* bbase = is_path ? bbase_p : bbase_t;
  const int nblk = is_path ? blocks_p : blocks_t;
  const int nbx = is_path ? nbx_p : nbx_t;
  constexpr int CPT = (IG_MAXB + 2 + 1023) / 1024;  // columns per thread
  __shared__ int part[4][IG_MAXB + 2];
  __shared__ int wtot[1024 / WAVE];
  const int g = threadIdx.x >> 8, cl = threadIdx.x & 255;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int per = (nblk + 3) / 4;
  const int r0 = min(g * per, nblk), r1 = min(r0 + per, nblk);
  for (int c = cl; c < nbx; c += 256) {
    int s = 0;
#pragma unroll 8
    for (int b = r0; b < r1; ++b) s += mat[(long)b * nbx + c];
    part[g][c] = s;
  }
  __syncthreads();
  // exclusive scan over the columns, CPT consecutive ones per thread
  int tot[CPT], tsum = 0;
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int c = threadIdx.x * CPT + j;
    tot[j] = c < nbx ? part[0][c] + part[1][c] + part[2][c] + part[3][c] : 0;
    tsum += tot[j];
  }
  int inc = tsum;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int up = __shfl_up(inc, off);
    if (lane >= off) inc += up;
  }
  if (lane == WAVE - 1) wtot[wave] = inc;
  __syncthreads();
  int run = inc - tsum;
  for (int w = 0; w < wave; ++w) run += wtot[w];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int c = threadIdx.x * CPT + j;
    if (c < nbx) {
      bbase[c] = run;
      if (c == nbx - 1) bbase[nbx] = run + tot[j];
      int acc = run;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int x = part[q][c];
        part[q][c] = acc;
        acc += x;
      }
    }
    run += tot[j];
  }
  __syncthreads();
  // in place, eight rows at a time: a load cannot pass an earlier store to
  // mat, so one row at a time would pay a round trip per row
  for (int c = cl; c < nbx; c += 256) {
    int acc = part[g][c];
    for (int b = r0; b < r1; b += 8) {
      int x[8];
#pragma unroll
      for (int q = 0; q < 8; ++q)
        x[q] = b + q < r1 ? mat[(long)(b + q) * nbx + c] : 0;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (b + q < r1) mat[(long)(b + q) * nbx + c] = acc;
        acc += x[q];
      }
    }
  }
}

template <int E>
__global__ __launch_bounds__(IG_BLOCK) void group_partition_kernel(
    GroupTable term, GroupTable path, int term_blocks, int logr,
    const int* __restrict__ mat_t, int nbx_t, int2* __restrict__ tmp_t,
    const int* __restrict__ mat_p, int nbx_p, int2* __restrict__ tmp_p) {
  const bool is_path = (int)blockIdx.x >= term_blocks;
  const GroupTable& t = is_path ? path : term;
  const int lb = (int)blockIdx.x - (is_path ? term_blocks : 0);
  const int nbx = is_path ? nbx_p : nbx_t;
  const int* row = (is_path ? mat_p : mat_t) + (long)lb * nbx;
  int2* tmp = is_path ? tmp_p : tmp_t;
  const long base = (long)lb * (IG_BLOCK * E);
  const int lane = threadIdx.x & (WAVE - 1);
  __shared__ int cur[IG_MAXB + 2];
  int v[E];
  load_entries<E>(t, base, v);
  for (int c = threadIdx.x; c < nbx; c += IG_BLOCK) cur[c] = row[c];
  __syncthreads();
  int pos[E];
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const unsigned long long m0 = __ballot(v[j] == 0);
    const unsigned long long m1 = __ballot(v[j] == 1);
    pos[j] = -1;
    if (v[j] > 1) {
      pos[j] = atomicAdd(&cur[group_column(v[j], logr, nbx)], 1);
    } else if (v[j] >= 0) {
      const unsigned long long m = v[j] == 0 ? m0 : m1;
      const int leader = __ffsll((long long)m) - 1;
      const int rank = (int)__popcll(m & ((1ull << lane) - 1));
      int b = 0;
      if (lane == leader) b = atomicAdd(&cur[v[j]], (int)__popcll(m));
      // every lane of the mask is active here, the leader among them
      pos[j] = __shfl(b, leader) + rank;
    }
  }
#pragma unroll
  for (int j = 0; j < E; ++j) {
    if (v[j] >= 0 && (unsigned long)pos[j] < (unsigned long)t.N) {
      const long e = base + j * IG_BLOCK + threadIdx.x;
      if (v[j] <= 1) {
        t.sorted_idx[pos[j]] = v[j];
        t.perm[pos[j]] = e;
      } else {
        tmp[pos[j]] = make_int2(v[j], (int)e);  // e < N < 2^31
      }
    }
  }
}

// One block per bucket.  The LDS image holds NC interleaved copies of the
// bucket's histogram (h[r * NC + copy], copy = lane % NC): a row that takes
// a large share of the entries would otherwise serialize the whole bucket
// on one LDS address.  Both passes walk tmp[] identically, so an entry meets
// the same copy in both.
template <int LOGR, int NC>
__global__ __launch_bounds__(IG_FIN_BLOCK) void group_bucket_finish_kernel(
    GroupTable term, GroupTable path, int term_buckets,
    const int* __restrict__ bbase_t, const int2* __restrict__ tmp_t,
    const int* __restrict__ bbase_p, const int2* __restrict__ tmp_p) {
  constexpr int R = 1 << LOGR;
  constexpr int RPT = R / IG_FIN_BLOCK;  // rows per thread in the scan
  const bool is_path = (int)blockIdx.x >= term_buckets;
  const GroupTable& t = is_path ? path : term;
  const int k = (int)blockIdx.x - (is_path ? term_buckets : 0);
  const int* bbase = is_path ? bbase_p : bbase_t;
  const int2* tmp = is_path ? tmp_p : tmp_t;
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int copy = lane & (NC - 1);
  const int row0 = k << LOGR;
  __shared__ int h[R * NC];
  __shared__ int wtot[IG_FIN_BLOCK / WAVE];
  const int N = (int)t.N;
  const int b0 = min(max(bbase[2 + k], 0), N);
  const int b1 = min(max(bbase[3 + k], b0), N);
  for (int i = threadIdx.x; i < R * NC; i += IG_FIN_BLOCK) h[i] = 0;
  __syncthreads();
  for (long i0 = b0; i0 < b1; i0 += IG_FIN_BLOCK * IG_FIN_U) {
    int2 x[IG_FIN_U];
#pragma unroll
    for (int j = 0; j < IG_FIN_U; ++j) {
      const long i = i0 + j * IG_FIN_BLOCK + threadIdx.x;
      x[j] = i < b1 ? tmp[i] : make_int2(-1, 0);
    }
#pragma unroll
    for (int j = 0; j < IG_FIN_U; ++j) {
      const int r = x[j].x - row0;
      if ((unsigned)r < (unsigned)R) atomicAdd(&h[r * NC + copy], 1);
    }
  }
  __syncthreads();
  int rc[RPT], tsum = 0;
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const int r = threadIdx.x * RPT + j;
    int s = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) s += h[r * NC + c];
    rc[j] = s;
    tsum += s;
  }
  int inc = tsum;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int up = __shfl_up(inc, off);
    if (lane >= off) inc += up;
  }
  if (lane == WAVE - 1) wtot[wave] = inc;
  __syncthreads();
  int run = b0 + inc - tsum;
  for (int w = 0; w < wave; ++w) run += wtot[w];
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const int r = threadIdx.x * RPT + j;
    int acc = run;  // the copies' cursors: consecutive shares of the run
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int x = h[r * NC + c];
      h[r * NC + c] = acc;
      acc += x;
    }
    run += rc[j];
    int cnt = rc[j], end = run;
    if (k == 0 && r <= 1) {  // rows 0 and 1 are columns of their own
      cnt = bbase[r + 1] - bbase[r];
      end = bbase[r + 1];
    }
    if (row0 + r < t.rows) {
      t.counts[row0 + r] = cnt;
      t.cursor[row0 + r] = end;
    }
  }
  __syncthreads();
  for (long i0 = b0; i0 < b1; i0 += IG_FIN_BLOCK * IG_FIN_U) {
    int2 x[IG_FIN_U];
#pragma unroll
    for (int j = 0; j < IG_FIN_U; ++j) {
      const long i = i0 + j * IG_FIN_BLOCK + threadIdx.x;
      x[j] = i < b1 ? tmp[i] : make_int2(-1, 0);
    }
#pragma unroll
    for (int j = 0; j < IG_FIN_U; ++j) {
      const int r = x[j].x - row0;
      if ((unsigned)r < (unsigned)R) {
        const int pos = atomicAdd(&h[r * NC + copy], 1);
        if (pos >= b0 && pos < b1) {
          t.sorted_idx[pos] = x[j].x;
          t.perm[pos] = x[j].y;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Both tables' heavy-row pre-pass (scatter_heavy.h) in one launch.
struct HeavyTable {
  const int* sorted_idx;
  const long* perm;
  const int* counts;
  float* dtable;
  long N;
  int S, off0, off1;
};

template <int NP>
__global__ __launch_bounds__(256) void embed_scatter_heavy_pair_kernel(
    HeavyTable term, HeavyTable path, int term_blocks,
    const bf16* __restrict__ gout, long M, int KP, int thr) {
  const bool is_path = (int)blockIdx.x >= term_blocks;
  const HeavyTable& t = is_path ? path : term;
  const long wid =
      (long)((int)blockIdx.x - (is_path ? term_blocks : 0)) *
          (blockDim.x / WAVE) + threadIdx.x / WAVE;
  scatter_heavy_chunk<NP>(wid, t.sorted_idx, t.perm, t.counts, gout, t.dtable,
                          t.N, M, KP, t.S, t.off0, t.off1, thr);
}

__global__ void clear_i32_pair_kernel(int* __restrict__ a, long na,
                                      int* __restrict__ b, long nb) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long j = i; j < na + nb; j += stride) {
    if (j < na) a[j] = 0;
    else b[j - na] = 0;
  }
}

extern "C" {

// Smallest bucket (rows) and tile (entries) the switches below can select:
// the scratch lengths are sized for them, so they cover every setting.
#define IG_MIN_R 1024
#define IG_MIN_TILE 1024

// `partial` length group_tables needs for histograms of these lengths: the
// four-kernel chain's scan sums, or the two-level sort's column starts
// (buckets + 3 per table).
long group_tables_partials(long rows_t, long rows_p) {
  return (rows_t + IG_SCAN - 1) / IG_SCAN + (rows_p + IG_SCAN - 1) / IG_SCAN +
         8;
}

// `tmp` length (ints) the two-level sort needs for M contexts: the (idx,
// entry) pairs of both tables, then the blocks x columns count matrices.
// Grows with M, so a buffer sized for a row capacity serves every smaller M.
long group_tables_tmp(long M, long rows_t, long rows_p) {
  const long bt = (2 * M + IG_MIN_TILE - 1) / IG_MIN_TILE;
  const long bp = (M + IG_MIN_TILE - 1) / IG_MIN_TILE;
  const long ct = (rows_t + IG_MIN_R - 1) / IG_MIN_R + 2;
  const long cp = (rows_p + IG_MIN_R - 1) / IG_MIN_R + 2;
  return 6 * M + bt * ct + bp * cp;
}

static int group_env(const char* name, int a, int b, int c, int dflt) {
  const char* e = getenv(name);
  const int x = e ? atoi(e) : dflt;
  return x == a || x == b || x == c ? x : dflt;
}

// counts_*: all-zero going in, the histograms coming out; cursor_* end at
// each run's END; sorted_*/perm_* hold 2M / M entries.  tmp (at least
// group_tables_tmp ints, 8-byte aligned) selects the two-level sort; without
// it, with C2V_GROUP_SORT=0 or with more than IG_MAXB buckets in a table the
// four-kernel chain runs.  The switches are read per call so that one
// process can compare the settings.
void launch_group_tables(const int* starts, const int* paths, const int* ends,
                         long M, int rows_t, int rows_p, int* counts_t,
                         int* counts_p, int* cursor_t, int* cursor_p,
                         int* partial, int* sorted_t, long* perm_t,
                         int* sorted_p, long* perm_p, int* tmp,
                         hipStream_t stream) {
  if (M <= 0) return;
  GroupTable term = {starts, ends, M, 2 * M, rows_t, counts_t, cursor_t,
                     sorted_t, perm_t};
  GroupTable path = {paths, paths, M, M, rows_p, counts_p, cursor_p,
                     sorted_p, perm_p};
  // rows per bucket and entries per count/partition block, swept on
  // hardware (kbench group_tables, PERF.md)
  const int R = group_env("C2V_GROUP_R", 1024, 2048, 4096, 2048);
  const int logr = R == 1024 ? 10 : R == 2048 ? 11 : 12;
  const int nb_t = (int)(((long)rows_t + R - 1) >> logr);
  const int nb_p = (int)(((long)rows_p + R - 1) >> logr);
  if (tmp != nullptr && group_env("C2V_GROUP_SORT", 0, 1, 1, 1) == 1 &&
      nb_t <= IG_MAXB && nb_p <= IG_MAXB) {
    const int tile = group_env("C2V_GROUP_TILE", 1024, 2048, 4096, 4096);
    const int tb = (int)((2 * M + tile - 1) / tile);
    const int pb = (int)((M + tile - 1) / tile);
    const int nbx_t = nb_t + 2, nbx_p = nb_p + 2;
    int2* tmp_t = (int2*)tmp;
    int2* tmp_p = tmp_t + 2 * M;
    int* mat_t = tmp + 6 * M;
    int* mat_p = mat_t + (long)tb * nbx_t;
    int* bbase_t = partial;
    int* bbase_p = partial + nbx_t + 1;
#define IG_TILE_LAUNCH(kernel, ...)                                           \
  do {                                                                        \
    if (tile == 1024)                                                         \
      kernel<4><<<tb + pb, IG_BLOCK, 0, stream>>>(term, path, tb, logr,       \
                                                  __VA_ARGS__);               \
    else if (tile == 2048)                                                    \
      kernel<8><<<tb + pb, IG_BLOCK, 0, stream>>>(term, path, tb, logr,       \
                                                  __VA_ARGS__);               \
    else                                                                      \
      kernel<16><<<tb + pb, IG_BLOCK, 0, stream>>>(term, path, tb, logr,      \
                                                   __VA_ARGS__);              \
  } while (0)
    IG_TILE_LAUNCH(group_bucket_count_kernel, mat_t, nbx_t, mat_p, nbx_p);
    group_bucket_offsets_kernel<<<2, 1024, 0, stream>>>(
        mat_t, tb, nbx_t, bbase_t, mat_p, pb, nbx_p, bbase_p);
    IG_TILE_LAUNCH(group_partition_kernel, mat_t, nbx_t, tmp_t, mat_p, nbx_p,
                   tmp_p);
#undef IG_TILE_LAUNCH
#define IG_FIN_LAUNCH(lr, nc)                                                 \
  group_bucket_finish_kernel<lr, nc>                                          \
      <<<nb_t + nb_p, IG_FIN_BLOCK, 0, stream>>>(term, path, nb_t, bbase_t,   \
                                                 tmp_t, bbase_p, tmp_p)
    if (logr == 10) IG_FIN_LAUNCH(10, 8);
    else if (logr == 11) IG_FIN_LAUNCH(11, 8);
    else IG_FIN_LAUNCH(12, 4);
#undef IG_FIN_LAUNCH
    return;
  }
  // entries per thread of the four-kernel chain, swept on hardware (PERF.md):
  // 2 beats 4 and 1; C2V_GROUP_E=1/4 select the others
  static const char* ee = getenv("C2V_GROUP_E");
  const int E = ee && (atoi(ee) == 1 || atoi(ee) == 4) ? atoi(ee) : 2;
  const long tile = (long)IG_BLOCK * E;
  const int tb = (int)((2 * M + tile - 1) / tile);
  const int pb = (int)((M + tile - 1) / tile);
  const int st = (rows_t + IG_SCAN - 1) / IG_SCAN;
  const int sp = (rows_p + IG_SCAN - 1) / IG_SCAN;
#define IG_LAUNCH(kernel)                                                     \
  do {                                                                        \
    if (E == 1)                                                               \
      kernel<1><<<tb + pb, IG_BLOCK, 0, stream>>>(term, path, tb);            \
    else if (E == 2)                                                          \
      kernel<2><<<tb + pb, IG_BLOCK, 0, stream>>>(term, path, tb);            \
    else                                                                      \
      kernel<4><<<tb + pb, IG_BLOCK, 0, stream>>>(term, path, tb);            \
  } while (0)
  IG_LAUNCH(group_count_pair_kernel);
  group_scan_partials_kernel<<<st + sp, IG_BLOCK, 0, stream>>>(
      counts_t, rows_t, counts_p, rows_p, st, partial);
  group_scan_apply_kernel<<<st + sp, IG_BLOCK, 0, stream>>>(
      counts_t, rows_t, counts_p, rows_p, st, partial, cursor_t, cursor_p);
  IG_LAUNCH(group_scatter_pair_kernel);
#undef IG_LAUNCH
}

void launch_embed_scatter_heavy_pair(
    const int* sorted_t, const long* perm_t, const int* counts_t,
    float* dtable_t, int S_t, const int* sorted_p, const long* perm_p,
    const int* counts_p, float* dtable_p, int S_p, const void* gout, long M,
    int KP, int thr, hipStream_t stream) {
  if (M <= 0) return;
  HeavyTable term = {sorted_t, perm_t, counts_t, dtable_t, 2 * M,
                     S_t, 0, S_t + S_p};
  HeavyTable path = {sorted_p, perm_p, counts_p, dtable_p, M, S_p, S_t, S_t};
  const int wpb = 4;
  const int tb = (int)(((2 * M + 15) / 16 + wpb - 1) / wpb);
  const int pb = (int)(((M + 15) / 16 + wpb - 1) / wpb);
  const int S = S_t > S_p ? S_t : S_p;
#define HPCASE(n)                                                             \
  case n:                                                                     \
    embed_scatter_heavy_pair_kernel<n><<<tb + pb, 256, 0, stream>>>(          \
        term, path, tb, (const bf16*)gout, M, KP, thr);                       \
    break;
  switch ((S + 127) / 128) {
    HPCASE(1) HPCASE(2) HPCASE(3) HPCASE(4)
    default:
      printf("embed_scatter_heavy_pair: unsupported S=%d\n", S);
  }
#undef HPCASE
}

void launch_clear_i32_pair(int* a, long na, int* b, long nb,
                           hipStream_t stream) {
  const int block = 256;
  const long n = na + nb;
  const int grid = (int)min((n + block - 1) / block, (long)4096);
  clear_i32_pair_kernel<<<grid > 0 ? grid : 1, block, 0, stream>>>(a, na, b,
                                                                   nb);
}

}  // extern "C"
