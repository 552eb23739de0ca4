// Counting sort of BOTH embedding tables' index lists in one chain of four
// launches (count, scan partials, scan apply, group), plus the both-tables
// forms of the table Adam's heavy-row pre-pass and histogram clear.
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

// Scan scratch length group_tables needs for histograms of these lengths.
long group_tables_partials(long rows_t, long rows_p) {
  return (rows_t + IG_SCAN - 1) / IG_SCAN + (rows_p + IG_SCAN - 1) / IG_SCAN;
}

// counts_*: all-zero going in, the histograms coming out; cursor_* end at
// each run's END; sorted_*/perm_* hold 2M / M entries.
void launch_group_tables(const int* starts, const int* paths, const int* ends,
                         long M, int rows_t, int rows_p, int* counts_t,
                         int* counts_p, int* cursor_t, int* cursor_p,
                         int* partial, int* sorted_t, long* perm_t,
                         int* sorted_p, long* perm_p, hipStream_t stream) {
  if (M <= 0) return;
  GroupTable term = {starts, ends, M, 2 * M, rows_t, counts_t, cursor_t,
                     sorted_t, perm_t};
  GroupTable path = {paths, paths, M, M, rows_p, counts_p, cursor_p,
                     sorted_p, perm_p};
  // entries per thread, swept on hardware (kbench group_tables and the
  // step, PERF.md): 2 beats 4 and 1; C2V_GROUP_E=1/4 select the others
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
