// K1/K2 fused triple embedding gather + concat, and K13 scatter-add backward.
// (reference op sites: model/model.py:48-51 forward; autograd of
// nn.Embedding for backward — reimagined as HBM-streaming CDNA4 kernels.)
//
// Layout: out[row, :] = [ term[starts[row]] | path[paths[row]] | term[ends[row]] ]
// with segment strides TS / PS / TS (8-element multiples = 16-B granules;
// dt=100 stores 104-wide) and a zero-filled tail up to KP (the combiner's
// 32-element K padding).  Pad columns of the tables are zero, so pad
// columns of the output are zero by construction.
//
// NOTE: the standalone forward gather and the atomic backward below are the
// reference/fallback path — the default forward fuses the gather into the
// combiner GEMM (combiner.hip GATHER=1) and the default backward is the
// sort-based scatter further down.

#include "common.h"
#include "scatter_heavy.h"

#include <hipcub/hipcub.hpp>

// One wave per output row (context); 4 waves per block; grid-stride over rows.
// Each lane copies 16-byte chunks; chunk -> segment resolved per lane.
__global__ void gather_concat_fwd_kernel(
    const int* __restrict__ starts, const int* __restrict__ paths,
    const int* __restrict__ ends, const bf16* __restrict__ term,
    const bf16* __restrict__ path, bf16* __restrict__ out,
    long M, int TS, int PS, int KP) {
  // KP >= 2*TS+PS (combiner K padding); tail chunks are zero-filled
  const int chunks = KP / 8;  // 16-B chunks per row
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int waves_per_block = blockDim.x / WAVE;
  long row = (long)blockIdx.x * waves_per_block + wave;
  const long stride = (long)gridDim.x * waves_per_block;

  for (; row < M; row += stride) {
    const long s = starts[row];
    const long p = paths[row];
    const long e = ends[row];
    const uint4* srow = (const uint4*)(term + s * TS);
    const uint4* prow = (const uint4*)(path + p * PS);
    const uint4* erow = (const uint4*)(term + e * TS);
    uint4* orow = (uint4*)(out + row * KP);
    const int ts8 = TS / 8, ps8 = PS / 8;
    for (int c = lane; c < chunks; c += WAVE) {
      uint4 v = {0, 0, 0, 0};
      if (c < ts8) v = srow[c];
      else if (c < ts8 + ps8) v = prow[c - ts8];
      else if (c < 2 * ts8 + ps8) v = erow[c - ts8 - ps8];
      orow[c] = v;
    }
  }
}

// Legacy backward (atomic-rate-bound; superseded by the sort-based scatter
// below — kept as the simple reference implementation for A/B): scatter-add
// grad rows into fp32 dense grad tables.  Pad contexts (starts == 0) carry
// exactly-zero grads (attention mask math) and are skipped entirely.
__global__ void gather_concat_bwd_kernel(
    const int* __restrict__ starts, const int* __restrict__ paths,
    const int* __restrict__ ends, const bf16* __restrict__ gout,
    float* __restrict__ dterm, float* __restrict__ dpath,
    long M, int TS, int PS) {
  const int KP = 2 * TS + PS;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int waves_per_block = blockDim.x / WAVE;
  long row = (long)blockIdx.x * waves_per_block + wave;
  const long stride = (long)gridDim.x * waves_per_block;
  const int chunks = KP / 4;  // 4 bf16 (8 B) per lane-chunk

  for (; row < M; row += stride) {
    const int s = starts[row];
    if (s == 0) continue;  // pad context: grad identically zero
    const long p = paths[row];
    const long e = ends[row];
    const bf16* grow = gout + row * KP;
    const int ts4 = TS / 4, ps4 = PS / 4;
    for (int c = lane; c < chunks; c += WAVE) {
      float* dst;
      int col4;
      if (c < ts4) { dst = dterm + (long)s * TS; col4 = c; }
      else if (c < ts4 + ps4) { dst = dpath + p * PS; col4 = c - ts4; }
      else { dst = dterm + e * TS; col4 = c - ts4 - ps4; }
      // 4 bf16 grads -> 4 fp32 atomic adds
      const bf16* gsrc = grow + c * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float g = bf2f(gsrc[j]);
        if (g != 0.0f) atomic_add_f32(dst + col4 * 4 + j, g);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// K13 v2: sort-based segmented scatter-add (atomic-free on the common path).
// The caller sorts the flattened index list (torch radix sort) and passes the
// permutation; each wave owns the runs that start inside its chunk and writes
// each touched table row with plain f32 stores.  Runs that cross a chunk
// boundary (heavy-hitter indexes like @question) are split across waves and
// combined with fp32 atomics — precision identical, order nondeterminism
// limited to boundary partials.
//
// Entry o in [0, N): o < M -> gout row o at column offset off0;
// o >= M -> gout row (o - M) at offset off1 (start/end entries of the
// terminal table share one sort; the path table passes N == M).
template <int NP, int MINW = 1>  // NP: ceil(S/128) column-pair iterations
                                  // per lane; MINW: forced waves/SIMD
__global__ __launch_bounds__(256, MINW) void embed_scatter_sorted_kernel(
    const int* __restrict__ sorted_idx, const long* __restrict__ perm,
    const bf16* __restrict__ gout, float* __restrict__ dtable,
    bf16* __restrict__ out_bf16, unsigned char* __restrict__ flags, long N,
    long M, int KP, int S, int off0, int off1, int R_unused) {
  // fixed chunk RT: all RT gradient loads are issued up front (independent
  // rows), THEN runs are scanned from registers — no load in the dependent
  // run-scan chain.
  constexpr int RT = 16;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave_in_block = threadIdx.x / WAVE;
  const long wid = (long)blockIdx.x * (blockDim.x / WAVE) + wave_in_block;
  const long c0 = wid * RT;
  if (c0 >= N) return;
  const int count = (int)min((long)RT, N - c0);

  int idx[RT];
  bf16x2 gv[RT][NP];
#pragma unroll
  for (int t = 0; t < RT; ++t) idx[t] = t < count ? sorted_idx[c0 + t] : -1;
  const int prev_idx = c0 > 0 ? sorted_idx[c0 - 1] : -1;
  const int next_idx = c0 + RT < N ? sorted_idx[c0 + RT] : -1;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    if (t < count) {
      const long o = perm[c0 + t];
      const bf16* grow =
          o < M ? gout + o * KP + off0 : gout + (o - M) * KP + off1;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int col = i * 128 + lane * 2;
        bf16x2 g = {bf16(0.f), bf16(0.f)};
        if (col < S) g = *(const bf16x2*)(grow + col);
        gv[t][i] = g;
      }
    }
  }

  // statically unrolled run scan (no dynamic register indexing): a running
  // accumulator is flushed whenever the index changes
  float acc[NP][2];
#pragma unroll
  for (int i = 0; i < NP; ++i) acc[i][0] = acc[i][1] = 0.f;
  bool run_from_start = true;
  int cur_id = idx[0];

  // interior runs (the single run of an index fully inside this chunk)
  // write the bf16 grad row DIRECTLY; boundary-crossing runs accumulate
  // fp32 partials in the persistent scratch and set the row's flag for the
  // combine pass (cast_clear_rows).
  auto flush = [&](int id, bool boundary) {
    if (id != 0) {  // index 0 is <PAD/>: pad contexts carry zero grads
      if (boundary) {
        float* drow = dtable + (long)id * S;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int col = i * 128 + lane * 2;
          if (col < S) {
            atomic_add_f32(drow + col, acc[i][0]);
            atomic_add_f32(drow + col + 1, acc[i][1]);
          }
        }
        if (lane == 0) flags[id] = 1;
      } else {
        bf16* brow = out_bf16 + (long)id * S;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int col = i * 128 + lane * 2;
          if (col < S) {
            bf16x2 v = {f2bf(acc[i][0]), f2bf(acc[i][1])};
            *(bf16x2*)(brow + col) = v;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) acc[i][0] = acc[i][1] = 0.f;
  };

#pragma unroll
  for (int t = 0; t < RT; ++t) {
    if (t < count) {
      if (t > 0 && idx[t] != cur_id) {
        // flush the run that just ended (head-crossing if it began at the
        // chunk start AND continues from the previous chunk)
        flush(cur_id, run_from_start && prev_idx == cur_id);
        run_from_start = false;
        cur_id = idx[t];
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        acc[i][0] += bf2f(gv[t][i][0]);
        acc[i][1] += bf2f(gv[t][i][1]);
      }
    }
  }
  // final run: tail-crossing if the next chunk starts with the same index
  flush(cur_id, (run_from_start && prev_idx == cur_id) || next_idx == cur_id);
}

// ---------------------------------------------------------------------------
// Heavy-row pre-pass of the row-gathering table Adam (adam.hip), one table:
// one wave per 16-entry chunk of the sorted order (scatter_heavy.h).
template <int NP>
__global__ __launch_bounds__(256) void embed_scatter_heavy_kernel(
    const int* __restrict__ sorted_idx, const long* __restrict__ perm,
    const int* __restrict__ counts, const bf16* __restrict__ gout,
    float* __restrict__ dtable, long N, long M, int KP, int S, int off0,
    int off1, int thr) {
  const long wid =
      (long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  scatter_heavy_chunk<NP>(wid, sorted_idx, perm, counts, gout, dtable, N, M,
                          KP, S, off0, off1, thr);
}

// ---------------------------------------------------------------------------
// Counting-sort pair (replaces torch.sort's merge path for grouping index
// lists by value):
//  1) histogram: counts[idx] += 1 over all entries,
//  2) host-side torch.cumsum -> exclusive offsets (cursor),
//  3) scatter_group: pos = cursor[idx]++ ; sorted_idx[pos] = idx;
//     perm[pos] = original position.
// Within-group order is nondeterministic (atomic race), which only permutes
// fp32 summation order inside a run.
// Indexes 0 (<PAD/>) and 1 (@question) are known heavy hitters: ragged
// real batches are ~half padding, so per-lane atomics serialize on one
// address (measured 870 us per call at the top11 shape).  Wave-aggregate
// those two values with ballots — one atomic per wave — and use plain
// per-lane atomics for everything else (duplicates within a wave are
// rare for ordinary indexes in a shuffled batch).
__global__ void count_indices_kernel(const int* __restrict__ idx,
                                     int* __restrict__ counts, long N) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & (WAVE - 1);
  for (long t = i; t < N; t += stride) {
    const int v = idx[t];
    const unsigned long long m0 = __ballot(v == 0);
    const unsigned long long m1 = __ballot(v == 1);
    if (v <= 1) {
      const unsigned long long m = (v == 0) ? m0 : m1;
      if (lane == __ffsll((long long)m) - 1)
        atomicAdd(&counts[v], __popcll(m));
    } else {
      atomicAdd(&counts[v], 1);
    }
  }
}

__global__ void scatter_group_kernel(const int* __restrict__ idx,
                                     int* __restrict__ cursor,
                                     int* __restrict__ sorted_idx,
                                     long* __restrict__ perm, long N) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & (WAVE - 1);
  for (long t = i; t < N; t += stride) {
    const int v = idx[t];
    const unsigned long long m0 = __ballot(v == 0);
    const unsigned long long m1 = __ballot(v == 1);
    int pos;
    if (v <= 1) {
      const unsigned long long m = (v == 0) ? m0 : m1;
      const int leader = __ffsll((long long)m) - 1;
      const int rank = (int)__popcll(m & ((1ull << lane) - 1));
      int base = 0;
      if (lane == leader) base = atomicAdd(&cursor[v], (int)__popcll(m));
      base = __shfl(base, leader);
      pos = base + rank;
    } else {
      pos = atomicAdd(&cursor[v], 1);
    }
    sorted_idx[pos] = v;
    perm[pos] = t;
  }
}

// ---------------------------------------------------------------------------
// Fused cast-and-clear: convert the fp32 scatter scratch to the bf16 grad
// tensor AND re-zero the touched fp32 rows (so the scratch is reusable next
// step without a full-buffer memset).  Rows with counts == 0 were never
// written: emit bf16 zeros without touching the fp32 buffer.
// Each wave screens 64 CONSECUTIVE rows with coalesced per-lane
// flags/counts loads, then ballots and processes only the rows needing
// work (a wave-per-row mapping makes every metadata read a solo
// cache-line touch — 360k of them — and ran latency-bound at 37 us vs
// ~8 us of actual byte traffic).
__global__ void cast_clear_rows_kernel(float* __restrict__ dtable,
                                       int* __restrict__ counts,
                                       unsigned char* __restrict__ flags,
                                       bf16* __restrict__ out, long T, int S) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int wpb = blockDim.x / WAVE;
  const long nchunks = (T + WAVE - 1) / WAVE;
  long chunk = (long)blockIdx.x * wpb + wave;
  const long stride = (long)gridDim.x * wpb;
  for (; chunk < nchunks; chunk += stride) {
    const long r0 = chunk * WAVE;
    const long rl = r0 + lane;
    const bool valid = rl < T;
    const bool boundary = valid && rl != 0 && flags[rl] != 0;
    // interior-touched rows were written bf16-direct by the scatter
    // kernel; row 0 (<PAD/>) always reads as untouched (its grads are
    // exactly zero)
    const bool interior =
        valid && !boundary && rl != 0 && counts[rl] > 0;
    const bool zero_row = valid && !boundary && !interior;
    if (boundary) flags[rl] = 0;
    // consume the histogram: the counts buffer is persistent and must be
    // all-zero before the next step's count_indices pass
    if (valid && counts[rl] != 0) counts[rl] = 0;
    const unsigned long long mb = __ballot(boundary);
    unsigned long long m = mb | __ballot(zero_row);
    while (m) {
      const int r = __ffsll((long long)m) - 1;
      m &= m - 1;
      const long row = r0 + r;
      const bool bnd = (mb >> r) & 1;
      float* frow = dtable + row * S;
      bf16* orow = out + row * S;
      for (int c0 = lane * 2; c0 < S; c0 += WAVE * 2) {
        bf16x2 o = {bf16(0.f), bf16(0.f)};
        if (bnd) {
          const float2 v = *(const float2*)(frow + c0);
          o[0] = f2bf(v.x);
          o[1] = f2bf(v.y);
          float2 zz = {0.f, 0.f};
          *(float2*)(frow + c0) = zz;
        }
        *(bf16x2*)(orow + c0) = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Exclusive prefix scan of counts[0..n-1] -> cursor[0..n-1] in three tiny
// kernels (1024 elements per block; the middle kernel scans the <=1600
// block sums serially in one block).  rocprim's lookback scan plus its
// init kernel plus the torch.zeros fills cost ~21 us per table per step
// at 360k-1.3M rows; this chain is ~6 us and needs no zeroed inputs.
#define SCAN_B 1024

__global__ __launch_bounds__(256) void scan_partials_kernel(
    const int* __restrict__ x, int* __restrict__ partial, long n) {
  const long b0 = (long)blockIdx.x * SCAN_B;
  int v = 0;
  for (int t = threadIdx.x; t < SCAN_B; t += 256) {
    const long i = b0 + t;
    v += i < n ? x[i] : 0;
  }
  // block reduce
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __shared__ int red[4];
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(1024) void scan_spine_kernel(
    int* __restrict__ partial, int nb) {
  // single block: exclusive scan of the block sums
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  // process in tiles of 1024 with a Hillis-Steele scan in LDS
  __shared__ int tile[1024];
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + threadIdx.x;
    int v = i < nb ? partial[i] : 0;
    tile[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      int add = threadIdx.x >= off ? tile[threadIdx.x - off] : 0;
      __syncthreads();
      tile[threadIdx.x] += add;
      __syncthreads();
    }
    const int incl = tile[threadIdx.x];
    if (i < nb) partial[i] = carry + incl - v;  // exclusive
    __syncthreads();
    if (threadIdx.x == 1023) carry += tile[1023];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void scan_apply_kernel(
    const int* __restrict__ x, const int* __restrict__ partial,
    int* __restrict__ out, long n) {
  const long b0 = (long)blockIdx.x * SCAN_B;
  __shared__ int tile[SCAN_B];
  for (int t = threadIdx.x; t < SCAN_B; t += 256) {
    const long i = b0 + t;
    tile[t] = i < n ? x[i] : 0;
  }
  __syncthreads();
  // serial-ish per-thread scan: each thread owns 4 consecutive elems
  // (SCAN_B/256); do a two-level exclusive scan in LDS
  __shared__ int tsum[256];
  {
    const int t0 = threadIdx.x * 4;
    int s0 = tile[t0] + tile[t0 + 1] + tile[t0 + 2] + tile[t0 + 3];
    tsum[threadIdx.x] = s0;
  }
  __syncthreads();
  // Hillis-Steele over the 256 thread sums
  for (int off = 1; off < 256; off <<= 1) {
    int add = threadIdx.x >= off ? tsum[threadIdx.x - off] : 0;
    __syncthreads();
    tsum[threadIdx.x] += add;
    __syncthreads();
  }
  {
    const int t0 = threadIdx.x * 4;
    int run = partial[blockIdx.x] +
              (threadIdx.x > 0 ? tsum[threadIdx.x - 1] : 0);
    for (int k = 0; k < 4; ++k) {
      const long i = b0 + t0 + k;
      if (i < n) out[i] = run;
      run += tile[t0 + k];
    }
  }
}

extern "C" {

void launch_exclusive_scan(const int* x, int* partial, int* out, long n,
                           hipStream_t stream) {
  const int nb = (int)((n + SCAN_B - 1) / SCAN_B);
  scan_partials_kernel<<<nb, 256, 0, stream>>>(x, partial, n);
  scan_spine_kernel<<<1, 1024, 0, stream>>>(partial, nb);
  scan_apply_kernel<<<nb, 256, 0, stream>>>(x, partial, out, n);
}

void launch_cast_clear_rows(float* dtable, const int* counts,
                            unsigned char* flags, void* out, long T, int S,
                            hipStream_t stream) {
  const int block = 256;
  const int wpb = block / WAVE;
  const long chunks = (T + WAVE - 1) / WAVE;
  const int grid = (int)min((chunks + wpb - 1) / wpb, (long)8192);
  cast_clear_rows_kernel<<<grid, block, 0, stream>>>(
      dtable, (int*)counts, flags, (bf16*)out, T, S);
}

void launch_count_indices(const int* idx, int* counts, long N,
                          hipStream_t stream) {
  const int block = 256;
  const int grid = (int)min((N + block - 1) / block, (long)4096);
  count_indices_kernel<<<grid, block, 0, stream>>>(idx, counts, N);
}

void launch_scatter_group(const int* idx, int* cursor, int* sorted_idx,
                          long* perm, long N, hipStream_t stream) {
  const int block = 256;
  const int grid = (int)min((N + block - 1) / block, (long)4096);
  scatter_group_kernel<<<grid, block, 0, stream>>>(idx, cursor, sorted_idx,
                                                   perm, N);
}

void launch_embed_scatter_sorted(const int* sorted_idx, const long* perm,
                                 const void* gout, float* dtable,
                                 void* out_bf16, unsigned char* flags, long N,
                                 long M, int KP, int S, int off0, int off1,
                                 int R, hipStream_t stream) {
  if (R <= 0) R = 16;  // entries per wave-chunk
  const long waves = (N + R - 1) / R;
  const int wpb = 4;
  const int grid = (int)((waves + wpb - 1) / wpb);
  const int np = (S + 127) / 128;
  // C2V_ESS_OCC=5/6 forces a waves/SIMD register cap (occupancy A/B)
  static const char* occ_env = getenv("C2V_ESS_OCC");
  const int occ = occ_env ? atoi(occ_env) : 0;
#define SCASE(n)                                                              \
  case n:                                                                     \
    if (occ == 6)                                                             \
      embed_scatter_sorted_kernel<n, 6><<<grid, 256, 0, stream>>>(            \
          sorted_idx, perm, (const bf16*)gout, dtable, (bf16*)out_bf16,       \
          flags, N, M, KP, S, off0, off1, R);                                 \
    else if (occ == 5)                                                        \
      embed_scatter_sorted_kernel<n, 5><<<grid, 256, 0, stream>>>(            \
          sorted_idx, perm, (const bf16*)gout, dtable, (bf16*)out_bf16,       \
          flags, N, M, KP, S, off0, off1, R);                                 \
    else                                                                      \
      embed_scatter_sorted_kernel<n><<<grid, 256, 0, stream>>>(               \
          sorted_idx, perm, (const bf16*)gout, dtable, (bf16*)out_bf16,       \
          flags, N, M, KP, S, off0, off1, R);                                 \
    break;
  switch (np) {
    SCASE(1) SCASE(2) SCASE(3) SCASE(4)
    default:
      printf("embed_scatter_sorted: unsupported S=%d\n", S);
  }
#undef SCASE
}

void launch_embed_scatter_heavy(const int* sorted_idx, const long* perm,
                                const int* counts, const void* gout,
                                float* dtable, long N, long M, int KP, int S,
                                int off0, int off1, int thr,
                                hipStream_t stream) {
  if (N <= 0) return;
  const long waves = (N + 15) / 16;
  const int wpb = 4;
  const int grid = (int)((waves + wpb - 1) / wpb);
#define HCASE(n)                                                              \
  case n:                                                                     \
    embed_scatter_heavy_kernel<n><<<grid, 256, 0, stream>>>(                  \
        sorted_idx, perm, counts, (const bf16*)gout, dtable, N, M, KP, S,     \
        off0, off1, thr);                                                     \
    break;
  switch ((S + 127) / 128) {
    HCASE(1) HCASE(2) HCASE(3) HCASE(4)
    default:
      printf("embed_scatter_heavy: unsupported S=%d\n", S);
  }
#undef HCASE
}

void launch_gather_concat_fwd(const int* starts, const int* paths,
                              const int* ends, const void* term,
                              const void* path, void* out, long M, int TS,
                              int PS, int KP, hipStream_t stream) {
  const int block = 256;
  const int waves_per_block = block / WAVE;
  int grid = (int)min((M + waves_per_block - 1) / waves_per_block, (long)16384);
  gather_concat_fwd_kernel<<<grid, block, 0, stream>>>(
      starts, paths, ends, (const bf16*)term, (const bf16*)path, (bf16*)out,
      M, TS, PS, KP);
}

void launch_gather_concat_bwd(const int* starts, const int* paths,
                              const int* ends, const void* gout, float* dterm,
                              float* dpath, long M, int TS, int PS,
                              hipStream_t stream) {
  const int block = 256;
  const int waves_per_block = block / WAVE;
  int grid = (int)min((M + waves_per_block - 1) / waves_per_block, (long)16384);
  gather_concat_bwd_kernel<<<grid, block, 0, stream>>>(
      starts, paths, ends, (const bf16*)gout, dterm, dpath, M, TS, PS);
}

}  // extern "C"

extern "C" {

// rocPRIM/hipCUB single-pass (decoupled-lookback) exclusive scan — one
// kernel pair instead of the 3-launch partials/spine/apply chain above.
// Used for the counting-sort cursor over the [T]/[P] histogram.
size_t cub_exclusive_scan_temp_bytes(long n) {
  size_t bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(
      nullptr, bytes, (const int*)nullptr, (int*)nullptr, (int)n,
      (hipStream_t)0);
  return bytes;
}

void launch_cub_exclusive_scan(const int* in, int* out, void* temp,
                               size_t temp_bytes, long n,
                               hipStream_t stream) {
  (void)hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, out, (int)n,
                                         stream);
}

}  // extern "C"
