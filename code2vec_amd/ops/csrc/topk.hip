// K19: per-row top-k (k <= 16) + log-sum-exp over a [B, L] matrix of bf16
// logits or fp32 attention weights, in ONE streaming pass (the prediction
// path: k most likely names with real probabilities, k most-attended
// path-contexts).
//
// Total order: descending value, ties to the SMALLEST column.  Every
// element is mapped to a unique 64-bit key
//     key = orderable(value) << 32 | ~column
// so "better" is a plain unsigned compare, the result is unique, and it
// does not depend on grid shape or chunking.  key 0 is the empty slot: it
// sorts below every real element (orderable(-inf) = 0x007FFFFF > 0), so a
// real -inf column beats an empty slot.  -0.0 is canonicalized to +0.0
// before keying (they compare equal in the oracle's stable sort).
//
// Selection is WAVE-cooperative rather than per-thread: a per-thread
// K-slot list has a weak threshold (each thread sees few elements), so
// nearly every wave step would run the insertion for some lane.  Here a
// wave keeps ONE sorted list, slot j in lane j of each 16-lane DPP row
// (all four rows hold identical copies), and tau = slot k-1 is a
// wave-uniform threshold.  A step first tests its elements against tau's
// value with one float compare each; only when some lane passes are keys
// built and the passing lanes inserted one at a time:
//     list[j] = max(list[j], min(key, list[j-1]))      (row_shr:1 DPP)
// which is 2 u64 compares for the whole wave, independent of k.  The
// expected number of insertions is ~k*ln(n/k) per wave.  No per-thread
// arrays exist, so nothing is runtime-indexed.
//
// Stage 1: grid = B * ceil(L / CHUNK) blocks of 256; block (row, chunk)
//   streams its chunk with aligned 16-B loads (rows that do not start on
//   a 16-B boundary shift the vector grid; only the vectors sticking out
//   of the chunk load element-wise), four loads in flight per thread,
//   with an online (max, sumexp) per thread alongside.  The waves share
//   their thresholds through LDS as a pre-filter.  The four wave lists
//   are merged by a rank sort through LDS (wave 0); the (max, sumexp)
//   pairs by a fixed xor tree and then in wave order.  One chunk: writes
//   vals/idx/lse directly.
//   Otherwise: part[B, nchunk, 16] keys and pm/ps[B, nchunk].
// Stage 2: one block per row streams the nchunk*16 candidate keys through
//   the same wave lists and merges (pm, ps) in fixed order into lse.
// No atomics anywhere; bitwise reproducible; no host sync.

#include "common.h"
#include "topk_keys.h"  // key order, wave lists, rank merge, lse merge

#define TOPK_CHUNK 32768
#define TOPK_UNR 4

template <typename T, int V>
__device__ __forceinline__ void load_vec(const T* p, float (&out)[V]) {
  if constexpr (V == 8) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = bf2f(v[j]);
  } else {
    static_assert(V == 4, "16-B vectors: bf16x8 or f32x4");
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = v[j];
  }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void row_topk_stage1_kernel(
    const T* __restrict__ x, long L, int nchunk, int k,
    u64* __restrict__ part, float* __restrict__ pm, float* __restrict__ ps,
    float* __restrict__ vals, long* __restrict__ idx,
    float* __restrict__ lse) {
  const long row = blockIdx.x / nchunk;
  const int chunk = blockIdx.x % nchunk;
  const T* xr = x + row * L;
  const long c0 = (long)chunk * TOPK_CHUNK;
  const long c1 = min(L, c0 + (long)TOPK_CHUNK);
  const int kq = k - 1;
  // elements by which the row start (hence every chunk start: CHUNK is a
  // V-multiple) sits past a 16-B boundary.  The vector grid starts that
  // many columns early so every full vector is an aligned 16-B load; the
  // at most two vectors per chunk that stick out of [c0, c1) load their
  // inside elements one by one.
  const int mis = (int)(((unsigned long long)xr / sizeof(T)) % V);
  // chunk-relative 32-bit positions from here on
  const T* xc = xr + c0;
  const int n = (int)(c1 - c0);
  const unsigned col0 = (unsigned)c0;

  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  __shared__ u64 sk[4 * TOPK_SLOTS];
  __shared__ float sm[4], ss[4];
  // each wave publishes the value of its own tau here.  Any wave's tau is
  // a lower bound of the block's k-th best, so the max over the four is a
  // valid (and much tighter) pre-filter for all of them.  Reads race with
  // the other waves' writes on purpose: a stale value is only a looser
  // bound, and the selected set does not depend on which bound was used.
  __shared__ volatile float s_tau[4];
  if (lane == 0) s_tau[wave] = NEG_INF;
  __syncthreads();

  u64 mine = 0, tau = 0;
  float tau_val = NEG_INF;
  float m = NEG_INF, s = 0.f;

  // wave-uniform trip count: every lane reaches every ballot
  for (int b0 = -mis; b0 < n; b0 += 256 * V * TOPK_UNR) {
    float xf[TOPK_UNR][V];
#pragma unroll
    for (int u = 0; u < TOPK_UNR; ++u) {
      const int rel = b0 + (u * 256 + (int)threadIdx.x) * V;
      if (rel >= 0 && rel + V <= n) {
        load_vec<T, V>(xc + rel, xf[u]);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
          xf[u][j] = (unsigned)(rel + j) < (unsigned)n ? (float)xc[rel + j]
                                                       : NEG_INF;
      }
    }
    float filt = fmaxf(fmaxf(s_tau[0], s_tau[1]), fmaxf(s_tau[2], s_tau[3]));
    filt = fmaxf(filt, tau_val);
#pragma unroll
    for (int u = 0; u < TOPK_UNR; ++u) {
      const int rel = b0 + (u * 256 + (int)threadIdx.x) * V;
      bool cand = false;
      float mv = NEG_INF;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        cand |= xf[u][j] >= filt;
        mv = fmaxf(mv, xf[u][j]);
      }
      // online (max, sumexp); skipped while everything seen is -inf
      if (mv > m) {
        s *= __expf(m - mv);
        m = mv;
      }
      if (m > NEG_INF) {
#pragma unroll
        for (int j = 0; j < V; ++j) s += __expf(xf[u][j] - m);
      }
      if (__ballot(cand)) {
        u64 key[V];
        bool beats = false;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const bool valid = (unsigned)(rel + j) < (unsigned)n;
          key[j] = valid ? topk_key(xf[u][j], col0 + (unsigned)(rel + j))
                         : 0ull;
          beats |= key[j] > tau;
        }
        if (__ballot(beats)) {  // ties with tau's value mostly stop here
#pragma unroll
          for (int j = 0; j < V; ++j) wave_push(mine, tau, key[j], kq);
          tau_val = tau ? topk_key_val(tau) : NEG_INF;
          if (lane == 0) s_tau[wave] = tau_val;
          filt = fmaxf(filt, tau_val);
        }
      }
    }
  }

  if (lane < TOPK_SLOTS) sk[wave * TOPK_SLOTS + lane] = mine;
  wave_lse_merge(m, s);
  if (lane == 0) {
    sm[wave] = m;
    ss[wave] = s;
  }
  __syncthreads();
  if (wave != 0) return;
  u64 my;
  const int rank = block_rank(sk, my);
  if (nchunk == 1) {
    if (rank < k) {
      vals[row * k + rank] = topk_key_val(my);
      idx[row * k + rank] = topk_key_col(my);
    }
  } else if (rank < TOPK_SLOTS) {
    part[(row * nchunk + chunk) * TOPK_SLOTS + rank] = my;
  }
  if (lane == 0) {
    float bm = sm[0], bs = ss[0];
    for (int w = 1; w < 4; ++w) lse_merge(bm, bs, sm[w], ss[w]);
    if (nchunk == 1) {
      lse[row] = bm == NEG_INF ? NEG_INF : bm + logf(bs);
    } else {
      pm[row * nchunk + chunk] = bm;
      ps[row * nchunk + chunk] = bs;
    }
  }
}

__global__ __launch_bounds__(256) void row_topk_stage2_kernel(
    const u64* __restrict__ part, const float* __restrict__ pm,
    const float* __restrict__ ps, int nchunk, int k,
    float* __restrict__ vals, long* __restrict__ idx,
    float* __restrict__ lse) {
  const long row = blockIdx.x;
  const u64* pr = part + row * nchunk * TOPK_SLOTS;
  const long n = (long)nchunk * TOPK_SLOTS;
  const int kq = k - 1;
  u64 mine = 0, tau = 0;
  for (long q0 = 0; q0 < n; q0 += 256) {
    const long q = q0 + threadIdx.x;
    const u64 key = q < n ? pr[q] : 0ull;
    wave_push(mine, tau, key, kq);
  }
  // (pm, ps) in fixed order: thread t takes chunks t, t+256, ... ascending
  float m = NEG_INF, s = 0.f;
  for (int c = threadIdx.x; c < nchunk; c += 256)
    lse_merge(m, s, pm[row * nchunk + c], ps[row * nchunk + c]);

  __shared__ u64 sk[4 * TOPK_SLOTS];
  __shared__ float sm[4], ss[4];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  if (lane < TOPK_SLOTS) sk[wave * TOPK_SLOTS + lane] = mine;
  wave_lse_merge(m, s);
  if (lane == 0) {
    sm[wave] = m;
    ss[wave] = s;
  }
  __syncthreads();
  if (wave != 0) return;
  u64 my;
  const int rank = block_rank(sk, my);
  if (rank < k) {
    vals[row * k + rank] = topk_key_val(my);
    idx[row * k + rank] = topk_key_col(my);
  }
  if (lane == 0) {
    float bm = sm[0], bs = ss[0];
    for (int w = 1; w < 4; ++w) lse_merge(bm, bs, sm[w], ss[w]);
    lse[row] = bm == NEG_INF ? NEG_INF : bm + logf(bs);
  }
}

extern "C" {

int row_topk_chunk() { return TOPK_CHUNK; }

// x: [B, L] bf16 (is_f32 = 0) or f32; 1 <= k <= 16, k <= L < 2^31 and
// B * ceil(L / CHUNK) < 2^31 are checked by the caller.  part/pm/ps are
// only touched when L > CHUNK.
void launch_row_topk(const void* x, int is_f32, long B, long L, int k,
                     void* part, float* pm, float* ps, float* vals,
                     long* idx, float* lse, hipStream_t stream) {
  if (B == 0) return;
  const int nchunk = (int)((L + TOPK_CHUNK - 1) / TOPK_CHUNK);
  const unsigned grid = (unsigned)(B * nchunk);
  u64* pp = (u64*)part;
  if (is_f32)
    row_topk_stage1_kernel<float, 4><<<grid, 256, 0, stream>>>(
        (const float*)x, L, nchunk, k, pp, pm, ps, vals, idx, lse);
  else
    row_topk_stage1_kernel<bf16, 8><<<grid, 256, 0, stream>>>(
        (const bf16*)x, L, nchunk, k, pp, pm, ps, vals, idx, lse);
  if (nchunk > 1)
    row_topk_stage2_kernel<<<(unsigned)B, 256, 0, stream>>>(
        pp, pm, ps, nchunk, k, vals, idx, lse);
}

// Stage 2 on its own, for K23 (head_topk.hip): its stage 1 leaves the same
// part[B, n, 16] keys and pm/ps[B, n] pairs, one per label slice.
void launch_row_topk_stage2(const void* part, const float* pm,
                            const float* ps, long B, int n, int k,
                            float* vals, long* idx, float* lse,
                            hipStream_t stream) {
  if (B == 0) return;
  row_topk_stage2_kernel<<<(unsigned)B, 256, 0, stream>>>(
      (const u64*)part, pm, ps, n, k, vals, idx, lse);
}

}  // extern "C"
