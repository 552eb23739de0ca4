// Heavy-row pre-pass of the row-gathering table Adam (adam.hip), shared by
// the per-table kernel (gather_concat.hip) and the both-tables kernel
// (index_group.hip).
#pragma once

#include "common.h"

// One wave reduces one aligned 16-entry chunk `wid` of a table's sorted
// order: the same chunking as embed_scatter_sorted_kernel, but only runs of
// rows with counts > thr are reduced (fp32 atomics into the persistent
// scratch); everything else is gathered by the Adam kernel itself.  A run
// longer than 2 chunks always reaches a chunk edge, so a chunk can hold a
// heavy run only as its head run (continuing from the previous chunk) or
// its tail run (continuing into the next): chunks with neither exit after
// four sorted_idx reads.  Index 0 (<PAD/>) carries zero grads and is skipped.
template <int NP>
__device__ __forceinline__ void scatter_heavy_chunk(
    long wid, const int* __restrict__ sorted_idx,
    const long* __restrict__ perm, const int* __restrict__ counts,
    const bf16* __restrict__ gout, float* __restrict__ dtable, long N, long M,
    int KP, int S, int off0, int off1, int thr) {
  constexpr int RT = 16;
  const int lane = threadIdx.x & (WAVE - 1);
  const long c0 = wid * RT;
  if (c0 >= N) return;
  const int count = (int)min((long)RT, N - c0);
  const int first = sorted_idx[c0];
  const int last = sorted_idx[c0 + count - 1];
  const int prev_idx = c0 > 0 ? sorted_idx[c0 - 1] : -1;
  const int next_idx = c0 + RT < N ? sorted_idx[c0 + RT] : -1;
  const bool hh = first > 0 && prev_idx == first && counts[first] > thr;
  const bool ht = last > 0 && next_idx == last && counts[last] > thr;
  if (!hh && !ht) return;
  const int hid = hh ? first : -1;
  const int tid = ht ? last : -1;

  int idx[RT];
  bf16x2 gv[RT][NP];
#pragma unroll
  for (int t = 0; t < RT; ++t) idx[t] = t < count ? sorted_idx[c0 + t] : -2;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
#pragma unroll
    for (int i = 0; i < NP; ++i) gv[t][i] = bf16x2{bf16(0.f), bf16(0.f)};
    if (idx[t] == hid || idx[t] == tid) {
      const long o = perm[c0 + t];
      const bf16* grow =
          o < M ? gout + o * KP + off0 : gout + (o - M) * KP + off1;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int col = i * 128 + lane * 2;
        if (col < S) gv[t][i] = *(const bf16x2*)(grow + col);
      }
    }
  }
  float acc_h[NP][2], acc_t[NP][2];
#pragma unroll
  for (int i = 0; i < NP; ++i)
    acc_h[i][0] = acc_h[i][1] = acc_t[i][0] = acc_t[i][1] = 0.f;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    if (idx[t] == hid) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        acc_h[i][0] += bf2f(gv[t][i][0]);
        acc_h[i][1] += bf2f(gv[t][i][1]);
      }
    } else if (idx[t] == tid) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        acc_t[i][0] += bf2f(gv[t][i][0]);
        acc_t[i][1] += bf2f(gv[t][i][1]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int col = i * 128 + lane * 2;
    if (col < S) {
      if (hh) {
        atomic_add_f32(dtable + (long)hid * S + col, acc_h[i][0]);
        atomic_add_f32(dtable + (long)hid * S + col + 1, acc_h[i][1]);
      }
      if (ht && tid != hid) {
        atomic_add_f32(dtable + (long)tid * S + col, acc_t[i][0]);
        atomic_add_f32(dtable + (long)tid * S + col + 1, acc_t[i][1]);
      }
    }
  }
}
