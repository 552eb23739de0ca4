// Tile selection shared by the fused score + top-k kernels (K20 sim_topk in
// sim_topk.hip, K23 head_topk in head_topk.hip): a wave holds the scores of
// 16 queries against a 16-row tile in the MFMA C layout and keeps 16 sorted
// lists in four 64-bit registers (topk_keys.h has the key order).
#pragma once

#include "common.h"
#include "topk_keys.h"

#define SIM_QT 16    // queries per block
#define SIM_ROWS 16  // index rows per tile

// v of lane `src` (0..63), per destination lane
__device__ __forceinline__ u64 bpermute_u64(int src, u64 v) {
  const unsigned lo =
      __builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)v);
  const unsigned hi =
      __builtin_amdgcn_ds_bpermute(src << 2, (int)(unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}

// One insert step on a list register: every DPP row r inserts ITS key kk
// (uniform within the row) into its own list.  A key that beats nothing —
// 0 above all — leaves the list as it is, so rows without a candidate ride
// along for free.
__device__ __forceinline__ void sim_rows_insert(u64& mine, u64 kk) {
  const u64 prev = row_shr1_u64(mine);
  const u64 lo = kk < prev ? kk : prev;
  mine = mine > lo ? mine : lo;
}

// Offer the 4 scores of every lane to the wave's lists.  row0 is the
// lane's first index row; rows >= N and the excluded row are masked.
//
// s_tau[query][wave] holds the value of every wave's k-th best so far.  Any
// wave's tau is a lower bound of the block's k-th best, so the max over the
// four is a valid and much tighter pre-filter for all of them.  Reads race
// with the other waves' writes on purpose: a stale value is only a looser
// bound, and the selected set does not depend on which bound was used.
__device__ __forceinline__ void sim_select(const f32x4& s, long row0, long N,
                                           long excl, int kq, u64 (&mine)[4],
                                           u64& tau, float& tau_val,
                                           volatile float* s_tau) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const volatile float* st = s_tau + 4 * (lane & 15);
  const float filt =
      fmaxf(fmaxf(fmaxf(st[0], st[1]), fmaxf(st[2], st[3])), tau_val);
  const bool cand = s[0] >= filt || s[1] >= filt || s[2] >= filt ||
                    s[3] >= filt;
  if (!__ballot(cand)) return;
  u64 key[4];
  bool beats = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long r = row0 + j;
    key[j] = (r < N && r != excl && s[j] >= filt)
                 ? topk_key(s[j], (unsigned)r)
                 : 0ull;
    beats |= key[j] > tau;
  }
  if (!__ballot(beats)) return;  // ties with tau's value mostly stop here
  // Lane 16h + c holds query c's scores against rows 4h + j.  For one
  // (j, h) the 16 lanes of DPP row h carry at most one candidate per query,
  // which is what one insert step per list register takes: row r of
  // register g fetches the key of lane 16h + 4g + r.  All branches below
  // are wave-uniform.
  const int drow = lane >> 4;
  unsigned touched = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const u64 kj = key[j] > tau ? key[j] : 0ull;
    const u64 m = __ballot(kj != 0ull);
    if (!m) continue;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const unsigned mh = (unsigned)(m >> (16 * h)) & 0xFFFFu;
      if (!mh) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (!((mh >> (4 * g)) & 0xFu)) continue;
        sim_rows_insert(mine[g], bpermute_u64(16 * h + 4 * g + drow, kj));
        touched |= 1u << g;
      }
    }
  }
  // thresholds of the lists that changed: query c = lane & 15 lives in
  // register c >> 2, DPP row c & 3.  A lane without a query (tau = ~0)
  // keeps its unbeatable threshold.
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    if (!(touched & (1u << g))) continue;
    const u64 t = bpermute_u64(16 * (lane & 3) + kq, mine[g]);
    if (((lane >> 2) & 3) == g && tau != ~0ull) {
      tau = t;
      tau_val = t ? topk_key_val(t) : NEG_INF;
    }
  }
  if (lane < SIM_QT) s_tau[4 * lane + wave] = tau_val;
}
