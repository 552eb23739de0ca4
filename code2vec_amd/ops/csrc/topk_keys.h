// Shared pieces of the top-k selection kernels (K19 row_topk in topk.hip,
// K20 sim_topk in sim_topk.hip, K23 head_topk in head_topk.hip): the 64-bit
// total-order key, the wave-cooperative sorted list, the rank merge of four
// wave lists and the (max, sumexp) merge of the log-sum-exp.
//
// Total order: descending value, ties to the SMALLEST column.  Every
// element is mapped to a unique 64-bit key
//     key = orderable(value) << 32 | ~column
// so "better" is a plain unsigned compare.  key 0 is the empty slot: it
// sorts below every real element (orderable(-inf) = 0x007FFFFF > 0).
// -0.0 is canonicalized to +0.0 before keying.
#pragma once

#include "common.h"

#define TOPK_SLOTS 16

typedef unsigned long long u64;

#define NEG_INF (-__builtin_inff())

__device__ __forceinline__ u64 topk_key(float x, unsigned col) {
  if (x == 0.f) x = 0.f;  // -0.0 -> +0.0
  const unsigned b = __float_as_uint(x);
  const unsigned hi = b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
  return ((u64)hi << 32) | (u64)(~col);
}

__device__ __forceinline__ float topk_key_val(u64 key) {
  const unsigned hi = (unsigned)(key >> 32);
  const unsigned b = (hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi;
  return __uint_as_float(b);
}

__device__ __forceinline__ long topk_key_col(u64 key) {
  return (long)(~(unsigned)key);
}

__device__ __forceinline__ u64 readlane_u64(u64 v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}

// value of lane-1 within each 16-lane row; lane 0 of a row gets ~0 (the
// "slot above the head" that nothing beats)
__device__ __forceinline__ u64 row_shr1_u64(u64 v) {
  const unsigned lo = __builtin_amdgcn_update_dpp(
      (int)0xFFFFFFFFu, (int)(unsigned)v, 0x111, 0xF, 0xF, false);
  const unsigned hi = __builtin_amdgcn_update_dpp(
      (int)0xFFFFFFFFu, (int)(unsigned)(v >> 32), 0x111, 0xF, 0xF, false);
  return ((u64)hi << 32) | lo;
}

// Insert every lane's key that beats tau into the wave's sorted list.
// Must be reached by all 64 lanes.  kq = k - 1 (wave-uniform).
__device__ __forceinline__ void wave_push(u64& mine, u64& tau, u64 key,
                                          int kq) {
  u64 mask = __ballot(key > tau);
  while (mask) {
    const int l = __builtin_ctzll(mask);
    const u64 kk = readlane_u64(key, l);
    const u64 prev = row_shr1_u64(mine);
    const u64 lo = kk < prev ? kk : prev;
    mine = mine > lo ? mine : lo;
    if ((int)(threadIdx.x & (WAVE - 1)) == l) key = 0;
    tau = readlane_u64(mine, kq);
    mask = __ballot(key > tau);
  }
}

// Merge the four wave lists (already in sk, one per 16 slots): returns this
// lane's rank (0 = best) among the 4 x 16 keys and its key in `my`.  Ranks
// are a permutation of 0..63 (empty keys tie-break by slot).  One wave.
__device__ __forceinline__ int block_rank(const u64* sk, u64& my) {
  const int lane = threadIdx.x & (WAVE - 1);
  my = sk[lane];
  int rank = 0;
#pragma unroll 8
  for (int j = 0; j < 4 * TOPK_SLOTS; ++j) {
    const u64 o = sk[j];
    rank += (o > my || (o == my && j < lane)) ? 1 : 0;
  }
  return rank;
}

// (max, sumexp) merge; an all -inf side contributes 0, never NaN
__device__ __forceinline__ void lse_merge(float& m, float& s, float om,
                                          float os) {
  const float M = fmaxf(m, om);
  if (M == NEG_INF) {
    s = 0.f;
    return;
  }
  s = s * __expf(m - M) + os * __expf(om - M);
  m = M;
}

__device__ __forceinline__ void wave_lse_merge(float& m, float& s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off);
    const float os = __shfl_xor(s, off);
    lse_merge(m, s, om, os);
  }
}
