// Shared helpers for the code2vec_amd CDNA4 (gfx950) kernels.
// Wavefront = 64 lanes everywhere; block sizes are multiples of 64.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define WAVE 64

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float bf2f(bf16 x) { return (float)x; }
__device__ __forceinline__ bf16 f2bf(float x) { return (bf16)x; }

// One element of the attention backward's gradient w.r.t. the combiner
// output: bf16(attn*dcv + ds*a).  Written out with contraction off — the
// ds*a product is rounded, then one FMA adds attn*dcv — which is what the
// dense attention_bwd_kernel has always compiled to.  attention_bwd (dense
// form) and the dout-recomputing combiner backward both call it, so the
// tensor the former writes and the registers the latter rebuilds hold the
// same bits whatever the surrounding code or compiler version.
__device__ __forceinline__ bf16 dccv_elem(float at, float dcv, float dsc,
                                          float a) {
#pragma clang fp contract(off)
  const float t = dsc * a;
  return f2bf(__builtin_fmaf(at, dcv, t));
}

// ---------------------------------------------------------------------------
// Counter-based RNG for dropout masks: deterministic, stateless, cheap
// (32-bit finalizer; the backward never replays it — the mask is recovered
// from the saved forward output, so only mask-distribution quality matters).
__device__ __forceinline__ float rng_uniform(unsigned long long seed,
                                             unsigned long long idx) {
  unsigned int h = (unsigned int)(idx ^ (idx >> 32)) * 0x9E3779B9u;
  h ^= (unsigned int)seed ^ (unsigned int)(seed >> 32) * 0x85EBCA6Bu;
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return (float)(h >> 8) * (1.0f / 16777216.0f);
}

// tanh via one v_exp (exact identity; skips libm's precise-path branches):
// tanh(x) = sign(x) * (1 - 2/(e^{2|x|} + 1))
__device__ __forceinline__ float fast_tanh(float x) {
  const float ax = fabsf(x);
  const float t = 1.0f - 2.0f / (__expf(2.0f * ax) + 1.0f);
  return copysignf(t, x);
}

// ---------------------------------------------------------------------------
// Wave reductions (64-wide).
__device__ __forceinline__ float wave_reduce_sum(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

__device__ __forceinline__ float wave_reduce_max(float x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off));
  return x;
}

// Reduce within 16-lane groups (lanes l..l+15 with the same l>>4).
__device__ __forceinline__ float group16_reduce_sum(float x) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

// One lane's share of a ccv-row dot product: s + sum_j v[j]*vec[j], j in
// order.  Written out with contraction off — each product is rounded, then
// added — which is what attention_fwd_kernel's phase 1 has always compiled
// to (packed multiplies feeding a chain of adds, no FMA).  The attention
// kernels and the combiner's score epilogue all go through it, so a score
// has the same bits wherever it is computed.
__device__ __forceinline__ float row_dot8(bf16x8 v, const float* vec,
                                          float s) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float t = bf2f(v[j]) * vec[j];
    s = s + t;
  }
  return s;
}

// per-16-lane-group dot of a ccv row against a vector
// (each lane covers cols (l&15)*8 + j + 128*i)
__device__ __forceinline__ float group_row_dot(const bf16* row,
                                               const float* vec, int EP,
                                               int lane16) {
  float s = 0.f;
  for (int e0 = lane16 * 8; e0 < EP; e0 += 128)
    s = row_dot8(*(const bf16x8*)(row + e0), vec + e0, s);
  return s;
}

// masked-score fill of the attention pools (reference NINF)
#define NINF_F (-3.4e38f)

// Block softmax over scores[C], in place (scores -> attn probabilities),
// also written to attn_out[base + c].  Shared by attention.hip and
// attention_packed.hip.  A thread touches only the entries c = tid + k *
// blockDim.x in every pass, so ``scores`` may be LDS or the block's own
// slice of attn_out (scores == attn_out + base).  red: >= 16 floats of LDS.
__device__ __forceinline__ void block_softmax(float* scores, float* red,
                                              float* attn_out, int C,
                                              long base) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int nwaves = blockDim.x / WAVE;
  float m = NINF_F;
  for (int c = threadIdx.x; c < C; c += blockDim.x) m = fmaxf(m, scores[c]);
  m = wave_reduce_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (wave == 0) {
    float v = lane < nwaves ? red[lane] : NINF_F;
    v = wave_reduce_max(v);
    if (lane == 0) red[0] = v;
  }
  __syncthreads();
  m = red[0];
  float ssum = 0.f;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float e = __expf(scores[c] - m);
    scores[c] = e;
    ssum += e;
  }
  ssum = wave_reduce_sum(ssum);
  if (lane == 0) red[8 + wave] = ssum;
  __syncthreads();
  if (wave == 0) {
    float v = lane < nwaves ? red[8 + lane] : 0.f;
    v = wave_reduce_sum(v);
    if (lane == 0) red[8] = v;
  }
  __syncthreads();
  const float inv_sum = 1.0f / red[8];
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    scores[c] *= inv_sum;
    attn_out[base + c] = scores[c];
  }
  __syncthreads();
}

// fp32 atomic add using the native global_atomic_add_f32 (no CAS loop).
__device__ __forceinline__ void atomic_add_f32(float* p, float v) {
  unsafeAtomicAdd(p, v);
}

#define C2V_CHECK_LAUNCH()                                                     \
  do {                                                                         \
    hipError_t e_ = hipGetLastError();                                         \
    if (e_ != hipSuccess) {                                                    \
      printf("kernel launch failed: %s\n", hipGetErrorString(e_));             \
    }                                                                          \
  } while (0)
