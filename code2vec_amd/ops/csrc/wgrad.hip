// K14 (wgrad): dW[KP, EP] = X^T[KP, M] @ dZ[M, EP] — the combiner weight
// gradient.  hipBLASLt leaves ~3.5x on the table for this skinny big-K shape
// (K = M up to 204800), so it is hand-written: split-K over blocks, each
// block MFMA-accumulates a full [KP, EP] fp32 partial over its row chunk and
// writes one partials slab (no atomics); host sums slabs (deterministic).
//
// Geometry: 512 threads = 8 waves; wave w owns KP-tiles [IT*w, IT*(w+1))
// where IT = (KP/16)/8; LDS stages per 32-row K-step: the X tile [32, KP]
// and dZ tile [32, EP], both repacked into MFMA-fragment images.
//
// MFMA 16x16x32_bf16 fragment maps (same as combiner.hip):
//   A: lane l holds A[i = l&15][k = (l>>4)*8 + j]  -> A = X^T: X[m][kp]
//   B: lane l holds B[k = (l>>4)*8 + j][col = l&15] -> dZ[m][ep]
//   C/D: lane l, reg r holds C[i = (l>>4)*4 + r][col = l&15]

#include <cstdlib>

#include "common.h"

// GATHER=1: the X operand is re-gathered from the embedding tables during
// staging (the fused forward never materializes the concat tensor).
template <int NT, int IT, int GATHER, int MINW = 1>
__global__ __launch_bounds__(512, MINW) void wgrad_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ dZ,
    float* __restrict__ partials, long M, int KP, int EP, long rows_per_block,
    const int* __restrict__ g_starts, const int* __restrict__ g_paths,
    const int* __restrict__ g_ends, const bf16* __restrict__ g_term,
    const bf16* __restrict__ g_path, int TS, int PS) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const long m0 = (long)blockIdx.x * rows_per_block;
  const long m1 = min(m0 + rows_per_block, M);

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // double-buffered fragment images:
  //   x_img [2][KP/16 tiles][64 lanes][8], dz_img [2][NT][64][8]
  // per-n-tile stride padded by 8 elements (16 B) so repack writes spread
  // across banks (unpadded 1024-B stride puts all 16 writers on one bank)
  const size_t NSTRIDE = 64 * 8 + 8;
  const size_t xsz = (size_t)(KP / 16) * NSTRIDE;
  bf16* x_img = (bf16*)smem;
  bf16* dz_img = x_img + 2 * xsz;  // [2][NT][NSTRIDE]

  f32x4 acc[IT][NT];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  // T14 split staging: issue the next K-step's global loads into registers
  // before this K-step's MFMAs, write them to the other LDS buffer after.
  constexpr int CX = 4;  // max 16-B x chunks/thread (KP <= 512, 512 thr)
  uint4 xr[CX];
  uint4 dzr;  // EP <= 128 -> exactly one dz chunk/thread
  auto stage_load = [&](long mb) {
    const int rows = (int)min((long)32, m1 - mb);
    const int chunks_x = 32 * KP / 8;
#pragma unroll
    for (int i = 0; i < CX; ++i) {
      const int c = threadIdx.x + i * 512;
      uint4 v = {0, 0, 0, 0};
      if (c < chunks_x) {
        const int krow = c / (KP / 8);
        const int col8 = (c % (KP / 8)) * 8;
        if (krow < rows) {
          if (GATHER) {
            const long r = mb + krow;
            if (col8 < TS)
              v = *(const uint4*)(g_term + (size_t)g_starts[r] * TS + col8);
            else if (col8 < TS + PS)
              v = *(const uint4*)(g_path + (size_t)g_paths[r] * PS + col8 - TS);
            else if (col8 < 2 * TS + PS)
              v = *(const uint4*)(g_term + (size_t)g_ends[r] * TS + col8 -
                                  TS - PS);
          } else {
            v = *(const uint4*)(X + (mb + krow) * KP + col8);
          }
        }
      }
      xr[i] = v;
    }
    {
      const int c = threadIdx.x;
      uint4 v = {0, 0, 0, 0};
      if (c < 32 * EP / 8) {
        const int krow = c / (EP / 8);
        if (krow < rows)
          v = *(const uint4*)(dZ + (mb + krow) * EP + (c % (EP / 8)) * 8);
      }
      dzr = v;
    }
  };
  auto stage_write = [&](int buf) {
    const int chunks_x = 32 * KP / 8;
#pragma unroll
    for (int i = 0; i < CX; ++i) {
      const int c = threadIdx.x + i * 512;
      if (c < chunks_x) {
        const int krow = c / (KP / 8);
        const int col8 = (c % (KP / 8)) * 8;
        bf16 vals[8];
        *(uint4*)vals = xr[i];
        const int n = col8 / 16;
        const int base_l = (col8 & 15) + (krow >> 3) * 16;
        const int jslot = krow & 7;
        bf16* dst = x_img + buf * xsz + (size_t)n * NSTRIDE;
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[(base_l + j) * 8 + jslot] = vals[j];
      }
    }
    {
      const int c = threadIdx.x;
      if (c < 32 * EP / 8) {
        const int krow = c / (EP / 8);
        const int col8 = (c % (EP / 8)) * 8;
        bf16 vals[8];
        *(uint4*)vals = dzr;
        const int n = col8 / 16;
        const int base_l = (col8 & 15) + (krow >> 3) * 16;
        const int jslot = krow & 7;
        bf16* dst = dz_img + (size_t)buf * NT * NSTRIDE + (size_t)n * NSTRIDE;
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[(base_l + j) * 8 + jslot] = vals[j];
      }
    }
  };

  if (m0 < m1) {
    stage_load(m0);
    stage_write(0);
    __syncthreads();
  }
  int buf = 0;
  for (long mb = m0; mb < m1; mb += 32) {
    if (mb + 32 < m1) stage_load(mb + 32);
    // MFMA: wave w covers KP-tiles [IT*w .. IT*w+IT)
    bf16x8 bfrag[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
      bfrag[n] = *(const bf16x8*)(dz_img + (size_t)buf * NT * NSTRIDE +
                                  (size_t)n * NSTRIDE + (size_t)lane * 8);
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int itile = IT * wave + i;
      if (itile >= KP / 16) break;
      const bf16x8 a = *(const bf16x8*)(x_img + buf * xsz +
                                        (size_t)itile * NSTRIDE +
                                        (size_t)lane * 8);
#pragma unroll
      for (int n = 0; n < NT; ++n)
        acc[i][n] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bfrag[n], acc[i][n], 0, 0, 0);
    }
    if (mb + 32 < m1) stage_write(buf ^ 1);
    buf ^= 1;
    __syncthreads();
  }

  // write this block's fp32 partial slab [KP, EP]
  float* slab = partials + (size_t)blockIdx.x * KP * EP;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int itile = IT * wave + i;
    if (itile >= KP / 16) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = itile * 16 + (lane >> 4) * 4 + r;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int col = n * 16 + (lane & 15);
        slab[(size_t)row * EP + col] = acc[i][n][r];
      }
    }
  }
}

// PIPELINED wgrad (X given, no gather): the same slabs, the same
// per-accumulator MFMA order (32-row K-steps ascending) — bit-identical
// partials — with H 32-row K-steps staged per loop iteration, so H times
// the bytes are in flight per CU while the MFMAs run (one block per CU:
// 28 KB per 32-row step at KP = 320).  Rows past the block's range stage
// as zeros, as before; a zero K-step leaves the accumulators unchanged.
template <int NT, int IT, int H>
__global__ __launch_bounds__(512) void wgrad_pipe_kernel(
    const bf16* __restrict__ X, const bf16* __restrict__ dZ,
    float* __restrict__ partials, long M, int KP, int EP,
    long rows_per_block) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const long m0 = (long)blockIdx.x * rows_per_block;
  const long m1 = min(m0 + rows_per_block, M);

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // fragment images per 32-row K-step, double-buffered per stage:
  //   x_img [2][H][KP/16 tiles][NSTRIDE], dz_img [2][H][NT][NSTRIDE]
  const size_t NSTRIDE = 64 * 8 + 8;
  const size_t xsz = (size_t)(KP / 16) * NSTRIDE;
  const size_t dsz = (size_t)NT * NSTRIDE;
  bf16* x_img = (bf16*)smem;
  bf16* dz_img = x_img + 2 * H * xsz;

  f32x4 acc[IT][NT];
#pragma unroll
  for (int i = 0; i < IT; ++i)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[i][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int CX = 4;  // max 16-B x chunks/thread/K-step (KP <= 512)
  uint4 xr[H][CX];
  uint4 dzr[H];
  auto stage_load = [&](long mb) {
    const int chunks_x = 32 * KP / 8;
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const long mh = mb + h * 32;
      const int rows = (int)max((long)0, min((long)32, m1 - mh));
#pragma unroll
      for (int i = 0; i < CX; ++i) {
        const int c = threadIdx.x + i * 512;
        uint4 v = {0, 0, 0, 0};
        if (c < chunks_x) {
          const int krow = c / (KP / 8);
          const int col8 = (c % (KP / 8)) * 8;
          if (krow < rows) v = *(const uint4*)(X + (mh + krow) * KP + col8);
        }
        xr[h][i] = v;
      }
      {
        const int c = threadIdx.x;
        uint4 v = {0, 0, 0, 0};
        if (c < 32 * EP / 8) {
          const int krow = c / (EP / 8);
          if (krow < rows)
            v = *(const uint4*)(dZ + (mh + krow) * EP + (c % (EP / 8)) * 8);
        }
        dzr[h] = v;
      }
    }
  };
  auto stage_write = [&](int buf) {
    const int chunks_x = 32 * KP / 8;
#pragma unroll
    for (int h = 0; h < H; ++h) {
#pragma unroll
      for (int i = 0; i < CX; ++i) {
        const int c = threadIdx.x + i * 512;
        if (c < chunks_x) {
          const int krow = c / (KP / 8);
          const int col8 = (c % (KP / 8)) * 8;
          bf16 vals[8];
          *(uint4*)vals = xr[h][i];
          const int n = col8 / 16;
          const int base_l = (col8 & 15) + (krow >> 3) * 16;
          const int jslot = krow & 7;
          bf16* dst = x_img + (buf * H + h) * xsz + (size_t)n * NSTRIDE;
#pragma unroll
          for (int j = 0; j < 8; ++j) dst[(base_l + j) * 8 + jslot] = vals[j];
        }
      }
      {
        const int c = threadIdx.x;
        if (c < 32 * EP / 8) {
          const int krow = c / (EP / 8);
          const int col8 = (c % (EP / 8)) * 8;
          bf16 vals[8];
          *(uint4*)vals = dzr[h];
          const int n = col8 / 16;
          const int base_l = (col8 & 15) + (krow >> 3) * 16;
          const int jslot = krow & 7;
          bf16* dst = dz_img + (buf * H + h) * dsz + (size_t)n * NSTRIDE;
#pragma unroll
          for (int j = 0; j < 8; ++j) dst[(base_l + j) * 8 + jslot] = vals[j];
        }
      }
    }
  };

  if (m0 < m1) {
    stage_load(m0);
    stage_write(0);
    __syncthreads();
  }
  int buf = 0;
  for (long mb = m0; mb < m1; mb += 32 * H) {
    const bool more = mb + 32 * H < m1;
    if (more) stage_load(mb + 32 * H);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      bf16x8 bfrag[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n)
        bfrag[n] = *(const bf16x8*)(dz_img + (buf * H + h) * dsz +
                                    (size_t)n * NSTRIDE + (size_t)lane * 8);
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const int itile = IT * wave + i;
        if (itile >= KP / 16) break;
        const bf16x8 a = *(const bf16x8*)(x_img + (buf * H + h) * xsz +
                                          (size_t)itile * NSTRIDE +
                                          (size_t)lane * 8);
#pragma unroll
        for (int n = 0; n < NT; ++n)
          acc[i][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, bfrag[n], acc[i][n], 0, 0, 0);
      }
    }
    if (more) stage_write(buf ^ 1);
    buf ^= 1;
    __syncthreads();
  }

  // write this block's fp32 partial slab [KP, EP]
  float* slab = partials + (size_t)blockIdx.x * KP * EP;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int itile = IT * wave + i;
    if (itile >= KP / 16) break;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = itile * 16 + (lane >> 4) * 4 + r;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int col = n * 16 + (lane & 15);
        slab[(size_t)row * EP + col] = acc[i][n][r];
      }
    }
  }
}

extern "C" {

void launch_wgrad_impl(const void* X, const void* dZ, float* partials,
                  long M, int KP, int EP, int nblocks, const int* starts,
                  const int* paths, const int* ends, const void* term,
                  const void* path, int TS, int PS, hipStream_t stream) {
  const long rows_per_block = ((M + nblocks - 1) / nblocks + 31) / 32 * 32;
  const int smem = 2 * ((KP / 16) + (EP / 16)) * (64 * 8 + 8) * 2;
  const int NT = EP / 16;
  const int IT = (KP / 16 + 7) / 8;
  // C2V_WGRAD_OCC=3/4 forces a waves/SIMD register cap (occupancy A/B;
  // 512-thread blocks make 4 the only level that adds a resident block)
  const char* occ_env = getenv("C2V_WGRAD_OCC");
  const int occ = occ_env ? atoi(occ_env) : 0;
  // supported shapes: KP/16 divisible into 8 waves; dispatch common cases
#define WCASE(nt, it)                                                        \
  if (NT == nt && IT == it) {                                                \
    if (starts)                                                              \
      wgrad_kernel<nt, it, 1><<<nblocks, 512, smem, stream>>>(               \
          nullptr, (const bf16*)dZ, partials, M, KP, EP, rows_per_block,     \
          starts, paths, ends, (const bf16*)term, (const bf16*)path, TS,     \
          PS);                                                               \
    else if (occ == 4)                                                       \
      wgrad_kernel<nt, it, 0, 4><<<nblocks, 512, smem, stream>>>(            \
          (const bf16*)X, (const bf16*)dZ, partials, M, KP, EP,              \
          rows_per_block, nullptr, nullptr, nullptr, nullptr, nullptr, 0,    \
          0);                                                                \
    else if (occ == 3)                                                       \
      wgrad_kernel<nt, it, 0, 3><<<nblocks, 512, smem, stream>>>(            \
          (const bf16*)X, (const bf16*)dZ, partials, M, KP, EP,              \
          rows_per_block, nullptr, nullptr, nullptr, nullptr, nullptr, 0,    \
          0);                                                                \
    else                                                                     \
      wgrad_kernel<nt, it, 0><<<nblocks, 512, smem, stream>>>(               \
          (const bf16*)X, (const bf16*)dZ, partials, M, KP, EP,              \
          rows_per_block, nullptr, nullptr, nullptr, nullptr, nullptr, 0,    \
          0);                                                                \
    return;                                                                  \
  }
  // NT > 8 (encode > 128) overflows the register budget -> callers fall
  // back to rocBLAS for those shapes (ops/functional.py gates on EP <= 128).
  WCASE(8, 1) WCASE(8, 2) WCASE(8, 3) WCASE(8, 4)
  WCASE(6, 1) WCASE(6, 2) WCASE(6, 3) WCASE(6, 4)
  WCASE(4, 1) WCASE(4, 2) WCASE(4, 3) WCASE(4, 4)
  WCASE(2, 1) WCASE(2, 2) WCASE(2, 3) WCASE(2, 4)
#undef WCASE
  printf("wgrad: unsupported KP=%d EP=%d\n", KP, EP);
}

void launch_wgrad(const void* X, const void* dZ, float* partials, long M,
                  int KP, int EP, int nblocks, hipStream_t stream) {
  launch_wgrad_impl(X, dZ, partials, M, KP, EP, nblocks, nullptr, nullptr,
                    nullptr, nullptr, nullptr, 0, 0, stream);
}

// Pipelined split-K wgrad: h = 32-row K-steps per stage (2 or 3), 0 =
// C2V_WGRAD_DEPTH or the shipped default.  Returns false where there is no
// instantiation (callers then use launch_wgrad).
bool launch_wgrad_pipe(const void* X, const void* dZ, float* partials, long M,
                       int KP, int EP, int nblocks, int h,
                       hipStream_t stream) {
  if (h == 0) {
    const char* de = getenv("C2V_WGRAD_DEPTH");
    h = de ? atoi(de) : 2;
  }
  const long rows_per_block = ((M + nblocks - 1) / nblocks + 31) / 32 * 32;
  const int NT = EP / 16;
  const int IT = (KP / 16 + 7) / 8;
  if (EP % 16 || KP % 16 || EP > 128 || KP > 512) return false;
  const int smem = 2 * h * ((KP / 16) + NT) * (64 * 8 + 8) * 2;
  if (smem > 160 * 1024) return false;
#define WPCASE(nt, it, hh)                                                   \
  if (NT == nt && IT == it && h == hh) {                                     \
    auto kern = wgrad_pipe_kernel<nt, it, hh>;                               \
    static int attr_smem = 0; /* > 64 KB of dynamic LDS is opt-in */         \
    if (smem > 65536 && smem > attr_smem) {                                  \
      hipFuncSetAttribute((const void*)kern,                                 \
                          hipFuncAttributeMaxDynamicSharedMemorySize, smem); \
      attr_smem = smem;                                                      \
    }                                                                        \
    kern<<<nblocks, 512, smem, stream>>>((const bf16*)X, (const bf16*)dZ,    \
                                         partials, M, KP, EP,                \
                                         rows_per_block);                    \
    return true;                                                             \
  }
  WPCASE(8, 1, 2) WPCASE(8, 2, 2) WPCASE(8, 3, 2) WPCASE(8, 4, 2)
#undef WPCASE
  return false;
}

void launch_wgrad_gather(const int* starts, const int* paths,
                         const int* ends, const void* term, const void* path,
                         int TS, int PS, const void* dZ, float* partials,
                         long M, int KP, int EP, int nblocks,
                         hipStream_t stream) {
  launch_wgrad_impl(nullptr, dZ, partials, M, KP, EP, nblocks, starts, paths,
                    ends, term, path, TS, PS, stream);
}

}  // extern "C"
