// Column sum of a bf16 [B, L] matrix -> fp32 [L] (output-head bias grad:
// dbias = sum_b dlogits[b, :]).  torch's generic reduce runs this at
// ~1 TB/s; a simple row-looped, column-parallel kernel streams at HBM BW.
// Blocks tile (L-chunk x row-chunk); row-chunk partials combine with one
// fp32 atomic per column per row-chunk (few per column).

#include "common.h"

__global__ __launch_bounds__(256) void colsum_bf16_kernel(
    const bf16* __restrict__ x, float* __restrict__ out, long B, long L,
    int rows_per_block) {
  const long col = (long)(blockIdx.x % ((L + 255) / 256)) * 256 + threadIdx.x;
  const int rchunk = blockIdx.x / ((L + 255) / 256);
  if (col >= L) return;
  const long r0 = (long)rchunk * rows_per_block;
  const long r1 = min(r0 + rows_per_block, B);
  float acc = 0.f;
  for (long b = r0; b < r1; ++b) acc += bf2f(x[b * L + col]);
  atomic_add_f32(out + col, acc);
}

// Tiny partial-slab reduce: p[S, N] f32 -> out[N] f32, one block per
// column (N is small: EP/KP-scale; S <= ~1024 reduction-partial rows).
// torch's generic reduce spends 10 us per call on these; this is ~2 us.
// The per-column reduction tree is one device function: thread t adds rows
// t, t+256, ... in ascending order, then the 64-lane xor tree, then the
// four wave sums in wave order.  Every kernel below goes through it, so
// they all produce the same bits for the same column.
__device__ __forceinline__ float slab_col_sum(const float* __restrict__ p,
                                              int S, int N, int col,
                                              float* red) {
  float acc = 0.f;
  for (int s = threadIdx.x; s < S; s += 256)
    acc += p[(long)s * N + col];
  acc = wave_reduce_sum(acc);
  const int wave = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) red[wave] = acc;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void slab_sum_f32_kernel(
    const float* __restrict__ p, float* __restrict__ out, int S, int N) {
  __shared__ float red[4];
  const float v = slab_col_sum(p, S, N, blockIdx.x, red);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// Two slab sums in one launch (dgamma and dbeta partials): blocks [0, N)
// reduce p0 into out0, blocks [N, 2N) reduce p1 into out1.
__global__ __launch_bounds__(256) void slab_sum2_f32_kernel(
    const float* __restrict__ p0, const float* __restrict__ p1,
    float* __restrict__ out0, float* __restrict__ out1, int S, int N) {
  __shared__ float red[4];
  const bool second = (int)blockIdx.x >= N;
  const int col = second ? blockIdx.x - N : blockIdx.x;
  const float v = slab_col_sum(second ? p1 : p0, S, N, col, red);
  if (threadIdx.x == 0) (second ? out1 : out0)[col] = v;
}

// Loss partials acc_p[S, 2] -> acc[2] = (sum w_y*nll, sum w_y) and
// loss = acc[0] / acc[1] (correctly rounded division), one block.
__global__ __launch_bounds__(256) void loss_reduce_kernel(
    const float* __restrict__ acc_p, float* __restrict__ acc,
    float* __restrict__ loss, int S) {
  __shared__ float red0[4];
  __shared__ float red1[4];
  const float a0 = slab_col_sum(acc_p, S, 2, 0, red0);
  const float a1 = slab_col_sum(acc_p, S, 2, 1, red1);
  if (threadIdx.x == 0) {
    acc[0] = a0;
    acc[1] = a1;
    loss[0] = __fdiv_rn(a0, a1);
  }
}

// wgrad split-K partials [S, KP, EP] f32 -> dw [EP, KP] bf16: slab sum,
// transpose and cast in one launch.  Block = 256 threads = 8 slab groups
// x 32 lanes; tile = 4 kp rows x 32 e columns, lane l holds the float4 at
// (kp0 + l/8, e0 + (l%8)*4), so each slab read is four full 128-B lines.
// SUMMATION ORDER (fixed): with per = ceil(S/8), group g adds slabs
// g*per .. min(S, (g+1)*per)-1 one by one in ascending order onto 0.0f
// (loads issued 8 at a time, adds in slab order); the eight group sums
// are then added in ascending g, ((g0+g1)+g2)+...+g7, through LDS; the
// result is rounded to bf16 once.  The transposed store also goes through
// LDS: 32 threads each write the 4 kp values of one e column (8 B).
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(
    const float* __restrict__ partials, bf16* __restrict__ dw, int S, int KP,
    int EP) {
  __shared__ f32x4 red[8][32];
  __shared__ float tile[4][33];
  const int etiles = EP / 32;
  const int kp0 = ((int)blockIdx.x / etiles) * 4;
  const int e0 = ((int)blockIdx.x % etiles) * 32;
  const int g = threadIdx.x >> 5;
  const int l = threadIdx.x & 31;
  const int per = (S + 7) / 8;
  const int s_lo = g * per;
  const int s_hi = min(S, s_lo + per);
  const size_t slab = (size_t)KP * EP;
  const float* src =
      partials + (size_t)(kp0 + (l >> 3)) * EP + e0 + (l & 7) * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = s_lo; s < s_hi; s += 8) {
    f32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (s + k < s_hi)
        v[k] = __builtin_nontemporal_load(
            (const f32x4*)(src + (size_t)(s + k) * slab));
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (s + k < s_hi) acc += v[k];
  }
  red[g][l] = acc;
  __syncthreads();
  if (g == 0) {
    f32x4 t = red[0][l];
#pragma unroll
    for (int k = 1; k < 8; ++k) t += red[k][l];
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[l >> 3][(l & 7) * 4 + j] = t[j];
  }
  __syncthreads();
  if (threadIdx.x < 32) {
    bf16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = f2bf(tile[r][threadIdx.x]);
    *(bf16x4*)(dw + (size_t)(e0 + threadIdx.x) * KP + kp0) = o;
  }
}

// K17: row max+argmax over bf16 logits (eval-path prediction).  One block
// per row; ties resolve to the SMALLEST index (torch.max semantics).
__global__ __launch_bounds__(256) void row_max_argmax_kernel(
    const bf16* __restrict__ x, float* __restrict__ vals,
    long* __restrict__ idx, long L) {
  const bf16* row = x + (long)blockIdx.x * L;
  float best = -3.4e38f;
  long bi = 0;
  for (long j = threadIdx.x; j < L; j += 256) {
    const float v = bf2f(row[j]);
    if (v > best || (v == best && j < bi)) {
      best = v;
      bi = j;
    }
  }
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off);
    const long oi = (long)__shfl_xor((long long)bi, off);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  __shared__ float rv[4];
  __shared__ long ri[4];
  if (lane == 0) {
    rv[wave] = best;
    ri[wave] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      if (rv[w] > best || (rv[w] == best && ri[w] < bi)) {
        best = rv[w];
        bi = ri[w];
      }
    }
    vals[blockIdx.x] = best;
    idx[blockIdx.x] = bi;
  }
}

extern "C" {

void launch_row_max_argmax(const void* x, float* vals, long* idx, long B,
                           long L, hipStream_t stream) {
  row_max_argmax_kernel<<<B, 256, 0, stream>>>((const bf16*)x, vals, idx,
                                               L);
}

void launch_slab_sum_f32(const float* p, float* out, int S, int N,
                         hipStream_t stream) {
  slab_sum_f32_kernel<<<N, 256, 0, stream>>>(p, out, S, N);
}

void launch_slab_sum2_f32(const float* p0, const float* p1, float* out0,
                          float* out1, int S, int N, hipStream_t stream) {
  slab_sum2_f32_kernel<<<2 * N, 256, 0, stream>>>(p0, p1, out0, out1, S, N);
}

void launch_loss_reduce(const float* acc_p, float* acc, float* loss, int S,
                        hipStream_t stream) {
  loss_reduce_kernel<<<1, 256, 0, stream>>>(acc_p, acc, loss, S);
}

// requires KP % 4 == 0 and EP % 32 == 0 (checked by the binding)
void launch_wgrad_reduce(const float* partials, void* dw, int S, int KP,
                         int EP, hipStream_t stream) {
  wgrad_reduce_kernel<<<(KP / 4) * (EP / 32), 256, 0, stream>>>(
      partials, (bf16*)dw, S, KP, EP);
}


void launch_colsum_bf16(const void* x, float* out, long B, long L,
                        hipStream_t stream) {
  const int rows_per_block = 32;  // wider grid: latency-bound otherwise
  const int lblocks = (int)((L + 255) / 256);
  const int rblocks = (int)((B + rows_per_block - 1) / rows_per_block);
  colsum_bf16_kernel<<<lblocks * rblocks, 256, 0, stream>>>(
      (const bf16*)x, out, B, L, rows_per_block);
}

}  // extern "C"
