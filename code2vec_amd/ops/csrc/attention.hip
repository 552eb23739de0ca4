// K7-K9 fused single-query attention + weighted pool, forward and backward.
// Reference math: model/model.py:62-69,90-105 —
//   scores[b,c] = sum_e ccv[b,c,e] * a[e]
//   scores = scores*mask + (1-mask)*NINF      (mask = starts>0; NINF=-3.4e38)
//   attn = softmax(scores, dim=C)
//   cv[b,e] = sum_c attn[b,c] * ccv[b,c,e]
//
// One workgroup (256 threads = 4 waves) per batch row; the [C, EP] ccv
// slice is staged in LDS once and reused by every phase.  Work is
// row-oriented: each 16-lane group owns one context at a time (8 columns
// per lane -> bf16x8 vector accesses, coalesced global writes in backward).

#include "common.h"

// ---------------------------------------------------------------------------
// ts = round8(E) <= EP: only the valid columns are staged/dotted — the
// EP-pad columns of ccv are zero and a/dcv pad is zero, so they never
// contribute; trimming them keeps the tile under the 53.3-KB line for
// 3 blocks/CU (54.8 KB = 2 blocks, a 33% occupancy loss).  Outputs in
// [ts, EP) are written as explicit zeros.
template <bool STAGE_LDS>
__global__ __launch_bounds__(256) void attention_fwd_kernel(
    const bf16* __restrict__ ccv, const float* __restrict__ a,
    const int* __restrict__ starts, float* __restrict__ cv,
    bf16* __restrict__ cvb, float* __restrict__ attn, int B, int C, int EP,
    int E, int ts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // layout: [ccv tile (opt)] [a f32 EP] [scores C] [red 64] [partials 4*EP]
  bf16* tile = (bf16*)smem;
  float* lds_a = (float*)(smem + (STAGE_LDS ? (size_t)C * ts * 2 : 0));
  float* scores = lds_a + EP;
  float* red = scores + C;
  float* partials = red + 64;
  const int rstride = STAGE_LDS ? ts : EP;  // tile vs global row stride

  // persistent grid: only 3 blocks fit per CU at this LDS size, so a
  // block-per-method grid (B=1024) runs an underfilled tail round;
  // looping methods over occupancy*CU blocks balances across CUs
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
  const bf16* src = ccv + (long)b * C * EP;
  for (int e = threadIdx.x; e < EP; e += blockDim.x) lds_a[e] = a[e];
  if (STAGE_LDS) {
    const int row_chunks = ts / 8;
    const int total = C * row_chunks;
    const uint4* s4 = (const uint4*)src;
    uint4* d4 = (uint4*)tile;
    for (int i = threadIdx.x; i < total; i += blockDim.x)
      d4[i] = s4[(i / row_chunks) * (EP / 8) + i % row_chunks];
  }
  __syncthreads();

  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int lane16 = lane & 15;
  const int group = (threadIdx.x >> 4);  // 16 groups of 16 lanes

  // phase 1: scores — each 16-lane group owns one context per iteration
  for (int c = group; c < C; c += 16) {
    const bf16* row = (STAGE_LDS ? tile : src) + (long)c * rstride;
    float s = group_row_dot(row, lds_a, ts, lane16);
    s = group16_reduce_sum(s);
    if (lane16 == 0) {
      const float mask = starts[(long)b * C + c] > 0 ? 1.0f : 0.0f;
      scores[c] = s * mask + (1.0f - mask) * NINF_F;
    }
  }
  __syncthreads();

  // phase 2: softmax (scores -> attn probabilities, also written out)
  block_softmax(scores, red, attn, C, (long)b * C);

  // phase 3: cv[e] = sum_c attn[c]*ccv[c,e] — each wave accumulates a
  // contiguous context span into per-lane column pairs, then cross-wave sum
  const int span = (C + 3) / 4;
  const int c_lo = wave * span;
  const int c_hi = min(C, c_lo + span);
  for (int e0 = lane * 2; e0 < EP; e0 += WAVE * 2) {
    float acc0 = 0.f, acc1 = 0.f;
    if (e0 < ts) {
      for (int c = c_lo; c < c_hi; ++c) {
        const bf16* row = (STAGE_LDS ? tile : src) + (long)c * rstride;
        const bf16x2 v = *(const bf16x2*)(row + e0);
        const float at = scores[c];
        acc0 += at * bf2f(v[0]);
        acc1 += at * bf2f(v[1]);
      }
    }
    partials[wave * EP + e0] = acc0;
    partials[wave * EP + e0 + 1] = acc1;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < EP; e += blockDim.x) {
    const float s = partials[e] + partials[EP + e] + partials[2 * EP + e] +
                    partials[3 * EP + e];
    cv[(long)b * EP + e] = s;
    // optional bf16 copy for the output head (saves a cast kernel)
    if (cvb) cvb[(long)b * EP + e] = f2bf(s);
  }
  __syncthreads();  // smem reused by the next method
  }
}

// ---------------------------------------------------------------------------
// Backward.  g[c] = dot(dcv, ccv[c]) (+ dattn[c]); sum_g = sum_c attn[c]*g[c];
// ds[c] = attn[c]*(g[c]-sum_g)*mask;  dccv[c,e] = attn[c]*dcv[e] + ds[c]*a[e];
// da[e] = sum_c ds[c]*ccv[c,e]  (per-block partials row, summed host-side).
//
// COMPACT=1 never writes dccv: it stores ds[B*C] (fp32) instead, and the
// combiner backward rebuilds every dccv element from attn, ds, dcv and a
// through dccv_elem() (common.h) — the same function the dense form uses,
// so both produce the same bits.  dcv is fp32, or bf16 when dcv_bf16 is
// set (the output head's gradient read without a cast kernel).
template <bool STAGE_LDS, bool COMPACT>
__global__ __launch_bounds__(256) void attention_bwd_kernel(
    const void* __restrict__ dcv, const float* __restrict__ dattn,
    const bf16* __restrict__ ccv, const float* __restrict__ a,
    const int* __restrict__ starts, const float* __restrict__ attn,
    bf16* __restrict__ dccv, float* __restrict__ ds_out,
    float* __restrict__ da, int B, int C, int EP, int E, int has_dattn,
    int dcv_bf16, int ts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* tile = (bf16*)smem;
  float* lds_dcv = (float*)(smem + (STAGE_LDS ? (size_t)C * ts * 2 : 0));
  float* lds_a = lds_dcv + EP;
  float* ds = lds_a + EP;        // [C]
  float* red = ds + C;           // [64]
  float* partials = red + 64;    // [4][EP] (da)
  const int rstride = STAGE_LDS ? ts : EP;

  // persistent grid (see attention_fwd_kernel)
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
  const bf16* src = ccv + (long)b * C * EP;
  for (int e = threadIdx.x; e < EP; e += blockDim.x) {
    lds_dcv[e] = dcv_bf16 ? bf2f(((const bf16*)dcv)[(long)b * EP + e])
                          : ((const float*)dcv)[(long)b * EP + e];
    lds_a[e] = a[e];
  }
  if (STAGE_LDS) {
    const int row_chunks = ts / 8;
    const int total = C * row_chunks;
    const uint4* s4 = (const uint4*)src;
    uint4* d4 = (uint4*)tile;
    for (int i = threadIdx.x; i < total; i += blockDim.x)
      d4[i] = s4[(i / row_chunks) * (EP / 8) + i % row_chunks];
  }
  __syncthreads();

  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int lane16 = lane & 15;
  const int group = (threadIdx.x >> 4);

  // phase A: g[c] (group-per-context) and block-reduced sum_g
  float part = 0.f;
  for (int c = group; c < C; c += 16) {
    const bf16* row = (STAGE_LDS ? tile : src) + (long)c * rstride;
    float g = group_row_dot(row, lds_dcv, ts, lane16);
    g = group16_reduce_sum(g);
    if (lane16 == 0) {
      if (has_dattn) g += dattn[(long)b * C + c];
      ds[c] = g;  // temporarily g
      part += attn[(long)b * C + c] * g;
    }
  }
  part = wave_reduce_sum(part);
  if (lane == 0) red[wave] = part;
  __syncthreads();
  if (wave == 0) {
    float v = lane < (blockDim.x / WAVE) ? red[lane] : 0.f;
    v = wave_reduce_sum(v);
    if (lane == 0) red[0] = v;
  }
  __syncthreads();
  const float sum_g = red[0];
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float at = attn[(long)b * C + c];
    const float mask = starts[(long)b * C + c] > 0 ? 1.0f : 0.0f;
    const float dsc = at * (ds[c] - sum_g) * mask;
    ds[c] = dsc;
    if (COMPACT) ds_out[(long)b * C + c] = dsc;
  }
  __syncthreads();

  // phase B: dccv rows (group-per-context, coalesced bf16x8 writes; none
  // when COMPACT) and per-lane da partial accumulators
  // da accumulation: this lane's columns are (lane16*8 + j) + 128*i;
  // statically unrolled i (dynamic array indexing would go to scratch)
  float da_acc[3][8] = {};  // EP <= 384
  for (int c = group; c < C; c += 16) {
    const float at = COMPACT ? 0.f : attn[(long)b * C + c];
    const float dsc = ds[c];
    const bf16* row = (STAGE_LDS ? tile : src) + (long)c * rstride;
    bf16* drow = COMPACT ? nullptr : dccv + ((long)b * C + c) * EP;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e0 = lane16 * 8 + 128 * i;
      if (e0 < ts) {
        bf16 v[8], o[8];
        *(uint4*)v = *(const uint4*)(row + e0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (!COMPACT)
            o[j] = dccv_elem(at, lds_dcv[e0 + j], dsc, lds_a[e0 + j]);
          da_acc[i][j] = __builtin_fmaf(dsc, bf2f(v[j]), da_acc[i][j]);
        }
        if (!COMPACT) *(uint4*)(drow + e0) = *(uint4*)o;
      } else if (!COMPACT && e0 < EP) {
        // pad columns: dcv/a pad is zero, so the grad is exactly zero
        const uint4 z = {0, 0, 0, 0};
        *(uint4*)(drow + e0) = z;
      }
    }
  }
  // combine da partials DETERMINISTICALLY: the 4 lane-groups of each
  // wave that share lane16 combine via a fixed shuffle tree, each wave
  // writes its own partials row, and the final 4-way sum runs in fixed
  // wave order.  (The previous LDS atomicAdd combine was ordering-
  // nondeterministic at the fp32 ulp — identical runs diverged after a
  // couple of bf16-rounded optimizer steps.)
  __syncthreads();  // ds/tile reads done; reuse partials region
  for (int e = threadIdx.x; e < 4 * EP; e += blockDim.x)
    if ((e % EP) >= ts) partials[e] = 0.f;  // tail cols no lane writes
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int e_base = lane16 * 8 + 128 * i;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = da_acc[i][j];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (lane < 16 && e_base < ts) partials[wave * EP + e_base + j] = v;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < EP; e += blockDim.x) {
    const float s4v = partials[e] + partials[EP + e] + partials[2 * EP + e] +
                      partials[3 * EP + e];
    da[(long)b * EP + e] = e < E ? s4v : 0.f;
  }
  __syncthreads();  // smem reused by the next method
  }
}

// ---------------------------------------------------------------------------
// Streaming forms for the training path (EP = 128, C <= ATTN_STREAM_MAX_C).
// No LDS tile and no persistent loop: one block per method, every row a
// lane needs is loaded into registers before its first use, so the whole
// method's traffic is in flight at once and LDS (~3 KB) no longer caps
// occupancy — all of B = 1024 methods are resident in one round.  Mappings,
// summation orders and reduction trees are those of the kernels above, so
// the results have the same bits.
#define ATTN_STREAM_MAX_C 200
#define ATTN_STREAM_SPAN ((ATTN_STREAM_MAX_C + 3) / 4)    // rows per wave
#define ATTN_STREAM_ROWS ((ATTN_STREAM_MAX_C + 15) / 16)  // rows per group

// Forward with phase 1 done elsewhere: raw_scores[b, c] = ccv[b, c] . a is
// produced by the combiner's epilogue (combiner.hip, SCORES = 1) through
// row_dot8 + group16_reduce_sum, exactly as phase 1 above computes it.
// What is left is mask, softmax and phase 3, which reads ccv once.
__global__ __launch_bounds__(256) void attention_fwd_scores_kernel(
    const bf16* __restrict__ ccv, const float* __restrict__ raw_scores,
    const int* __restrict__ starts, float* __restrict__ cv,
    bf16* __restrict__ cvb, float* __restrict__ attn, int C, int ts) {
  constexpr int EP = 128;
  __shared__ float scores[256];
  __shared__ float red[64];
  __shared__ float partials[4 * EP];
  const int b = blockIdx.x;
  const bf16* src = ccv + (long)b * C * EP;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;

  // thread t owns context t's score (C <= 256).  Issued BEFORE the rows:
  // loads return in order, so the softmax waits only for these two.
  const int ct = min((int)threadIdx.x, C - 1);
  const float s_t = raw_scores[(long)b * C + ct];
  const int st_t = starts[(long)b * C + ct];

  // phase 3's rows, all issued before anything waits: wave w owns contexts
  // [c_lo, c_hi), lane owns columns e0, e0+1
  const int span = (C + 3) / 4;
  const int c_lo = wave * span;
  const int c_hi = min(C, c_lo + span);
  const int e0 = lane * 2;
  // Branch-free: a guarded load becomes a branch with its own wait, which
  // serializes the stream.  Rows past the span re-read row C-1 (in bounds,
  // same lines) and are never used; columns in [ts, EP) exist in memory
  // (pad) and are never used either.  Rows stay raw bf16 pairs until the
  // FMA chain so the prefetch costs one register per row.
  unsigned r[ATTN_STREAM_SPAN];
#pragma unroll
  for (int k = 0; k < ATTN_STREAM_SPAN; ++k)
    r[k] = *(const unsigned*)(src + (long)min(c_lo + k, C - 1) * EP + e0);

  {
    // unconditional (entries >= C are never read): under a branch the
    // compiler sinks the two loads into it, behind the rows
    const float mask = st_t > 0 ? 1.0f : 0.0f;
    scores[threadIdx.x] = s_t * mask + (1.0f - mask) * NINF_F;
  }
  __syncthreads();

  block_softmax(scores, red, attn, C, (long)b * C);

  // phase 3 from registers: sequential in c, one FMA per element (what
  // attention_fwd_kernel's phase 3 compiles to)
  float acc0 = 0.f, acc1 = 0.f;
  if (e0 < ts) {
#pragma unroll
    for (int k = 0; k < ATTN_STREAM_SPAN; ++k) {
      if (c_lo + k < c_hi) {
        const float at = scores[c_lo + k];
        // bf16 -> f32 is the bit pattern moved to the high half
        acc0 = __builtin_fmaf(at, __uint_as_float(r[k] << 16), acc0);
        acc1 = __builtin_fmaf(at, __uint_as_float(r[k] & 0xffff0000u), acc1);
      }
    }
  }
  partials[wave * EP + e0] = acc0;
  partials[wave * EP + e0 + 1] = acc1;
  __syncthreads();
  for (int e = threadIdx.x; e < EP; e += blockDim.x) {
    const float s = partials[e] + partials[EP + e] + partials[2 * EP + e] +
                    partials[3 * EP + e];
    cv[(long)b * EP + e] = s;
    cvb[(long)b * EP + e] = f2bf(s);
  }
}

// Compact backward with the method's rows in registers: 16-lane group g
// owns contexts g, g+16, ... (at most ATTN_STREAM_ROWS of them), a lane
// holds its 8 columns of each as one bf16x8.  Phase A and phase B both
// read those registers.
__global__ __launch_bounds__(256) void attention_bwd_compact_reg_kernel(
    const void* __restrict__ dcv, const float* __restrict__ dattn,
    const bf16* __restrict__ ccv, const int* __restrict__ starts,
    const float* __restrict__ attn, float* __restrict__ ds_out,
    float* __restrict__ da, int C, int E, int has_dattn, int dcv_bf16,
    int ts) {
  constexpr int EP = 128;
  __shared__ __attribute__((aligned(16))) float lds_dcv[EP];
  __shared__ float ds[ATTN_STREAM_ROWS * 16];
  __shared__ float lds_attn[256];
  __shared__ float lds_dattn[256];
  __shared__ float red[64];
  __shared__ float partials[4 * EP];
  const int b = blockIdx.x;
  const bf16* src = ccv + (long)b * C * EP;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int lane16 = lane & 15;
  const int group = (threadIdx.x >> 4);
  const int e0 = lane16 * 8;

  // per-context and per-column inputs first (thread t owns context t and
  // column t & 127): loads return in order, so whatever is issued before
  // the rows can be consumed while the rows are still in flight
  const int ct = min((int)threadIdx.x, C - 1);
  const float at_t = attn[(long)b * C + ct];
  const int st_t = starts[(long)b * C + ct];
  const float dat_t = has_dattn ? dattn[(long)b * C + ct] : 0.f;
  const long dcv_i = (long)b * EP + (threadIdx.x & (EP - 1));
  const float dcv_t = dcv_bf16 ? bf2f(((const bf16*)dcv)[dcv_i])
                               : ((const float*)dcv)[dcv_i];

  // branch-free, as in attention_fwd_scores_kernel: rows past C re-read
  // row C-1 and pad columns are loaded, neither is ever used
  bf16x8 r[ATTN_STREAM_ROWS];
#pragma unroll
  for (int k = 0; k < ATTN_STREAM_ROWS; ++k)
    r[k] = *(const bf16x8*)(src + (long)min(group + 16 * k, C - 1) * EP + e0);
  if (threadIdx.x < EP) lds_dcv[threadIdx.x] = dcv_t;
  lds_attn[threadIdx.x] = at_t;
  lds_dattn[threadIdx.x] = dat_t;
  __syncthreads();

  // phase A: g[c] and block-reduced sum_g
  float part = 0.f;
#pragma unroll
  for (int k = 0; k < ATTN_STREAM_ROWS; ++k) {
    const int c = group + 16 * k;
    if (c < C) {
      float g = e0 < ts ? row_dot8(r[k], lds_dcv + e0, 0.f) : 0.f;
      g = group16_reduce_sum(g);
      if (lane16 == 0) {
        if (has_dattn) g += lds_dattn[c];
        ds[c] = g;  // temporarily g
        part = __builtin_fmaf(lds_attn[c], g, part);
      }
    }
  }
  part = wave_reduce_sum(part);
  if (lane == 0) red[wave] = part;
  __syncthreads();
  if (wave == 0) {
    float v = lane < (blockDim.x / WAVE) ? red[lane] : 0.f;
    v = wave_reduce_sum(v);
    if (lane == 0) red[0] = v;
  }
  __syncthreads();
  const float sum_g = red[0];
  if ((int)threadIdx.x < C) {
    const float mask = st_t > 0 ? 1.0f : 0.0f;
    const float dsc = at_t * (ds[threadIdx.x] - sum_g) * mask;
    ds[threadIdx.x] = dsc;
    ds_out[(long)b * C + threadIdx.x] = dsc;
  }
  __syncthreads();

  // phase B: per-lane da partial accumulators over the group's rows
  float da_acc[8] = {};
#pragma unroll
  for (int k = 0; k < ATTN_STREAM_ROWS; ++k) {
    const int c = group + 16 * k;
    if (c < C && e0 < ts) {
      const float dsc = ds[c];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        da_acc[j] = __builtin_fmaf(dsc, bf2f(r[k][j]), da_acc[j]);
    }
  }
  // deterministic combine, as in attention_bwd_kernel: fixed shuffle tree
  // over the wave's four groups, one partials row per wave, fixed 4-way sum
  for (int e = threadIdx.x; e < 4 * EP; e += blockDim.x)
    if ((e % EP) >= ts) partials[e] = 0.f;  // tail cols no lane writes
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = da_acc[j];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lane < 16 && e0 < ts) partials[wave * EP + e0 + j] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < EP; e += blockDim.x) {
    const float s4v = partials[e] + partials[EP + e] + partials[2 * EP + e] +
                      partials[3 * EP + e];
    da[(long)b * EP + e] = e < E ? s4v : 0.f;
  }
}

// grid = min(B, occupancy * CUs): just enough resident blocks that the
// persistent method loop balances across CUs with no tail round
template <typename K>
static int attn_grid(K kern, size_t smem, int B) {
  static int ncu = 0;
  if (ncu == 0)
    hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0);
  int occ = 0;
  hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, 256, smem);
  if (occ < 1) occ = 1;
  const long g = (long)occ * (ncu > 0 ? ncu : 256);
  return (int)(g < B ? g : B);
}

extern "C" {

static size_t attn_smem(int C, int EP, int ts, bool stage, bool bwd) {
  size_t s = stage ? (size_t)C * ts * 2 : 0;
  s += (size_t)EP * 4;            // a (fwd) / dcv (bwd)
  if (bwd) s += (size_t)EP * 4;   // a (bwd extra)
  s += (size_t)C * 4;             // scores / ds
  s += 64 * 4;                    // reduction scratch
  s += (size_t)4 * EP * 4;        // partials
  return s;
}

static int attn_ts(int E, int EP) {
  int ts = (E + 7) & ~7;
  return ts > EP ? EP : ts;
}

void launch_attention_fwd(const void* ccv, const float* a, const int* starts,
                          float* cv, void* cvb, float* attn, int B, int C,
                          int EP, int E, hipStream_t stream) {
  const int ts = attn_ts(E, EP);
  bool stage = attn_smem(C, EP, ts, true, false) <= 160 * 1024 - 1024;
  size_t smem = attn_smem(C, EP, ts, stage, false);
  if (stage)
    attention_fwd_kernel<true>
        <<<attn_grid(attention_fwd_kernel<true>, smem, B), 256, smem,
           stream>>>((const bf16*)ccv, a, starts, cv, (bf16*)cvb, attn, B, C, EP,
                     E, ts);
  else
    attention_fwd_kernel<false>
        <<<attn_grid(attention_fwd_kernel<false>, smem, B), 256, smem,
           stream>>>((const bf16*)ccv, a, starts, cv, (bf16*)cvb, attn, B, C, EP,
                     E, ts);
}

// dccv != nullptr: dense form (dccv written, ds_out unused);
// dccv == nullptr: compact form (ds_out[B*C] written, no dccv)
void launch_attention_bwd(const void* dcv, int dcv_bf16, const float* dattn,
                          const void* ccv, const float* a, const int* starts,
                          const float* attn, void* dccv, float* ds_out,
                          float* da, int B, int C, int EP, int E,
                          int has_dattn, hipStream_t stream) {
  const int ts = attn_ts(E, EP);
  bool stage = attn_smem(C, EP, ts, true, true) <= 160 * 1024 - 1024;
  size_t smem = attn_smem(C, EP, ts, stage, true);
#define ABWD(st, cp)                                                          \
  attention_bwd_kernel<st, cp>                                                \
      <<<attn_grid(attention_bwd_kernel<st, cp>, smem, B), 256, smem,         \
         stream>>>(dcv, dattn, (const bf16*)ccv, a, starts, attn,             \
                   (bf16*)dccv, ds_out, da, B, C, EP, E, has_dattn, dcv_bf16, \
                   ts)
  if (dccv) {
    if (stage) ABWD(true, false); else ABWD(false, false);
  } else {
    if (stage) ABWD(true, true); else ABWD(false, true);
  }
#undef ABWD
}

// the streaming kernels' shape gate (callers fall back to the kernels
// above when it does not hold)
int attention_stream_supported(int C, int EP) {
  return EP == 128 && C >= 1 && C <= ATTN_STREAM_MAX_C;
}

void launch_attention_fwd_scores(const void* ccv, const float* raw_scores,
                                 const int* starts, float* cv, void* cvb,
                                 float* attn, int B, int C, int EP, int E,
                                 hipStream_t stream) {
  if (!attention_stream_supported(C, EP) || B < 1) return;
  attention_fwd_scores_kernel<<<B, 256, 0, stream>>>(
      (const bf16*)ccv, raw_scores, starts, cv, (bf16*)cvb, attn, C,
      attn_ts(E, EP));
}

void launch_attention_bwd_compact_reg(const void* dcv, int dcv_bf16,
                                      const float* dattn, const void* ccv,
                                      const int* starts, const float* attn,
                                      float* ds_out, float* da, int B, int C,
                                      int EP, int E, int has_dattn,
                                      hipStream_t stream) {
  if (!attention_stream_supported(C, EP) || B < 1) return;
  attention_bwd_compact_reg_kernel<<<B, 256, 0, stream>>>(
      dcv, dattn, (const bf16*)ccv, starts, attn, ds_out, da, C, E,
      has_dattn, dcv_bf16, attn_ts(E, EP));
}

}  // extern "C"
