// K21 / K22 segmented attention pool over a packed (ragged) batch: forward
// (K21) and backward (K22, second half of this file).
// Math of attention_fwd_kernel (attention.hip), per method b whose rows are
// [offsets[b], offsets[b+1]) of ccv [M, EP]:
//   scores[c] = sum_e ccv[c,e] * a[e]            (ts = round8(E) columns)
//   scores = scores*mask + (1-mask)*NINF          (mask = starts>0)
//   attn = softmax(scores over the method's rows)
//   cv[b,e] = sum_c attn[c] * ccv[c,e]            (columns [ts, EP) zero)
//
// One workgroup (256 threads = 4 waves) per method, the three phases of
// attention_fwd_kernel with its mappings and summation orders: 16-lane
// groups own one row at a time in phase 1, each wave pools a contiguous
// quarter of the rows in phase 3, a fixed 4-way sum combines the waves.
// Nothing is sized by the method's length n: methods of up to APK_CHUNK
// rows keep their scores in LDS; a longer one parks its masked raw scores
// in its own slice of the attn output, which the softmax then overwrites
// in place (written and re-read by this block only, across
// __syncthreads()).  Both forms run the same arithmetic in the same order,
// so a method's bits depend on its own rows alone: not on B, its position,
// its neighbours' lengths or the grid.  No atomics.  Rows are re-read from
// global memory (L2) in phase 3.  Phases 1 and 3 keep several rows' loads
// in flight (APK_ROWS, APK_PF): a long method is one block, so its time is
// what a heavy-tailed batch waits for.

#include "common.h"

#define APK_CHUNK 256  // scores kept in LDS up to this many rows
#define APK_ROWS 4     // phase 1: rows per group in flight
#define APK_PF 8       // phase 3: rows per lane in flight

// scores: LDS [APK_CHUNK] or attn + lo.  src/st/attn_seg point at the
// method's first row.
__device__ __forceinline__ void pool_segment(
    const bf16* src, const int* st, const float* lds_a, float* scores,
    float* red, float* partials, float* attn_seg, float* cv_row, bf16* cvb_row,
    int n, int EP, int ts) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int lane16 = lane & 15;
  const int group = (threadIdx.x >> 4);  // 16 groups of 16 lanes

  // phase 1: masked scores, one row per 16-lane group; APK_ROWS rows of a
  // group are loaded before the first is reduced (branch-free: a row past
  // the end re-reads row n-1, in bounds, and is dropped), so a long
  // method is not one load latency per row
  for (int c = group; c < n; c += 16 * APK_ROWS) {
    float s[APK_ROWS];
#pragma unroll
    for (int k = 0; k < APK_ROWS; ++k)
      s[k] = group_row_dot(src + (long)min(c + 16 * k, n - 1) * EP, lds_a, ts,
                           lane16);
#pragma unroll
    for (int k = 0; k < APK_ROWS; ++k) s[k] = group16_reduce_sum(s[k]);
    if (lane16 == 0) {
#pragma unroll
      for (int k = 0; k < APK_ROWS; ++k) {
        const int ck = c + 16 * k;
        if (ck < n) {
          const float mask = st[ck] > 0 ? 1.0f : 0.0f;
          scores[ck] = s[k] * mask + (1.0f - mask) * NINF_F;
        }
      }
    }
  }
  __syncthreads();

  // phase 2: softmax in place, probabilities written to attn
  block_softmax(scores, red, attn_seg, n, 0);

  // phase 3: each wave pools a contiguous span of rows into per-lane
  // column pairs, then a fixed-order sum over the four waves
  const int span = (n + 3) / 4;
  const int c_lo = min(n, wave * span);
  const int c_hi = min(n, c_lo + span);
  for (int e0 = lane * 2; e0 < EP; e0 += WAVE * 2) {
    float acc0 = 0.f, acc1 = 0.f;
    if (e0 < ts) {
      // sequential in c, one FMA per element; APK_PF rows are in flight at
      // a time (raw bf16 pairs: bf16 -> f32 is the bit pattern moved to the
      // high half), the order of the sum does not change
      const bf16* col = src + e0;
      int c = c_lo;
      for (; c + APK_PF <= c_hi; c += APK_PF) {
        unsigned r[APK_PF];
        float at[APK_PF];
#pragma unroll
        for (int k = 0; k < APK_PF; ++k)
          r[k] = *(const unsigned*)(col + (long)(c + k) * EP);
#pragma unroll
        for (int k = 0; k < APK_PF; ++k) at[k] = scores[c + k];
#pragma unroll
        for (int k = 0; k < APK_PF; ++k) {
          acc0 = __builtin_fmaf(at[k], __uint_as_float(r[k] << 16), acc0);
          acc1 = __builtin_fmaf(at[k], __uint_as_float(r[k] & 0xffff0000u),
                                acc1);
        }
      }
      for (; c < c_hi; ++c) {
        const unsigned r = *(const unsigned*)(col + (long)c * EP);
        const float at = scores[c];
        acc0 = __builtin_fmaf(at, __uint_as_float(r << 16), acc0);
        acc1 = __builtin_fmaf(at, __uint_as_float(r & 0xffff0000u), acc1);
      }
    }
    partials[wave * EP + e0] = acc0;
    partials[wave * EP + e0 + 1] = acc1;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < EP; e += blockDim.x) {
    const float s = partials[e] + partials[EP + e] + partials[2 * EP + e] +
                    partials[3 * EP + e];
    cv_row[e] = s;
    cvb_row[e] = f2bf(s);
  }
}

// attn is read back by the block that wrote it: no __restrict__ on it
__global__ __launch_bounds__(256) void attention_packed_fwd_kernel(
    const bf16* __restrict__ ccv, const float* __restrict__ a,
    const int* __restrict__ starts, const int* __restrict__ offsets,
    float* __restrict__ cv, bf16* __restrict__ cvb, float* attn, long M,
    int EP, int ts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // layout: [a f32 EP] [scores APK_CHUNK] [red 64] [partials 4*EP]
  float* lds_a = (float*)smem;
  float* lds_scores = lds_a + EP;
  float* red = lds_scores + APK_CHUNK;
  float* partials = red + 64;

  const long b = blockIdx.x;
  // offsets are built by the host wrapper (0 = o[0] < o[1] < ... = M); the
  // clamp only keeps a caller's mistake inside the buffers
  const long lo = max(0L, min((long)offsets[b], M));
  const long hi = max(lo, min((long)offsets[b + 1], M));
  const int n = (int)(hi - lo);

  for (int e = threadIdx.x; e < EP; e += blockDim.x) lds_a[e] = a[e];
  __syncthreads();

  const bf16* src = ccv + lo * EP;  // 64-bit row addressing
  if (n <= APK_CHUNK)
    pool_segment(src, starts + lo, lds_a, lds_scores, red, partials,
                 attn + lo, cv + b * EP, cvb + b * EP, n, EP, ts);
  else
    pool_segment(src, starts + lo, lds_a, attn + lo, red, partials,
                 attn + lo, cv + b * EP, cvb + b * EP, n, EP, ts);
}

// ---------------------------------------------------------------------------
// K22: backward of the pool above, the packed counterpart of
// attention_bwd_kernel<STAGE = 0, COMPACT> (attention.hip).  Per method b:
//   g[c] = dcv[b] . ccv[c] (+ dattn[c]);   sum_g = sum_c attn[c] * g[c]
//   ds[c] = attn[c] * (g[c] - sum_g) * mask[c]
//   da_p[b, e] = sum_c ds[c] * ccv[c, e]
//   COMPACT = 0: dccv[c, e] = dccv_elem(attn[c], dcv[b, e], ds[c], a[e])
// One 256-thread block per method with attention_bwd_kernel's mappings and
// reduction trees (a 16-lane group owns row c = group + 16k, the sum_g
// chain of a group runs in ascending c, wave_reduce_sum then the 4-wave
// sum, per-lane da_acc, the fixed shfl_xor 16/32 tree and the fixed 4-way
// wave sum), so at equal lengths the bits are those of the padded kernels,
// and a method's ds slice and da_p row depend on its own rows only.
// g/ds of up to APK_CHUNK rows live in LDS; a longer method parks them in
// its own slice of ds_out, rewritten in place by this block across
// __syncthreads() (the forward's trick with attn).  The dense form takes
// ds_out as a workspace for that.  COMPACT also writes the row -> method
// map seg[M] the packed combiner backward reads.  No atomics.
#define APK_BROWS 4  // phases A and B: rows per group in flight

// gbuf: LDS [APK_CHUNK] or ds_seg.  Every pointer with a _seg/_row suffix
// and src/st point at the method's first row / the method's row.
template <bool COMPACT>
__device__ __forceinline__ void pool_segment_bwd(
    const bf16* src, const int* st, const float* attn_seg,
    const float* dattn_seg, const float* lds_dcv, const float* lds_a,
    float* gbuf, float* red, float* partials, float* ds_seg, int* seg_seg,
    bf16* dccv_seg, float* da_row, int b, int n, int EP, int E, int ts) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int lane16 = lane & 15;
  const int group = (threadIdx.x >> 4);

  // phase A: g[c] (group-per-row, APK_BROWS rows loaded before the first
  // is reduced; a row past the end re-reads row n-1 and is dropped) and
  // the block-reduced sum_g
  float part = 0.f;
  for (int c = group; c < n; c += 16 * APK_BROWS) {
    float g[APK_BROWS];
#pragma unroll
    for (int k = 0; k < APK_BROWS; ++k)
      g[k] = group_row_dot(src + (long)min(c + 16 * k, n - 1) * EP, lds_dcv,
                           ts, lane16);
#pragma unroll
    for (int k = 0; k < APK_BROWS; ++k) g[k] = group16_reduce_sum(g[k]);
    if (lane16 == 0) {
#pragma unroll
      for (int k = 0; k < APK_BROWS; ++k) {
        const int ck = c + 16 * k;
        if (ck < n) {
          float gk = g[k];
          if (dattn_seg) gk += dattn_seg[ck];
          gbuf[ck] = gk;  // temporarily g
          part = __builtin_fmaf(attn_seg[ck], gk, part);
        }
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
  for (int c = threadIdx.x; c < n; c += blockDim.x) {
    const float at = attn_seg[c];
    const float mask = st[c] > 0 ? 1.0f : 0.0f;
    const float dsc = at * (gbuf[c] - sum_g) * mask;
    gbuf[c] = dsc;
    if (COMPACT) {
      if (gbuf != ds_seg) ds_seg[c] = dsc;
      seg_seg[c] = b;
    }
  }
  __syncthreads();

  // phase B: per-lane da accumulators (and the dccv rows of the dense
  // form).  This lane's columns are (lane16*8 + j) + 128*i, i statically
  // unrolled.  APK_BROWS rows are loaded before the first FMA; each
  // accumulator still takes its rows in ascending c.  A lane whose columns
  // lie past ts inside a live 128-column pass loads the last valid granule
  // instead (in bounds) and drops it.
  float da_acc[3][8] = {};  // EP <= 384
  for (int c = group; c < n; c += 16 * APK_BROWS) {
    uint4 raw[APK_BROWS][3];
#pragma unroll
    for (int k = 0; k < APK_BROWS; ++k) {
      const bf16* row = src + (long)min(c + 16 * k, n - 1) * EP;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (128 * i < ts)
          raw[k][i] = *(const uint4*)(row + min(lane16 * 8 + 128 * i, ts - 8));
    }
#pragma unroll
    for (int k = 0; k < APK_BROWS; ++k) {
      const int ck = c + 16 * k;
      if (ck < n) {
        const float at = COMPACT ? 0.f : attn_seg[ck];
        const float dsc = gbuf[ck];
        bf16* drow = COMPACT ? nullptr : dccv_seg + (long)ck * EP;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int e0 = lane16 * 8 + 128 * i;
          if (e0 < ts) {
            bf16 v[8], o[8];
            *(uint4*)v = raw[k][i];
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
    }
  }
  // deterministic combine, as in attention_bwd_kernel
  __syncthreads();
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
    da_row[e] = e < E ? s4v : 0.f;
  }
}

// ds_out is read back by the block that wrote it: no __restrict__ on it
template <bool COMPACT>
__global__ __launch_bounds__(256) void attention_packed_bwd_kernel(
    const void* __restrict__ dcv, const float* __restrict__ dattn,
    const bf16* __restrict__ ccv, const float* __restrict__ a,
    const int* __restrict__ starts, const int* __restrict__ offsets,
    const float* __restrict__ attn, bf16* __restrict__ dccv, float* ds_out,
    int* __restrict__ seg, float* __restrict__ da, long M, int EP, int E,
    int dcv_bf16, int ts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // layout: [dcv f32 EP] [a f32 EP] [g/ds APK_CHUNK] [red 64] [partials 4*EP]
  float* lds_dcv = (float*)smem;
  float* lds_a = lds_dcv + EP;
  float* lds_ds = lds_a + EP;
  float* red = lds_ds + APK_CHUNK;
  float* partials = red + 64;

  const long b = blockIdx.x;
  // as in the forward: the clamp only keeps a caller's mistake in bounds
  const long lo = max(0L, min((long)offsets[b], M));
  const long hi = max(lo, min((long)offsets[b + 1], M));
  const int n = (int)(hi - lo);

  for (int e = threadIdx.x; e < EP; e += blockDim.x) {
    lds_dcv[e] = dcv_bf16 ? bf2f(((const bf16*)dcv)[b * EP + e])
                          : ((const float*)dcv)[b * EP + e];
    lds_a[e] = a[e];
  }
  __syncthreads();

  pool_segment_bwd<COMPACT>(
      ccv + lo * EP, starts + lo, attn + lo, dattn ? dattn + lo : nullptr,
      lds_dcv, lds_a, n <= APK_CHUNK ? lds_ds : ds_out + lo, red, partials,
      ds_out + lo, COMPACT ? seg + lo : nullptr,
      COMPACT ? nullptr : dccv + lo * EP, da + b * EP, (int)b, n, EP, E, ts);
}

extern "C" {

int attention_packed_chunk() { return APK_CHUNK; }

void launch_attention_packed_fwd(const void* ccv, const float* a,
                                 const int* starts, const int* offsets,
                                 float* cv, void* cvb, float* attn, long M,
                                 long B, int EP, int E, hipStream_t stream) {
  if (B < 1) return;
  int ts = (E + 7) & ~7;
  if (ts > EP) ts = EP;
  const size_t smem = ((size_t)EP + APK_CHUNK + 64 + 4 * (size_t)EP) * 4;
  attention_packed_fwd_kernel<<<(unsigned)B, 256, smem, stream>>>(
      (const bf16*)ccv, a, starts, offsets, cv, (bf16*)cvb, attn, M, EP, ts);
}

// dccv != nullptr: dense form (dccv written, ds_out a workspace, seg unused);
// dccv == nullptr: compact form (ds_out [M] and seg [M] written, no dccv)
void launch_attention_packed_bwd(const void* dcv, int dcv_bf16,
                                 const float* dattn, const void* ccv,
                                 const float* a, const int* starts,
                                 const int* offsets, const float* attn,
                                 void* dccv, float* ds_out, int* seg,
                                 float* da, long M, long B, int EP, int E,
                                 hipStream_t stream) {
  if (B < 1) return;
  int ts = (E + 7) & ~7;
  if (ts > EP) ts = EP;
  const size_t smem = (2 * (size_t)EP + APK_CHUNK + 64 + 4 * (size_t)EP) * 4;
  if (dccv)
    attention_packed_bwd_kernel<false><<<(unsigned)B, 256, smem, stream>>>(
        dcv, dattn, (const bf16*)ccv, a, starts, offsets, attn, (bf16*)dccv,
        ds_out, seg, da, M, EP, E, dcv_bf16, ts);
  else
    attention_packed_bwd_kernel<true><<<(unsigned)B, 256, smem, stream>>>(
        dcv, dattn, (const bf16*)ccv, a, starts, offsets, attn, nullptr,
        ds_out, seg, da, M, EP, E, dcv_bf16, ts);
}

}  // extern "C"
