// K16: fused Adam step (semantics of torch.optim.Adam, reference main.py:138).
//   g = grad + wd * p;  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g
//   p -= lr * (m/bc1) / (sqrt(v/bc2) + eps)
// bf16 params keep an fp32 master (updated in fp32, rounded once); moments
// are fp32.  Vectorized 4-wide; one kernel per parameter tensor.

#include <cstdlib>

#include "common.h"

// bc_pow: DEVICE double[2] = (beta1^t, beta2^t), advanced once per
// optimizer step by adam_tick_kernel — device-resident so a hipGraph-
// captured training step keeps the bias correction advancing per replay
// (a host-computed inv_bc argument would freeze t at capture time).
__global__ void adam_tick_kernel(double* __restrict__ bc_pow, float b1,
                                 float b2) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    bc_pow[0] *= (double)b1;
    bc_pow[1] *= (double)b2;
  }
}

// One Adam update of 4 consecutive elements with every rounding written
// out (no compiler contraction inside).  The pattern — gradient FMA for all
// four, moment FMAs for elements 0-1, separate multiply and add for
// elements 2-3 — is what adam_bf16_kernel has always compiled to (the
// compiler contracted the packed pair but not the two scalar lanes).  It is
// fixed in source so that adam_bf16_kernel and adam_table_bf16_kernel
// produce the same bits whatever their register allocation or the compiler
// version, and so that a table updates identically through either kernel.
__device__ __forceinline__ bf16x4 adam_update4(f32x4& mm, f32x4& vv,
                                               f32x4& pp, const bf16x4 gg,
                                               float lr, float b1, float b2,
                                               float eps, float wd,
                                               float inv_bc1, float inv_bc2) {
#pragma clang fp contract(off)
  bf16x4 pout;
  const float omb1 = 1.f - b1, omb2 = 1.f - b2;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float grad = __builtin_fmaf(wd, pp[k], bf2f(gg[k]));
    const float gm = omb1 * grad;
    const float gv = (omb2 * grad) * grad;
    if (k < 2) {
      mm[k] = __builtin_fmaf(b1, mm[k], gm);
      vv[k] = __builtin_fmaf(b2, vv[k], gv);
    } else {
      mm[k] = b1 * mm[k] + gm;
      vv[k] = b2 * vv[k] + gv;
    }
    pp[k] = pp[k] - (lr * (mm[k] * inv_bc1)) / (sqrtf(vv[k] * inv_bc2) + eps);
    pout[k] = f2bf(pp[k]);
  }
  return pout;
}

template <int NT, int U, int MINW = 1>  // NT: nontemporal; U: independent
                          // 4-elem chunks per loop iteration; MINW: forced
                          // waves/SIMD (C2V_ADAM_OCC occupancy A/B)
__global__ __launch_bounds__(256, MINW) void adam_bf16_kernel(bf16* __restrict__ p,
                                 const bf16* __restrict__ g,
                                 float* __restrict__ master,
                                 float* __restrict__ m, float* __restrict__ v,
                                 long n, float lr, float b1, float b2,
                                 float eps, float wd,
                                 const double* __restrict__ bc_pow) {
  const float inv_bc1 = (float)(1.0 / (1.0 - bc_pow[0]));
  const float inv_bc2 = (float)(1.0 / (1.0 - bc_pow[1]));
  const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long cstride = (long)gridDim.x * blockDim.x * 4;  // chunk stride
  const long stride = cstride * U;
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  for (long i = i0; i < n; i += stride) {
    f32x4v mm[U], vv[U], pp[U];
    bf16x4 gg[U];
    bool ok[U];
    // all loads issue before any compute/store (outstanding-load depth)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long iu = i + (long)u * cstride;
      ok[u] = iu + 4 <= n;
      if (ok[u]) {
        if (NT) {
          mm[u] = __builtin_nontemporal_load((const f32x4v*)(m + iu));
          vv[u] = __builtin_nontemporal_load((const f32x4v*)(v + iu));
          pp[u] = __builtin_nontemporal_load((const f32x4v*)(master + iu));
          gg[u] = __builtin_nontemporal_load((const bf16x4*)(g + iu));
        } else {
          mm[u] = *(const f32x4v*)(m + iu);
          vv[u] = *(const f32x4v*)(v + iu);
          pp[u] = *(const f32x4v*)(master + iu);
          gg[u] = *(const bf16x4*)(g + iu);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long iu = i + (long)u * cstride;
      if (ok[u]) {
        const bf16x4 pout = adam_update4(mm[u], vv[u], pp[u], gg[u], lr, b1,
                                         b2, eps, wd, inv_bc1, inv_bc2);
        if (NT) {
          __builtin_nontemporal_store(mm[u], (f32x4v*)(m + iu));
          __builtin_nontemporal_store(vv[u], (f32x4v*)(v + iu));
          __builtin_nontemporal_store(pp[u], (f32x4v*)(master + iu));
          __builtin_nontemporal_store(pout, (bf16x4*)(p + iu));
        } else {
          *(f32x4v*)(m + iu) = mm[u];
          *(f32x4v*)(v + iu) = vv[u];
          *(f32x4v*)(master + iu) = pp[u];
          *(bf16x4*)(p + iu) = pout;
        }
      } else if (iu < n) {
        for (long j = iu; j < n && j < iu + 4; ++j) {
          float grad = bf2f(g[j]) + wd * master[j];
          m[j] = b1 * m[j] + (1.f - b1) * grad;
          v[j] = b2 * v[j] + (1.f - b2) * grad * grad;
          master[j] -= lr * (m[j] * inv_bc1) / (sqrtf(v[j] * inv_bc2) + eps);
          p[j] = f2bf(master[j]);
        }
      }
    }
  }
}

// K16b: row-gathering table Adam.  Same flat streaming structure as
// adam_bf16_kernel, but the bf16 gradient is never read from a dense
// table: each thread rebuilds its 4 gradient elements from the counting
// sort the embedding backward already ran.  Row `r` owns the sorted run
// [cursor[r] - counts[r], cursor[r]); entry k of the run is gout row
// perm[k] (addressing as in embed_scatter_sorted_kernel).  The fp32
// association reproduces the scatter path: one partial per aligned
// 16-entry chunk of the sorted order starting from +0, partials added in
// ascending chunk order, ONE rounding to bf16, then the unchanged update.
// Row 0 (<PAD/>) and untouched rows take gradient +0 without a gather.
// Rows with counts > thr were pre-reduced into the fp32 scratch by
// embed_scatter_heavy_kernel: read, round, re-zero.  counts is cleared by
// the trailing clear_i32_kernel (several threads share a row, so no reader
// may clear it).
constexpr int TA_CHUNK = 16;  // embed_scatter_sorted_kernel's RT

template <int U, int TA_B>  // U: 4-element groups per thread (ILP); TA_B:
                            // gathered entries in flight per group
__global__ __launch_bounds__(256) void adam_table_bf16_kernel(
    bf16* __restrict__ p, const bf16* __restrict__ gout,
    const long* __restrict__ perm, const int* __restrict__ counts,
    const int* __restrict__ cursor, float* __restrict__ scratch,
    float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
    long n, unsigned S4, long N, long M, int KP, int off0, int off1, int thr,
    float lr, float b1, float b2, float eps, float wd,
    const double* __restrict__ bc_pow) {
  const float inv_bc1 = (float)(1.0 / (1.0 - bc_pow[0]));
  const float inv_bc2 = (float)(1.0 / (1.0 - bc_pow[1]));
  const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long cstride = (long)gridDim.x * blockDim.x * 4;  // chunk stride
  const long stride = cstride * U;
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  const f32x4v zero4 = {0.f, 0.f, 0.f, 0.f};
  for (long i = i0; i < n; i += stride) {
    f32x4v mm[U], vv[U], pp[U], tot[U], part[U];
    bool ok[U];
    int k[U], end[U];
    unsigned col[U];
    bool heavy[U];
    // streaming loads first: they are in flight while the dependent
    // counts -> perm -> gout chain resolves
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long iu = i + (long)u * cstride;
      ok[u] = iu < n;  // n % 4 == 0 (S % 4 == 0): no partial group
      k[u] = end[u] = 0;
      col[u] = 0;
      heavy[u] = false;
      tot[u] = part[u] = zero4;
      if (ok[u]) {
        mm[u] = __builtin_nontemporal_load((const f32x4v*)(m + iu));
        vv[u] = __builtin_nontemporal_load((const f32x4v*)(v + iu));
        pp[u] = __builtin_nontemporal_load((const f32x4v*)(master + iu));
        const unsigned q = (unsigned)(iu >> 2);
        const unsigned row = q / S4;
        col[u] = (q - row * S4) * 4;
        int cnt = row != 0 ? counts[row] : 0;
        const int e = cursor[row];
        // a run outside [0, N) can only come from a broken counts
        // invariant: never follow it out of bounds
        if (cnt < 0 || e > N || cnt > e) cnt = 0;
        heavy[u] = cnt > thr;
        end[u] = heavy[u] ? 0 : e;
        k[u] = heavy[u] ? 0 : e - cnt;
      }
    }
    // gather: TA_B entries of every group in flight at once; the first
    // round covers almost every row (mean run length is a few entries)
    bool more = true;
    while (more) {
      long o[U][TA_B];
      bf16x4 g[U][TA_B];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < TA_B; ++j)
          if (k[u] + j < end[u]) o[u][j] = perm[k[u] + j];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < TA_B; ++j)
          if (k[u] + j < end[u]) {
            const long oo = o[u][j];
            const bf16* grow = oo < M ? gout + oo * KP + off0
                                      : gout + (oo - M) * KP + off1;
            g[u][j] = *(const bf16x4*)(grow + col[u]);
          }
      more = false;
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int j = 0; j < TA_B; ++j)
          if (k[u] + j < end[u]) {
            if (((k[u] + j) & (TA_CHUNK - 1)) == 0) {
              tot[u] += part[u];
              part[u] = zero4;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) part[u][c] += bf2f(g[u][j][c]);
          }
        k[u] += TA_B;
        more = more || k[u] < end[u];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long iu = i + (long)u * cstride;
      if (ok[u]) {
        tot[u] += part[u];
        if (heavy[u]) {
          tot[u] = *(const f32x4v*)(scratch + iu);
          *(f32x4v*)(scratch + iu) = zero4;
        }
        bf16x4 gg;  // the ONE rounding of the gradient to bf16
#pragma unroll
        for (int c = 0; c < 4; ++c) gg[c] = f2bf(tot[u][c]);
        const bf16x4 pout = adam_update4(mm[u], vv[u], pp[u], gg, lr, b1, b2,
                                         eps, wd, inv_bc1, inv_bc2);
        __builtin_nontemporal_store(mm[u], (f32x4v*)(m + iu));
        __builtin_nontemporal_store(vv[u], (f32x4v*)(v + iu));
        __builtin_nontemporal_store(pp[u], (f32x4v*)(master + iu));
        __builtin_nontemporal_store(pout, (bf16x4*)(p + iu));
      }
    }
  }
}

__global__ void clear_i32_kernel(int* __restrict__ x, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long j = i; j < n; j += stride) x[j] = 0;
}

__global__ void adam_f32_kernel(float* __restrict__ p,
                                const float* __restrict__ g,
                                float* __restrict__ m, float* __restrict__ v,
                                long n, float lr, float b1, float b2,
                                float eps, float wd,
                                const double* __restrict__ bc_pow) {
  const float inv_bc1 = (float)(1.0 / (1.0 - bc_pow[0]));
  const float inv_bc2 = (float)(1.0 / (1.0 - bc_pow[1]));
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long j = i; j < n; j += stride) {
    float grad = g[j] + wd * p[j];
    m[j] = b1 * m[j] + (1.f - b1) * grad;
    v[j] = b2 * v[j] + (1.f - b2) * grad * grad;
    p[j] -= lr * (m[j] * inv_bc1) / (sqrtf(v[j] * inv_bc2) + eps);
  }
}

// Multi-tensor f32 Adam: the model's small fp32 params (LN gamma/beta,
// attention vector, head bias) update in ONE launch instead of four —
// grid-strides the concatenated element space, resolving the owning
// tensor with an unrolled prefix-offset scan (<= 8 tensors).
#define ADAM_MT_MAX 8
struct AdamF32Args {
  float* p[ADAM_MT_MAX];
  const float* g[ADAM_MT_MAX];
  float* m[ADAM_MT_MAX];
  float* v[ADAM_MT_MAX];
  long off[ADAM_MT_MAX + 1];
};

__global__ void adam_f32_multi_kernel(AdamF32Args args, int ntens,
                                      long total, float lr, float b1,
                                      float b2, float eps, float wd,
                                      const double* __restrict__ bc_pow) {
  const float inv_bc1 = (float)(1.0 / (1.0 - bc_pow[0]));
  const float inv_bc2 = (float)(1.0 / (1.0 - bc_pow[1]));
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long j = i; j < total; j += stride) {
    int t = 0;
#pragma unroll
    for (int k = 1; k < ADAM_MT_MAX; ++k)
      if (k < ntens && j >= args.off[k]) t = k;
    const long e = j - args.off[t];
    float* p = args.p[t];
    const float* g = args.g[t];
    float* m = args.m[t];
    float* v = args.v[t];
    float grad = g[e] + wd * p[e];
    m[e] = b1 * m[e] + (1.f - b1) * grad;
    v[e] = b2 * v[e] + (1.f - b2) * grad * grad;
    p[e] -= lr * (m[e] * inv_bc1) / (sqrtf(v[e] * inv_bc2) + eps);
  }
}

extern "C" {

void launch_adam_f32_multi(float** ps, const float** gs, float** ms,
                           float** vs, const long* ns, int ntens,
                           const double* bc_pow, float lr, float b1,
                           float b2, float eps, float wd,
                           hipStream_t stream) {
  AdamF32Args a;
  long total = 0;
  for (int t = 0; t < ntens; ++t) {
    a.p[t] = ps[t]; a.g[t] = gs[t]; a.m[t] = ms[t]; a.v[t] = vs[t];
    a.off[t] = total;
    total += ns[t];
  }
  a.off[ntens] = total;
  for (int t = ntens; t < ADAM_MT_MAX; ++t) {
    a.p[t] = nullptr; a.g[t] = nullptr; a.m[t] = nullptr; a.v[t] = nullptr;
    if (t > ntens) a.off[t] = total;
  }
  const int block = 256;
  const int grid = (int)min((total + block - 1) / block, (long)4096);
  adam_f32_multi_kernel<<<grid, block, 0, stream>>>(
      a, ntens, total, lr, b1, b2, eps, wd, bc_pow);
}

void launch_adam_tick(double* bc_pow, float b1, float b2,
                      hipStream_t stream) {
  adam_tick_kernel<<<1, 1, 0, stream>>>(bc_pow, b1, b2);
}

void launch_adam_bf16(void* p, const void* g, float* master, float* m,
                      float* v, long n, const double* bc_pow, float lr,
                      float b1, float b2, float eps, float wd,
                      hipStream_t stream) {
  const int block = 256;
  // defaults swept on hardware against the same-box D2D copy ceiling
  // (5.5 TB/s): ILP 2 / grid 64k runs the 3.2-GB table update at 5.2 TB/s
  // = 94% of achievable (kbench adam membw)
  const char* ge = getenv("C2V_ADAM_GRID");
  const long cap = ge ? atol(ge) : 65536;
  const char* ue = getenv("C2V_ADAM_ILP");
  const int U = ue ? atoi(ue) : 2;
  const long want = (n / (4 * U) + block - 1) / block;
  const int grid = (int)min(want > 0 ? want : 1, cap);
  const char* nt_env = getenv("C2V_ADAM_NT");
  const int nt = (nt_env == nullptr || nt_env[0] != '0') ? 1 : 0;
  // C2V_ADAM_OCC=5 forces a 5-waves/SIMD register cap (occupancy A/B)
  static const char* occ_env = getenv("C2V_ADAM_OCC");
  const bool occ5 = occ_env && occ_env[0] == '5';
#define ADAM_CASE(NTV, UV)                                                  \
  if (nt == NTV && U == UV) {                                               \
    if (occ5)                                                               \
      adam_bf16_kernel<NTV, UV, 5><<<grid, block, 0, stream>>>(             \
          (bf16*)p, (const bf16*)g, master, m, v, n, lr, b1, b2, eps, wd,   \
          bc_pow);                                                          \
    else                                                                    \
      adam_bf16_kernel<NTV, UV><<<grid, block, 0, stream>>>(                \
          (bf16*)p, (const bf16*)g, master, m, v, n, lr, b1, b2, eps, wd,   \
          bc_pow);                                                          \
    return;                                                                 \
  }
  ADAM_CASE(1, 1) ADAM_CASE(1, 2) ADAM_CASE(1, 4)
  ADAM_CASE(0, 1) ADAM_CASE(0, 2) ADAM_CASE(0, 4)
  adam_bf16_kernel<1, 2><<<grid, block, 0, stream>>>(
      (bf16*)p, (const bf16*)g, master, m, v, n, lr, b1, b2, eps, wd,
      bc_pow);
}

// Table Adam from a deferred gradient record (see adam_table_bf16_kernel);
// T rows of S columns, S % 4 == 0 and T * S / 4 < 2^32 (checked by the
// binding).  With clear_counts it also restores the all-zero invariant of
// counts[0..ncounts); without, the caller clears after every reader of the
// histogram is done (both tables in one launch, index_group.hip).
void launch_adam_table_bf16(void* p, const void* gout, const long* perm,
                            int* counts, const int* cursor, float* scratch,
                            float* master, float* m, float* v, long T, int S,
                            long ncounts, long N, long M, int KP, int off0,
                            int off1, int thr, const double* bc_pow, float lr,
                            float b1, float b2, float eps, float wd,
                            int clear_counts, hipStream_t stream) {
  const int block = 256;
  const long n = T * S;
  // same grid rule as launch_adam_bf16
  static const char* ge = getenv("C2V_ADAM_GRID");
  const long cap = ge ? atol(ge) : 65536;
  // defaults swept on hardware (kbench table_adam, PERF.md): ILP 1 with 2
  // gathered entries in flight fits 64 VGPRs = 8 waves/SIMD and keeps the
  // streaming rate of adam_bf16_kernel; ILP 2 / depth 4 (144 VGPRs, 3
  // waves) lost 20%.  C2V_TABLE_ADAM_ILP=2 / C2V_TABLE_ADAM_DEPTH=4 select
  // the other variants for A/B.
  static const char* ue = getenv("C2V_TABLE_ADAM_ILP");
  static const char* de = getenv("C2V_TABLE_ADAM_DEPTH");
  const int U = ue && atoi(ue) == 2 ? 2 : 1;
  const int D = de && atoi(de) == 4 ? 4 : 2;
  const long want = (n / (4 * U) + block - 1) / block;
  const int grid = (int)min(want > 0 ? want : 1, cap);
#define TADAM_LAUNCH(UV, DV)                                                 \
  adam_table_bf16_kernel<UV, DV><<<grid, block, 0, stream>>>(                \
      (bf16*)p, (const bf16*)gout, perm, counts, cursor, scratch, master, m, \
      v, n, (unsigned)(S / 4), N, M, KP, off0, off1, thr, lr, b1, b2, eps,   \
      wd, bc_pow)
  if (U == 1 && D == 4) TADAM_LAUNCH(1, 4);
  else if (U == 1) TADAM_LAUNCH(1, 2);
  else if (D == 4) TADAM_LAUNCH(2, 4);
  else TADAM_LAUNCH(2, 2);
#undef TADAM_LAUNCH
  if (!clear_counts) return;
  const int cgrid = (int)min((ncounts + block - 1) / block, (long)4096);
  clear_i32_kernel<<<cgrid > 0 ? cgrid : 1, block, 0, stream>>>(counts,
                                                                ncounts);
}

void launch_adam_f32(float* p, const float* g, float* m, float* v, long n,
                     const double* bc_pow, float lr, float b1, float b2,
                     float eps, float wd, hipStream_t stream) {
  const int block = 256;
  const long want = (n + block - 1) / block;
  const int grid = (int)min(want > 0 ? want : 1, (long)4096);
  adam_f32_kernel<<<grid, block, 0, stream>>>(p, g, m, v, n, lr, b1, b2, eps,
                                              wd, bc_pow);
}

}  // extern "C"
