// Python bindings for the code2vec_amd HIP kernel library (_c2v_hip).
// Pure C++ TU: declares the extern "C" launchers implemented in the .hip
// files and validates tensor dtype/contiguity/shape before launching on the
// current torch HIP stream.

#include <torch/extension.h>

#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <map>

#define CHK(x) TORCH_CHECK(x, #x)
#define CHK_CONTIG(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")
#define CHK_CUDA(t) TORCH_CHECK((t).is_cuda(), #t " must be on GPU")
#define CHK_DT(t, dt) TORCH_CHECK((t).scalar_type() == dt, #t " dtype mismatch")

extern "C" {
void launch_gather_concat_fwd(const int*, const int*, const int*, const void*,
                              const void*, void*, long, int, int, int,
                              hipStream_t);
void launch_gather_concat_bwd(const int*, const int*, const int*, const void*,
                              float*, float*, long, int, int, hipStream_t);
void launch_embed_scatter_sorted(const int*, const long*, const void*, float*,
                                 void*, unsigned char*, long, long, int, int,
                                 int, int, int, hipStream_t);
void launch_embed_scatter_heavy(const int*, const long*, const int*,
                                const void*, float*, long, long, int, int,
                                int, int, int, hipStream_t);
void launch_adam_table_bf16(void*, const void*, const long*, int*, const int*,
                            float*, float*, float*, float*, long, int, long,
                            long, long, int, int, int, int, const double*,
                            float, float, float, float, float, int,
                            hipStream_t);
long group_tables_partials(long, long);
long group_tables_tmp(long, long, long);
void launch_group_tables(const int*, const int*, const int*, long, int, int,
                         int*, int*, int*, int*, int*, int*, long*, int*,
                         long*, int*, hipStream_t);
void launch_embed_scatter_heavy_pair(const int*, const long*, const int*,
                                     float*, int, const int*, const long*,
                                     const int*, float*, int, const void*,
                                     long, int, int, hipStream_t);
void launch_clear_i32_pair(int*, long, int*, long, hipStream_t);
void launch_count_indices(const int*, int*, long, hipStream_t);
void launch_cast_clear_rows(float*, const int*, unsigned char*, void*, long,
                            int, hipStream_t);
void launch_scatter_group(const int*, int*, int*, long*, long, hipStream_t);
void launch_exclusive_scan(const int*, int*, int*, long, hipStream_t);
size_t cub_exclusive_scan_temp_bytes(long);
void launch_cub_exclusive_scan(const int*, int*, void*, size_t, long,
                               hipStream_t);
void launch_combiner_fwd(const void*, const void*, const float*, const float*,
                         void*, void*, float*, float*, long, int, int, int,
                         float, unsigned long long,
                         const unsigned long long*, int, hipStream_t);
int launch_combiner_fwd_scores(const void*, const void*, const float*,
                               const float*, void*, void*, float*, float*,
                               long, int, int, int, float, unsigned long long,
                               const unsigned long long*, int, const float*,
                               float*, hipStream_t);
void launch_bump_u64(void*, unsigned long long, hipStream_t);
void launch_gather_combiner_fwd(const int*, const int*, const int*,
                                const void*, const void*, int, int,
                                const void*, const float*, const float*,
                                void*, void*, float*, float*, long, int, int,
                                int, float, unsigned long long,
                                const unsigned long long*, hipStream_t);
void launch_wgrad_gather(const int*, const int*, const int*, const void*,
                         const void*, int, int, const void*, float*, long,
                         int, int, int, hipStream_t);
void launch_combiner_bwd(const void*, const void*, const void*, const float*,
                         const float*, const float*, const float*, void*,
                         float*, float*, long, int, int, float, hipStream_t);
void launch_combiner_bwd_recompute(const float*, const float*, const void*,
                                   int, const float*, int, const void*,
                                   const void*, const float*, const float*,
                                   const float*, const float*, void*, float*,
                                   float*, long, int, float, hipStream_t);
void launch_attention_fwd(const void*, const float*, const int*, float*,
                          void*, float*, int, int, int, int, hipStream_t);
void launch_attention_bwd(const void*, int, const float*, const void*,
                          const float*, const int*, const float*, void*,
                          float*, float*, int, int, int, int, int,
                          hipStream_t);
int attention_stream_supported(int, int);
void launch_attention_fwd_scores(const void*, const float*, const int*,
                                 float*, void*, float*, int, int, int, int,
                                 hipStream_t);
void launch_attention_bwd_compact_reg(const void*, int, const float*,
                                      const void*, const int*, const float*,
                                      float*, float*, int, int, int, int, int,
                                      hipStream_t);
int attention_packed_chunk();
void launch_attention_packed_fwd(const void*, const float*, const int*,
                                 const int*, float*, void*, float*, long, long,
                                 int, int, hipStream_t);
void launch_attention_packed_bwd(const void*, int, const float*, const void*,
                                 const float*, const int*, const int*,
                                 const float*, void*, float*, int*, float*,
                                 long, long, int, int, hipStream_t);
void launch_combiner_bwd_recompute_packed(
    const float*, const float*, const void*, int, const float*, const int*,
    long, const void*, const void*, const float*, const float*, const float*,
    const float*, void*, float*, float*, long, int, float, hipStream_t);
void launch_slab_sum2_f32(const float*, const float*, float*, float*, int,
                          int, hipStream_t);
void launch_loss_reduce(const float*, float*, float*, int, hipStream_t);
void launch_wgrad_reduce(const float*, void*, int, int, int, hipStream_t);
void launch_lsm_nll_fwd(const void*, const long*, const float*, float*,
                        float*, int, long, hipStream_t);
void launch_lsm_nll_bwd(const void*, const long*, const float*, const float*,
                        const float*, const float*, void*, int, long,
                        hipStream_t);
bool launch_wgrad_pipe(const void*, const void*, float*, long, int, int, int,
                       int, hipStream_t);
void launch_wgrad(const void*, const void*, float*, long, int, int, int,
                  hipStream_t);
void launch_dgrad(const void*, const void*, void*, long, int, int,
                  hipStream_t);
void launch_head_wgrad(const void*, const void*, void*, long, long, int,
                       hipStream_t);
void launch_head_dgrad(const void*, const void*, float*, long, long,
                       hipStream_t);
void launch_transpose_w(const void*, void*, long, hipStream_t);
void launch_dgrad2(const void*, const void*, void*, long, long, hipStream_t);
void launch_slab_sum_bf16(const float*, void*, int, long, hipStream_t);
void launch_slab_sum_f32(const float*, float*, int, int, hipStream_t);
void launch_colsum_bf16(const void*, float*, long, long, hipStream_t);
void launch_row_max_argmax(const void*, float*, long*, long, long,
                           hipStream_t);
int row_topk_chunk();
void launch_row_topk(const void*, int, long, long, int, void*, float*, float*,
                     float*, long*, float*, hipStream_t);
int sim_topk_query_tile();
int sim_topk_row_tile();
void launch_sim_topk(const void*, const void*, const long*, long, long, int,
                     int, int, void*, float*, long*, hipStream_t);
int sim_range_waves();
void launch_sim_range_count(const void*, const void*, const long*,
                            const long*, float, long, long, int, int, int*,
                            hipStream_t);
void launch_sim_range_fill(const void*, const void*, const long*, const long*,
                           float, long, long, int, int, const long*, long,
                           long*, float*, hipStream_t);
void launch_head_topk(const void*, const void*, const float*, float, long,
                      long, int, int, int, void*, float*, float*, float*,
                      long*, float*, hipStream_t);
void launch_head_bwd_prep(const long*, const float*, const float*,
                          const float*, const float*, float*, long,
                          hipStream_t);
void launch_swizzle_cv(const void*, void*, long, long, hipStream_t);
void launch_inv_rownorm(const void*, float*, long, hipStream_t);
void launch_rowscale(const void*, const float*, void*, long, hipStream_t);
void launch_angular_fwd(const void*, const void*, const long*, void*, void*,
                        long, long, float, float, float, hipStream_t);
void launch_angular_dcos(const void*, const void*, const long*, void*, long,
                         long, float, float, float, hipStream_t);
void launch_norm_project(const void*, const void*, const float*, void*,
                         long, hipStream_t);
void launch_head_bwd_dw(const void*, const void*, const float*, void*,
                        float*, long, long, hipStream_t);
bool launch_head_bwd_dw_pipe(const void*, const void*, const float*, void*,
                             float*, long, long, int, hipStream_t);
void launch_head_bwd_dcv_pipe(const void*, const void*, const float*, float*,
                              long, long, int, int, hipStream_t);
void launch_head_bwd_dcv_rc(const void*, const void*, const void*,
                            const float*, const float*, float*, long, long,
                            int, hipStream_t);
void launch_head_bwd_dcv(const void*, const void*, const float*, float*,
                         long, long, int, hipStream_t);
void launch_head_fwd(const void*, const void*, const float*, void*, float*,
                     float*, long, long, int, int, hipStream_t);
void launch_swizzle_a(const void*, void*, long, long, hipStream_t);
void launch_lsm_finalize(const void*, const float*, const float*, const long*,
                         const float*, float*, float*, int, long, int,
                         hipStream_t);
void launch_lsm_partial(const void*, float*, float*, int, long, hipStream_t);
void launch_adam_tick(double*, float, float, hipStream_t);
void launch_adam_f32_multi(float**, const float**, float**, float**,
                           const long*, int, const double*, float, float,
                           float, float, float, hipStream_t);
void launch_adam_bf16(void*, const void*, float*, float*, float*, long,
                      const double*, float, float, float, float, float,
                      hipStream_t);
void launch_adam_f32(float*, const float*, float*, float*, long,
                     const double*, float, float, float, float, float,
                     hipStream_t);
}

static hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

void gather_concat_fwd(torch::Tensor starts, torch::Tensor paths,
                       torch::Tensor ends, torch::Tensor term,
                       torch::Tensor path, torch::Tensor out) {
  CHK_CUDA(starts); CHK_CONTIG(starts); CHK_DT(starts, torch::kInt32);
  CHK_CONTIG(paths); CHK_CONTIG(ends);
  CHK_DT(term, torch::kBFloat16); CHK_CONTIG(term);
  CHK_DT(path, torch::kBFloat16); CHK_CONTIG(path);
  CHK_DT(out, torch::kBFloat16); CHK_CONTIG(out);
  const long M = starts.numel();
  const int TS = term.size(1), PS = path.size(1);
  TORCH_CHECK(out.size(0) == M && out.size(1) >= 2 * TS + PS, "out shape");
  TORCH_CHECK(TS % 8 == 0 && PS % 8 == 0, "segment strides must be 8-mult");
  TORCH_CHECK(out.size(1) % 8 == 0, "out width must be 8-mult");
  launch_gather_concat_fwd(starts.data_ptr<int>(), paths.data_ptr<int>(),
                           ends.data_ptr<int>(), term.data_ptr(),
                           path.data_ptr(), out.data_ptr(), M, TS, PS,
                           (int)out.size(1), cur_stream());
}

void gather_concat_bwd(torch::Tensor starts, torch::Tensor paths,
                       torch::Tensor ends, torch::Tensor gout,
                       torch::Tensor dterm, torch::Tensor dpath) {
  CHK_CUDA(gout); CHK_CONTIG(gout); CHK_DT(gout, torch::kBFloat16);
  CHK_DT(dterm, torch::kFloat32); CHK_CONTIG(dterm);
  CHK_DT(dpath, torch::kFloat32); CHK_CONTIG(dpath);
  const long M = starts.numel();
  const int TS = dterm.size(1), PS = dpath.size(1);
  launch_gather_concat_bwd(starts.data_ptr<int>(), paths.data_ptr<int>(),
                           ends.data_ptr<int>(), gout.data_ptr(),
                           dterm.data_ptr<float>(), dpath.data_ptr<float>(),
                           M, TS, PS, cur_stream());
}

void embed_scatter_sorted(torch::Tensor sorted_idx, torch::Tensor perm,
                          torch::Tensor gout, torch::Tensor dtable,
                          torch::Tensor out_bf16, torch::Tensor flags,
                          int64_t M, int64_t KP, int64_t off0, int64_t off1,
                          int64_t R) {
  CHK_CUDA(sorted_idx); CHK_CONTIG(sorted_idx);
  CHK_DT(sorted_idx, torch::kInt32); CHK_DT(perm, torch::kInt64);
  CHK_DT(gout, torch::kBFloat16); CHK_CONTIG(gout);
  CHK_DT(dtable, torch::kFloat32); CHK_CONTIG(dtable);
  CHK_DT(out_bf16, torch::kBFloat16); CHK_CONTIG(out_bf16);
  CHK_DT(flags, torch::kUInt8);
  const long N = sorted_idx.numel();
  const int S = dtable.size(1);
  launch_embed_scatter_sorted(sorted_idx.data_ptr<int>(),
                              perm.data_ptr<long>(), gout.data_ptr(),
                              dtable.data_ptr<float>(), out_bf16.data_ptr(),
                              flags.data_ptr<unsigned char>(), N, M, (int)KP,
                              S, (int)off0, (int)off1, (int)R, cur_stream());
}

void cast_clear_rows(torch::Tensor dtable, torch::Tensor counts,
                     torch::Tensor flags, torch::Tensor out) {
  CHK_CUDA(dtable); CHK_CONTIG(dtable); CHK_DT(dtable, torch::kFloat32);
  CHK_DT(counts, torch::kInt32); CHK_DT(out, torch::kBFloat16);
  CHK_DT(flags, torch::kUInt8); CHK_CONTIG(out);
  const long T = dtable.size(0);
  const int S = dtable.size(1);
  TORCH_CHECK(counts.numel() >= T && flags.numel() >= T, "counts/flags");
  launch_cast_clear_rows(dtable.data_ptr<float>(), counts.data_ptr<int>(),
                         flags.data_ptr<unsigned char>(), out.data_ptr(), T,
                         S, cur_stream());
}

// rng_off: int64 [1] DEVICE scalar holding the dropout counter offset;
// consumed by the kernel and advanced by M*EP on the same stream (device-
// side state so hipGraph replays keep drawing fresh masks).
void combiner_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor gamma,
                  torch::Tensor beta, torch::Tensor out, torch::Tensor z,
                  torch::Tensor mean, torch::Tensor rstd, int64_t E,
                  double p, int64_t seed, torch::Tensor rng_off,
                  int64_t epilogue_mode) {
  CHK_CUDA(x); CHK_CONTIG(x); CHK_DT(x, torch::kBFloat16);
  CHK_CONTIG(w); CHK_DT(w, torch::kBFloat16);
  CHK_DT(gamma, torch::kFloat32); CHK_DT(beta, torch::kFloat32);
  CHK_DT(out, torch::kBFloat16); CHK_DT(z, torch::kBFloat16);
  CHK_DT(mean, torch::kFloat32); CHK_DT(rstd, torch::kFloat32);
  const long M = x.size(0);
  const int KP = x.size(1), EP = w.size(0);  // w is TRANSPOSED: [EP, KP]
  TORCH_CHECK(w.size(1) == KP && KP % 32 == 0 && EP % 32 == 0, "w shape");
  CHK_DT(rng_off, torch::kInt64);
  launch_combiner_fwd(x.data_ptr(), w.data_ptr(), gamma.data_ptr<float>(),
                      beta.data_ptr<float>(), out.data_ptr(), z.data_ptr(),
                      mean.data_ptr<float>(), rstd.data_ptr<float>(), M, KP,
                      EP, (int)E, (float)p, (unsigned long long)seed,
                      (const unsigned long long*)rng_off.data_ptr(),
                      (int)epilogue_mode, cur_stream());
  if (p > 0.0)
    launch_bump_u64(rng_off.data_ptr(), (unsigned long long)(M * EP),
                    cur_stream());
}

// combiner_fwd that also emits the attention pool's raw scores
// raw_scores[M] = out . a from its flush (EP = 128, staged epilogue).
// Returns false, with raw_scores untouched, when the shape or epilogue
// mode has no score-emitting kernel; out/z/mean/rstd are written either
// way, with the bits of combiner_fwd.
bool combiner_fwd_scores(torch::Tensor x, torch::Tensor w,
                         torch::Tensor gamma, torch::Tensor beta,
                         torch::Tensor a, torch::Tensor out, torch::Tensor z,
                         torch::Tensor mean, torch::Tensor rstd,
                         torch::Tensor raw_scores, int64_t E, double p,
                         int64_t seed, torch::Tensor rng_off,
                         int64_t epilogue_mode) {
  CHK_CUDA(x); CHK_CONTIG(x); CHK_DT(x, torch::kBFloat16);
  CHK_CONTIG(w); CHK_DT(w, torch::kBFloat16);
  CHK_DT(gamma, torch::kFloat32); CHK_DT(beta, torch::kFloat32);
  CHK_DT(out, torch::kBFloat16); CHK_DT(z, torch::kBFloat16);
  CHK_CONTIG(out); CHK_CONTIG(z);
  CHK_DT(mean, torch::kFloat32); CHK_DT(rstd, torch::kFloat32);
  CHK_CUDA(a); CHK_CONTIG(a); CHK_DT(a, torch::kFloat32);
  CHK_CUDA(raw_scores); CHK_CONTIG(raw_scores);
  CHK_DT(raw_scores, torch::kFloat32);
  const long M = x.size(0);
  const int KP = x.size(1), EP = w.size(0);  // w is TRANSPOSED: [EP, KP]
  TORCH_CHECK(w.size(1) == KP && KP % 32 == 0 && EP % 32 == 0, "w shape");
  TORCH_CHECK(a.numel() == EP && raw_scores.numel() == M &&
              out.numel() == M * EP && z.numel() == M * EP &&
              mean.numel() == M && rstd.numel() == M &&
              gamma.numel() == EP && beta.numel() == EP,
              "combiner_fwd_scores shapes");
  CHK_DT(rng_off, torch::kInt64);
  const int wrote = launch_combiner_fwd_scores(
      x.data_ptr(), w.data_ptr(), gamma.data_ptr<float>(),
      beta.data_ptr<float>(), out.data_ptr(), z.data_ptr(),
      mean.data_ptr<float>(), rstd.data_ptr<float>(), M, KP, EP, (int)E,
      (float)p, (unsigned long long)seed,
      (const unsigned long long*)rng_off.data_ptr(), (int)epilogue_mode,
      a.data_ptr<float>(), raw_scores.data_ptr<float>(), cur_stream());
  if (p > 0.0)
    launch_bump_u64(rng_off.data_ptr(), (unsigned long long)(M * EP),
                    cur_stream());
  return wrote != 0;
}

void gather_combiner_fwd(torch::Tensor starts, torch::Tensor paths,
                         torch::Tensor ends, torch::Tensor term,
                         torch::Tensor path, torch::Tensor w,
                         torch::Tensor gamma, torch::Tensor beta,
                         torch::Tensor out, torch::Tensor z,
                         torch::Tensor mean, torch::Tensor rstd, int64_t KP,
                         int64_t E, double p, int64_t seed,
                         torch::Tensor rng_off) {
  CHK_CUDA(starts); CHK_CONTIG(starts); CHK_DT(starts, torch::kInt32);
  CHK_DT(term, torch::kBFloat16); CHK_CONTIG(term);
  CHK_DT(path, torch::kBFloat16); CHK_CONTIG(path);
  CHK_CONTIG(w); CHK_DT(w, torch::kBFloat16);
  CHK_DT(out, torch::kBFloat16); CHK_DT(z, torch::kBFloat16);
  const long M = starts.numel();
  const int EP = w.size(0);
  const int TS = term.size(1), PS = path.size(1);
  TORCH_CHECK(w.size(1) == KP && KP >= 2 * TS + PS, "shapes");
  CHK_DT(rng_off, torch::kInt64);
  launch_gather_combiner_fwd(
      starts.data_ptr<int>(), paths.data_ptr<int>(), ends.data_ptr<int>(),
      term.data_ptr(), path.data_ptr(), TS, PS, w.data_ptr(),
      gamma.data_ptr<float>(), beta.data_ptr<float>(), out.data_ptr(),
      z.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(), M,
      (int)KP, EP, (int)E, (float)p, (unsigned long long)seed,
      (const unsigned long long*)rng_off.data_ptr(), cur_stream());
  if (p > 0.0)
    launch_bump_u64(rng_off.data_ptr(),
                    (unsigned long long)(M * (long)w.size(0)),
                    cur_stream());
}

void wgrad_gather(torch::Tensor starts, torch::Tensor paths,
                  torch::Tensor ends, torch::Tensor term, torch::Tensor path,
                  torch::Tensor dz, torch::Tensor partials, int64_t KP) {
  CHK_CUDA(dz); CHK_CONTIG(dz); CHK_DT(dz, torch::kBFloat16);
  CHK_DT(partials, torch::kFloat32); CHK_CONTIG(partials);
  const long M = starts.numel();
  const int EP = dz.size(1);
  const int TS = term.size(1), PS = path.size(1);
  TORCH_CHECK(partials.size(1) == KP && partials.size(2) == EP, "partials");
  launch_wgrad_gather(starts.data_ptr<int>(), paths.data_ptr<int>(),
                      ends.data_ptr<int>(), term.data_ptr(), path.data_ptr(),
                      TS, PS, dz.data_ptr(), partials.data_ptr<float>(), M,
                      (int)KP, EP, partials.size(0), cur_stream());
}

void combiner_bwd(torch::Tensor dout, torch::Tensor z, torch::Tensor out,
                  torch::Tensor mean, torch::Tensor rstd, torch::Tensor gamma,
                  torch::Tensor beta, torch::Tensor dz, torch::Tensor dgamma,
                  torch::Tensor dbeta, int64_t E, double p) {
  CHK_CUDA(dout); CHK_CONTIG(dout); CHK_DT(dout, torch::kBFloat16);
  CHK_CONTIG(z); CHK_CONTIG(out); CHK_DT(out, torch::kBFloat16);
  CHK_DT(dz, torch::kBFloat16);
  const long M = z.size(0);
  const int EP = z.size(1);
  launch_combiner_bwd(dout.data_ptr(), z.data_ptr(), out.data_ptr(),
                      mean.data_ptr<float>(), rstd.data_ptr<float>(),
                      gamma.data_ptr<float>(), beta.data_ptr<float>(),
                      dz.data_ptr(), dgamma.data_ptr<float>(),
                      dbeta.data_ptr<float>(), M, EP, (int)E, (float)p,
                      cur_stream());
}

void group_by_index(torch::Tensor idx, torch::Tensor counts,
                    torch::Tensor cursor, torch::Tensor sorted_idx,
                    torch::Tensor perm, bool count_only) {
  CHK_CUDA(idx); CHK_CONTIG(idx); CHK_DT(idx, torch::kInt32);
  const long N = idx.numel();
  if (count_only) {
    launch_count_indices(idx.data_ptr<int>(), counts.data_ptr<int>(), N,
                         cur_stream());
  } else {
    launch_scatter_group(idx.data_ptr<int>(), cursor.data_ptr<int>(),
                         sorted_idx.data_ptr<int>(), perm.data_ptr<long>(), N,
                         cur_stream());
  }
}

void attention_fwd(torch::Tensor ccv, torch::Tensor a, torch::Tensor starts,
                   torch::Tensor cv, torch::Tensor attn, int64_t E) {
  CHK_CUDA(ccv); CHK_CONTIG(ccv); CHK_DT(ccv, torch::kBFloat16);
  CHK_DT(a, torch::kFloat32); CHK_DT(cv, torch::kFloat32);
  CHK_DT(attn, torch::kFloat32); CHK_DT(starts, torch::kInt32);
  const int B = ccv.size(0), C = ccv.size(1), EP = ccv.size(2);
  launch_attention_fwd(ccv.data_ptr(), a.data_ptr<float>(),
                       starts.data_ptr<int>(), cv.data_ptr<float>(), nullptr,
                       attn.data_ptr<float>(), B, C, EP, (int)E,
                       cur_stream());
}

// attention_fwd that also emits cv rounded to bf16 (cvb [B, EP])
void attention_fwd_cvb(torch::Tensor ccv, torch::Tensor a,
                       torch::Tensor starts, torch::Tensor cv,
                       torch::Tensor cvb, torch::Tensor attn, int64_t E) {
  CHK_CUDA(ccv); CHK_CONTIG(ccv); CHK_DT(ccv, torch::kBFloat16);
  CHK_DT(a, torch::kFloat32); CHK_DT(cv, torch::kFloat32);
  CHK_DT(attn, torch::kFloat32); CHK_DT(starts, torch::kInt32);
  CHK_DT(cvb, torch::kBFloat16); CHK_CONTIG(cvb); CHK_CONTIG(cv);
  CHK_CONTIG(attn); CHK_CONTIG(starts);
  const int B = ccv.size(0), C = ccv.size(1), EP = ccv.size(2);
  TORCH_CHECK(cv.numel() == (long)B * EP && cvb.numel() == (long)B * EP &&
              attn.numel() == (long)B * C && starts.numel() == (long)B * C &&
              a.numel() == EP, "attention_fwd_cvb shapes");
  launch_attention_fwd(ccv.data_ptr(), a.data_ptr<float>(),
                       starts.data_ptr<int>(), cv.data_ptr<float>(),
                       cvb.data_ptr(), attn.data_ptr<float>(), B, C, EP,
                       (int)E, cur_stream());
}

// compact attention backward: writes ds [B*C] f32 and the da partials, no
// dccv.  dcv is f32 or bf16 [B, EP].
void attention_bwd_compact(torch::Tensor dcv, torch::Tensor dattn,
                           torch::Tensor ccv, torch::Tensor a,
                           torch::Tensor starts, torch::Tensor attn,
                           torch::Tensor ds, torch::Tensor da, int64_t E,
                           bool has_dattn) {
  CHK_CUDA(dcv); CHK_CONTIG(dcv); CHK_CONTIG(ccv);
  CHK_DT(ccv, torch::kBFloat16);
  const bool dcv_bf16 = dcv.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(dcv_bf16 || dcv.scalar_type() == torch::kFloat32,
              "dcv must be f32 or bf16");
  CHK_DT(ds, torch::kFloat32); CHK_CONTIG(ds);
  CHK_DT(da, torch::kFloat32); CHK_CONTIG(da);
  CHK_DT(attn, torch::kFloat32); CHK_CONTIG(attn);
  CHK_DT(a, torch::kFloat32); CHK_DT(starts, torch::kInt32);
  CHK_CONTIG(starts);
  const int B = ccv.size(0), C = ccv.size(1), EP = ccv.size(2);
  TORCH_CHECK(dcv.numel() == (long)B * EP && ds.numel() == (long)B * C &&
              da.numel() == (long)B * EP && attn.numel() == (long)B * C &&
              starts.numel() == (long)B * C && a.numel() == EP && EP <= 384,
              "attention_bwd_compact shapes");
  if (has_dattn) {
    CHK_DT(dattn, torch::kFloat32); CHK_CONTIG(dattn);
    TORCH_CHECK(dattn.numel() == (long)B * C, "dattn shape");
  }
  launch_attention_bwd(dcv.data_ptr(), dcv_bf16 ? 1 : 0,
                       has_dattn ? dattn.data_ptr<float>() : nullptr,
                       ccv.data_ptr(), a.data_ptr<float>(),
                       starts.data_ptr<int>(), attn.data_ptr<float>(),
                       nullptr, ds.data_ptr<float>(), da.data_ptr<float>(),
                       B, C, EP, (int)E, has_dattn ? 1 : 0, cur_stream());
}

// shape gate of the two streaming attention kernels below
bool attention_stream_ok(int64_t C, int64_t EP) {
  return attention_stream_supported((int)C, (int)EP) != 0;
}

// attention forward from precomputed raw scores [B*C] (combiner_fwd_scores):
// mask, softmax, weighted pool; writes cv, cvb (bf16 copy) and attn
void attention_fwd_scores(torch::Tensor ccv, torch::Tensor raw_scores,
                          torch::Tensor starts, torch::Tensor cv,
                          torch::Tensor cvb, torch::Tensor attn, int64_t E) {
  CHK_CUDA(ccv); CHK_CONTIG(ccv); CHK_DT(ccv, torch::kBFloat16);
  CHK_CUDA(raw_scores); CHK_CONTIG(raw_scores);
  CHK_DT(raw_scores, torch::kFloat32);
  CHK_DT(cv, torch::kFloat32); CHK_CONTIG(cv);
  CHK_DT(cvb, torch::kBFloat16); CHK_CONTIG(cvb);
  CHK_DT(attn, torch::kFloat32); CHK_CONTIG(attn);
  CHK_DT(starts, torch::kInt32); CHK_CONTIG(starts);
  TORCH_CHECK(ccv.dim() == 3, "ccv must be [B, C, EP]");
  const int B = ccv.size(0), C = ccv.size(1), EP = ccv.size(2);
  TORCH_CHECK(attention_stream_supported(C, EP),
              "attention_fwd_scores: needs EP = 128 and 1 <= C <= 200");
  TORCH_CHECK(E >= 1 && E <= EP && raw_scores.numel() == (long)B * C &&
              cv.numel() == (long)B * EP && cvb.numel() == (long)B * EP &&
              attn.numel() == (long)B * C && starts.numel() == (long)B * C,
              "attention_fwd_scores shapes");
  launch_attention_fwd_scores(ccv.data_ptr(), raw_scores.data_ptr<float>(),
                              starts.data_ptr<int>(), cv.data_ptr<float>(),
                              cvb.data_ptr(), attn.data_ptr<float>(), B, C,
                              EP, (int)E, cur_stream());
}

// attention_bwd_compact with the method's rows held in registers
// (EP = 128, C <= 200); same outputs, same bits
void attention_bwd_compact_reg(torch::Tensor dcv, torch::Tensor dattn,
                               torch::Tensor ccv, torch::Tensor starts,
                               torch::Tensor attn, torch::Tensor ds,
                               torch::Tensor da, int64_t E, bool has_dattn) {
  CHK_CUDA(dcv); CHK_CONTIG(dcv); CHK_CUDA(ccv); CHK_CONTIG(ccv);
  CHK_DT(ccv, torch::kBFloat16);
  const bool dcv_bf16 = dcv.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(dcv_bf16 || dcv.scalar_type() == torch::kFloat32,
              "dcv must be f32 or bf16");
  CHK_DT(ds, torch::kFloat32); CHK_CONTIG(ds);
  CHK_DT(da, torch::kFloat32); CHK_CONTIG(da);
  CHK_DT(attn, torch::kFloat32); CHK_CONTIG(attn);
  CHK_DT(starts, torch::kInt32); CHK_CONTIG(starts);
  TORCH_CHECK(ccv.dim() == 3, "ccv must be [B, C, EP]");
  const int B = ccv.size(0), C = ccv.size(1), EP = ccv.size(2);
  TORCH_CHECK(attention_stream_supported(C, EP),
              "attention_bwd_compact_reg: needs EP = 128 and 1 <= C <= 200");
  TORCH_CHECK(E >= 1 && E <= EP && dcv.numel() == (long)B * EP &&
              ds.numel() == (long)B * C && da.numel() == (long)B * EP &&
              attn.numel() == (long)B * C && starts.numel() == (long)B * C,
              "attention_bwd_compact_reg shapes");
  if (has_dattn) {
    CHK_DT(dattn, torch::kFloat32); CHK_CONTIG(dattn);
    TORCH_CHECK(dattn.numel() == (long)B * C, "dattn shape");
  }
  launch_attention_bwd_compact_reg(
      dcv.data_ptr(), dcv_bf16 ? 1 : 0,
      has_dattn ? dattn.data_ptr<float>() : nullptr, ccv.data_ptr(),
      starts.data_ptr<int>(), attn.data_ptr<float>(), ds.data_ptr<float>(),
      da.data_ptr<float>(), B, C, EP, (int)E, has_dattn ? 1 : 0,
      cur_stream());
}

// K21 segmented attention pool over a packed batch: ccv [M, EP] bf16,
// starts [M] i32, offsets [B+1] i32 on the device (method b owns rows
// [offsets[b], offsets[b+1])); writes cv [B, EP] f32, cvb [B, EP] bf16 and
// attn [M] f32.  The kernel trusts offsets: functional.attention_pool_packed
// derives them from host-checked lengths and is the only caller.
void attention_pool_packed(torch::Tensor ccv, torch::Tensor a,
                           torch::Tensor starts, torch::Tensor offsets,
                           torch::Tensor cv, torch::Tensor cvb,
                           torch::Tensor attn, int64_t E, int64_t chunk) {
  CHK_CUDA(ccv); CHK_CONTIG(ccv); CHK_DT(ccv, torch::kBFloat16);
  CHK_CUDA(a); CHK_CONTIG(a); CHK_DT(a, torch::kFloat32);
  CHK_CUDA(starts); CHK_CONTIG(starts); CHK_DT(starts, torch::kInt32);
  CHK_CUDA(offsets); CHK_CONTIG(offsets); CHK_DT(offsets, torch::kInt32);
  CHK_CUDA(cv); CHK_CONTIG(cv); CHK_DT(cv, torch::kFloat32);
  CHK_CUDA(cvb); CHK_CONTIG(cvb); CHK_DT(cvb, torch::kBFloat16);
  CHK_CUDA(attn); CHK_CONTIG(attn); CHK_DT(attn, torch::kFloat32);
  TORCH_CHECK(ccv.dim() == 2, "ccv must be [M, EP]");
  TORCH_CHECK(chunk == attention_packed_chunk(),
              "attention_pool_packed: score chunk differs from the compiled ",
              attention_packed_chunk());
  const long M = ccv.size(0);
  const int EP = ccv.size(1);
  const long B = offsets.numel() - 1;
  TORCH_CHECK(EP % 32 == 0 && EP >= 32 && EP <= 1024 && E >= 1 && E <= EP,
              "attention_pool_packed: EP must be a multiple of 32 in "
              "32..1024 and 1 <= E <= EP");
  TORCH_CHECK(B >= 1 && B <= M && M < (1L << 31) && a.numel() == EP &&
              starts.numel() == M && attn.numel() == M &&
              cv.numel() == B * EP && cvb.numel() == B * EP,
              "attention_pool_packed shapes");
  TORCH_CHECK((uintptr_t)ccv.data_ptr() % 16 == 0, "ccv must be 16-B aligned");
  launch_attention_packed_fwd(ccv.data_ptr(), a.data_ptr<float>(),
                              starts.data_ptr<int>(), offsets.data_ptr<int>(),
                              cv.data_ptr<float>(), cvb.data_ptr(),
                              attn.data_ptr<float>(), M, B, EP, (int)E,
                              cur_stream());
}

// combiner backward that rebuilds dout = bf16(attn*dcv + ds*a) in
// registers (EP = 128); attn/ds [M] f32, dcv [M / C, 128] f32 or bf16
void combiner_bwd_recompute(torch::Tensor attn, torch::Tensor ds,
                            torch::Tensor dcv, torch::Tensor a, int64_t C,
                            torch::Tensor z, torch::Tensor out,
                            torch::Tensor mean, torch::Tensor rstd,
                            torch::Tensor gamma, torch::Tensor beta,
                            torch::Tensor dz, torch::Tensor dgamma,
                            torch::Tensor dbeta, int64_t E, double p) {
  CHK_CUDA(z); CHK_CONTIG(z); CHK_DT(z, torch::kBFloat16);
  CHK_CONTIG(out); CHK_DT(out, torch::kBFloat16);
  CHK_CONTIG(dz); CHK_DT(dz, torch::kBFloat16);
  CHK_CONTIG(attn); CHK_DT(attn, torch::kFloat32);
  CHK_CONTIG(ds); CHK_DT(ds, torch::kFloat32);
  CHK_CONTIG(dcv); CHK_CONTIG(a); CHK_DT(a, torch::kFloat32);
  CHK_DT(mean, torch::kFloat32); CHK_DT(rstd, torch::kFloat32);
  CHK_DT(gamma, torch::kFloat32); CHK_DT(dgamma, torch::kFloat32);
  CHK_DT(dbeta, torch::kFloat32);
  const bool dcv_bf16 = dcv.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(dcv_bf16 || dcv.scalar_type() == torch::kFloat32,
              "dcv must be f32 or bf16");
  const long M = z.size(0);
  const int EP = z.size(1);
  TORCH_CHECK(EP == 128 && C > 0 && M % C == 0 && M < (1L << 31) &&
              attn.numel() == M && ds.numel() == M &&
              dcv.numel() == (M / C) * EP && a.numel() == EP &&
              out.numel() == M * EP && dz.numel() == M * EP &&
              mean.numel() == M && rstd.numel() == M && gamma.numel() == EP,
              "combiner_bwd_recompute shapes");
  const long nblocks = std::min<long>((M + 3) / 4, 1024);
  TORCH_CHECK(dgamma.numel() == nblocks * EP && dbeta.numel() == nblocks * EP,
              "dgamma/dbeta partials must be [min(ceil(M/4), 1024), EP]");
  launch_combiner_bwd_recompute(
      attn.data_ptr<float>(), ds.data_ptr<float>(), dcv.data_ptr(),
      dcv_bf16 ? 1 : 0, a.data_ptr<float>(), (int)C, z.data_ptr(),
      out.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
      gamma.data_ptr<float>(), beta.data_ptr<float>(), dz.data_ptr(),
      dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), M, (int)E, (float)p,
      cur_stream());
}

// K22 segmented attention backward over a packed batch (the backward of
// attention_pool_packed): dcv [B, EP] f32 or bf16, ccv [M, EP] bf16, starts /
// attn [M], offsets [B+1] i32 on the device, dattn [M] f32 or empty.
// Compact form (dccv undefined/empty): writes ds [M] f32, seg [M] i32 (row ->
// method) and da_p [B, EP].  Dense form: writes dccv [M, EP] bf16 and da_p;
// ds [M] is its workspace.  As in the forward, the kernel trusts offsets.
static void attention_packed_bwd_impl(
    torch::Tensor dcv, torch::Tensor dattn, torch::Tensor ccv, torch::Tensor a,
    torch::Tensor starts, torch::Tensor offsets, torch::Tensor attn,
    torch::Tensor* dccv, torch::Tensor ds, torch::Tensor* seg,
    torch::Tensor da, int64_t E, bool has_dattn, int64_t chunk) {
  CHK_CUDA(dcv); CHK_CONTIG(dcv);
  const bool dcv_bf16 = dcv.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(dcv_bf16 || dcv.scalar_type() == torch::kFloat32,
              "dcv must be f32 or bf16");
  CHK_CUDA(ccv); CHK_CONTIG(ccv); CHK_DT(ccv, torch::kBFloat16);
  CHK_CUDA(a); CHK_CONTIG(a); CHK_DT(a, torch::kFloat32);
  CHK_CUDA(starts); CHK_CONTIG(starts); CHK_DT(starts, torch::kInt32);
  CHK_CUDA(offsets); CHK_CONTIG(offsets); CHK_DT(offsets, torch::kInt32);
  CHK_CUDA(attn); CHK_CONTIG(attn); CHK_DT(attn, torch::kFloat32);
  CHK_CUDA(ds); CHK_CONTIG(ds); CHK_DT(ds, torch::kFloat32);
  CHK_CUDA(da); CHK_CONTIG(da); CHK_DT(da, torch::kFloat32);
  TORCH_CHECK(ccv.dim() == 2, "ccv must be [M, EP]");
  TORCH_CHECK(dcv.dim() == 2, "dcv must be [B, EP]");
  TORCH_CHECK(chunk == attention_packed_chunk(),
              "attention_packed_bwd: score chunk differs from the compiled ",
              attention_packed_chunk());
  const long M = ccv.size(0);
  const int EP = ccv.size(1);
  const long B = dcv.size(0);
  TORCH_CHECK(EP % 32 == 0 && EP >= 32 && EP <= 384 && E >= 1 && E <= EP,
              "attention_packed_bwd: EP must be a multiple of 32 in 32..384 "
              "and 1 <= E <= EP");
  TORCH_CHECK(offsets.numel() == B + 1,
              "attention_packed_bwd: offsets must have B + 1 entries");
  TORCH_CHECK(B >= 1 && B <= M && M < (1L << 31) && dcv.size(1) == EP &&
              a.numel() == EP && starts.numel() == M && attn.numel() == M &&
              ds.numel() == M && da.numel() == B * EP,
              "attention_packed_bwd shapes");
  TORCH_CHECK((uintptr_t)ccv.data_ptr() % 16 == 0, "ccv must be 16-B aligned");
  if (has_dattn) {
    CHK_CUDA(dattn); CHK_CONTIG(dattn); CHK_DT(dattn, torch::kFloat32);
    TORCH_CHECK(dattn.numel() == M, "dattn shape");
  }
  void* dccv_p = nullptr;
  int* seg_p = nullptr;
  if (dccv) {
    CHK_CUDA(*dccv); CHK_CONTIG(*dccv); CHK_DT(*dccv, torch::kBFloat16);
    TORCH_CHECK(dccv->numel() == M * EP, "dccv shape");
    TORCH_CHECK((uintptr_t)dccv->data_ptr() % 16 == 0,
                "dccv must be 16-B aligned");
    dccv_p = dccv->data_ptr();
  } else {
    CHK_CUDA(*seg); CHK_CONTIG(*seg); CHK_DT(*seg, torch::kInt32);
    TORCH_CHECK(seg->numel() == M, "seg shape");
    seg_p = seg->data_ptr<int>();
  }
  launch_attention_packed_bwd(
      dcv.data_ptr(), dcv_bf16 ? 1 : 0,
      has_dattn ? dattn.data_ptr<float>() : nullptr, ccv.data_ptr(),
      a.data_ptr<float>(), starts.data_ptr<int>(), offsets.data_ptr<int>(),
      attn.data_ptr<float>(), dccv_p, ds.data_ptr<float>(), seg_p,
      da.data_ptr<float>(), M, B, EP, (int)E, cur_stream());
}

void attention_packed_bwd_compact(
    torch::Tensor dcv, torch::Tensor dattn, torch::Tensor ccv, torch::Tensor a,
    torch::Tensor starts, torch::Tensor offsets, torch::Tensor attn,
    torch::Tensor ds, torch::Tensor seg, torch::Tensor da, int64_t E,
    bool has_dattn, int64_t chunk) {
  attention_packed_bwd_impl(dcv, dattn, ccv, a, starts, offsets, attn,
                            nullptr, ds, &seg, da, E, has_dattn, chunk);
}

void attention_packed_bwd(
    torch::Tensor dcv, torch::Tensor dattn, torch::Tensor ccv, torch::Tensor a,
    torch::Tensor starts, torch::Tensor offsets, torch::Tensor attn,
    torch::Tensor dccv, torch::Tensor ds_ws, torch::Tensor da, int64_t E,
    bool has_dattn, int64_t chunk) {
  attention_packed_bwd_impl(dcv, dattn, ccv, a, starts, offsets, attn, &dccv,
                            ds_ws, nullptr, da, E, has_dattn, chunk);
}

// combiner_bwd_recompute for a packed batch: the method of a row is
// seg[row] (i32 [M], written by attention_packed_bwd_compact), dcv is
// [B, 128] f32 or bf16.  Same grid and partial layout.
void combiner_bwd_recompute_packed(
    torch::Tensor attn, torch::Tensor ds, torch::Tensor dcv, torch::Tensor a,
    torch::Tensor seg, torch::Tensor z, torch::Tensor out, torch::Tensor mean,
    torch::Tensor rstd, torch::Tensor gamma, torch::Tensor beta,
    torch::Tensor dz, torch::Tensor dgamma, torch::Tensor dbeta, int64_t E,
    double p) {
  CHK_CUDA(z); CHK_CONTIG(z); CHK_DT(z, torch::kBFloat16);
  CHK_CUDA(out); CHK_CONTIG(out); CHK_DT(out, torch::kBFloat16);
  CHK_CUDA(dz); CHK_CONTIG(dz); CHK_DT(dz, torch::kBFloat16);
  CHK_CUDA(attn); CHK_CONTIG(attn); CHK_DT(attn, torch::kFloat32);
  CHK_CUDA(ds); CHK_CONTIG(ds); CHK_DT(ds, torch::kFloat32);
  CHK_CUDA(seg); CHK_CONTIG(seg); CHK_DT(seg, torch::kInt32);
  CHK_CUDA(dcv); CHK_CONTIG(dcv);
  CHK_CUDA(a); CHK_CONTIG(a); CHK_DT(a, torch::kFloat32);
  CHK_CUDA(mean); CHK_CONTIG(mean); CHK_DT(mean, torch::kFloat32);
  CHK_CUDA(rstd); CHK_CONTIG(rstd); CHK_DT(rstd, torch::kFloat32);
  CHK_CUDA(gamma); CHK_CONTIG(gamma); CHK_DT(gamma, torch::kFloat32);
  CHK_CUDA(beta); CHK_CONTIG(beta); CHK_DT(beta, torch::kFloat32);
  CHK_CUDA(dgamma); CHK_CONTIG(dgamma); CHK_DT(dgamma, torch::kFloat32);
  CHK_CUDA(dbeta); CHK_CONTIG(dbeta); CHK_DT(dbeta, torch::kFloat32);
  const bool dcv_bf16 = dcv.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(dcv_bf16 || dcv.scalar_type() == torch::kFloat32,
              "dcv must be f32 or bf16");
  TORCH_CHECK(z.dim() == 2 && dcv.dim() == 2, "z must be [M, EP], dcv [B, EP]");
  const long M = z.size(0);
  const int EP = z.size(1);
  const long B = dcv.size(0);
  TORCH_CHECK(EP == 128 && B >= 1 && B <= M && M < (1L << 31) &&
              E >= 1 && E <= EP && attn.numel() == M && ds.numel() == M &&
              seg.numel() == M && dcv.size(1) == EP && a.numel() == EP &&
              out.numel() == M * EP && dz.numel() == M * EP &&
              mean.numel() == M && rstd.numel() == M && gamma.numel() == EP &&
              beta.numel() == EP,
              "combiner_bwd_recompute_packed shapes");
  const long nblocks = std::min<long>((M + 3) / 4, 1024);
  TORCH_CHECK(dgamma.numel() == nblocks * EP && dbeta.numel() == nblocks * EP,
              "dgamma/dbeta partials must be [min(ceil(M/4), 1024), EP]");
  launch_combiner_bwd_recompute_packed(
      attn.data_ptr<float>(), ds.data_ptr<float>(), dcv.data_ptr(),
      dcv_bf16 ? 1 : 0, a.data_ptr<float>(), seg.data_ptr<int>(), B,
      z.data_ptr(), out.data_ptr(), mean.data_ptr<float>(),
      rstd.data_ptr<float>(), gamma.data_ptr<float>(),
      beta.data_ptr<float>(), dz.data_ptr(), dgamma.data_ptr<float>(),
      dbeta.data_ptr<float>(), M, (int)E, (float)p, cur_stream());
}

void attention_bwd(torch::Tensor dcv, torch::Tensor dattn, torch::Tensor ccv,
                   torch::Tensor a, torch::Tensor starts, torch::Tensor attn,
                   torch::Tensor dccv, torch::Tensor da, int64_t E,
                   bool has_dattn) {
  CHK_CUDA(dcv); CHK_CONTIG(dcv); CHK_DT(dcv, torch::kFloat32);
  CHK_DT(dccv, torch::kBFloat16); CHK_DT(da, torch::kFloat32);
  const int B = ccv.size(0), C = ccv.size(1), EP = ccv.size(2);
  TORCH_CHECK(dccv.data_ptr() != nullptr, "dccv must be allocated");
  launch_attention_bwd(dcv.data_ptr<float>(), 0,
                       has_dattn ? dattn.data_ptr<float>() : nullptr,
                       ccv.data_ptr(), a.data_ptr<float>(),
                       starts.data_ptr<int>(), attn.data_ptr<float>(),
                       dccv.data_ptr(), nullptr, da.data_ptr<float>(), B, C,
                       EP, (int)E, has_dattn ? 1 : 0, cur_stream());
}

void logsoftmax_nll_fwd(torch::Tensor logits, torch::Tensor label,
                        torch::Tensor weight, torch::Tensor lse,
                        torch::Tensor acc) {
  CHK_CUDA(logits); CHK_CONTIG(logits); CHK_DT(logits, torch::kBFloat16);
  CHK_DT(label, torch::kInt64); CHK_DT(lse, torch::kFloat32);
  const int B = logits.size(0);
  const long L = logits.size(1);
  TORCH_CHECK(acc.numel() == 2L * B, "acc must be [B, 2] partials");
  const float* wp = weight.defined() && weight.numel() > 0
                        ? weight.data_ptr<float>()
                        : nullptr;
  launch_lsm_nll_fwd(logits.data_ptr(), label.data_ptr<long>(), wp,
                     lse.data_ptr<float>(), acc.data_ptr<float>(), B, L,
                     cur_stream());
}

void logsoftmax_nll_bwd(torch::Tensor logits, torch::Tensor label,
                        torch::Tensor weight, torch::Tensor lse,
                        torch::Tensor acc, torch::Tensor gscale,
                        torch::Tensor dlogits) {
  CHK_CUDA(logits); CHK_CONTIG(dlogits); CHK_DT(dlogits, torch::kBFloat16);
  const int B = logits.size(0);
  const long L = logits.size(1);
  const float* wp = weight.defined() && weight.numel() > 0
                        ? weight.data_ptr<float>()
                        : nullptr;
  launch_lsm_nll_bwd(logits.data_ptr(), label.data_ptr<long>(), wp,
                     lse.data_ptr<float>(), acc.data_ptr<float>(),
                     gscale.data_ptr<float>(), dlogits.data_ptr(), B, L,
                     cur_stream());
}

// (max, sumexp) partials over 16384-col chunks -> pm/ps[GX][B]
void lsm_partial(torch::Tensor logits, torch::Tensor pm, torch::Tensor ps) {
  CHK_CUDA(logits); CHK_CONTIG(logits); CHK_DT(logits, torch::kBFloat16);
  CHK_DT(pm, torch::kFloat32); CHK_CONTIG(pm); CHK_CONTIG(ps);
  const int B = logits.size(0);
  const long L = logits.size(1);
  const long GX = (L + 16383) / 16384;
  TORCH_CHECK(pm.numel() == GX * B && ps.numel() == GX * B,
              "lsm_partial partials shape");
  launch_lsm_partial(logits.data_ptr(), pm.data_ptr<float>(),
                     ps.data_ptr<float>(), B, L, cur_stream());
}

void dgrad(torch::Tensor dz, torch::Tensor w2, torch::Tensor dx) {
  CHK_CUDA(dz); CHK_CONTIG(dz); CHK_DT(dz, torch::kBFloat16);
  CHK_CONTIG(w2); CHK_DT(w2, torch::kBFloat16);
  CHK_CONTIG(dx); CHK_DT(dx, torch::kBFloat16);
  const long M = dz.size(0);
  const int EP = dz.size(1), KP = w2.size(0);
  TORCH_CHECK(w2.size(1) == EP && dx.size(1) == KP, "dgrad shapes");
  launch_dgrad(dz.data_ptr(), w2.data_ptr(), dx.data_ptr(), M, KP, EP,
               cur_stream());
}

void head_wgrad(torch::Tensor dlogits, torch::Tensor cv, torch::Tensor dw) {
  CHK_CUDA(dlogits); CHK_CONTIG(dlogits); CHK_DT(dlogits, torch::kBFloat16);
  CHK_CONTIG(cv); CHK_DT(cv, torch::kBFloat16);
  CHK_CONTIG(dw); CHK_DT(dw, torch::kBFloat16);
  const long B = dlogits.size(0), L = dlogits.size(1);
  const int EP = cv.size(1);
  TORCH_CHECK(dw.size(0) == L && dw.size(1) == EP, "dw shape");
  TORCH_CHECK(B % 32 == 0 && L % 8 == 0, "head_wgrad shape gates");
  launch_head_wgrad(dlogits.data_ptr(), cv.data_ptr(), dw.data_ptr(), L, B,
                    EP, cur_stream());
}

// logits = cv @ w^T + bias; pm/ps (optional, pass undefined tensors to
// skip) receive per-(row, 64-col-block) online-softmax partials.
void head_fwd(torch::Tensor cv, torch::Tensor w, torch::Tensor bias,
              torch::Tensor out, torch::Tensor pm, torch::Tensor ps) {
  CHK_CUDA(cv); CHK_CONTIG(cv); CHK_DT(cv, torch::kBFloat16);
  CHK_CONTIG(w); CHK_DT(w, torch::kBFloat16);
  CHK_DT(bias, torch::kFloat32); CHK_CONTIG(bias);
  CHK_CONTIG(out); CHK_DT(out, torch::kBFloat16);
  const long B = cv.size(0), L = w.size(0);
  const int EP = cv.size(1);
  TORCH_CHECK(w.size(1) == EP && EP % 32 == 0, "head_fwd EP");
  TORCH_CHECK(out.size(0) == B && out.size(1) == L && bias.numel() == L,
              "head_fwd shapes");
  float* pmp = nullptr;
  float* psp = nullptr;
  if (pm.defined() && pm.numel() > 0) {
    const long GXL = (L + 255) / 256;  // [lab_block, B] layout
    CHK_DT(pm, torch::kFloat32); CHK_CONTIG(pm);
    TORCH_CHECK(pm.numel() == B * GXL && ps.numel() == B * GXL, "partials");
    pmp = pm.data_ptr<float>();
    psp = ps.data_ptr<float>();
  }
  launch_head_fwd(cv.data_ptr(), w.data_ptr(), bias.data_ptr<float>(),
                  out.data_ptr(), pmp, psp, B, L, EP, /*aimg=*/0,
                  cur_stream());
}

// head_fwd consuming the swizzle_a W image ([ceil(L/256)*16, 4, 64, 8]);
// out/pm/ps contracts as head_fwd
void head_fwd_img(torch::Tensor cv, torch::Tensor wimg, torch::Tensor bias,
                  torch::Tensor out, torch::Tensor pm, torch::Tensor ps,
                  int64_t L) {
  CHK_CUDA(cv); CHK_CONTIG(cv); CHK_DT(cv, torch::kBFloat16);
  CHK_CONTIG(wimg); CHK_DT(wimg, torch::kBFloat16);
  CHK_DT(bias, torch::kFloat32); CHK_CONTIG(bias);
  CHK_CONTIG(out); CHK_DT(out, torch::kBFloat16);
  const long B = cv.size(0);
  const int EP = cv.size(1);
  TORCH_CHECK(EP == 128, "head_fwd_img is EP=128 only");
  TORCH_CHECK(wimg.numel() == (L + 255) / 256 * 16 * 2048,
              "wimg must be [ceil(L/256)*16, 4, 64, 8]");
  TORCH_CHECK(out.size(0) == B && out.size(1) == L && bias.numel() == L,
              "head_fwd_img shapes");
  float* pmp = nullptr;
  float* psp = nullptr;
  if (pm.defined() && pm.numel() > 0) {
    const long GXL = (L + 255) / 256;
    CHK_DT(pm, torch::kFloat32); CHK_CONTIG(pm);
    TORCH_CHECK(pm.numel() == B * GXL && ps.numel() == B * GXL, "partials");
    pmp = pm.data_ptr<float>();
    psp = ps.data_ptr<float>();
  }
  launch_head_fwd(cv.data_ptr(), wimg.data_ptr(), bias.data_ptr<float>(),
                  out.data_ptr(), pmp, psp, B, L, EP, /*aimg=*/1,
                  cur_stream());
}

void swizzle_a(torch::Tensor w, torch::Tensor wimg) {
  CHK_CUDA(w); CHK_CONTIG(w); CHK_DT(w, torch::kBFloat16);
  CHK_CONTIG(wimg); CHK_DT(wimg, torch::kBFloat16);
  const long L = w.size(0);
  TORCH_CHECK(w.size(1) == 128, "w must be [L, 128]");
  const long nrt = wimg.numel() / 2048;
  TORCH_CHECK(nrt * 2048 == wimg.numel() && nrt >= (L + 15) / 16,
              "wimg must be [nrt >= ceil(L/16), 4, 64, 8]");
  launch_swizzle_a(w.data_ptr(), wimg.data_ptr(), L, nrt, cur_stream());
}

void logsoftmax_nll_finalize(torch::Tensor logits, torch::Tensor pm,
                             torch::Tensor ps, torch::Tensor label,
                             torch::Tensor weight, torch::Tensor lse,
                             torch::Tensor acc) {
  CHK_CUDA(logits); CHK_CONTIG(logits); CHK_DT(logits, torch::kBFloat16);
  CHK_DT(pm, torch::kFloat32); CHK_CONTIG(pm);
  CHK_DT(lse, torch::kFloat32);
  const int B = logits.size(0);
  const long L = logits.size(1);
  // GX derived from the partials shape: 256-col blocks from the head_fwd
  // epilogue, 4096-col blocks from lsm_partial — finalize is generic
  const int GX = (int)(pm.numel() / B);
  TORCH_CHECK((long)GX * B == pm.numel() && ps.numel() == pm.numel(),
              "partials");
  TORCH_CHECK(acc.numel() == 2L * ((B + 15) / 16),
              "acc must be [(B+15)/16, 2] partials");
  const float* wp = weight.defined() && weight.numel() > 0
                        ? weight.data_ptr<float>()
                        : nullptr;
  launch_lsm_finalize(logits.data_ptr(), pm.data_ptr<float>(),
                      ps.data_ptr<float>(), label.data_ptr<long>(), wp,
                      lse.data_ptr<float>(), acc.data_ptr<float>(), B, L, GX,
                      cur_stream());
}

// dcv split-K partials: partials[ceil(L/512), B, 128] f32; wt = W
// transposed [EP=128, L]
void head_dgrad(torch::Tensor dlogits, torch::Tensor wt,
                torch::Tensor partials) {
  CHK_CUDA(dlogits); CHK_CONTIG(dlogits); CHK_DT(dlogits, torch::kBFloat16);
  CHK_CONTIG(wt); CHK_DT(wt, torch::kBFloat16);
  CHK_DT(partials, torch::kFloat32); CHK_CONTIG(partials);
  const long B = dlogits.size(0), L = dlogits.size(1);
  TORCH_CHECK(wt.size(0) == 128 && wt.size(1) == L, "wt must be [128, L]");
  TORCH_CHECK(L % 8 == 0, "head_dgrad needs L % 8 == 0");
  TORCH_CHECK(partials.numel() == (L + 511) / 512 * B * 128, "partials");
  launch_head_dgrad(dlogits.data_ptr(), wt.data_ptr(),
                    partials.data_ptr<float>(), B, L, cur_stream());
}

// Fused head+loss backward prep: coef_lse[B, 4] = (coef_b, lse_b, y_b, 0).
// exclusive prefix scan x[0..n-1] -> out[0..n-1] (int32); partial is a
// scratch of >= ceil(n/1024) ints
void exclusive_scan(torch::Tensor x, torch::Tensor partial,
                    torch::Tensor out) {
  CHK_CUDA(x); CHK_CONTIG(x); CHK_DT(x, torch::kInt32);
  CHK_CONTIG(partial); CHK_DT(partial, torch::kInt32);
  CHK_CONTIG(out); CHK_DT(out, torch::kInt32);
  const long n = x.numel();
  TORCH_CHECK(out.numel() >= n, "scan out too small");
  TORCH_CHECK(partial.numel() >= (n + 1023) / 1024, "scan partial too small");
  launch_exclusive_scan(x.data_ptr<int>(), partial.data_ptr<int>(),
                        out.data_ptr<int>(), n, cur_stream());
}

long cub_scan_temp_bytes(long n) {
  return (long)cub_exclusive_scan_temp_bytes(n);
}

// hipCUB decoupled-lookback exclusive scan; temp is a uint8 scratch of
// at least cub_scan_temp_bytes(n)
void cub_exclusive_scan(torch::Tensor x, torch::Tensor temp,
                        torch::Tensor out) {
  CHK_CUDA(x); CHK_CONTIG(x); CHK_DT(x, torch::kInt32);
  CHK_CONTIG(out); CHK_DT(out, torch::kInt32);
  const long n = x.numel();
  TORCH_CHECK(out.numel() >= n, "scan out too small");
  TORCH_CHECK(temp.numel() >= (long)cub_exclusive_scan_temp_bytes(n),
              "cub scan temp too small");
  launch_cub_exclusive_scan(x.data_ptr<int>(), out.data_ptr<int>(),
                            temp.data_ptr(), (size_t)temp.numel(), n,
                            cur_stream());
}

void head_bwd_prep(torch::Tensor label, torch::Tensor weight,
                   torch::Tensor acc, torch::Tensor gscale, torch::Tensor lse,
                   torch::Tensor coef_lse) {
  CHK_CUDA(lse); CHK_DT(lse, torch::kFloat32); CHK_DT(label, torch::kInt64);
  CHK_CONTIG(coef_lse); CHK_DT(coef_lse, torch::kFloat32);
  const long B = label.numel();
  TORCH_CHECK(coef_lse.numel() == 4 * B, "coef_lse must be [B, 4]");
  const float* wp = weight.defined() && weight.numel() > 0
                        ? weight.data_ptr<float>()
                        : nullptr;
  launch_head_bwd_prep(label.data_ptr<long>(), wp, acc.data_ptr<float>(),
                       gscale.data_ptr<float>(), lse.data_ptr<float>(),
                       coef_lse.data_ptr<float>(), B, cur_stream());
}

// [N, 128] -> B-fragment image [nchunk, 8, 64, 8]; nchunk (from the
// output shape) must cover N at the consumer's stage granularity.
void swizzle_cv(torch::Tensor cv, torch::Tensor cvimg) {
  CHK_CUDA(cv); CHK_CONTIG(cv); CHK_DT(cv, torch::kBFloat16);
  CHK_CONTIG(cvimg); CHK_DT(cvimg, torch::kBFloat16);
  const long B = cv.size(0);
  TORCH_CHECK(cv.size(1) == 128, "operand must be [N, 128]");
  const long nchunk = cvimg.numel() / 4096;
  TORCH_CHECK(nchunk * 4096 == cvimg.numel() && nchunk >= (B + 31) / 32,
              "image shape must be [nchunk >= ceil(N/32), 8, 64, 8]");
  launch_swizzle_cv(cv.data_ptr(), cvimg.data_ptr(), B, nchunk,
                    cur_stream());
}

// Fused head+loss backward kernel 1: dw[L, 128] bf16 + dbias[L] f32 from
// (logits, coef_lse) with G recomputed in-kernel; cvimg = swizzle_cv(cv).
void head_bwd_dw(torch::Tensor logits, torch::Tensor cvimg,
                 torch::Tensor coef_lse, torch::Tensor dw,
                 torch::Tensor dbias) {
  CHK_CUDA(logits); CHK_CONTIG(logits); CHK_DT(logits, torch::kBFloat16);
  CHK_CONTIG(cvimg); CHK_DT(cvimg, torch::kBFloat16);
  CHK_CONTIG(coef_lse); CHK_DT(coef_lse, torch::kFloat32);
  CHK_CONTIG(dw); CHK_DT(dw, torch::kBFloat16);
  CHK_CONTIG(dbias); CHK_DT(dbias, torch::kFloat32);
  const long B = logits.size(0), L = logits.size(1);
  TORCH_CHECK(cvimg.numel() == (B + 63) / 64 * 2 * 4096, "cvimg shape");
  TORCH_CHECK(L % 8 == 0 && B % 8 == 0, "head_bwd_dw shape gates");
  TORCH_CHECK(L < (1L << 24), "label index carried as f32 needs L < 2^24");
  TORCH_CHECK(coef_lse.numel() == 4 * B, "coef_lse must be [B, 4]");
  TORCH_CHECK(dw.size(0) == L && dw.size(1) == 128 && dbias.numel() == L,
              "head_bwd_dw output shapes");
  launch_head_bwd_dw(logits.data_ptr(), cvimg.data_ptr(),
                     coef_lse.data_ptr<float>(), dw.data_ptr(),
                     dbias.data_ptr<float>(), B, L, cur_stream());
}

// Fused head+loss backward kernel 2: dcv split-K partials
// [ceil(L/chunk), B, 128] f32 with G recomputed; wimg = swizzle_cv(W)
// at 128-label granularity ([ceil(L/128)*4, 8, 64, 8]).
void head_bwd_dcv(torch::Tensor logits, torch::Tensor wimg,
                  torch::Tensor coef_lse, torch::Tensor partials,
                  long chunk) {
  CHK_CUDA(logits); CHK_CONTIG(logits); CHK_DT(logits, torch::kBFloat16);
  CHK_CONTIG(wimg); CHK_DT(wimg, torch::kBFloat16);
  CHK_CONTIG(coef_lse); CHK_DT(coef_lse, torch::kFloat32);
  CHK_DT(partials, torch::kFloat32); CHK_CONTIG(partials);
  const long B = logits.size(0), L = logits.size(1);
  TORCH_CHECK(wimg.numel() == (L + 127) / 128 * 4 * 4096,
              "wimg must be [ceil(L/128)*4, 8, 64, 8]");
  TORCH_CHECK(L % 8 == 0 && chunk % 128 == 0, "head_bwd_dcv shape gates");
  TORCH_CHECK(L < (1L << 24), "label index carried as f32 needs L < 2^24");
  TORCH_CHECK(coef_lse.numel() == 4 * B, "coef_lse must be [B, 4]");
  TORCH_CHECK(partials.numel() == (L + chunk - 1) / chunk * B * 128,
              "head_bwd_dcv partials shape");
  launch_head_bwd_dcv(logits.data_ptr(), wimg.data_ptr(),
                      coef_lse.data_ptr<float>(),
                      partials.data_ptr<float>(), B, L, (int)chunk,
                      cur_stream());
}

// Pipelined head_bwd_dw (bit-identical outputs): depth = 64-row
// sub-stages per K-loop stage, 0 = C2V_HB_DW_DEPTH or the shipped default.
void head_bwd_dw_pipe(torch::Tensor logits, torch::Tensor cvimg,
                      torch::Tensor coef_lse, torch::Tensor dw,
                      torch::Tensor dbias, long depth) {
  CHK_CUDA(logits); CHK_CONTIG(logits); CHK_DT(logits, torch::kBFloat16);
  CHK_CONTIG(cvimg); CHK_DT(cvimg, torch::kBFloat16);
  CHK_CONTIG(coef_lse); CHK_DT(coef_lse, torch::kFloat32);
  CHK_CONTIG(dw); CHK_DT(dw, torch::kBFloat16);
  CHK_CONTIG(dbias); CHK_DT(dbias, torch::kFloat32);
  const long B = logits.size(0), L = logits.size(1);
  TORCH_CHECK(B > 0 && L > 0, "head_bwd_dw_pipe needs B, L > 0");
  TORCH_CHECK(cvimg.numel() == (B + 63) / 64 * 2 * 4096, "cvimg shape");
  TORCH_CHECK(L % 8 == 0 && B % 8 == 0, "head_bwd_dw_pipe shape gates");
  TORCH_CHECK(L < (1L << 24), "label index carried as f32 needs L < 2^24");
  TORCH_CHECK(coef_lse.numel() == 4 * B, "coef_lse must be [B, 4]");
  TORCH_CHECK(dw.size(0) == L && dw.size(1) == 128 && dbias.numel() == L,
              "head_bwd_dw_pipe output shapes");
  TORCH_CHECK(launch_head_bwd_dw_pipe(
                  logits.data_ptr(), cvimg.data_ptr(),
                  coef_lse.data_ptr<float>(), dw.data_ptr(),
                  dbias.data_ptr<float>(), B, L, (int)depth, cur_stream()),
              "head_bwd_dw_pipe: no instantiation for this depth / "
              "C2V_HBDW_VARIANT");
}

// Pipelined head_bwd_dcv (bit-identical partials): dbuf = 1 double-buffers
// the W image in LDS, 0 keeps one buffer, -1 = C2V_HB_DCV_DBUF or the
// shipped default.
void head_bwd_dcv_pipe(torch::Tensor logits, torch::Tensor wimg,
                       torch::Tensor coef_lse, torch::Tensor partials,
                       long chunk, long dbuf) {
  CHK_CUDA(logits); CHK_CONTIG(logits); CHK_DT(logits, torch::kBFloat16);
  CHK_CONTIG(wimg); CHK_DT(wimg, torch::kBFloat16);
  CHK_CONTIG(coef_lse); CHK_DT(coef_lse, torch::kFloat32);
  CHK_DT(partials, torch::kFloat32); CHK_CONTIG(partials);
  const long B = logits.size(0), L = logits.size(1);
  TORCH_CHECK(B > 0 && L > 0, "head_bwd_dcv_pipe needs B, L > 0");
  TORCH_CHECK(wimg.numel() == (L + 127) / 128 * 4 * 4096,
              "wimg must be [ceil(L/128)*4, 8, 64, 8]");
  TORCH_CHECK(L % 8 == 0 && chunk > 0 && chunk % 128 == 0,
              "head_bwd_dcv_pipe shape gates");
  TORCH_CHECK(L < (1L << 24), "label index carried as f32 needs L < 2^24");
  TORCH_CHECK(coef_lse.numel() == 4 * B, "coef_lse must be [B, 4]");
  TORCH_CHECK(partials.numel() == (L + chunk - 1) / chunk * B * 128,
              "head_bwd_dcv_pipe partials shape");
  launch_head_bwd_dcv_pipe(logits.data_ptr(), wimg.data_ptr(),
                           coef_lse.data_ptr<float>(),
                           partials.data_ptr<float>(), B, L, (int)chunk,
                           (int)dbuf, cur_stream());
}

// Streaming dcv: logits never read — recomputed per wave from the
// swizzle_a fragment images of cv ([B,128]) and W ([L,128]) plus the f32
// bias [L].
void head_bwd_dcv_rc(torch::Tensor cvimg_a, torch::Tensor wimg_a,
                     torch::Tensor wimg, torch::Tensor bias,
                     torch::Tensor coef_lse, torch::Tensor partials, long B,
                     long L, long chunk) {
  CHK_CUDA(wimg); CHK_CONTIG(wimg); CHK_DT(wimg, torch::kBFloat16);
  CHK_CONTIG(cvimg_a); CHK_DT(cvimg_a, torch::kBFloat16);
  CHK_CONTIG(wimg_a); CHK_DT(wimg_a, torch::kBFloat16);
  CHK_CUDA(bias); CHK_CONTIG(bias); CHK_DT(bias, torch::kFloat32);
  CHK_CONTIG(coef_lse); CHK_DT(coef_lse, torch::kFloat32);
  CHK_DT(partials, torch::kFloat32); CHK_CONTIG(partials);
  TORCH_CHECK(bias.numel() == L, "bias must be [L]");
  TORCH_CHECK(wimg.numel() == (L + 127) / 128 * 4 * 4096,
              "wimg must be [ceil(L/128)*4, 8, 64, 8]");
  TORCH_CHECK(cvimg_a.numel() >= (B + 127) / 128 * 8 * 2048,
              "cvimg_a too small for B");
  TORCH_CHECK(wimg_a.numel() >= (L + 255) / 256 * 16 * 2048,
              "wimg_a too small for L");
  TORCH_CHECK(L % 8 == 0 && chunk % 128 == 0, "head_bwd_dcv_rc shape gates");
  TORCH_CHECK(L < (1L << 24), "label index carried as f32 needs L < 2^24");
  TORCH_CHECK(coef_lse.numel() == 4 * B, "coef_lse must be [B, 4]");
  TORCH_CHECK(partials.numel() == (L + chunk - 1) / chunk * B * 128,
              "head_bwd_dcv_rc partials shape");
  launch_head_bwd_dcv_rc(cvimg_a.data_ptr(), wimg_a.data_ptr(),
                         wimg.data_ptr(), bias.data_ptr<float>(),
                         coef_lse.data_ptr<float>(),
                         partials.data_ptr<float>(), B, L, (int)chunk,
                         cur_stream());
}

// K11 angular-margin building blocks (all [N, 128] bf16 row spaces)
void inv_rownorm(torch::Tensor x, torch::Tensor inv) {
  CHK_CUDA(x); CHK_CONTIG(x); CHK_DT(x, torch::kBFloat16);
  CHK_DT(inv, torch::kFloat32);
  TORCH_CHECK(x.size(1) == 128 && inv.numel() == x.size(0), "inv_rownorm");
  launch_inv_rownorm(x.data_ptr(), inv.data_ptr<float>(), x.size(0),
                     cur_stream());
}

void rowscale(torch::Tensor x, torch::Tensor inv, torch::Tensor out) {
  CHK_CUDA(x); CHK_CONTIG(x); CHK_DT(x, torch::kBFloat16);
  CHK_CONTIG(out); CHK_DT(out, torch::kBFloat16);
  TORCH_CHECK(x.size(1) == 128 && out.sizes() == x.sizes() &&
              inv.numel() == x.size(0), "rowscale");
  launch_rowscale(x.data_ptr(), inv.data_ptr<float>(), out.data_ptr(),
                  x.size(0), cur_stream());
}

void angular_fwd(torch::Tensor ucv, torch::Tensor uw, torch::Tensor label,
                 torch::Tensor out, torch::Tensor cos_out, double cos_m,
                 double sin_m, double s) {
  CHK_CUDA(ucv); CHK_CONTIG(ucv); CHK_DT(ucv, torch::kBFloat16);
  CHK_CONTIG(uw); CHK_DT(uw, torch::kBFloat16);
  CHK_DT(label, torch::kInt64);
  CHK_CONTIG(out); CHK_DT(out, torch::kBFloat16);
  CHK_CONTIG(cos_out); CHK_DT(cos_out, torch::kBFloat16);
  const long B = ucv.size(0), L = uw.size(0);
  TORCH_CHECK(ucv.size(1) == 128 && uw.size(1) == 128 &&
              out.size(0) == B && out.size(1) == L &&
              cos_out.sizes() == out.sizes() && label.numel() == B,
              "angular_fwd shapes");
  launch_angular_fwd(ucv.data_ptr(), uw.data_ptr(), label.data_ptr<long>(),
                     out.data_ptr(), cos_out.data_ptr(), B, L, (float)cos_m,
                     (float)sin_m, (float)s, cur_stream());
}

void angular_dcos(torch::Tensor dout, torch::Tensor cosm,
                  torch::Tensor label, torch::Tensor dcos, double cos_m,
                  double sin_m, double s) {
  CHK_CUDA(dout); CHK_CONTIG(dout); CHK_DT(dout, torch::kBFloat16);
  CHK_CONTIG(cosm); CHK_DT(cosm, torch::kBFloat16);
  CHK_CONTIG(dcos); CHK_DT(dcos, torch::kBFloat16);
  const long B = dout.size(0), L = dout.size(1);
  TORCH_CHECK(cosm.sizes() == dout.sizes() && dcos.sizes() == dout.sizes()
              && label.numel() == B, "angular_dcos shapes");
  launch_angular_dcos(dout.data_ptr(), cosm.data_ptr(),
                      label.data_ptr<long>(), dcos.data_ptr(), B, L,
                      (float)cos_m, (float)sin_m, (float)s, cur_stream());
}

void norm_project(torch::Tensor du, torch::Tensor u, torch::Tensor inv,
                  torch::Tensor out) {
  CHK_CUDA(du); CHK_CONTIG(du); CHK_DT(du, torch::kBFloat16);
  CHK_CONTIG(u); CHK_DT(u, torch::kBFloat16);
  CHK_CONTIG(out); CHK_DT(out, torch::kBFloat16);
  TORCH_CHECK(du.size(1) == 128 && u.sizes() == du.sizes() &&
              out.sizes() == du.sizes() && inv.numel() == du.size(0),
              "norm_project shapes");
  launch_norm_project(du.data_ptr(), u.data_ptr(), inv.data_ptr<float>(),
                      out.data_ptr(), du.size(0), cur_stream());
}

// K17: per-row (max value, argmax) over bf16 logits (torch.max ties)
void row_max_argmax(torch::Tensor x, torch::Tensor vals, torch::Tensor idx) {
  CHK_CUDA(x); CHK_CONTIG(x); CHK_DT(x, torch::kBFloat16);
  CHK_DT(vals, torch::kFloat32); CHK_DT(idx, torch::kInt64);
  const long B = x.size(0), L = x.size(1);
  TORCH_CHECK(vals.numel() == B && idx.numel() == B, "row_max_argmax");
  launch_row_max_argmax(x.data_ptr(), vals.data_ptr<float>(),
                        idx.data_ptr<long>(), B, L, cur_stream());
}

// K19: per-row top-k + log-sum-exp.  x: [B, L] bf16 or f32; vals f32
// [B, k], idx i64 [B, k] (descending value, ties to the smallest column),
// lse f32 [B].  part (i64 [B, nchunk, 16]) and pm/ps (f32 [B, nchunk])
// are the per-chunk partials, only read when L > chunk; `chunk` is the
// caller's idea of the chunk width and must match the compiled one.
void row_topk(torch::Tensor x, int64_t k, int64_t chunk, torch::Tensor part,
              torch::Tensor pm, torch::Tensor ps, torch::Tensor vals,
              torch::Tensor idx, torch::Tensor lse) {
  CHK_CUDA(x); CHK_CONTIG(x);
  TORCH_CHECK(x.dim() == 2, "row_topk: x must be [B, L]");
  const bool is_f32 = x.scalar_type() == torch::kFloat32;
  TORCH_CHECK(is_f32 || x.scalar_type() == torch::kBFloat16,
              "row_topk: x must be bf16 or f32");
  const long B = x.size(0), L = x.size(1);
  TORCH_CHECK(chunk == row_topk_chunk(), "row_topk: chunk width ", chunk,
              " != compiled ", row_topk_chunk());
  TORCH_CHECK(k >= 1 && k <= 16, "row_topk: k must be in 1..16, got ", k);
  TORCH_CHECK(k <= L, "row_topk: k = ", k, " exceeds row length ", L);
  TORCH_CHECK(L < (1L << 31), "row_topk: L must be < 2^31");
  const long nchunk = (L + chunk - 1) / chunk;
  TORCH_CHECK(B * nchunk < (1L << 31), "row_topk: grid too large");
  CHK_CUDA(vals); CHK_CONTIG(vals); CHK_DT(vals, torch::kFloat32);
  CHK_CUDA(idx); CHK_CONTIG(idx); CHK_DT(idx, torch::kInt64);
  CHK_CUDA(lse); CHK_CONTIG(lse); CHK_DT(lse, torch::kFloat32);
  TORCH_CHECK(vals.numel() == B * k && idx.numel() == B * k &&
              lse.numel() == B, "row_topk: output shapes");
  void* pp = nullptr;
  float* pmp = nullptr;
  float* psp = nullptr;
  if (nchunk > 1) {
    CHK_CUDA(part); CHK_CONTIG(part); CHK_DT(part, torch::kInt64);
    CHK_CUDA(pm); CHK_CONTIG(pm); CHK_DT(pm, torch::kFloat32);
    CHK_CUDA(ps); CHK_CONTIG(ps); CHK_DT(ps, torch::kFloat32);
    TORCH_CHECK(part.numel() >= B * nchunk * 16 && pm.numel() >= B * nchunk
                && ps.numel() >= B * nchunk, "row_topk: partials too small");
    pp = part.data_ptr();
    pmp = pm.data_ptr<float>();
    psp = ps.data_ptr<float>();
  }
  launch_row_topk(x.data_ptr(), is_f32 ? 1 : 0, B, L, (int)k, pp, pmp, psp,
                  vals.data_ptr<float>(), idx.data_ptr<long>(),
                  lse.data_ptr<float>(), cur_stream());
}

// K20: fused similarity + top-k.  q [nq, EP] bf16, db [N, EP] bf16;
// vals f32 [nq, k], idx i64 [nq, k] in K19's order (descending score, ties
// to the smallest index row).  exclude (i64 [nq], or an empty tensor for
// none) names one index row per query that is never returned, -1 = none.
// part (i64 [nq, nsplit, 16]) is only touched when nsplit > 1.
// query_tile/row_tile are the caller's idea of the kernel's tiles.
void sim_topk(torch::Tensor q, torch::Tensor db, torch::Tensor exclude,
              int64_t k, int64_t nsplit, int64_t query_tile, int64_t row_tile,
              torch::Tensor part, torch::Tensor vals, torch::Tensor idx) {
  CHK_CUDA(q); CHK_CONTIG(q); CHK_DT(q, torch::kBFloat16);
  CHK_CUDA(db); CHK_CONTIG(db); CHK_DT(db, torch::kBFloat16);
  TORCH_CHECK(q.dim() == 2 && db.dim() == 2,
              "sim_topk: q must be [nq, EP] and db [N, EP]");
  const long nq = q.size(0), EP = q.size(1), N = db.size(0);
  TORCH_CHECK(db.size(1) == EP, "sim_topk: q has EP = ", EP, ", db has ",
              db.size(1));
  TORCH_CHECK(EP % 32 == 0 && EP >= 32 && EP <= 512,
              "sim_topk: EP must be a multiple of 32 in 32..512, got ", EP);
  TORCH_CHECK(query_tile == sim_topk_query_tile() &&
              row_tile == sim_topk_row_tile(),
              "sim_topk: tiles ", query_tile, "x", row_tile,
              " != compiled ", sim_topk_query_tile(), "x",
              sim_topk_row_tile());
  TORCH_CHECK(k >= 1 && k <= 16, "sim_topk: k must be in 1..16, got ", k);
  TORCH_CHECK(N < (1L << 31) && nq < (1L << 31),
              "sim_topk: N and nq must be < 2^31");
  TORCH_CHECK(k <= N, "sim_topk: k = ", k, " exceeds the index's ", N,
              " rows");
  const long* ex = nullptr;
  if (exclude.numel() > 0) {
    CHK_CUDA(exclude); CHK_CONTIG(exclude); CHK_DT(exclude, torch::kInt64);
    TORCH_CHECK(exclude.dim() == 1 && exclude.size(0) == nq,
                "sim_topk: exclude must be [nq]");
    TORCH_CHECK(k <= N - 1, "sim_topk: with exclude, k = ", k,
                " must be below the index's ", N, " rows");
    ex = exclude.data_ptr<long>();
  }
  const long nqt = (nq + query_tile - 1) / query_tile;
  TORCH_CHECK(nsplit >= 1 && nsplit * std::max(nqt, 1L) < (1L << 31),
              "sim_topk: nsplit = ", nsplit, " gives an invalid grid");
  CHK_CUDA(vals); CHK_CONTIG(vals); CHK_DT(vals, torch::kFloat32);
  CHK_CUDA(idx); CHK_CONTIG(idx); CHK_DT(idx, torch::kInt64);
  TORCH_CHECK(vals.numel() == nq * k && idx.numel() == nq * k,
              "sim_topk: output shapes");
  void* pp = nullptr;
  if (nsplit > 1) {
    CHK_CUDA(part); CHK_CONTIG(part); CHK_DT(part, torch::kInt64);
    TORCH_CHECK(part.numel() >= nq * nsplit * 16,
                "sim_topk: partials too small");
    pp = part.data_ptr();
  }
  launch_sim_topk(q.data_ptr(), db.data_ptr(), ex, nq, N, (int)EP, (int)k,
                  (int)nsplit, pp, vals.data_ptr<float>(),
                  idx.data_ptr<long>(), cur_stream());
}

// K24: similarity range search, checks shared by its two passes.  Returns
// the number of (query, slice, wave) segments, nq * nsplit * waves.
static long sim_range_check(const char* op, const torch::Tensor& q,
                            const torch::Tensor& db,
                            const torch::Tensor& exclude,
                            const torch::Tensor& after, double threshold,
                            int64_t nsplit, int64_t query_tile,
                            int64_t row_tile, int64_t waves,
                            const long** ex, const long** af) {
  CHK_CUDA(q); CHK_CONTIG(q); CHK_DT(q, torch::kBFloat16);
  CHK_CUDA(db); CHK_CONTIG(db); CHK_DT(db, torch::kBFloat16);
  TORCH_CHECK(q.dim() == 2 && db.dim() == 2, op,
              ": q must be [nq, EP] and db [N, EP]");
  const long nq = q.size(0), EP = q.size(1), N = db.size(0);
  TORCH_CHECK(db.size(1) == EP, op, ": q has EP = ", EP, ", db has ",
              db.size(1));
  TORCH_CHECK(EP % 32 == 0 && EP >= 32 && EP <= 512, op,
              ": EP must be a multiple of 32 in 32..512, got ", EP);
  TORCH_CHECK(query_tile == sim_topk_query_tile() &&
              row_tile == sim_topk_row_tile() && waves == sim_range_waves(),
              op, ": tiles ", query_tile, "x", row_tile, " in ", waves,
              " waves != compiled ", sim_topk_query_tile(), "x",
              sim_topk_row_tile(), " in ", sim_range_waves());
  TORCH_CHECK(N >= 1 && N < (1L << 31) && nq < (1L << 31), op,
              ": N must be in 1..2^31-1 and nq < 2^31");
  TORCH_CHECK(std::isfinite((float)threshold), op,
              ": threshold must be finite in fp32, got ", threshold);
  *ex = nullptr;
  if (exclude.numel() > 0) {
    CHK_CUDA(exclude); CHK_CONTIG(exclude); CHK_DT(exclude, torch::kInt64);
    TORCH_CHECK(exclude.dim() == 1 && exclude.size(0) == nq, op,
                ": exclude must be [nq]");
    *ex = exclude.data_ptr<long>();
  }
  *af = nullptr;
  if (after.numel() > 0) {
    CHK_CUDA(after); CHK_CONTIG(after); CHK_DT(after, torch::kInt64);
    TORCH_CHECK(after.dim() == 1 && after.size(0) == nq, op,
                ": after must be [nq]");
    *af = after.data_ptr<long>();
  }
  const long nqt = (nq + query_tile - 1) / query_tile;
  TORCH_CHECK(nsplit >= 1 && nsplit * std::max(nqt, 1L) < (1L << 31), op,
              ": nsplit = ", nsplit, " gives an invalid grid");
  return nq * nsplit * waves;
}

// K24 count pass: counts i32 [nq, nsplit, waves] = hits of every (query,
// slice, wave), in the order the fill pass writes them.
void sim_range_count(torch::Tensor q, torch::Tensor db, torch::Tensor exclude,
                     torch::Tensor after, double threshold, int64_t nsplit,
                     int64_t query_tile, int64_t row_tile, int64_t waves,
                     torch::Tensor counts) {
  const long *ex, *af;
  const long nseg = sim_range_check("sim_range_count", q, db, exclude, after,
                                    threshold, nsplit, query_tile, row_tile,
                                    waves, &ex, &af);
  CHK_CUDA(counts); CHK_CONTIG(counts); CHK_DT(counts, torch::kInt32);
  TORCH_CHECK(counts.numel() == nseg, "sim_range_count: counts must hold ",
              nseg, " entries");
  launch_sim_range_count(q.data_ptr(), db.data_ptr(), ex, af,
                         (float)threshold, q.size(0), db.size(0),
                         (int)q.size(1), (int)nsplit,
                         counts.data_ptr<int>(), cur_stream());
}

// K24 fill pass: cur i64 [nq * nsplit * waves + 1] are the exclusive
// cursors of the count pass run with the same arguments (last entry: the
// total); rows i64 [nnz] and scores f32 [nnz] receive the hits.
void sim_range_fill(torch::Tensor q, torch::Tensor db, torch::Tensor exclude,
                    torch::Tensor after, double threshold, int64_t nsplit,
                    int64_t query_tile, int64_t row_tile, int64_t waves,
                    torch::Tensor cur, torch::Tensor rows,
                    torch::Tensor scores) {
  const long *ex, *af;
  const long nseg = sim_range_check("sim_range_fill", q, db, exclude, after,
                                    threshold, nsplit, query_tile, row_tile,
                                    waves, &ex, &af);
  CHK_CUDA(cur); CHK_CONTIG(cur); CHK_DT(cur, torch::kInt64);
  CHK_CUDA(rows); CHK_CONTIG(rows); CHK_DT(rows, torch::kInt64);
  CHK_CUDA(scores); CHK_CONTIG(scores); CHK_DT(scores, torch::kFloat32);
  TORCH_CHECK(cur.numel() == nseg + 1, "sim_range_fill: cur must hold ",
              nseg + 1, " entries");
  TORCH_CHECK(rows.dim() == 1 && scores.dim() == 1 &&
              rows.numel() == scores.numel(),
              "sim_range_fill: rows and scores must be [nnz]");
  launch_sim_range_fill(q.data_ptr(), db.data_ptr(), ex, af,
                        (float)threshold, q.size(0), db.size(0),
                        (int)q.size(1), (int)nsplit, cur.data_ptr<long>(),
                        rows.numel(), rows.data_ptr<long>(),
                        scores.data_ptr<float>(), cur_stream());
}

// K23: fused head + top-k + log-sum-exp.  q [nq, EP] bf16, w [L, EP] bf16,
// bias f32 [L] (or an empty tensor for none); logits scale * q.w + bias are
// never written.  vals f32 [nq, k], idx i64 [nq, k] in K19's order, lse f32
// [nq] over all L labels.  part (i64 [nq, nsplit, 16]) and pm/ps (f32
// [nq, nsplit]) are only touched when nsplit > 1.  query_tile/row_tile are
// the caller's idea of the kernel's tiles (K20's).
void head_topk(torch::Tensor q, torch::Tensor w, torch::Tensor bias,
               double scale, int64_t k, int64_t nsplit, int64_t query_tile,
               int64_t row_tile, torch::Tensor part, torch::Tensor pm,
               torch::Tensor ps, torch::Tensor vals, torch::Tensor idx,
               torch::Tensor lse) {
  CHK_CUDA(q); CHK_CONTIG(q); CHK_DT(q, torch::kBFloat16);
  CHK_CUDA(w); CHK_CONTIG(w); CHK_DT(w, torch::kBFloat16);
  TORCH_CHECK(q.dim() == 2 && w.dim() == 2,
              "head_topk: q must be [nq, EP] and w [L, EP]");
  const long nq = q.size(0), EP = q.size(1), L = w.size(0);
  TORCH_CHECK(w.size(1) == EP, "head_topk: q has EP = ", EP, ", w has ",
              w.size(1));
  TORCH_CHECK(EP % 32 == 0 && EP >= 32 && EP <= 512,
              "head_topk: EP must be a multiple of 32 in 32..512, got ", EP);
  TORCH_CHECK(query_tile == sim_topk_query_tile() &&
              row_tile == sim_topk_row_tile(),
              "head_topk: tiles ", query_tile, "x", row_tile,
              " != compiled ", sim_topk_query_tile(), "x",
              sim_topk_row_tile());
  TORCH_CHECK(k >= 1 && k <= 16, "head_topk: k must be in 1..16, got ", k);
  TORCH_CHECK(L < (1L << 31) && nq < (1L << 31),
              "head_topk: L and nq must be < 2^31");
  TORCH_CHECK(k <= L, "head_topk: k = ", k, " exceeds the head's ", L,
              " labels");
  const float sc = (float)scale;
  TORCH_CHECK(std::isfinite(sc) && sc > 0.f,
              "head_topk: scale must be finite and > 0, got ", scale);
  const float* bp = nullptr;
  if (bias.numel() > 0) {
    CHK_CUDA(bias); CHK_CONTIG(bias); CHK_DT(bias, torch::kFloat32);
    TORCH_CHECK(bias.dim() == 1 && bias.size(0) == L,
                "head_topk: bias must be [L]");
    bp = bias.data_ptr<float>();
  }
  const long nqt = (nq + query_tile - 1) / query_tile;
  TORCH_CHECK(nsplit >= 1 && nsplit * std::max(nqt, 1L) < (1L << 31),
              "head_topk: nsplit = ", nsplit, " gives an invalid grid");
  CHK_CUDA(vals); CHK_CONTIG(vals); CHK_DT(vals, torch::kFloat32);
  CHK_CUDA(idx); CHK_CONTIG(idx); CHK_DT(idx, torch::kInt64);
  CHK_CUDA(lse); CHK_CONTIG(lse); CHK_DT(lse, torch::kFloat32);
  TORCH_CHECK(vals.numel() == nq * k && idx.numel() == nq * k &&
              lse.numel() == nq, "head_topk: output shapes");
  void* pp = nullptr;
  float* pmp = nullptr;
  float* psp = nullptr;
  if (nsplit > 1) {
    CHK_CUDA(part); CHK_CONTIG(part); CHK_DT(part, torch::kInt64);
    CHK_CUDA(pm); CHK_CONTIG(pm); CHK_DT(pm, torch::kFloat32);
    CHK_CUDA(ps); CHK_CONTIG(ps); CHK_DT(ps, torch::kFloat32);
    TORCH_CHECK(part.numel() >= nq * nsplit * 16 &&
                pm.numel() >= nq * nsplit && ps.numel() >= nq * nsplit,
                "head_topk: partials too small");
    pp = part.data_ptr();
    pmp = pm.data_ptr<float>();
    psp = ps.data_ptr<float>();
  }
  launch_head_topk(q.data_ptr(), w.data_ptr(), bp, sc, nq, L, (int)EP, (int)k,
                   (int)nsplit, pp, pmp, psp, vals.data_ptr<float>(),
                   idx.data_ptr<long>(), lse.data_ptr<float>(), cur_stream());
}

void transpose_w(torch::Tensor w, torch::Tensor wt) {
  CHK_CUDA(w); CHK_CONTIG(w); CHK_DT(w, torch::kBFloat16);
  CHK_CONTIG(wt); CHK_DT(wt, torch::kBFloat16);
  const long L = w.size(0);
  TORCH_CHECK(w.size(1) == 128 && wt.size(0) == 128 && wt.size(1) == L &&
              L % 8 == 0, "transpose_w shapes");
  launch_transpose_w(w.data_ptr(), wt.data_ptr(), L, cur_stream());
}

void slab_sum_bf16(torch::Tensor partials, torch::Tensor out) {
  CHK_CUDA(partials); CHK_CONTIG(partials);
  CHK_DT(partials, torch::kFloat32);
  CHK_CONTIG(out); CHK_DT(out, torch::kBFloat16);
  const long N = out.numel();
  const long S = partials.numel() / N;
  TORCH_CHECK(N > 0 && S * N == partials.numel(), "slab shapes");
  launch_slab_sum_bf16(partials.data_ptr<float>(), out.data_ptr(), (int)S,
                       N, cur_stream());
}

// dgamma + dbeta partial slabs in one launch (same tree as slab_sum_f32)
void slab_sum2_f32(torch::Tensor p0, torch::Tensor p1, torch::Tensor out0,
                   torch::Tensor out1) {
  CHK_CUDA(p0); CHK_CONTIG(p0); CHK_DT(p0, torch::kFloat32);
  CHK_CUDA(p1); CHK_CONTIG(p1); CHK_DT(p1, torch::kFloat32);
  CHK_CONTIG(out0); CHK_DT(out0, torch::kFloat32);
  CHK_CONTIG(out1); CHK_DT(out1, torch::kFloat32);
  const int N = (int)out0.numel();
  TORCH_CHECK(N > 0 && out1.numel() == N && p0.numel() == p1.numel() &&
              p0.numel() % N == 0, "slab_sum2_f32 shapes");
  launch_slab_sum2_f32(p0.data_ptr<float>(), p1.data_ptr<float>(),
                       out0.data_ptr<float>(), out1.data_ptr<float>(),
                       (int)(p0.numel() / N), N, cur_stream());
}

// acc_p [S, 2] -> acc [2], loss [1] = acc[0] / acc[1]
void loss_reduce(torch::Tensor acc_p, torch::Tensor acc, torch::Tensor loss) {
  CHK_CUDA(acc_p); CHK_CONTIG(acc_p); CHK_DT(acc_p, torch::kFloat32);
  CHK_CONTIG(acc); CHK_DT(acc, torch::kFloat32);
  CHK_CONTIG(loss); CHK_DT(loss, torch::kFloat32);
  TORCH_CHECK(acc.numel() == 2 && loss.numel() == 1 &&
              acc_p.numel() % 2 == 0, "loss_reduce shapes");
  launch_loss_reduce(acc_p.data_ptr<float>(), acc.data_ptr<float>(),
                     loss.data_ptr<float>(), (int)(acc_p.numel() / 2),
                     cur_stream());
}

// wgrad partial slabs [S, KP, EP] f32 -> dw [EP, KP] bf16
void wgrad_reduce(torch::Tensor partials, torch::Tensor dw) {
  CHK_CUDA(partials); CHK_CONTIG(partials);
  CHK_DT(partials, torch::kFloat32);
  CHK_CUDA(dw); CHK_CONTIG(dw); CHK_DT(dw, torch::kBFloat16);
  TORCH_CHECK(partials.dim() == 3 && dw.dim() == 2, "wgrad_reduce dims");
  const long S = partials.size(0), KP = partials.size(1),
             EP = partials.size(2);
  TORCH_CHECK(S > 0 && S < (1 << 20) && KP % 4 == 0 && EP % 32 == 0 &&
              KP > 0 && EP > 0 && dw.size(0) == EP && dw.size(1) == KP,
              "wgrad_reduce shapes");
  launch_wgrad_reduce(partials.data_ptr<float>(), dw.data_ptr(), (int)S,
                      (int)KP, (int)EP, cur_stream());
}

void slab_sum_f32(torch::Tensor p, torch::Tensor out) {
  CHK_CUDA(p); CHK_CONTIG(p); CHK_DT(p, torch::kFloat32);
  CHK_CONTIG(out); CHK_DT(out, torch::kFloat32);
  const int N = (int)out.numel();
  const int S = (int)(p.numel() / N);
  TORCH_CHECK((long)S * N == p.numel(), "slab_sum_f32 shapes");
  launch_slab_sum_f32(p.data_ptr<float>(), out.data_ptr<float>(), S, N,
                      cur_stream());
}

// dx = dz @ w2^T with w2 = [KP, EP=128] (the re-transposed combiner weight)
void dgrad2(torch::Tensor dz, torch::Tensor w2, torch::Tensor dx) {
  CHK_CUDA(dz); CHK_CONTIG(dz); CHK_DT(dz, torch::kBFloat16);
  CHK_CONTIG(w2); CHK_DT(w2, torch::kBFloat16);
  CHK_CONTIG(dx); CHK_DT(dx, torch::kBFloat16);
  const long M = dz.size(0), KP = w2.size(0);
  TORCH_CHECK(dz.size(1) == 128 && w2.size(1) == 128, "dgrad2 EP");
  TORCH_CHECK(dx.size(0) == M && dx.size(1) == KP && KP % 8 == 0,
              "dgrad2 shapes");
  launch_dgrad2(dz.data_ptr(), w2.data_ptr(), dx.data_ptr(), M, KP,
                cur_stream());
}

void colsum_bf16(torch::Tensor x, torch::Tensor out) {
  CHK_CUDA(x); CHK_CONTIG(x); CHK_DT(x, torch::kBFloat16);
  CHK_DT(out, torch::kFloat32);
  launch_colsum_bf16(x.data_ptr(), out.data_ptr<float>(), x.size(0),
                     x.size(1), cur_stream());
}

void wgrad(torch::Tensor x, torch::Tensor dz, torch::Tensor partials) {
  CHK_CUDA(x); CHK_CONTIG(x); CHK_DT(x, torch::kBFloat16);
  CHK_CONTIG(dz); CHK_DT(dz, torch::kBFloat16);
  CHK_DT(partials, torch::kFloat32); CHK_CONTIG(partials);
  const long M = x.size(0);
  const int KP = x.size(1), EP = dz.size(1);
  TORCH_CHECK(partials.size(1) == KP && partials.size(2) == EP, "partials");
  launch_wgrad(x.data_ptr(), dz.data_ptr(), partials.data_ptr<float>(), M,
               KP, EP, partials.size(0), cur_stream());
}

// Pipelined split-K wgrad (bit-identical slabs): depth = 32-row K-steps
// per stage, 0 = C2V_WGRAD_DEPTH or the shipped default.
void wgrad_pipe(torch::Tensor x, torch::Tensor dz, torch::Tensor partials,
                long depth) {
  CHK_CUDA(x); CHK_CONTIG(x); CHK_DT(x, torch::kBFloat16);
  CHK_CONTIG(dz); CHK_DT(dz, torch::kBFloat16);
  CHK_DT(partials, torch::kFloat32); CHK_CONTIG(partials);
  const long M = x.size(0);
  const int KP = x.size(1), EP = dz.size(1);
  TORCH_CHECK(dz.size(0) == M, "wgrad_pipe: x and dz row counts differ");
  TORCH_CHECK(partials.dim() == 3 && partials.size(1) == KP &&
                  partials.size(2) == EP, "partials");
  TORCH_CHECK(launch_wgrad_pipe(x.data_ptr(), dz.data_ptr(),
                                partials.data_ptr<float>(), M, KP, EP,
                                partials.size(0), (int)depth, cur_stream()),
              "wgrad_pipe: no instantiation for KP=", KP, " EP=", EP,
              " depth=", depth);
}

// bc_pow: float64 [2] DEVICE tensor = (beta1^t, beta2^t); advance it with
// adam_tick once per optimizer step (device-resident so hipGraph replays
// keep the bias correction advancing).
void adam_tick(torch::Tensor bc_pow, double b1, double b2) {
  CHK_CUDA(bc_pow); CHK_DT(bc_pow, torch::kFloat64);
  TORCH_CHECK(bc_pow.numel() == 2, "bc_pow must be [2]");
  launch_adam_tick((double*)bc_pow.data_ptr(), (float)b1, (float)b2,
                   cur_stream());
}

void adam_step_bf16(torch::Tensor p, torch::Tensor g, torch::Tensor master,
                    torch::Tensor m, torch::Tensor v, torch::Tensor bc_pow,
                    double lr, double b1, double b2, double eps, double wd) {
  CHK_CUDA(p); CHK_DT(p, torch::kBFloat16); CHK_DT(g, torch::kBFloat16);
  CHK_DT(master, torch::kFloat32); CHK_DT(bc_pow, torch::kFloat64);
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == master.numel(), "sizes");
  launch_adam_bf16(p.data_ptr(), g.data_ptr(), master.data_ptr<float>(),
                   m.data_ptr<float>(), v.data_ptr<float>(), p.numel(),
                   (const double*)bc_pow.data_ptr(), (float)lr, (float)b1,
                   (float)b2, (float)eps, (float)wd, cur_stream());
}

// Shared shape checks of the deferred table-gradient record: N sorted
// entries (N == M, or 2M with two column offsets) over gout [M, KP].
static void check_table_record(const torch::Tensor& perm,
                               const torch::Tensor& counts,
                               const torch::Tensor& gout, long T, int S,
                               int64_t M, int64_t KP, int64_t off0,
                               int64_t off1) {
  CHK_CUDA(gout); CHK_CONTIG(gout); CHK_DT(gout, torch::kBFloat16);
  CHK_CONTIG(perm); CHK_DT(perm, torch::kInt64);
  CHK_CONTIG(counts); CHK_DT(counts, torch::kInt32);
  const long N = perm.numel();
  TORCH_CHECK(M > 0 && (N == M || N == 2 * M), "record: N must be M or 2M");
  TORCH_CHECK(gout.numel() >= M * KP, "record: gout smaller than [M, KP]");
  TORCH_CHECK(off0 >= 0 && off1 >= 0 && off0 + S <= KP && off1 + S <= KP,
              "record: column window outside gout");
  TORCH_CHECK(counts.numel() >= T + 1, "record: counts shorter than T + 1");
}

// Heavy-row pre-pass of adam_table_bf16: rows with counts > thr are
// reduced into the persistent fp32 scratch `dtable` [T, S].
void embed_scatter_heavy(torch::Tensor sorted_idx, torch::Tensor perm,
                         torch::Tensor counts, torch::Tensor gout,
                         torch::Tensor dtable, int64_t M, int64_t KP,
                         int64_t off0, int64_t off1, int64_t thr) {
  CHK_CUDA(sorted_idx); CHK_CONTIG(sorted_idx);
  CHK_DT(sorted_idx, torch::kInt32);
  CHK_DT(dtable, torch::kFloat32); CHK_CONTIG(dtable);
  TORCH_CHECK(dtable.dim() == 2, "dtable must be [T, S]");
  const long T = dtable.size(0);
  const int S = dtable.size(1);
  check_table_record(perm, counts, gout, T, S, M, KP, off0, off1);
  TORCH_CHECK(sorted_idx.numel() == perm.numel(), "sorted_idx/perm sizes");
  TORCH_CHECK(S % 2 == 0 && S <= 512 && KP % 2 == 0 && off0 % 2 == 0 &&
                  off1 % 2 == 0, "embed_scatter_heavy: S/KP/offset alignment");
  TORCH_CHECK(thr >= 32, "embed_scatter_heavy: thr must be >= 32");
  launch_embed_scatter_heavy(sorted_idx.data_ptr<int>(),
                             perm.data_ptr<long>(), counts.data_ptr<int>(),
                             gout.data_ptr(), dtable.data_ptr<float>(),
                             perm.numel(), M, (int)KP, S, (int)off0,
                             (int)off1, (int)thr, cur_stream());
}

// Row-gathering table Adam: p bf16 [T, S] updated from the deferred record
// (gout, perm, counts, cursor) instead of a dense gradient; consumes
// counts (left all-zero) and the heavy rows of `scratch` (re-zeroed).
static void adam_table_bf16_impl(
    torch::Tensor p, torch::Tensor gout, torch::Tensor perm,
    torch::Tensor counts, torch::Tensor cursor, torch::Tensor scratch,
    torch::Tensor master, torch::Tensor m, torch::Tensor v,
    torch::Tensor bc_pow, int64_t M, int64_t KP, int64_t off0, int64_t off1,
    int64_t thr, double lr, double b1, double b2, double eps, double wd,
    bool clear_counts) {
  CHK_CUDA(p); CHK_CONTIG(p); CHK_DT(p, torch::kBFloat16);
  TORCH_CHECK(p.dim() == 2, "p must be [T, S]");
  const long T = p.size(0);
  const int S = p.size(1);
  check_table_record(perm, counts, gout, T, S, M, KP, off0, off1);
  CHK_CONTIG(cursor); CHK_DT(cursor, torch::kInt32);
  TORCH_CHECK(cursor.numel() >= T, "cursor shorter than T");
  CHK_DT(scratch, torch::kFloat32); CHK_CONTIG(scratch);
  CHK_DT(master, torch::kFloat32); CHK_CONTIG(master);
  CHK_DT(m, torch::kFloat32); CHK_CONTIG(m);
  CHK_DT(v, torch::kFloat32); CHK_CONTIG(v);
  CHK_DT(bc_pow, torch::kFloat64);
  const long n = T * S;
  TORCH_CHECK(scratch.numel() == n && master.numel() == n &&
                  m.numel() == n && v.numel() == n, "state sizes");
  TORCH_CHECK(S % 4 == 0 && KP % 4 == 0 && off0 % 4 == 0 && off1 % 4 == 0,
              "adam_table_bf16: S, KP and offsets must be multiples of 4");
  TORCH_CHECK(n / 4 < (1L << 32), "adam_table_bf16: table too large");
  TORCH_CHECK(thr >= 32, "adam_table_bf16: thr must be >= 32");
  launch_adam_table_bf16(
      p.data_ptr(), gout.data_ptr(), perm.data_ptr<long>(),
      counts.data_ptr<int>(), cursor.data_ptr<int>(),
      scratch.data_ptr<float>(), master.data_ptr<float>(),
      m.data_ptr<float>(), v.data_ptr<float>(), T, S, counts.numel(),
      perm.numel(), M, (int)KP, (int)off0, (int)off1, (int)thr,
      (const double*)bc_pow.data_ptr(), (float)lr, (float)b1, (float)b2,
      (float)eps, (float)wd, clear_counts ? 1 : 0, cur_stream());
}

void adam_table_bf16(torch::Tensor p, torch::Tensor gout, torch::Tensor perm,
                     torch::Tensor counts, torch::Tensor cursor,
                     torch::Tensor scratch, torch::Tensor master,
                     torch::Tensor m, torch::Tensor v, torch::Tensor bc_pow,
                     int64_t M, int64_t KP, int64_t off0, int64_t off1,
                     int64_t thr, double lr, double b1, double b2, double eps,
                     double wd) {
  adam_table_bf16_impl(p, gout, perm, counts, cursor, scratch, master, m, v,
                       bc_pow, M, KP, off0, off1, thr, lr, b1, b2, eps, wd,
                       true);
}

// adam_table_bf16 that leaves the histogram in place: the caller clears both
// tables' histograms with clear_i32_pair once both Adam kernels are queued.
void adam_table_bf16_keep_counts(
    torch::Tensor p, torch::Tensor gout, torch::Tensor perm,
    torch::Tensor counts, torch::Tensor cursor, torch::Tensor scratch,
    torch::Tensor master, torch::Tensor m, torch::Tensor v,
    torch::Tensor bc_pow, int64_t M, int64_t KP, int64_t off0, int64_t off1,
    int64_t thr, double lr, double b1, double b2, double eps, double wd) {
  adam_table_bf16_impl(p, gout, perm, counts, cursor, scratch, master, m, v,
                       bc_pow, M, KP, off0, off1, thr, lr, b1, b2, eps, wd,
                       false);
}

// ---------------------------------------------------------------------------
// Both embedding tables' counting sort in one chain (index_group.hip),
// optionally on a side stream so it overlaps the forward and backward
// kernels between the batch's arrival and the optimizer step.

namespace {
struct GroupStream {
  hipStream_t side = nullptr;
  hipEvent_t ready = nullptr;  // current stream -> side stream
  hipEvent_t done = nullptr;   // side stream -> adopting/retiring stream
  torch::Tensor tmp;           // scratch a side-stream chain allocated itself
};
std::map<int, GroupStream>& group_streams() {
  static std::map<int, GroupStream> m;
  return m;
}
GroupStream& group_stream_for(int device) {
  auto& m = group_streams();
  auto it = m.find(device);
  if (it == m.end()) {
    // one stream from torch's pool for the life of the process
    GroupStream g;
    g.side = c10::hip::getStreamFromPool(false, device).stream();
    C10_HIP_CHECK(hipEventCreateWithFlags(&g.ready, hipEventDisableTiming));
    C10_HIP_CHECK(hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
    it = m.emplace(device, g).first;
  }
  return it->second;
}
void check_i32(const torch::Tensor& t, long n, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == torch::kInt32 && t.numel() >= n,
              "group_tables: ", what, " must be contiguous int32 on the GPU "
              "with at least ", n, " elements");
}
}  // namespace

// Returns true if the chain went to the side stream: the consumer must then
// call group_tables_wait() on its stream before touching any output.  While
// the current stream is capturing, or with side_stream false, the chain is
// launched on the current stream.  ``tmp`` is the two-level sort's scratch
// (group_tables_tmp_len ints); a caller on the hot path passes a persistent
// buffer, without it one is allocated here.
bool group_tables(torch::Tensor starts, torch::Tensor paths,
                  torch::Tensor ends, torch::Tensor counts_t,
                  torch::Tensor counts_p, torch::Tensor cursor_t,
                  torch::Tensor cursor_p, torch::Tensor partial,
                  torch::Tensor sorted_t, torch::Tensor perm_t,
                  torch::Tensor sorted_p, torch::Tensor perm_p,
                  int64_t rows_t, int64_t rows_p, bool side_stream,
                  c10::optional<torch::Tensor> tmp) {
  const long M = starts.numel();
  TORCH_CHECK(M > 0 && 2 * M < (1L << 31), "group_tables: bad entry count");
  TORCH_CHECK(rows_t > 0 && rows_p > 0 && rows_t < (1L << 31) &&
                  rows_p < (1L << 31), "group_tables: bad histogram length");
  check_i32(starts, M, "starts"); check_i32(paths, M, "paths");
  check_i32(ends, M, "ends");
  TORCH_CHECK(paths.numel() == M && ends.numel() == M,
              "group_tables: starts/paths/ends sizes differ");
  check_i32(counts_t, rows_t, "counts_t"); check_i32(counts_p, rows_p, "counts_p");
  check_i32(cursor_t, rows_t, "cursor_t"); check_i32(cursor_p, rows_p, "cursor_p");
  check_i32(partial, group_tables_partials(rows_t, rows_p), "partial");
  check_i32(sorted_t, 2 * M, "sorted_t"); check_i32(sorted_p, M, "sorted_p");
  CHK_CUDA(perm_t); CHK_CONTIG(perm_t); CHK_DT(perm_t, torch::kInt64);
  CHK_CUDA(perm_p); CHK_CONTIG(perm_p); CHK_DT(perm_p, torch::kInt64);
  TORCH_CHECK(perm_t.numel() >= 2 * M && perm_p.numel() >= M,
              "group_tables: perm buffers too short");

  auto cur = at::hip::getCurrentHIPStream();
  hipStream_t launch_on = cur.stream();
  bool on_side = false;
  GroupStream* gs = nullptr;
  if (side_stream) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    C10_HIP_CHECK(hipStreamIsCapturing(cur.stream(), &cap));
    if (cap == hipStreamCaptureStatusNone) {
      gs = &group_stream_for(cur.device_index());
      // the side stream inherits everything the current stream is ordered
      // after: the previous step's consumers of these buffers and whatever
      // produced the indices
      C10_HIP_CHECK(hipEventRecord(gs->ready, cur.stream()));
      C10_HIP_CHECK(hipStreamWaitEvent(gs->side, gs->ready, 0));
      launch_on = gs->side;
      on_side = true;
    }
  }
  const long tmp_len = group_tables_tmp(M, rows_t, rows_p);
  torch::Tensor scratch;
  if (tmp.has_value()) {
    scratch = *tmp;
    check_i32(scratch, tmp_len, "tmp");
    TORCH_CHECK((uintptr_t)scratch.data_ptr() % 8 == 0,
                "group_tables: tmp must be 8-byte aligned");
  } else {
    scratch = torch::empty({tmp_len}, starts.options());
    if (on_side) {
      // the allocator knows the block on the current stream only: keep it
      // until the next chain, and free the previous one no earlier than
      // the current stream is ordered after the chain that used it
      if (gs->tmp.defined())
        C10_HIP_CHECK(hipStreamWaitEvent(cur.stream(), gs->done, 0));
      gs->tmp = scratch;
    }
  }
  launch_group_tables(
      starts.data_ptr<int>(), paths.data_ptr<int>(), ends.data_ptr<int>(), M,
      (int)rows_t, (int)rows_p, counts_t.data_ptr<int>(),
      counts_p.data_ptr<int>(), cursor_t.data_ptr<int>(),
      cursor_p.data_ptr<int>(), partial.data_ptr<int>(),
      sorted_t.data_ptr<int>(), perm_t.data_ptr<long>(),
      sorted_p.data_ptr<int>(), perm_p.data_ptr<long>(),
      scratch.data_ptr<int>(), launch_on);
  if (on_side) C10_HIP_CHECK(hipEventRecord(gs->done, gs->side));
  return on_side;
}

// Order the current stream after the latest side-stream group_tables chain.
void group_tables_wait() {
  auto cur = at::hip::getCurrentHIPStream();
  auto& m = group_streams();
  auto it = m.find(cur.device_index());
  TORCH_CHECK(it != m.end(), "group_tables_wait: no side-stream grouping");
  C10_HIP_CHECK(hipStreamWaitEvent(cur.stream(), it->second.done, 0));
}

int64_t group_tables_partials_len(int64_t rows_t, int64_t rows_p) {
  return group_tables_partials(rows_t, rows_p);
}

int64_t group_tables_tmp_len(int64_t M, int64_t rows_t, int64_t rows_p) {
  return group_tables_tmp(M, rows_t, rows_p);
}

// embed_scatter_heavy for both tables of one group_tables record pair:
// gout [M, KP] = [start (S_t) | path (S_p) | end (S_t) | pad].
void embed_scatter_heavy_pair(torch::Tensor sorted_t, torch::Tensor perm_t,
                              torch::Tensor counts_t, torch::Tensor dtable_t,
                              torch::Tensor sorted_p, torch::Tensor perm_p,
                              torch::Tensor counts_p, torch::Tensor dtable_p,
                              torch::Tensor gout, int64_t M, int64_t KP,
                              int64_t thr) {
  CHK_DT(dtable_t, torch::kFloat32); CHK_CONTIG(dtable_t);
  CHK_DT(dtable_p, torch::kFloat32); CHK_CONTIG(dtable_p);
  TORCH_CHECK(dtable_t.dim() == 2 && dtable_p.dim() == 2,
              "dtable must be [T, S]");
  const int St = dtable_t.size(1), Sp = dtable_p.size(1);
  check_table_record(perm_t.narrow(0, 0, 2 * M), counts_t, gout,
                     dtable_t.size(0), St, M, KP, 0, St + Sp);
  check_table_record(perm_p.narrow(0, 0, M), counts_p, gout,
                     dtable_p.size(0), Sp, M, KP, St, St);
  check_i32(sorted_t, 2 * M, "sorted_t"); check_i32(sorted_p, M, "sorted_p");
  TORCH_CHECK(St % 2 == 0 && Sp % 2 == 0 && St <= 512 && Sp <= 512 &&
                  KP % 2 == 0, "embed_scatter_heavy_pair: S/KP alignment");
  TORCH_CHECK(thr >= 32, "embed_scatter_heavy_pair: thr must be >= 32");
  launch_embed_scatter_heavy_pair(
      sorted_t.data_ptr<int>(), perm_t.data_ptr<long>(),
      counts_t.data_ptr<int>(), dtable_t.data_ptr<float>(), St,
      sorted_p.data_ptr<int>(), perm_p.data_ptr<long>(),
      counts_p.data_ptr<int>(), dtable_p.data_ptr<float>(), Sp,
      gout.data_ptr(), M, (int)KP, (int)thr, cur_stream());
}

void clear_i32_pair(torch::Tensor a, torch::Tensor b) {
  check_i32(a, 0, "a"); check_i32(b, 0, "b");
  launch_clear_i32_pair(a.data_ptr<int>(), a.numel(), b.data_ptr<int>(),
                        b.numel(), cur_stream());
}

void adam_step_f32(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                   torch::Tensor v, torch::Tensor bc_pow, double lr,
                   double b1, double b2, double eps, double wd) {
  CHK_CUDA(p); CHK_DT(p, torch::kFloat32); CHK_DT(g, torch::kFloat32);
  CHK_DT(bc_pow, torch::kFloat64);
  launch_adam_f32(p.data_ptr<float>(), g.data_ptr<float>(),
                  m.data_ptr<float>(), v.data_ptr<float>(), p.numel(),
                  (const double*)bc_pow.data_ptr(), (float)lr, (float)b1,
                  (float)b2, (float)eps, (float)wd, cur_stream());
}

// One launch for up to 8 small fp32 params (grads must be fp32 and
// contiguous); element-order within each tensor identical to the
// per-tensor kernel, so the update is bitwise-equal to 4 separate calls.
void adam_step_f32_multi(std::vector<torch::Tensor> ps,
                         std::vector<torch::Tensor> gs,
                         std::vector<torch::Tensor> ms,
                         std::vector<torch::Tensor> vs,
                         torch::Tensor bc_pow, double lr, double b1,
                         double b2, double eps, double wd) {
  const int n = (int)ps.size();
  TORCH_CHECK(n >= 1 && n <= 8, "adam_step_f32_multi: 1..8 tensors");
  TORCH_CHECK((int)gs.size() == n && (int)ms.size() == n &&
              (int)vs.size() == n, "adam_step_f32_multi: list sizes");
  CHK_DT(bc_pow, torch::kFloat64);
  float* pp[8]; const float* gp[8]; float* mp[8]; float* vp[8]; long ns[8];
  for (int t = 0; t < n; ++t) {
    CHK_CUDA(ps[t]); CHK_CONTIG(ps[t]); CHK_DT(ps[t], torch::kFloat32);
    CHK_CONTIG(gs[t]); CHK_DT(gs[t], torch::kFloat32);
    TORCH_CHECK(ps[t].numel() == gs[t].numel() &&
                ps[t].numel() == ms[t].numel() &&
                ps[t].numel() == vs[t].numel(), "sizes");
    pp[t] = ps[t].data_ptr<float>();
    gp[t] = gs[t].data_ptr<float>();
    mp[t] = ms[t].data_ptr<float>();
    vp[t] = vs[t].data_ptr<float>();
    ns[t] = ps[t].numel();
  }
  launch_adam_f32_multi(pp, gp, mp, vp, ns, n,
                        (const double*)bc_pow.data_ptr(), (float)lr,
                        (float)b1, (float)b2, (float)eps, (float)wd,
                        cur_stream());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("gather_concat_fwd", &gather_concat_fwd);
  m.def("gather_concat_bwd", &gather_concat_bwd);
  m.def("embed_scatter_sorted", &embed_scatter_sorted);
  m.def("group_by_index", &group_by_index);
  m.def("cast_clear_rows", &cast_clear_rows);
  m.def("combiner_fwd", &combiner_fwd);
  m.def("gather_combiner_fwd", &gather_combiner_fwd);
  m.def("wgrad_gather", &wgrad_gather);
  m.def("combiner_bwd", &combiner_bwd);
  m.def("attention_fwd", &attention_fwd);
  m.def("attention_bwd", &attention_bwd);
  m.def("attention_fwd_cvb", &attention_fwd_cvb);
  m.def("attention_bwd_compact", &attention_bwd_compact);
  m.def("combiner_fwd_scores", &combiner_fwd_scores);
  m.def("attention_stream_ok", &attention_stream_ok);
  m.def("attention_fwd_scores", &attention_fwd_scores);
  m.def("attention_bwd_compact_reg", &attention_bwd_compact_reg);
  m.def("attention_pool_packed", &attention_pool_packed);
  m.def("combiner_bwd_recompute", &combiner_bwd_recompute);
  m.def("attention_packed_bwd_compact", &attention_packed_bwd_compact);
  m.def("attention_packed_bwd", &attention_packed_bwd);
  m.def("combiner_bwd_recompute_packed", &combiner_bwd_recompute_packed);
  m.def("slab_sum2_f32", &slab_sum2_f32);
  m.def("loss_reduce", &loss_reduce);
  m.def("wgrad_reduce", &wgrad_reduce);
  m.def("logsoftmax_nll_fwd", &logsoftmax_nll_fwd);
  m.def("logsoftmax_nll_bwd", &logsoftmax_nll_bwd);
  m.def("wgrad", &wgrad);
  m.def("wgrad_pipe", &wgrad_pipe);
  m.def("colsum_bf16", &colsum_bf16);
  m.def("head_fwd", &head_fwd);
  m.def("head_fwd_img", &head_fwd_img);
  m.def("swizzle_a", &swizzle_a);
  m.def("logsoftmax_nll_finalize", &logsoftmax_nll_finalize);
  m.def("lsm_partial", &lsm_partial);
  m.def("head_wgrad", &head_wgrad);
  m.def("head_dgrad", &head_dgrad);
  m.def("exclusive_scan", &exclusive_scan);
  m.def("cub_exclusive_scan", &cub_exclusive_scan);
  m.def("cub_scan_temp_bytes", &cub_scan_temp_bytes);
  m.def("head_bwd_prep", &head_bwd_prep);
  m.def("swizzle_cv", &swizzle_cv);
  m.def("row_max_argmax", &row_max_argmax);
  m.def("row_topk", &row_topk);
  m.def("sim_topk", &sim_topk);
  m.def("sim_range_count", &sim_range_count);
  m.def("sim_range_fill", &sim_range_fill);
  m.def("head_topk", &head_topk);
  m.def("inv_rownorm", &inv_rownorm);
  m.def("rowscale", &rowscale);
  m.def("angular_fwd", &angular_fwd);
  m.def("angular_dcos", &angular_dcos);
  m.def("norm_project", &norm_project);
  m.def("head_bwd_dw", &head_bwd_dw);
  m.def("head_bwd_dcv", &head_bwd_dcv);
  m.def("head_bwd_dcv_rc", &head_bwd_dcv_rc);
  m.def("head_bwd_dw_pipe", &head_bwd_dw_pipe);
  m.def("head_bwd_dcv_pipe", &head_bwd_dcv_pipe);
  m.def("transpose_w", &transpose_w);
  m.def("dgrad2", &dgrad2);
  m.def("slab_sum_bf16", &slab_sum_bf16);
  m.def("slab_sum_f32", &slab_sum_f32);
  m.def("dgrad", &dgrad);
  m.def("adam_tick", &adam_tick);
  m.def("adam_step_bf16", &adam_step_bf16);
  m.def("adam_step_f32", &adam_step_f32);
  m.def("embed_scatter_heavy", &embed_scatter_heavy);
  m.def("adam_table_bf16", &adam_table_bf16);
  m.def("adam_step_f32_multi", &adam_step_f32_multi);
  m.def("adam_table_bf16_keep_counts", &adam_table_bf16_keep_counts);
  m.def("group_tables", &group_tables, py::arg("starts"), py::arg("paths"),
        py::arg("ends"), py::arg("counts_t"), py::arg("counts_p"),
        py::arg("cursor_t"), py::arg("cursor_p"), py::arg("partial"),
        py::arg("sorted_t"), py::arg("perm_t"), py::arg("sorted_p"),
        py::arg("perm_p"), py::arg("rows_t"), py::arg("rows_p"),
        py::arg("side_stream"), py::arg("tmp") = py::none());
  m.def("group_tables_tmp_len", &group_tables_tmp_len);
  m.def("group_tables_wait", &group_tables_wait);
  m.def("group_tables_partials_len", &group_tables_partials_len);
  m.def("embed_scatter_heavy_pair", &embed_scatter_heavy_pair);
  m.def("clear_i32_pair", &clear_i32_pair);
}
