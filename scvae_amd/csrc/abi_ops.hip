// The stand-alone entries of the C ABI (include/scvae_hip.h): single kernels and helpers on the
// caller's stream that touch no plan -- the optimiser update, the GEMMs, the likelihood and latent
// kernels, minibatch fetch, batch-norm pieces, noise.  The plan's entries are in plan.hip.
#include "plan.hpp"   // (count_tiles_of; no entry here takes a scvae_plan)

// every extent and leading dimension of the GEMM entries is narrowed to int: refuse what does not
// fit before the cast
static inline bool fits_int(int64_t v) { return v >= 0 && v <= INT32_MAX; }

extern "C" {

int scvae_adam_clip_step(float* theta, float* grad, float* m, float* v, int64_t n,
                         float grad_scale, float lr_t, float beta1, float beta2, float epsilon,
                         void* stream) {
  SCVAE_ARG(n >= 0);
  return scvae::adam_clip_step((hipStream_t)stream, theta, grad, m, v, (size_t)n, grad_scale, lr_t,
                               beta1, beta2, epsilon);
}

int scvae_gemm(int32_t ta, int32_t tb, const float* A, const float* B, const float* bias, float* C,
               int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t relu,
               int32_t accumulate, void* workspace, int64_t workspace_bytes, void* stream) {
  SCVAE_ARG(fits_int(M) && fits_int(N) && fits_int(K) && fits_int(lda) && fits_int(ldb) &&
            fits_int(ldc) && workspace_bytes >= 0);
  SCVAE_ARG(lda >= (ta ? M : K) && ldb >= (tb ? K : N) && ldc >= N);
  return scvae::gemm((hipStream_t)stream, ta != 0, tb != 0, A, B, bias, C, (int)M, (int)N, (int)K,
                     (int)lda, (int)ldb, (int)ldc, relu ? scvae::ACT_RELU : scvae::ACT_NONE,
                     accumulate != 0, (float*)workspace, (size_t)workspace_bytes);
}
int scvae_count_gemm(int32_t mode, const float* x, int64_t ldx, int64_t rows, int64_t cols,
                     const float* other, int64_t ld_other, int64_t N, const float* bias,
                     int32_t relu, float* C, int64_t ldc, void* workspace, int64_t workspace_bytes,
                     void* stream) {
  SCVAE_ARG(workspace_bytes >= 0);
  SCVAE_ARG(fits_int(ldx) && fits_int(rows) && fits_int(cols) && fits_int(ld_other) &&
            fits_int(N) && fits_int(ldc));
  SCVAE_ARG(ldx >= cols && ld_other >= N && ldc >= N);
  return scvae::count_gemm((hipStream_t)stream, mode, x, (int)ldx, (int)rows, (int)cols, other,
                           (int)ld_other, (int)N, bias, relu ? scvae::ACT_RELU : scvae::ACT_NONE,
                           C, (int)ldc, workspace, (size_t)workspace_bytes);
}
int64_t scvae_count_gemm_workspace_bytes(int32_t mode, int64_t rows, int64_t cols, int64_t N) {
  if (!scvae::count_gemm_supported((int)N)) return -1;
  return (int64_t)scvae::count_gemm_workspace_bytes(mode, (int)rows, (int)cols, (int)N);
}
int scvae_check_counts(const float* values, int64_t n, int32_t* bad, void* stream) {
  SCVAE_ARG(n >= 0);
  return scvae::check_counts((hipStream_t)stream, values, (size_t)n, bad);
}
int scvae_gemm_route(int32_t ta, int32_t tb, int64_t M, int64_t N, int64_t K, int64_t ldb,
                     int64_t workspace_bytes, int32_t out[4]) {
  SCVAE_ARG(out && fits_int(M) && fits_int(N) && fits_int(K) && fits_int(ldb) &&
            workspace_bytes >= 0);
  const scvae::GemmRoute r = scvae::gemm_route(ta != 0, tb != 0, (int)M, (int)N, (int)K, (int)ldb,
                                               (size_t)workspace_bytes);
  out[0] = r.kernel; out[1] = r.splits; out[2] = r.k_chunk; out[3] = r.reducer;
  return 0;
}
int scvae_count_gemm_route(int32_t mode, int64_t rows, int64_t cols, int64_t N, int32_t x_is_u16,
                           int32_t indexed, int32_t out[8]) {
  SCVAE_ARG(out && (mode == 0 || mode == 1) && fits_int(rows) && fits_int(cols) && fits_int(N));
  SCVAE_ARG(scvae::count_gemm_supported((int)N) && (!indexed || x_is_u16));
  const scvae::CountGemmRoute r = scvae::count_gemm_route(mode, (int)rows, (int)cols, (int)N,
                                                          x_is_u16 != 0, indexed != 0);
  out[0] = r.k_main; out[1] = r.splits; out[2] = r.k_chunk; out[3] = r.direct;
  out[4] = r.tiles; out[5] = r.pair; out[6] = r.waves; out[7] = 0;
  return 0;
}
int64_t scvae_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  return (int64_t)scvae::gemm_workspace_bytes((int)M, (int)N, (int)K);
}

int scvae_loglik_fwd(int32_t kind, const float* t, const float* const* pre, const float* row_const,
                     float* ll, int64_t rows, int64_t cells, int64_t F, void* stream) {
  SCVAE_ARG(pre && ((kind >= 0 && kind <= 3) || kind == scvae::LK_BERNOULLI));
  scvae::HeadPtrs hp = {{nullptr, nullptr, nullptr}};
  for (int j = 0; j < scvae::likelihood_heads(kind); ++j) hp.p[j] = const_cast<float*>(pre[j]);
  return scvae::loglik_fwd((hipStream_t)stream, kind, t, (int)F, hp, (int)F, row_const, ll,
                           (int)rows, (int)cells, (int)F);
}
int scvae_loglik_bwd(int32_t kind, const float* t, float* const* pre, const float* gw,
                     const float* row_const, float* ll, int64_t rows, int64_t cells, int64_t F,
                     void* stream) {
  SCVAE_ARG(pre && ((kind >= 0 && kind <= 3) || kind == scvae::LK_BERNOULLI));
  scvae::HeadPtrs hp = {{nullptr, nullptr, nullptr}};
  for (int j = 0; j < scvae::likelihood_heads(kind); ++j) hp.p[j] = pre[j];
  return scvae::loglik_bwd((hipStream_t)stream, kind, t, (int)F, hp, (int)F, gw, row_const, ll,
                           (int)rows, (int)cells, (int)F);
}
int64_t scvae_decoder_fused_workspace_bytes(int64_t rows, int64_t H, int64_t F) {
  if (!scvae::decoder_fused_train_supported(1, (int)H, 1)) return -1;
  return (int64_t)(scvae::decoder_fused_workspace_floats((int)rows, (int)H, (int)F, true) *
                   sizeof(float));
}
int32_t scvae_decoder_fused_variant(int32_t kind, int64_t H) {
  if (kind < 0 || (kind > 3 && kind != scvae::LK_BERNOULLI) ||
      !scvae::decoder_fused_supported((int)H))
    return 0;
  return scvae::decoder_fused_variant(scvae::likelihood_heads(kind), (int)H);
}
int32_t scvae_default_head_arith(void) { return scvae::default_head_arith(); }
int32_t scvae_default_dd_atomics(void) { return scvae::default_dd_atomics(); }
int scvae_decoder_train_kernel_name(int32_t kind, int64_t H, int64_t rows, int32_t arith,
                                    int32_t u16, char* out, int64_t n) {
  SCVAE_ARG(out && n > 0);
  out[0] = 0;
  const int which = scvae_decoder_train_kernel(kind, H, arith);
  SCVAE_ARG(which > 0);
  const int P = scvae::likelihood_heads(kind);
  if (which == 3) {
    scvae::decoder_fused3_train_kernel_name(kind, (int)H, (int)rows, u16 != 0, out, (size_t)n,
                                            arith == 2 ? 6 : 9);
  } else if (which == 2) {
    snprintf(out, (size_t)n, "decoder_head2_kernel<%d, true, %s>", kind,
             (P <= 2 && H > 96 && H <= 111) ? "true|false" : "false");
  } else {
    snprintf(out, (size_t)n, "decoder_head_kernel<%d, true, %d>", kind, P >= 3 ? 32 : 64);
  }
  return 0;
}
int32_t scvae_decoder_train_kernel(int32_t kind, int64_t H, int32_t arith) {
  if (kind < 0 || (kind > 3 && kind != scvae::LK_BERNOULLI) || (arith < 0 || arith > 2) ||
      !scvae::decoder_fused_train_supported(scvae::likelihood_heads(kind), (int)H, arith))
    return 0;
  return scvae::decoder_train_kernel(scvae::likelihood_heads(kind), (int)H, arith);
}
static int decoder_fused_entry(int32_t kind, int32_t train, const float* d, int64_t rows, int64_t H,
                               const float* const* W, const float* const* b, float* const* dW,
                               float* const* db, int64_t F, scvae::Targets t, int64_t cells,
                               const float* gw, const float* row_const, float* ll, float* dd,
                               void* workspace, void* stream) {
  SCVAE_ARG(((kind >= 0 && kind <= 3) || kind == scvae::LK_BERNOULLI) && W && b);
  // bits 8, 9, 11 of `train`: the arithmetic of this call (none: the process default)
  const int arith_bits = train & (SCVAE_HEADS_FP32 | SCVAE_HEADS_BF16X9 | SCVAE_HEADS_BF16X6);
  SCVAE_ARG((train & ~0xF03) == 0 && (arith_bits & (arith_bits - 1)) == 0);
  const int dd_mode = (train & SCVAE_HEADS_DD_ATOMICS) ? 1 : 0;
  const int arith = (train & SCVAE_HEADS_FP32) ? 0
                    : (train & SCVAE_HEADS_BF16X9) ? 1
                    : (train & SCVAE_HEADS_BF16X6) ? 2 : scvae::default_head_arith();
  train &= 3;
  // (even widths up to 126: every arithmetic; the bf16x9 kernel's wider range -- odd widths, up
  //  to 256 -- for training and, its forward half, forward-only calls)
  SCVAE_ARG(scvae::decoder_fused_train_supported(scvae::likelihood_heads(kind), (int)H, arith));
  scvae::HeadParams hp;
  for (int j = 0; j < 3; ++j) {
    const bool on = j < scvae::likelihood_heads(kind);
    hp.W[j] = on ? W[j] : nullptr;
    hp.b[j] = on ? b[j] : nullptr;
    hp.dW[j] = (on && dW) ? dW[j] : nullptr;
    hp.db[j] = (on && db) ? db[j] : nullptr;
  }
  if (train) {
    SCVAE_ARG(dW && db);
    return scvae::decoder_fused_train((hipStream_t)stream, kind, d, (int)rows, (int)H, hp, (int)F,
                                      t, (int)cells, gw, row_const, ll, dd, (float*)workspace,
                                      arith, (train & 2) != 0, nullptr, dd_mode);
  }
  return scvae::decoder_fused_forward((hipStream_t)stream, kind, d, (int)rows, (int)H, hp, (int)F,
                                      t, (int)cells, row_const, ll, (float*)workspace, arith);
}
int scvae_decoder_fused(int32_t kind, int32_t train, const float* d, int64_t rows, int64_t H,
                        const float* const* W, const float* const* b, float* const* dW,
                        float* const* db, int64_t F, const float* t, int64_t cells,
                        const float* gw, const float* row_const, float* ll, float* dd,
                        void* workspace, void* stream) {
  return decoder_fused_entry(kind, train, d, rows, H, W, b, dW, db, F,
                             scvae::targets_f32(t, (int)F), cells, gw, row_const, ll, dd,
                             workspace, stream);
}
int scvae_decoder_fused_u16(int32_t kind, int32_t train, const float* d, int64_t rows, int64_t H,
                            const float* const* W, const float* const* b, float* const* dW,
                            float* const* db, int64_t F, const uint16_t* t, int64_t ldt,
                            int64_t cells, const float* gw, const float* row_const, float* ll,
                            float* dd, void* workspace, void* stream) {
  SCVAE_ARG(t && ldt >= (F + 63) / 64 * 64 && (ldt & 7) == 0 && ((uintptr_t)t & 15) == 0);
  return decoder_fused_entry(kind, train, d, rows, H, W, b, dW, db, F,
                             scvae::targets_u16(t, (int)ldt), cells, gw, row_const, ll, dd,
                             workspace, stream);
}
int scvae_likelihood_elementwise(int32_t kind, const float* t, const float* const* pre,
                                 float* log_prob, float* mean, float* variance, int64_t n,
                                 void* stream) {
  SCVAE_ARG(pre && ((kind >= 0 && kind <= 3) || kind == LK_BERNOULLI) && n >= 0);
  scvae::HeadPtrs hp = {{nullptr, nullptr, nullptr}};
  for (int j = 0; j < scvae::likelihood_heads(kind); ++j) hp.p[j] = const_cast<float*>(pre[j]);
  return scvae::loglik_elementwise((hipStream_t)stream, kind, t, hp, log_prob, mean, variance,
                                   (size_t)n);
}
int scvae_gauss_latent_fwd(const float* mu_pre, const float* ls_pre, const float* eps, float* z,
                           float* kl_elem, float* kl_cell, int64_t S, int64_t cells, int64_t L,
                           int32_t deterministic, void* stream) {
  return scvae::gauss_latent_fwd((hipStream_t)stream, mu_pre, ls_pre, eps, z, kl_elem, kl_cell,
                                 nullptr, (int)S, (int)cells, (int)L, deterministic);
}
int scvae_dropout_apply(const float* in, float* out, int64_t rows, int64_t cols, float keep,
                        uint64_t seed, int32_t site, int32_t accumulate, void* stream) {
  SCVAE_ARG(site >= 0 && cols > 0 && cols <= INT32_MAX);
  return scvae::dropout_apply((hipStream_t)stream, in, (int)cols, out, (int)cols, rows, (int)cols,
                              keep, seed, (uint32_t)site, accumulate);
}
int scvae_csr_minibatch(const int64_t* indptr, const int32_t* indices, const float* values,
                        const int64_t* rows, int64_t n, int64_t F, void* out, int64_t ld,
                        int32_t as_u16, const float* row_values, float* row_values_out,
                        void* stream) {
  SCVAE_ARG(as_u16 == 0 || as_u16 == 1);
  if (as_u16)
    return scvae::csr_densify_u16((hipStream_t)stream, indptr, indices, values, rows, (int)n,
                                  (int)F, static_cast<uint16_t*>(out), (int)ld, row_values,
                                  row_values_out);
  return scvae::csr_densify((hipStream_t)stream, indptr, indices, values, rows, (int)n, (int)F,
                            static_cast<float*>(out), (int)ld, row_values, row_values_out);
}

int scvae_csr_densify_u16(const int64_t* indptr, const int32_t* indices, const float* values,
                          const int64_t* rows, int64_t n, int64_t F, uint16_t* out, int64_t ld,
                          void* stream) {
  return scvae::csr_densify_u16((hipStream_t)stream, indptr, indices, values, rows, (int)n, (int)F,
                                out, (int)ld);
}

int scvae_count_gemm_u16(int32_t mode, const uint16_t* x, int64_t ldx, int64_t rows, int64_t cols,
                         const float* other, int64_t ld_other, int64_t N, const float* bias,
                         int32_t relu, float* C, int64_t ldc, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  SCVAE_ARG(workspace_bytes >= 0);
  SCVAE_ARG(fits_int(ldx) && fits_int(rows) && fits_int(cols) && fits_int(ld_other) &&
            fits_int(N) && fits_int(ldc));
  SCVAE_ARG(ldx >= cols && ld_other >= N && ldc >= N);
  return scvae::count_gemm_u16((hipStream_t)stream, mode, x, (int)ldx, (int)rows, (int)cols, other,
                               (int)ld_other, (int)N, bias,
                               relu ? scvae::ACT_RELU : scvae::ACT_NONE, C, (int)ldc, workspace,
                               (size_t)workspace_bytes);
}

int scvae_count_gemm_u16_rows(int32_t mode, const uint16_t* x, int64_t ldx, int64_t rows,
                              int64_t cols,
                              const float* other, int64_t ld_other, int64_t N, const float* bias,
                              int32_t relu, float* C, int64_t ldc, void* workspace,
                              int64_t workspace_bytes, const int64_t* x_rows, void* stream) {
  SCVAE_ARG(workspace_bytes >= 0 && x_rows);
  SCVAE_ARG(fits_int(ldx) && fits_int(rows) && fits_int(cols) && fits_int(ld_other) &&
            fits_int(N) && fits_int(ldc));
  SCVAE_ARG(ldx >= cols && ld_other >= N && ldc >= N);
  return scvae::count_gemm_u16((hipStream_t)stream, mode, x, (int)ldx, (int)rows, (int)cols, other,
                               (int)ld_other, (int)N, bias,
                               relu ? scvae::ACT_RELU : scvae::ACT_NONE, C, (int)ldc, workspace,
                               (size_t)workspace_bytes, x_rows);
}

int64_t scvae_count_tiles_padded(int64_t F) {
  return scvae::count_tiles_supported((int)F) && F > 0 && F <= 65536 ? scvae::count_tiles_padded((int)F) : -1;
}
int scvae_csr_row_entries(const int64_t* indptr, const float* values, int64_t n_rows, int32_t* out,
                          void* stream) {
  return scvae::csr_row_entries((hipStream_t)stream, indptr, values, n_rows, out);
}
int scvae_csr_count_tiles(const int64_t* indptr, const int32_t* indices, const float* values,
                          const int64_t* rows, int64_t n, int64_t F,
                          const scvae_count_tiles* tiles, void* stream) {
  SCVAE_ARG(tiles && n >= 0 && n <= INT32_MAX && F > 0 && F <= 65536);
  return scvae::csr_count_tiles((hipStream_t)stream, indptr, indices, values, rows, (int)n, (int)F,
                                scvae::count_tiles_of(tiles));
}
int scvae_count_gemm_tiles(int32_t mode, const scvae_count_tiles* tiles, const uint16_t* x,
                           int64_t ldx, int64_t rows, int64_t cols, const float* other,
                           int64_t ld_other, int64_t N, const float* bias, int32_t relu, float* C,
                           int64_t ldc, void* workspace, int64_t workspace_bytes, void* stream) {
  SCVAE_ARG(tiles && workspace_bytes >= 0);
  return scvae::count_gemm_tiles((hipStream_t)stream, mode, scvae::count_tiles_of(tiles), x, (int)ldx,
                                 (int)rows, (int)cols, other, (int)ld_other, (int)N, bias,
                                 relu ? scvae::ACT_RELU : scvae::ACT_NONE, C, (int)ldc, workspace,
                                 (size_t)workspace_bytes);
}

int scvae_csr_densify(const int64_t* indptr, const int32_t* indices, const float* values,
                      const int64_t* rows, int64_t n, int64_t F, float* out, void* stream) {
  return scvae::csr_densify((hipStream_t)stream, indptr, indices, values, rows, (int)n, (int)F, out,
                            (int)F);
}
int scvae_csr_row_lgamma1p(const int64_t* indptr, const float* values, int64_t n_rows, float* out,
                           void* stream) {
  return scvae::csr_row_lgamma1p((hipStream_t)stream, indptr, values, n_rows, out);
}
int scvae_gather_rows(const float* src, const int64_t* rows, int64_t n, float* out, void* stream) {
  return scvae::gather_rows_f32((hipStream_t)stream, src, rows, (int)n, out);
}
int scvae_bn_merge(const float* gathered, const int64_t* counts, int64_t ranks, int64_t n,
                   float* out, void* stream) {
  return scvae::bn_merge((hipStream_t)stream, gathered, counts, (int)ranks, (int)n, out);
}
int64_t scvae_bn_workspace_floats(int64_t N) {
  return N > 0 ? (int64_t)scvae::bn_partial_floats(1, (int)N) : -1;
}
int scvae_bn_stats(const float* a, int64_t lda, int64_t rows, int64_t N, float* mean, float* var,
                   float* workspace, void* stream) {
  SCVAE_ARG(rows > 0 && rows <= INT32_MAX && N > 0 && lda >= N);
  return scvae::bn_stats((hipStream_t)stream, a, (int)lda, (int)rows, 1, (int)N, mean, var,
                         workspace);
}
int scvae_bn_apply_relu_fwd(const float* a, int64_t lda, const float* mean, const float* var,
                            const float* beta, float* h, int64_t ldh, int64_t rows, int64_t N,
                            int32_t relu, void* stream) {
  SCVAE_ARG(a && mean && var && beta && h && rows >= 0 && N > 0 && lda >= N && ldh >= N);
  if (rows == 0) return 0;
  return scvae::bn_apply((hipStream_t)stream, a, (int)lda, mean, var, (int)N, beta, h, (int)ldh,
                         (int)rows, 1, (int)N, relu ? 1 : 0);
}
int scvae_bn_apply_relu_bwd(const float* dh, int64_t lddh, const float* h, int64_t ldh,
                            const float* a, int64_t lda, const float* mean, const float* var,
                            int64_t rows, int64_t N, int32_t relu, float* da, int64_t ldda,
                            float* dbeta, float* workspace, void* stream) {
  SCVAE_ARG(dh && h && a && mean && var && da && dbeta && workspace && rows > 0 && N > 0);
  SCVAE_ARG(lddh >= N && ldh >= N && lda >= N && ldda >= N && rows <= INT32_MAX);
  float* s1 = workspace;
  float* s2 = workspace + N;
  float* partial = workspace + 2 * N;
  int rc = scvae::bn_bwd_stats((hipStream_t)stream, dh, (int)lddh, h, (int)ldh, a, (int)lda, mean,
                               var, (int)rows, 1, (int)N, relu ? 1 : 0, s1, s2, partial, dbeta,
                               nullptr, nullptr, rows);
  if (rc) return rc;
  return scvae::bn_bwd_apply((hipStream_t)stream, dh, (int)lddh, h, (int)ldh, a, (int)lda, mean,
                             var, s1, s2, (int)rows, 1, (int)N, relu ? 1 : 0, 1.f / (float)rows,
                             da, (int)ldda);
}
int scvae_softplus_gaussian_logprob_pair_fwd(const float* qm, const float* qs, const float* Wpm,
                                             const float* bpm, const float* Wps,
                                             const float* bps, const float* eps, float* z,
                                             float* klz, float* qvar, int64_t K, int64_t S,
                                             int64_t B, int64_t L, void* stream) {
  SCVAE_ARG(K > 0 && S > 0 && B >= 0 && K <= 65535 && B <= INT32_MAX);
  return scvae::softplus_gaussian_fwd((hipStream_t)stream, qm, qs, Wpm, bpm, Wps, bps, eps, z,
                                      klz, qvar, (int)K, (int)S, (int)B, (int)L);
}
int scvae_softplus_gaussian_logprob_pair_bwd(const float* qm, const float* qs, const float* Wpm,
                                             const float* bpm, const float* Wps,
                                             const float* bps, const float* eps, const float* dz,
                                             const float* gklz, float* dqm, float* dqs,
                                             float* dprior, int64_t K, int64_t S, int64_t B,
                                             int64_t L, void* stream) {
  SCVAE_ARG(Wpm && bpm && Wps && bps && K > 0 && S > 0 && B >= 0 && L > 0);
  return scvae::softplus_gaussian_bwd((hipStream_t)stream, qm, qs, Wpm, bpm, Wps, bps, eps, dz,
                                      gklz, dqm, dqs, dprior, (int)K, (int)S, (int)B, (int)L);
}
int scvae_mvn_tril_logprob_pair_fwd(const float* qloc, const float* qscale, const float* Wpl,
                                    const float* bpl, const float* Wps, const float* bps,
                                    const float* eps, float* z, float* klz, float* qvar,
                                    float* qcov, int64_t K, int64_t S, int64_t B, int64_t L,
                                    void* stream) {
  SCVAE_ARG(K > 0 && S > 0 && B >= 0 && L > 0 && L <= 64 && K <= 65535 && B <= INT32_MAX &&
            S <= INT32_MAX);
  return scvae::mvn_tril_fwd((hipStream_t)stream, qloc, qscale, Wpl, bpl, Wps, bps, eps, z, klz,
                             qvar, qcov, (int)K, (int)S, (int)B, (int)L);
}
int scvae_mvn_tril_logprob_pair_bwd(const float* qloc, const float* qscale, const float* Wpl,
                                    const float* bpl, const float* Wps, const float* bps,
                                    const float* eps, const float* dz, const float* gklz,
                                    float* dqloc, float* dqscale, float* dprior, int64_t K,
                                    int64_t S, int64_t B, int64_t L, void* stream) {
  SCVAE_ARG(K > 0 && S > 0 && B >= 0 && L > 0 && L <= 64 && K <= 65535 && B <= INT32_MAX &&
            S <= INT32_MAX);
  return scvae::mvn_tril_bwd((hipStream_t)stream, qloc, qscale, Wpl, bpl, Wps, bps, eps, dz, gklz,
                             dqloc, dqscale, dprior, (int)K, (int)S, (int)B, (int)L);
}
int scvae_mvn_tril_prior_stats(const float* Wpl, const float* bpl, const float* Wps,
                               const float* bps, int64_t K, int64_t L, float* means,
                               float* variances, float* covariances, void* stream) {
  SCVAE_ARG(K > 0 && K <= INT32_MAX && L > 0 && L <= 64);
  return scvae::mvn_tril_prior_stats((hipStream_t)stream, Wpl, bpl, Wps, bps, (int)K, (int)L,
                                     means, variances, covariances);
}
int scvae_categorical_entropy_kl_fwd(const float* logits, float* y, float* kl_y_cell, int64_t B,
                                     int64_t K, const float* prior_logits, void* stream) {
  SCVAE_ARG(logits && y && kl_y_cell && B >= 0 && K > 0 && B <= INT32_MAX);
  return scvae::categorical_fwd((hipStream_t)stream, logits, y, kl_y_cell, (int)B, (int)K,
                                prior_logits);
}
int scvae_categorical_entropy_kl_bwd(const float* y, const float* dy, const float* gate, float c,
                                     float* dlogits, int64_t B, int64_t K,
                                     const float* prior_logits, void* stream) {
  SCVAE_ARG(y && dy && gate && dlogits && B >= 0 && K > 0 && B <= INT32_MAX);
  return scvae::categorical_bwd_gated((hipStream_t)stream, y, dy, gate, c, dlogits, (int)B,
                                      (int)K, prior_logits);
}
int scvae_mixture_elbo_fwd(const float* ll, const float* klz, const float* y,
                           const float* kl_y_cell, int64_t K, int64_t S, int64_t B, float inv_gb,
                           float w, float free_nats, float share, const float* prior_logits,
                           float* sums, float* scalars, float* gate, float* rec_cell,
                           void* stream) {
  SCVAE_ARG(ll && klz && y && kl_y_cell && sums && scalars && gate);
  SCVAE_ARG(K > 0 && S > 0 && B > 0 && K <= INT32_MAX && S <= INT32_MAX && B <= INT32_MAX);
  int rc = scvae::gmvae_elbo((hipStream_t)stream, ll, klz, y, kl_y_cell, (int)K, (int)S, (int)B,
                             inv_gb, sums, rec_cell);
  if (rc) return rc;
  // (the uniform prior's threshold as a step forms it; recomputed on the device otherwise)
  const float thr = free_nats * logf((float)K);
  return scvae::gmvae_elbo_finish((hipStream_t)stream, sums, w, thr, free_nats != 0.f, share,
                                  scalars, gate, prior_logits, (int)K, free_nats);
}
int scvae_mixture_elbo_bwd(const float* ll, const float* klz, const float* y, int64_t K,
                           int64_t S, int64_t B, float w, float inv_gb, float* gw, float* gklz,
                           float* dy, void* stream) {
  SCVAE_ARG(ll && klz && y && gw && gklz && dy);
  SCVAE_ARG(K > 0 && S > 0 && B >= 0 && K <= INT32_MAX && S <= INT32_MAX && B <= INT32_MAX);
  return scvae::gmvae_elbo_bwd((hipStream_t)stream, ll, klz, y, nullptr, (int)K, (int)S, (int)B,
                               w, inv_gb, gw, gklz, dy);
}
int scvae_prior_logits_bwd(const float* y, const float* prior_logits, const float* gate, float c,
                           float off_scale, float free_nats, int64_t B, int64_t K, float* dprior,
                           void* stream) {
  SCVAE_ARG(y && prior_logits && gate && dprior && B >= 0 && K > 0 && B <= INT32_MAX &&
            K <= INT32_MAX);
  return scvae::prior_logits_bwd((hipStream_t)stream, y, prior_logits, gate, c, off_scale,
                                 free_nats, (int)B, (int)K, dprior);
}
int64_t scvae_group_col_sum_workspace_floats(int64_t G, int64_t N) {
  return G > 0 && N > 0 && G <= 65535 && N <= INT32_MAX
             ? (int64_t)scvae::bn_partial_floats((int)G, (int)N)
             : -1;
}
int scvae_group_col_sum(const float* a, int64_t lda, int64_t R, int64_t G, int64_t N, float scale,
                        float* out, float* workspace, void* stream) {
  SCVAE_ARG(a && out && workspace && R > 0 && G > 0 && N > 0 && lda >= N);
  SCVAE_ARG(R <= INT32_MAX && G <= 65535 && N <= INT32_MAX && lda <= INT32_MAX);
  return scvae::group_col_sum((hipStream_t)stream, a, (int)lda, (int)R, (int)G, (int)N, scale,
                              out, workspace);
}
int scvae_sum_groups(const float* a, const float* w, int64_t ldw, int64_t G, int64_t R, int64_t N,
                     float* out, void* stream) {
  SCVAE_ARG(a && out && G > 0 && R >= 0 && N > 0 && (!w || ldw >= G));
  SCVAE_ARG(G <= INT32_MAX && R <= INT32_MAX && N <= INT32_MAX && ldw <= INT32_MAX);
  return scvae::sum_groups((hipStream_t)stream, a, w, (int)ldw, (int)G, (int)R, (int)N, out);
}
int scvae_add_group_rows(const float* a0, const float* rows, float* out, int64_t K, int64_t B,
                         int64_t N, int32_t relu, void* stream) {
  SCVAE_ARG(a0 && rows && out && K > 0 && B >= 0 && N > 0);
  SCVAE_ARG(K <= INT32_MAX && B <= INT32_MAX && N <= INT32_MAX);
  return scvae::add_group_rows((hipStream_t)stream, a0, rows, out, (int)K, (int)B, (int)N,
                               relu ? 1 : 0);
}
int scvae_prior_stats(const float* Wpm, const float* bpm, const float* Wps, const float* bps,
                      int64_t K, int64_t L, float* means, float* variances, void* stream) {
  SCVAE_ARG(Wpm && bpm && Wps && bps && means && variances && K > 0 && L > 0 &&
            K * L <= INT32_MAX - 255);
  return scvae::prior_stats((hipStream_t)stream, Wpm, bpm, Wps, bps, (int)K, (int)L, means,
                            variances);
}
int scvae_iw_logmeanexp(const float* ll, const float* kl_cell, int32_t kl_per_sample,
                        int32_t n_iw, int32_t n_mc, int64_t B, float kl_weight, float row_scale,
                        float* scalars, float* gw, void* stream) {
  SCVAE_ARG(ll && kl_cell && scalars && n_iw > 0 && n_mc > 0 && B > 0 && B <= INT32_MAX);
  return scvae::vae_elbo((hipStream_t)stream, ll, kl_cell, kl_per_sample ? 1 : 0, n_iw, n_mc,
                         (int)B, kl_weight, row_scale, scalars, gw);
}
int scvae_pxmean_stats(int32_t kind, const float* const* pre, int64_t S, int64_t B, int64_t F,
                       const float* weight, int64_t ldw, int32_t accumulate, float* p_x_mean,
                       float* mean_of_var, float* var_of_mean, void* stream) {
  // (constrained Poisson: head 0 is the rate lambda * N, as px_statistics takes it in a step)
  SCVAE_ARG(pre && kind >= 0 && kind <= LK_BERNOULLI && S > 0 && B >= 0 && F > 0);
  scvae::HeadPtrs hp = {{nullptr, nullptr, nullptr}};
  for (int j = 0; j < scvae::likelihood_heads(kind); ++j) hp.p[j] = const_cast<float*>(pre[j]);
  return scvae::px_statistics((hipStream_t)stream, kind, hp, (int)F, (int)S, (int)B, (int)F,
                              weight, (int)ldw, accumulate ? 1 : 0, p_x_mean, mean_of_var,
                              var_of_mean);
}
int scvae_philox_normal(float* out, int64_t rows, int64_t cols, int64_t row_offset, uint64_t seed,
                        uint64_t stream_id, void* stream) {
  return scvae::philox_normal((hipStream_t)stream, out, rows, (int)cols, row_offset, seed,
                              stream_id);
}
int scvae_philox_normal_blocks(float* out, int64_t blocks, int64_t block_rows, int64_t cols,
                               int64_t block_stride, int64_t row_offset, uint64_t seed,
                               uint64_t stream_id, void* stream) {
  SCVAE_ARG(blocks >= 0 && block_rows >= 0);
  return scvae::philox_normal((hipStream_t)stream, out, blocks * block_rows, (int)cols, row_offset,
                              seed, stream_id, block_rows, block_stride);
}

}  // extern "C"
