// The latent stage of the "full-covariance gaussian mixture" GMVAE (du:75-93, 347-349;
// gm:2936-3048, 3270-3292; distributions/multivariate_normal.py:90-149): posterior q(z|x,y=k) and
// prior p(z|y=k) are MultivariateNormalTriL(loc, scale_tril = fill_triangular(scales)) with
// scales = max(softplus(pre), FLT_MIN) on all T = L (L + 1) / 2 entries, off-diagonals included.
//
// One wave per (k, b), L <= 64, lane i owns row i.  Both triangles live in LDS, packed row by
// row (element (i, j) at i (i + 1) / 2 + j); fill_triangular's index map is applied while
// loading.  Lane i reading (i, j) for one j: the triangular numbers of 32 consecutive i are
// distinct modulo 32, so the 32 banks of a ds_read_b32 half-wave see no conflict; lane i reading
// (j, i) of one row j is contiguous.  The sample loop runs inside the wave.  Everything is plain
// loads, stores and wave shuffles: fixed summation order, bit-repeatable.
#include "common.hpp"
#include "kernels.hpp"

namespace scvae {

namespace {

constexpr int MVN_WAVES = 4;              // waves (cells) per workgroup at most
constexpr int MVN_LDS_BUDGET = 48 * 1024; // bytes of LDS a workgroup may ask for

__host__ __device__ constexpr int tri(int i) { return (i * (i + 1)) >> 1; }

// position in the length-T vector x of element (i, j), j <= i, of tfp's fill_triangular(x):
// reshape(concat(x[L:], reverse(x)), [L, L]), lower triangle kept
__device__ __forceinline__ int fill_src(int i, int j, int L, int T) {
  const int idx = i * L + j;
  return idx < T - L ? L + idx : L * L - 1 - idx;
}

// softplus, then the lower end of clip_by_value(., 0 + tiny, inf - tiny) (gm:2976-2980).
// Evaluated in fp64 and rounded once, with the library's logf / expf and true divisions in the
// rest of this file instead of the fast intrinsics and reciprocals: a triangle entry is computed
// once per cell and reused L times, and the prior's gradient g (1 - u_i^2) / P_ii cancels where
// |u_i| is near 1 -- there one ulp of P_ii is 2 u^2 / (1 - u^2) + 1 ulps of the gradient (15 in
// the one-element case of tests/test_gpu_fullcov_kernels.py, which missed fp64 by 2.2e-6 with
// __expf and r * (1 / P_ii), by 1.5e-6 with expf / log1pf in fp32).
__device__ __forceinline__ float softplus_exact(float pre) {
  const double a = (double)pre;
  return (float)(fmax(a, 0.0) + log1p(exp(-fabs(a))));
}
__device__ __forceinline__ float scale_activation(float pre) {
  return fmaxf(softplus_exact(pre), F32_TINY);
}
// its derivative: sigmoid, zero where the clip holds the value
__device__ __forceinline__ float scale_derivative(float pre) {
  if (!(softplus_exact(pre) >= F32_TINY)) return 0.f;
  const float e = expf(-fabsf(pre));
  return (pre >= 0.f ? 1.f : e) / (1.f + e);
}

// LDS written by some lanes of this wave is read by others: order the accesses (one wave:
// its LDS operations complete in order, the compiler must not move them across)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// the value lane `j` holds (j uniform over the wave)
__device__ __forceinline__ float lane_value(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

// dst (packed lower triangle) = scale_activation(w[src] + b[src]); b == nullptr: none
__device__ __forceinline__ void load_tril(float* dst, const float* __restrict__ w,
                                          const float* __restrict__ b, int L, int T, int lane) {
  for (int idx = lane; idx < L * L; idx += WAVE) {
    const int i = idx / L, j = idx - i * L;
    if (j <= i) {
      const int s = fill_src(i, j, L, T);
      dst[tri(i) + j] = scale_activation(b ? w[s] + b[s] : w[s]);
    }
  }
}

// u = P^-1 r by forward substitution, column by column: L dependent steps.  r is consumed.
// pd = P_ii of this lane's row (1 in lanes i >= L, which pass r = 0 and get 0).
__device__ __forceinline__ float solve_lower(const float* P, float r, float pd, int L, int i) {
  float u = 0.f;
  for (int j = 0; j < L; ++j) {
    const float uj = lane_value(r / pd, j);
    if (i == j) u = uj;
    if (i > j && i < L) r = fmaf(-P[tri(i) + j], uj, r);
  }
  return u;
}
// v = P^-T u by back substitution, from the last column to the first
__device__ __forceinline__ float solve_lower_transposed(const float* P, float r, float pd, int L,
                                                        int i) {
  float v = 0.f;
  for (int j = L - 1; j >= 0; --j) {
    const float vj = lane_value(r / pd, j);
    if (i == j) v = vj;
    if (i < j) r = fmaf(-P[tri(j) + i], vj, r);
  }
  return v;
}

int waves_per_block(size_t floats_per_wave) {
  int w = (int)(MVN_LDS_BUDGET / (floats_per_wave * sizeof(float)));
  return w < 1 ? 1 : (w > MVN_WAVES ? MVN_WAVES : w);
}

}  // namespace

// z[k,s,b,:] = loc + A eps[k,s,b,:];  klz[k,s,b] = log q(z) - log p(z|y=k)
//   = (|u|^2 - |eps|^2) / 2 + sum_i (log P_ii - log A_ii),  u = P^-1 (z - loc_p)
// qvar (optional) [K*B, L] = diag(A A^T), qcov (optional) [K*B, L, L] = A A^T
__global__ __launch_bounds__(MVN_WAVES * WAVE) void mvn_tril_fwd_kernel(
    const float* __restrict__ qloc, const float* __restrict__ qsc, const float* __restrict__ Wpl,
    const float* __restrict__ bpl, const float* __restrict__ Wps, const float* __restrict__ bps,
    const float* __restrict__ eps, float* __restrict__ z, float* __restrict__ klz,
    float* __restrict__ qvar, float* __restrict__ qcov, int K, int S, int B, int L) {
  extern __shared__ float mvn_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t kb = (size_t)blockIdx.x * (blockDim.x >> 6) + w;
  if (kb >= (size_t)K * B) return;
  const int k = (int)(kb / B), b = (int)(kb - (size_t)k * B);
  const int T = tri(L);
  float* A = mvn_lds + (size_t)w * (2 * T + WAVE);
  float* P = A + T;
  float* ev = P + T;   // this sample's eps
  load_tril(A, qsc + kb * T, nullptr, L, T, lane);
  load_tril(P, Wps + (size_t)k * T, bps, L, T, lane);
  wave_lds_sync();
  const int i = lane;
  const bool on = i < L;
  float mq = 0.f, mp = 0.f, pd = 1.f, ld = 0.f;
  if (on) {
    mq = qloc[kb * L + i];
    mp = Wpl[(size_t)k * L + i] + bpl[i];
    pd = P[tri(i) + i];
    ld = logf(pd) - logf(A[tri(i) + i]);
  }
  const float logdet = wave_sum(ld);
  if (qvar && on) {
    float v = 0.f;
    for (int j = 0; j <= i; ++j) v = fmaf(A[tri(i) + j], A[tri(i) + j], v);
    qvar[kb * L + i] = v;
  }
  if (qcov) {
    for (int idx = lane; idx < L * L; idx += WAVE) {
      const int r = idx / L, c = idx - r * L;
      const int n = min(r, c);
      float v = 0.f;
      for (int m = 0; m <= n; ++m) v = fmaf(A[tri(r) + m], A[tri(c) + m], v);
      qcov[kb * L * L + idx] = v;
    }
  }
  for (int s = 0; s < S; ++s) {
    const size_t row = ((size_t)k * S + s) * B + b;
    const float e = on ? eps[row * L + i] : 0.f;
    wave_lds_sync();
    ev[lane] = e;
    wave_lds_sync();
    float zz = mq;
    if (on) {
      for (int j = 0; j <= i; ++j) zz = fmaf(A[tri(i) + j], ev[j], zz);
      z[row * L + i] = zz;
    }
    const float u = solve_lower(P, on ? zz - mp : 0.f, pd, L, i);
    const float t = wave_sum(0.5f * (u * u - e * e));
    if (lane == 0) klz[row] = t + logdet;
  }
}

int mvn_tril_fwd(hipStream_t st, const float* qloc, const float* qsc, const float* Wpl,
                 const float* bpl, const float* Wps, const float* bps, const float* eps, float* z,
                 float* klz, float* qvar, float* qcov, int K, int S, int B, int L) {
  SCVAE_ARG(qloc && qsc && Wpl && bpl && Wps && bps && eps && z && klz);
  SCVAE_ARG(L > 0 && L <= WAVE && K > 0 && S > 0 && B >= 0);
  if (B == 0) return 0;
  const size_t per_wave = 2 * (size_t)tri(L) + WAVE;
  const int W = waves_per_block(per_wave);
  const size_t cells = (size_t)K * B;
  const size_t blocks = (cells + W - 1) / W;
  SCVAE_ARG(blocks <= 0x7FFFFFFF);
  hipLaunchKernelGGL(mvn_tril_fwd_kernel, dim3((unsigned)blocks), dim3(W * WAVE),
                     W * per_wave * sizeof(float), st, qloc, qsc, Wpl, bpl, Wps, bps, eps, z, klz,
                     qvar, qcov, K, S, B, L);
  SCVAE_LAUNCH_CHECK("mvn_tril_fwd_kernel");
  return 0;
}

// backward of the above.  dz [K,S,B,L]: gradient from the decoder; g = gklz [K,S,B]: d loss /
// d klz.  With v = P^-T u:  dz_tot = dz + g v;  d loc = sum_s dz_tot;
//   dA = tril(sum_s dz_tot eps^T) - diag(sum_s g / A_ii);
//   per cell: d loc_p = -sum_s g v;  dP = tril(-sum_s g v u^T) + diag(sum_s g / P_ii)
// (-P^-T (g u u^T) = -g v u^T), then back through fill_triangular and the scale activation.
// Outputs dqloc [K*B, L], dqsc [K*B, T] and the per-cell prior gradients dpr [K*B, L + T] =
// (d loc_p | d prior scale pre-activations), to be summed over b in a fixed order.
__global__ __launch_bounds__(MVN_WAVES * WAVE) void mvn_tril_bwd_kernel(
    const float* __restrict__ qloc, const float* __restrict__ qsc, const float* __restrict__ Wpl,
    const float* __restrict__ bpl, const float* __restrict__ Wps, const float* __restrict__ bps,
    const float* __restrict__ eps, const float* __restrict__ dz, const float* __restrict__ gklz,
    float* __restrict__ dqloc, float* __restrict__ dqsc, float* __restrict__ dpr, int K, int S,
    int B, int L) {
  extern __shared__ float mvn_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t kb = (size_t)blockIdx.x * (blockDim.x >> 6) + w;
  if (kb >= (size_t)K * B) return;
  const int k = (int)(kb / B), b = (int)(kb - (size_t)k * B);
  const int T = tri(L);
  float* A = mvn_lds + (size_t)w * (4 * T + 2 * WAVE);
  float* P = A + T;
  float* GA = P + T;    // sum_s dz_tot eps^T, lower triangle
  float* GP = GA + T;   // -sum_s g v u^T, lower triangle
  float* ev = GP + T;
  float* uv = ev + WAVE;
  load_tril(A, qsc + kb * T, nullptr, L, T, lane);
  load_tril(P, Wps + (size_t)k * T, bps, L, T, lane);
  for (int t = lane; t < T; t += WAVE) { GA[t] = 0.f; GP[t] = 0.f; }
  wave_lds_sync();
  const int i = lane;
  const bool on = i < L;
  float mq = 0.f, mp = 0.f, pd = 1.f, ad = 1.f;
  if (on) {
    mq = qloc[kb * L + i];
    mp = Wpl[(size_t)k * L + i] + bpl[i];
    pd = P[tri(i) + i];
    ad = A[tri(i) + i];
  }
  float dmq = 0.f, dmp = 0.f, gsum = 0.f;
  for (int s = 0; s < S; ++s) {
    const size_t row = ((size_t)k * S + s) * B + b;
    const float e = on ? eps[row * L + i] : 0.f;
    const float dzi = on ? dz[row * L + i] : 0.f;
    const float g = gklz[row];
    wave_lds_sync();
    ev[lane] = e;
    wave_lds_sync();
    float zz = mq;
    if (on)
      for (int j = 0; j <= i; ++j) zz = fmaf(A[tri(i) + j], ev[j], zz);
    const float u = solve_lower(P, on ? zz - mp : 0.f, pd, L, i);
    const float v = solve_lower_transposed(P, u, pd, L, i);
    const float gv = g * v;
    const float dzt = dzi + gv;
    dmq += dzt;
    dmp -= gv;
    gsum += g;
    uv[lane] = u;
    wave_lds_sync();
    if (on) {
      for (int j = 0; j <= i; ++j) {
        GA[tri(i) + j] = fmaf(dzt, ev[j], GA[tri(i) + j]);
        GP[tri(i) + j] = fmaf(-gv, uv[j], GP[tri(i) + j]);
      }
    }
  }
  float* dp = dpr + kb * (size_t)(L + T);
  if (on) {
    GA[tri(i) + i] -= gsum / ad;
    GP[tri(i) + i] += gsum / pd;
    dqloc[kb * L + i] = dmq;
    dp[i] = dmp;
  }
  wave_lds_sync();
  for (int idx = lane; idx < L * L; idx += WAVE) {
    const int r = idx / L, c = idx - r * L;
    if (c <= r) {
      const int src = fill_src(r, c, L, T);
      // a clipped entry's gradient is selected, not multiplied: sum_s g / FLT_MIN on a clipped
      // diagonal overflows once |sum_s g| passes 4, and inf * 0 is NaN
      const float da = scale_derivative(qsc[kb * T + src]);
      const float dpd = scale_derivative(Wps[(size_t)k * T + src] + bps[src]);
      dqsc[kb * T + src] = da == 0.f ? 0.f : GA[tri(r) + c] * da;
      dp[L + src] = dpd == 0.f ? 0.f : GP[tri(r) + c] * dpd;
    }
  }
}

int mvn_tril_bwd(hipStream_t st, const float* qloc, const float* qsc, const float* Wpl,
                 const float* bpl, const float* Wps, const float* bps, const float* eps,
                 const float* dz, const float* gklz, float* dqloc, float* dqsc, float* dpr, int K,
                 int S, int B, int L) {
  SCVAE_ARG(qloc && qsc && Wpl && bpl && Wps && bps && eps && dz && gklz && dqloc && dqsc && dpr);
  SCVAE_ARG(L > 0 && L <= WAVE && K > 0 && S > 0 && B >= 0);
  if (B == 0) return 0;
  const size_t per_wave = 4 * (size_t)tri(L) + 2 * WAVE;
  const int W = waves_per_block(per_wave);
  const size_t cells = (size_t)K * B;
  const size_t blocks = (cells + W - 1) / W;
  SCVAE_ARG(blocks <= 0x7FFFFFFF);
  hipLaunchKernelGGL(mvn_tril_bwd_kernel, dim3((unsigned)blocks), dim3(W * WAVE),
                     W * per_wave * sizeof(float), st, qloc, qsc, Wpl, bpl, Wps, bps, eps, dz, gklz,
                     dqloc, dqsc, dpr, K, S, B, L);
  SCVAE_LAUNCH_CHECK("mvn_tril_bwd_kernel");
  return 0;
}

// p(z|y=k) statistics for logging (gm:2879-2893): means = loc_p, variances = diag(P P^T) (the
// square of the batch mean of the stddev: the prior does not depend on the cell), covariances
// (optional) [K, L, L] = P P^T.  One wave per cluster.
__global__ __launch_bounds__(WAVE) void mvn_tril_prior_stats_kernel(
    const float* __restrict__ Wpl, const float* __restrict__ bpl, const float* __restrict__ Wps,
    const float* __restrict__ bps, int L, float* __restrict__ means, float* __restrict__ variances,
    float* __restrict__ covariances) {
  extern __shared__ float mvn_lds[];
  const int k = blockIdx.x, lane = threadIdx.x;
  const int T = tri(L);
  float* P = mvn_lds;
  load_tril(P, Wps + (size_t)k * T, bps, L, T, lane);
  wave_lds_sync();
  if (lane < L) means[(size_t)k * L + lane] = Wpl[(size_t)k * L + lane] + bpl[lane];
  for (int idx = lane; idx < L * L; idx += WAVE) {
    const int r = idx / L, c = idx - r * L;
    const int n = min(r, c);
    float v = 0.f;
    for (int m = 0; m <= n; ++m) v = fmaf(P[tri(r) + m], P[tri(c) + m], v);
    if (covariances) covariances[(size_t)k * L * L + idx] = v;
    if (r == c) variances[(size_t)k * L + r] = v;
  }
}

int mvn_tril_prior_stats(hipStream_t s, const float* Wpl, const float* bpl, const float* Wps,
                         const float* bps, int K, int L, float* means, float* variances,
                         float* covariances) {
  SCVAE_ARG(Wpl && bpl && Wps && bps && means && variances && K > 0 && L > 0 && L <= WAVE);
  hipLaunchKernelGGL(mvn_tril_prior_stats_kernel, dim3(K), dim3(WAVE), tri(L) * sizeof(float), s,
                     Wpl, bpl, Wps, bps, L, means, variances, covariances);
  SCVAE_LAUNCH_CHECK("mvn_tril_prior_stats_kernel");
  return 0;
}

}  // namespace scvae
