// Exact t-SNE of the latent values (scvae/analyses/decomposition/decomposition.py:78-91 fits
// sklearn.manifold.TSNE for analyses/subanalyses.py:595-673; the objective and the optimiser
// here are scikit-learn's TSNE(method="exact"): two components, Euclidean metric, one degree of
// freedom), over every pair of cells.  X is [N, L] fp32 with row pitch ldx, 1 <= L <= 128,
// 2 <= N <= 2^22.  The joint probabilities are never stored: every pass forms them per pair from
// the rows, the precision beta_i and the normaliser S_i of each row,
//
//   d2(i, j) = sum_l (x_il - x_jl)^2, the direct form in fp32 (0 exactly for equal rows)
//   p(j | i) = exp(-beta_i d2) / S_i,  S_i = sum_{j != i} exp(-beta_i d2), 1e-8 where that is 0
//   P_ij = max((p(j | i) + p(i | j)) / sumP, eps) exaggeration        eps = 2^-52
//   w_ij = 1 / (1 + |y_i - y_j|^2),  Z = sum_{i != j} w_ij
//   grad_i = 4 (A_i - R_i / Z),  A_i = sum_j P_ij w_ij (y_i - y_j),  R_i = sum_j w_ij^2 (y_i - y_j)
//   KL = sum_{i != j} P_ij log(P_ij / max(w_ij / Z, eps))
//
// exp(v), v <= 0, is v_exp_f32 of v log2(e): 1 ulp of the instruction and the rounding of the
// product, (1 + |v|) 2^-23 relative in all; results below 2^-126 are flushed to 0.
//
// Perplexity search (tsne_perplexity_kernel): a workgroup of 256 threads takes one row i at a
// time.  It writes the row's N squared distances once into its own row of the workspace and
// then runs scikit-learn's _binary_search_perplexity over them: every step is one pass over the
// parked distances, thread t adding columns t, t + 256, ... in fp64, the 256 partial sums joined
// by a binary tree in LDS.  beta is held in fp32 throughout, so the beta that is returned is the
// beta that was tested.
//
// All-pairs pass (tsne_pair_kernel): the tiling of silhouette.hip.  A workgroup of 256 threads
// owns 64 rows i and walks all columns j in tiles of 64; both row blocks lie in LDS
// coordinate-major, [l][row] with a pitch of 68 floats; thread (ti, tj) = (t / 16, t % 16) holds
// the 4 x 4 pairs of rows 4 ti .. + 3 and columns 4 tj .. + 3.  The i block is resident; the j
// block comes in chunks of 32 coordinates (the last chunk may be short) through two LDS buffers,
// the loads of the chunk after the next in flight in registers.  y_j, -beta_j log2(e) and
// 1 / (S_j sumP) of a tile travel with its first chunk, through three LDS buffers: with a single
// chunk per tile a wave may store the tile after the next while another still reads this one.
//
// Summation order (no atomics; the same inputs give the same bits): a thread adds its 4 columns
// of a tile in fp32, in order, and adds that to its fp64 running sum, tile after tile; the 16
// threads of a row are joined at the end by a 4-level xor tree in fp64.  Z, the KL divergence and
// the gradient norm are joined over the rows by one workgroup: thread t adds rows t, t + 1024,
// ... in fp64, then a binary tree.
#include "../../include/scvae_hip.h"
#include "common.hpp"

namespace scvae {
namespace {

constexpr int TSNE_THREADS = 256;
constexpr int TSNE_TILE = 64;    // rows of a block, columns of a tile
constexpr int TSNE_PITCH = 68;   // floats per coordinate in LDS: 16-byte aligned, off the banks
constexpr int TSNE_CHUNK = 32;   // coordinates of the j tile in LDS at a time
constexpr int TSNE_LOADS = TSNE_TILE * TSNE_CHUNK / TSNE_THREADS;  // per thread and chunk
constexpr int TSNE_EXTRA = 4 * TSNE_TILE;  // y_j (2), -beta_j log2(e), 1 / (S_j sumP) of a tile
constexpr int TSNE_MAX_L = 128;
constexpr int64_t TSNE_MAX_N = (int64_t)1 << 22;
constexpr int TSNE_SEARCH_ROWS = 512;    // rows of parked distances, one per workgroup
constexpr int TSNE_SEARCH_STEPS = 100;
constexpr double TSNE_SEARCH_TOLERANCE = 1e-5;
constexpr double TSNE_EMPTY_ROW_SUM = 1e-8;
constexpr float TSNE_EPS = 2.220446049250313e-16f;   // 2^-52, the fp64 machine epsilon
constexpr float TSNE_LOG2_E = 1.4426950408889634f;
constexpr int TSNE_JOIN_THREADS = 1024;
constexpr int TSNE_SUMS = 5;     // A (2), R (2) and Z of a row
constexpr int64_t TSNE_HEAD_BYTES = 64;  // Z, ahead of the rows' sums in the workspace

typedef float tsne_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float tsne_exp2(float v) { return __builtin_amdgcn_exp2f(v); }

// rows [r0, r0 + 64) x coordinates [l0, l0 + 32) of x into registers: lane l = t % 32 takes
// coordinate l0 + l of rows t / 32, t / 32 + 8, ...; rows >= N and coordinates >= L read as 0
__device__ __forceinline__ void tsne_fetch(const float* __restrict__ x, int64_t ldx, int64_t N,
                                           int L, int64_t r0, int l0, float* v) {
  const int l = l0 + (threadIdx.x & (TSNE_CHUNK - 1));
  const int64_t r = r0 + (threadIdx.x / TSNE_CHUNK);
#pragma unroll
  for (int u = 0; u < TSNE_LOADS; ++u) {
    const int64_t row = r + u * (TSNE_THREADS / TSNE_CHUNK);
    v[u] = (l < L && row < N) ? x[row * ldx + l] : 0.f;
  }
}
// ... and into LDS, dst[l][row] with l counted from the chunk's first coordinate
__device__ __forceinline__ void tsne_store(const float* v, float* dst) {
  float* p = dst + (threadIdx.x & (TSNE_CHUNK - 1)) * TSNE_PITCH + threadIdx.x / TSNE_CHUNK;
#pragma unroll
  for (int u = 0; u < TSNE_LOADS; ++u) p[u * (TSNE_THREADS / TSNE_CHUNK)] = v[u];
}
// what thread t stages of the columns [j0, j0 + 64): kind t / 64 of column j0 + t % 64;
// 0 for columns >= N
__device__ __forceinline__ float tsne_fetch_extra(const float* __restrict__ y,
                                                  const float* __restrict__ beta,
                                                  const float* __restrict__ row_sum,
                                                  float inv_sum_p, int64_t N, int64_t j0) {
  const int kind = threadIdx.x >> 6;
  const int64_t j = j0 + (threadIdx.x & 63);
  if (j >= N) return 0.f;
  if (kind < 2) return y[2 * j + kind];
  if (kind == 2) return -beta[j] * TSNE_LOG2_E;
  return inv_sum_p / row_sum[j];
}

// the sum of v over the 16 lanes that share a row (the 16 tj of one ti), the same bits in every
// lane: both partners of every step add the same two numbers
__device__ __forceinline__ double tsne_row_sum(double v) {
  v += __shfl_xor(v, 1, WAVE);
  v += __shfl_xor(v, 2, WAVE);
  v += __shfl_xor(v, 4, WAVE);
  v += __shfl_xor(v, 8, WAVE);
  return v;
}

// the sum of the NT values red[0 .. NT) by a binary tree; valid in every thread afterwards
template <int NT>
__device__ __forceinline__ double tsne_tree(double* red) {
  __syncthreads();
  for (int off = NT / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  return red[0];
}

// One row at a time per workgroup: distances into dist[blockIdx.x][N], then the search.
// ratio[i] = sum_{j != i} exp(-beta_i d2) / S_i with S_i as it is stored, rounded to fp32.
__global__ __launch_bounds__(TSNE_THREADS) void tsne_perplexity_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, int L, double log_perplexity,
    float* __restrict__ beta_out, float* __restrict__ sum_out, int32_t* __restrict__ steps_out,
    double* __restrict__ ratio_out, float* __restrict__ dist) {
  __shared__ float xi[TSNE_MAX_L];
  __shared__ double red_p[TSNE_THREADS], red_dp[TSNE_THREADS];
  __shared__ float next_beta;
  __shared__ int done;
  float* d = dist + (size_t)blockIdx.x * (size_t)N;
  for (int64_t i = blockIdx.x; i < N; i += gridDim.x) {
    __syncthreads();  // the row before is finished with xi
    if ((int)threadIdx.x < L) xi[threadIdx.x] = x[i * ldx + threadIdx.x];
    __syncthreads();
    for (int64_t j = threadIdx.x; j < N; j += TSNE_THREADS) {
      const float* __restrict__ xj = x + j * ldx;
      float s = 0.f;
      for (int l = 0; l < L; ++l) {
        const float t = xi[l] - xj[l];
        s = fmaf(t, t, s);
      }
      d[j] = s;   // read back by this thread only
    }
    float beta = 1.f, beta_min = -INFINITY, beta_max = INFINITY;   // (the bounds: thread 0)
    for (int step = 0;; ++step) {
      const float nb = -beta * TSNE_LOG2_E;
      double sp = 0.0, sdp = 0.0;
      for (int64_t j = threadIdx.x; j < N; j += TSNE_THREADS) {
        if (j == i) continue;
        const float d2 = d[j];
        const float p = tsne_exp2(nb * d2);
        sp += (double)p;
        sdp = fma((double)d2, (double)p, sdp);
      }
      red_p[threadIdx.x] = sp;
      const double total_p = tsne_tree<TSNE_THREADS>(red_p);
      red_dp[threadIdx.x] = sdp;
      const double total_dp = tsne_tree<TSNE_THREADS>(red_dp);
      if (threadIdx.x == 0) {
        const double S = total_p > 0.0 ? total_p : TSNE_EMPTY_ROW_SUM;   // scikit-learn's rule
        const double difference = log(S) + (double)beta * total_dp / S - log_perplexity;
        const bool found = fabs(difference) <= TSNE_SEARCH_TOLERANCE;
        if (found || step + 1 == TSNE_SEARCH_STEPS) {
          const float S32 = (float)S;
          beta_out[i] = beta;
          sum_out[i] = S32;
          steps_out[i] = found ? step : TSNE_SEARCH_STEPS;
          ratio_out[i] = total_p / (double)S32;
          done = 1;
        } else {
          if (difference > 0.0) {   // too many neighbours: a narrower kernel
            beta_min = beta;
            beta = beta_max == INFINITY ? beta * 2.f : (beta + beta_max) * 0.5f;
          } else {
            beta_max = beta;
            beta = beta_min == -INFINITY ? beta * 0.5f : (beta + beta_min) * 0.5f;
          }
          next_beta = beta;
          done = 0;
        }
      }
      __syncthreads();
      if (done) break;
      beta = next_beta;
    }
  }
}

// KL = false: sums[row] = A (2), R (2), Z of the row.  KL = true: kl_rows[row] = the row's
// share of the KL divergence, with Z read from *z_total.
// dynamic LDS: the i block [L rounded up to 32][68], two j chunks [32][68], three [4][64] of
// the tiles' y_j, -beta_j log2(e), 1 / (S_j sumP)
template <bool KL>
__global__ __launch_bounds__(TSNE_THREADS) void tsne_pair_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, int L, const float* __restrict__ beta,
    const float* __restrict__ row_sum, float inv_sum_p, const float* __restrict__ y,
    float exaggeration, double* __restrict__ sums, const double* __restrict__ z_total,
    double* __restrict__ kl_rows) {
  extern __shared__ __align__(16) float tsne_lds[];
  const int chunks = (L + TSNE_CHUNK - 1) / TSNE_CHUNK;
  float* xi = tsne_lds;
  float* xj = xi + (size_t)chunks * TSNE_CHUNK * TSNE_PITCH;
  float* extra = xj + 2 * TSNE_CHUNK * TSNE_PITCH;
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const int64_t i0 = (int64_t)blockIdx.x * TSNE_TILE;
  const int64_t tiles = (N + TSNE_TILE - 1) / TSNE_TILE;

  float v[TSNE_LOADS];
  for (int ch = 0; ch < chunks; ++ch) {
    tsne_fetch(x, ldx, N, L, i0, ch * TSNE_CHUNK, v);
    tsne_store(v, xi + (size_t)ch * TSNE_CHUNK * TSNE_PITCH);
  }
  // this thread's four rows (a row >= N takes the values of the last row; it is not written)
  float yix[4], yiy[4], nbi[4], ci[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = i0 + 4 * ti + r < N ? i0 + 4 * ti + r : N - 1;
    yix[r] = y[2 * row], yiy[r] = y[2 * row + 1];
    nbi[r] = -beta[row] * TSNE_LOG2_E;
    ci[r] = inv_sum_p / row_sum[row];
  }
  float inv_z = 0.f;
  if (KL) inv_z = (float)(1.0 / *z_total);
  double acc[KL ? 1 : TSNE_SUMS][4];
#pragma unroll
  for (int k = 0; k < (KL ? 1 : TSNE_SUMS); ++k)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[k][r] = 0.0;

  // The j chunks pass through two LDS buffers in turn: step k = (tile, chunk) reads buffer k & 1
  // while the chunk of step k + 1 is stored into the other one and the chunk of step k + 2 is
  // fetched into registers -- one barrier a step.  (A fetch past the last row reads nothing.)
  constexpr int BUFFER = TSNE_CHUNK * TSNE_PITCH;
  tsne_fetch(x, ldx, N, L, 0, 0, v);
  tsne_store(v, xj);
  float e = tsne_fetch_extra(y, beta, row_sum, inv_sum_p, N, 0);
  extra[threadIdx.x] = e;
  if (chunks > 1) {
    tsne_fetch(x, ldx, N, L, 0, TSNE_CHUNK, v);
  } else {
    tsne_fetch(x, ldx, N, L, TSNE_TILE, 0, v);
    e = tsne_fetch_extra(y, beta, row_sum, inv_sum_p, N, TSNE_TILE);
  }
  __syncthreads();  // the i block, step 0's chunk, tile 0's extras
  int step = 0;

  for (int64_t t = 0; t < tiles; ++t) {
    const int64_t j0 = t * TSNE_TILE;
    tsne_f2 d2[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r) d2[r][0] = d2[r][1] = tsne_f2{0.f, 0.f};
    for (int ch = 0; ch < chunks; ++ch, ++step) {
      tsne_store(v, xj + ((step + 1) & 1) * BUFFER);
      if (ch + 1 == chunks) extra[(int)((t + 1) % 3) * TSNE_EXTRA + threadIdx.x] = e;
      {
        int ch2 = ch + 2;
        int64_t t2 = t;
        if (ch2 >= chunks) ch2 -= chunks, ++t2;
        if (ch2 >= chunks) ch2 -= chunks, ++t2;
        tsne_fetch(x, ldx, N, L, t2 * TSNE_TILE, ch2 * TSNE_CHUNK, v);
        if (ch2 == 0) e = tsne_fetch_extra(y, beta, row_sum, inv_sum_p, N, t2 * TSNE_TILE);
      }
      const int lc = L - ch * TSNE_CHUNK < TSNE_CHUNK ? L - ch * TSNE_CHUNK : TSNE_CHUNK;
      const float* pi = xi + (size_t)ch * TSNE_CHUNK * TSNE_PITCH + 4 * ti;
      const float* pj = xj + (step & 1) * BUFFER + 4 * tj;
      // the reads of coordinate l + 1 are in flight while l is used
      float4 p = *reinterpret_cast<const float4*>(pi);
      float4 q = *reinterpret_cast<const float4*>(pj);
#pragma unroll 2
      for (int l = 0; l < lc; ++l) {
        const int next = (l + 1 < lc ? l + 1 : l) * TSNE_PITCH;
        const float4 p_next = *reinterpret_cast<const float4*>(pi + next);
        const float4 q_next = *reinterpret_cast<const float4*>(pj + next);
        const tsne_f2 q01 = {q.x, q.y}, q23 = {q.z, q.w};
        const float pr[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const tsne_f2 pp = {pr[r], pr[r]};
          const tsne_f2 d0 = pp - q01, d1 = pp - q23;
          d2[r][0] = __builtin_elementwise_fma(d0, d0, d2[r][0]);
          d2[r][1] = __builtin_elementwise_fma(d1, d1, d2[r][1]);
        }
        p = p_next, q = q_next;
      }
      __syncthreads();  // the next step's chunk is stored; this one's readers are done
    }

    const float* ex = extra + (int)(t % 3) * TSNE_EXTRA + 4 * tj;
    const float4 jx = *reinterpret_cast<const float4*>(ex);
    const float4 jy = *reinterpret_cast<const float4*>(ex + TSNE_TILE);
    const float4 jb = *reinterpret_cast<const float4*>(ex + 2 * TSNE_TILE);
    const float4 jc = *reinterpret_cast<const float4*>(ex + 3 * TSNE_TILE);
    const float yjx[4] = {jx.x, jx.y, jx.z, jx.w}, yjy[4] = {jy.x, jy.y, jy.z, jy.w};
    const float nbj[4] = {jb.x, jb.y, jb.z, jb.w}, cj[4] = {jc.x, jc.y, jc.z, jc.w};
    // only the tile of the block's own rows and the last tile hold pairs that do not count
    const bool edge = j0 == i0 || j0 + TSNE_TILE > N;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float dr[4] = {d2[r][0].x, d2[r][0].y, d2[r][1].x, d2[r][1].y};
      float part[KL ? 1 : TSNE_SUMS];
#pragma unroll
      for (int k = 0; k < (KL ? 1 : TSNE_SUMS); ++k) part[k] = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float P = fmaxf(fmaf(tsne_exp2(nbi[r] * dr[c]), ci[r],
                                   tsne_exp2(nbj[c] * dr[c]) * cj[c]), TSNE_EPS) * exaggeration;
        const float dx = yix[r] - yjx[c], dy = yiy[r] - yjy[c];
        const float w = fast_rcp(fmaf(dx, dx, fmaf(dy, dy, 1.f)));
        bool counts = true;
        if (edge) {
          const int64_t j = j0 + 4 * tj + c;
          counts = j < N && j != i0 + 4 * ti + r;
        }
        if (KL) {
          const float Q = fmaxf(w * inv_z, TSNE_EPS);
          const float term = P * (fast_log(P) - fast_log(Q));
          part[0] += counts ? term : 0.f;
        } else {
          const float wc = counts ? w : 0.f;
          const float pw = P * wc, ww = wc * wc;
          part[0] = fmaf(pw, dx, part[0]);
          part[1] = fmaf(pw, dy, part[1]);
          part[2] = fmaf(ww, dx, part[2]);
          part[3] = fmaf(ww, dy, part[3]);
          part[4] += wc;
        }
      }
#pragma unroll
      for (int k = 0; k < (KL ? 1 : TSNE_SUMS); ++k) acc[k][r] += (double)part[k];
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = i0 + 4 * ti + r;
#pragma unroll
    for (int k = 0; k < (KL ? 1 : TSNE_SUMS); ++k) {
      const double total = tsne_row_sum(acc[k][r]);
      if (tj == 0 && row < N) {
        if (KL) kl_rows[row] = total;
        else sums[row * TSNE_SUMS + k] = total;
      }
    }
  }
}

// One workgroup: *z_total = Z = the sum of the rows' Z, grad[i] = 4 (A_i - R_i / Z) rounded to
// fp32, *grad_norm (optional) = the Euclidean norm of grad as it is stored.
__global__ __launch_bounds__(TSNE_JOIN_THREADS) void tsne_gradient_kernel(
    const double* __restrict__ sums, int64_t N, float* __restrict__ grad,
    double* __restrict__ z_total, double* __restrict__ grad_norm) {
  __shared__ double red[TSNE_JOIN_THREADS];
  double z = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += TSNE_JOIN_THREADS) z += sums[i * TSNE_SUMS + 4];
  red[threadIdx.x] = z;
  const double Z = tsne_tree<TSNE_JOIN_THREADS>(red);
  double square = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += TSNE_JOIN_THREADS) {
    const double* s = sums + i * TSNE_SUMS;
    const float gx = (float)(4.0 * (s[0] - s[2] / Z)), gy = (float)(4.0 * (s[1] - s[3] / Z));
    grad[2 * i] = gx, grad[2 * i + 1] = gy;
    square += (double)gx * (double)gx + (double)gy * (double)gy;
  }
  __syncthreads();  // every thread has read red[0]
  red[threadIdx.x] = square;
  const double total = tsne_tree<TSNE_JOIN_THREADS>(red);
  if (threadIdx.x == 0) {
    *z_total = Z;
    if (grad_norm) *grad_norm = sqrt(total);
  }
}

// One workgroup: *out = the sum of rows[0 .. N)
__global__ __launch_bounds__(TSNE_JOIN_THREADS) void tsne_sum_kernel(
    const double* __restrict__ rows, int64_t N, double* __restrict__ out) {
  __shared__ double red[TSNE_JOIN_THREADS];
  double sum = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += TSNE_JOIN_THREADS) sum += rows[i];
  red[threadIdx.x] = sum;
  const double total = tsne_tree<TSNE_JOIN_THREADS>(red);
  if (threadIdx.x == 0) *out = total;
}

// scikit-learn's _gradient_descent step, element by element.  The sign of update * grad is
// taken from the fp64 product, which neither underflows nor rounds.
__global__ __launch_bounds__(TSNE_THREADS) void tsne_update_kernel(
    float* __restrict__ y, float* __restrict__ update, float* __restrict__ gains,
    const float* __restrict__ grad, int64_t elements, float momentum, float learning_rate,
    float min_gain) {
  const int64_t k = (int64_t)blockIdx.x * TSNE_THREADS + threadIdx.x;
  if (k >= elements) return;
  const float g = grad[k], u = update[k];
  float gain = gains[k];
  gain = (double)u * (double)g < 0.0 ? gain + 0.2f : gain * 0.8f;
  gain = fmaxf(gain, min_gain);
  const float u_new = momentum * u - learning_rate * gain * g;
  gains[k] = gain;
  update[k] = u_new;
  y[k] += u_new;
}

__host__ int64_t tsne_search_rows(int64_t N) {
  return N < TSNE_SEARCH_ROWS ? N : TSNE_SEARCH_ROWS;
}

}  // namespace
}  // namespace scvae

#define SCVAE_TSNE_SIZES(N, L)                        \
  SCVAE_ARG(L >= 1 && L <= scvae::TSNE_MAX_L);        \
  SCVAE_ARG(N >= 2 && N <= scvae::TSNE_MAX_N)

extern "C" {

// the larger of: the rows' conditional sums (8 N) and the parked distances of the search
// (4 N per workgroup); Z, the rows' five sums (40 N) and their KL shares (8 N) of a pass
int64_t scvae_tsne_workspace_bytes(int64_t N, int64_t L) {
  using namespace scvae;
  SCVAE_TSNE_SIZES(N, L);
  const int64_t search = 8 * N + (4 * tsne_search_rows(N) * N + 7) / 8 * 8;
  const int64_t pass = TSNE_HEAD_BYTES + 8 * (TSNE_SUMS + 1) * N;
  return search > pass ? search : pass;
}

int scvae_tsne_perplexity(const float* x, int64_t ldx, int64_t N, int64_t L, double perplexity,
                          float* beta, float* row_sum, int32_t* steps, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  using namespace scvae;
  SCVAE_TSNE_SIZES(N, L);
  SCVAE_ARG(x && beta && row_sum && steps && workspace && ldx >= L);
  SCVAE_ARG(perplexity > 0.0 && perplexity < 1e300);
  SCVAE_ARG(((uintptr_t)workspace & 7) == 0 &&
            workspace_bytes >= scvae_tsne_workspace_bytes(N, L));
  double* ratio = static_cast<double*>(workspace);
  float* dist = reinterpret_cast<float*>(ratio + N);
  hipLaunchKernelGGL(tsne_perplexity_kernel, dim3((unsigned)tsne_search_rows(N)),
                     dim3(TSNE_THREADS), 0, (hipStream_t)stream, x, ldx, N, (int)L,
                     log(perplexity), beta, row_sum, steps, ratio, dist);
  SCVAE_LAUNCH_CHECK("tsne_perplexity_kernel");
  return 0;
}

int scvae_tsne_gradient(const float* x, int64_t ldx, int64_t N, int64_t L, const float* beta,
                        const float* row_sum, double sum_p, const float* y, float exaggeration,
                        float* grad, double* kl, double* grad_norm, void* workspace,
                        int64_t workspace_bytes, void* stream) {
  using namespace scvae;
  SCVAE_TSNE_SIZES(N, L);
  SCVAE_ARG(x && beta && row_sum && y && grad && workspace && ldx >= L);
  SCVAE_ARG(sum_p > 0.0 && sum_p < 1e300 && exaggeration > 0.f);
  SCVAE_ARG(((uintptr_t)workspace & 7) == 0 &&
            workspace_bytes >= scvae_tsne_workspace_bytes(N, L));
  hipStream_t st = (hipStream_t)stream;
  double* z_total = static_cast<double*>(workspace);
  double* sums = reinterpret_cast<double*>(static_cast<char*>(workspace) + TSNE_HEAD_BYTES);
  double* kl_rows = sums + TSNE_SUMS * N;
  const int chunks = ((int)L + TSNE_CHUNK - 1) / TSNE_CHUNK;
  const size_t lds =
      ((size_t)(chunks + 2) * TSNE_CHUNK * TSNE_PITCH + 3 * TSNE_EXTRA) * sizeof(float);
  const unsigned blocks = (unsigned)((N + TSNE_TILE - 1) / TSNE_TILE);
  const float inv_sum_p = (float)(1.0 / sum_p);
  SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(tsne_pair_kernel<false>), (int)lds));
  hipLaunchKernelGGL(tsne_pair_kernel<false>, dim3(blocks), dim3(TSNE_THREADS), lds, st, x, ldx,
                     N, (int)L, beta, row_sum, inv_sum_p, y, exaggeration, sums,
                     (const double*)nullptr, (double*)nullptr);
  SCVAE_LAUNCH_CHECK("tsne_pair_kernel");
  hipLaunchKernelGGL(tsne_gradient_kernel, dim3(1), dim3(TSNE_JOIN_THREADS), 0, st, sums, N,
                     grad, z_total, grad_norm);
  SCVAE_LAUNCH_CHECK("tsne_gradient_kernel");
  if (kl) {
    SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(tsne_pair_kernel<true>), (int)lds));
    hipLaunchKernelGGL(tsne_pair_kernel<true>, dim3(blocks), dim3(TSNE_THREADS), lds, st, x, ldx,
                       N, (int)L, beta, row_sum, inv_sum_p, y, exaggeration, (double*)nullptr,
                       (const double*)z_total, kl_rows);
    SCVAE_LAUNCH_CHECK("tsne_pair_kernel (KL divergence)");
    hipLaunchKernelGGL(tsne_sum_kernel, dim3(1), dim3(TSNE_JOIN_THREADS), 0, st, kl_rows, N, kl);
    SCVAE_LAUNCH_CHECK("tsne_sum_kernel");
  }
  return 0;
}

int scvae_tsne_update(float* y, float* update, float* gains, const float* grad, int64_t N,
                      float momentum, float learning_rate, float min_gain, void* stream) {
  using namespace scvae;
  SCVAE_ARG(y && update && gains && grad);
  SCVAE_ARG(N >= 1 && N <= TSNE_MAX_N);
  const int64_t elements = 2 * N;
  hipLaunchKernelGGL(tsne_update_kernel,
                     dim3((unsigned)((elements + TSNE_THREADS - 1) / TSNE_THREADS)),
                     dim3(TSNE_THREADS), 0, (hipStream_t)stream, y, update, gains, grad, elements,
                     momentum, learning_rate, min_gain);
  SCVAE_LAUNCH_CHECK("tsne_update_kernel");
  return 0;
}

}  // extern "C"
