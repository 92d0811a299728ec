// Exact silhouette values of a clustering of the latent values
// (scvae/analyses/metrics/clustering.py:120-142: the "silhouette score" of a label prediction;
// the definition is scikit-learn's silhouette_samples with the Euclidean metric), over every
// pair of cells.  X is [N, L] fp32 with row pitch ldx, its rows grouped by cluster;
// offsets[K + 1] (device int64) gives the clusters' row ranges.  1 <= L <= 256, 3 <= N < 2^31,
// 2 <= K <= N - 1.
//
//   a_i = sum_{j in A, j != i} d(i, j) / (|A| - 1)         A the cluster of i
//   b_i = min_{B != A} sum_{j in B} d(i, j) / |B|
//   s_i = (b_i - a_i) / max(a_i, b_i), 0 when |A| = 1 or max(a_i, b_i) = 0
//   d(i, j) = sqrt(sum_l (x_il - x_jl)^2), the direct form in fp32 (d(i, i) = 0 exactly, so the
//   own row needs no special case)
//
// Shape: a workgroup of 256 threads owns SIL_TILE = 64 rows i and walks all columns j in tiles
// of 64.  Both row blocks lie in LDS coordinate-major, [l][row] with a pitch of 68 floats: thread
// (ti, tj) = (t / 16, t % 16) holds the 4 x 4 pairs of rows 4 ti .. + 3 and columns 4 tj .. + 3, so
// one 16-byte LDS read of four x_i and one of four x_j serve 16 pairs per coordinate (the x_j
// reads of a wave cover 64 consecutive floats, the x_i reads are four broadcast addresses:
// no bank conflicts).  The i block is resident for the life of the workgroup; the j block comes
// in chunks of SIL_CHUNK = 32 coordinates through two LDS buffers, the global loads of the
// chunk after the next in flight in registers while this one is used.
//
// Because the rows are grouped, the columns pass cluster by cluster: every row keeps one running
// fp64 sum for the cluster the walk is in, and closes it at the cluster's end into a (its own
// cluster) or into the running minimum b.  A cluster may end anywhere inside a column tile, and
// the 64 rows of a block may belong to different clusters: a tile is cut into the segments of
// the clusters it meets, and "own cluster" is decided per row.
//
// Summation order (no floating-point atomics; the same inputs give the same bits): within one
// tile segment a row's distances are added in fp32 -- a thread's 4 columns in order, then a
// 4-level xor tree over the 16 threads of the row -- at most T = SIL_TILE = 64 non-negative
// terms, 7 additions deep.  Segments and tiles are joined in fp64, in column order.
#include "../../include/scvae_hip.h"
#include "common.hpp"

namespace scvae {
namespace {

constexpr int SIL_THREADS = 256;
constexpr int SIL_TILE = 64;    // rows of a block, columns of a tile; T, the longest fp32 sum
constexpr int SIL_PITCH = 68;   // floats per coordinate in LDS: 16-byte aligned, off the banks
constexpr int SIL_CHUNK = 32;   // coordinates of the j tile in LDS at a time
constexpr int SIL_LOADS = SIL_TILE * SIL_CHUNK / SIL_THREADS;  // per thread and chunk
constexpr int SIL_MAX_L = 256;

typedef float sil_f2 __attribute__((ext_vector_type(2)));

// rows [r0, r0 + 64) x coordinates [l0, l0 + 32) of x into registers: lane l = t % 32 takes
// coordinate l0 + l of rows t / 32, t / 32 + 8, ...; rows >= N and coordinates >= L read as 0
__device__ __forceinline__ void sil_fetch(const float* __restrict__ x, int64_t ldx, int64_t N,
                                          int L, int64_t r0, int l0, float* v) {
  const int l = l0 + (threadIdx.x & (SIL_CHUNK - 1));
  const int64_t r = r0 + (threadIdx.x / SIL_CHUNK);
#pragma unroll
  for (int u = 0; u < SIL_LOADS; ++u) {
    const int64_t row = r + u * (SIL_THREADS / SIL_CHUNK);
    v[u] = (l < L && row < N) ? x[row * ldx + l] : 0.f;
  }
}
// ... and into LDS, dst[l][row] with l counted from the chunk's first coordinate
__device__ __forceinline__ void sil_store(const float* v, float* dst) {
  float* p = dst + (threadIdx.x & (SIL_CHUNK - 1)) * SIL_PITCH + threadIdx.x / SIL_CHUNK;
#pragma unroll
  for (int u = 0; u < SIL_LOADS; ++u) p[u * (SIL_THREADS / SIL_CHUNK)] = v[u];
}

// sqrt of v >= 0 to 1 ulp; the hardware instruction takes no denormal input, so tiny squares
// are scaled up by 2^64 and their roots down by 2^32
__device__ __forceinline__ float sil_sqrt(float v) {
  const bool tiny = v < 0x1p-96f;
  const float r = __builtin_amdgcn_sqrtf(tiny ? v * 0x1p+64f : v);
  return tiny ? r * 0x1p-32f : r;
}

template <int CTRL>
__device__ __forceinline__ float sil_dpp(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// the sum of v over the 16 lanes of a DPP row (the 16 tj of one ti), the same bits in every
// lane: neighbours (quad_perm [1,0,3,2]), pairs ([2,3,0,1]), then the two quads of a half
// (row_half_mirror) and the two halves (row_mirror).  Both partners of every step add the same
// two numbers.
__device__ __forceinline__ float sil_row_sum(float v) {
  v += sil_dpp<0xB1>(v);
  v += sil_dpp<0x4E>(v);
  v += sil_dpp<0x141>(v);
  v += sil_dpp<0x140>(v);
  return v;
}

// the cluster of row i: the c with offsets[c] <= i < offsets[c + 1] (0 <= c < K whatever the
// offsets hold)
__device__ __forceinline__ int sil_cluster_of(const int64_t* __restrict__ offsets, int K,
                                              int64_t i) {
  int lo = 0, hi = K - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// dynamic LDS: the i block [L rounded up to 32][68], two j chunks [32][68]
__global__ __launch_bounds__(SIL_THREADS) void silhouette_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, int L,
    const int64_t* __restrict__ offsets, int K, float* __restrict__ a_out,
    float* __restrict__ b_out, float* __restrict__ s_out, float* __restrict__ s_keep) {
  extern __shared__ __align__(16) float sil_lds[];
  const int chunks = (L + SIL_CHUNK - 1) / SIL_CHUNK;
  float* xi = sil_lds;
  float* xj = xi + (size_t)chunks * SIL_CHUNK * SIL_PITCH;
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const int64_t i0 = (int64_t)blockIdx.x * SIL_TILE;
  const int64_t tiles = (N + SIL_TILE - 1) / SIL_TILE;

  float v[SIL_LOADS];
  for (int ch = 0; ch < chunks; ++ch) {
    sil_fetch(x, ldx, N, L, i0, ch * SIL_CHUNK, v);
    sil_store(v, xi + (size_t)ch * SIL_CHUNK * SIL_PITCH);
  }
  // per row of the block, kept by the row's first thread (tj = 0) in LDS -- they are touched
  // only where a cluster ends, and registers are what bounds the waves on a SIMD: the row's
  // cluster, a, and the running minimum b
  __shared__ int own[SIL_TILE];
  __shared__ double a[SIL_TILE], b[SIL_TILE];
  double run[4];    // a row's distance sum over the cluster the walk is in (the same in all tj)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = i0 + 4 * ti + r;
    if (tj == 0) {
      own[4 * ti + r] = sil_cluster_of(offsets, K, row < N ? row : N - 1);
      a[4 * ti + r] = 0.0, b[4 * ti + r] = INFINITY;
    }
    run[r] = 0.0;
  }

  // The j chunks pass through two LDS buffers in turn: step k = (tile, chunk) reads buffer k & 1
  // while the chunk of step k + 1 is stored into the other one and the chunk of step k + 2 is
  // fetched into registers -- one barrier a step.  (A fetch past the last row reads nothing.)
  constexpr int BUFFER = SIL_CHUNK * SIL_PITCH;
  sil_fetch(x, ldx, N, L, 0, 0, v);
  sil_store(v, xj);
  if (chunks > 1) sil_fetch(x, ldx, N, L, 0, SIL_CHUNK, v);
  else sil_fetch(x, ldx, N, L, SIL_TILE, 0, v);
  __syncthreads();  // the i block, step 0's chunk, own / a / b
  int step = 0;

  int c = 0;                      // the cluster the walk is in, and where it ends
  int64_t c_begin = 0, c_end = offsets[1];
  for (int64_t t = 0; t < tiles; ++t) {
    const int64_t j0 = t * SIL_TILE;
    sil_f2 acc[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r][0] = acc[r][1] = sil_f2{0.f, 0.f};
    for (int ch = 0; ch < chunks; ++ch, ++step) {
      sil_store(v, xj + ((step + 1) & 1) * BUFFER);
      {
        int ch2 = ch + 2;
        int64_t t2 = t;
        if (ch2 >= chunks) ch2 -= chunks, ++t2;
        if (ch2 >= chunks) ch2 -= chunks, ++t2;
        sil_fetch(x, ldx, N, L, t2 * SIL_TILE, ch2 * SIL_CHUNK, v);
      }
      const int lc = L - ch * SIL_CHUNK < SIL_CHUNK ? L - ch * SIL_CHUNK : SIL_CHUNK;
      const float* pi = xi + (size_t)ch * SIL_CHUNK * SIL_PITCH + 4 * ti;
      const float* pj = xj + (step & 1) * BUFFER + 4 * tj;
      // the reads of coordinate l + 1 are in flight while l is used
      float4 p = *reinterpret_cast<const float4*>(pi);
      float4 q = *reinterpret_cast<const float4*>(pj);
#pragma unroll 2
      for (int l = 0; l < lc; ++l) {
        const int next = (l + 1 < lc ? l + 1 : l) * SIL_PITCH;
        const float4 p_next = *reinterpret_cast<const float4*>(pi + next);
        const float4 q_next = *reinterpret_cast<const float4*>(pj + next);
        const sil_f2 q01 = {q.x, q.y}, q23 = {q.z, q.w};
        const float pr[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const sil_f2 pp = {pr[r], pr[r]};
          const sil_f2 d0 = pp - q01, d1 = pp - q23;
          acc[r][0] = __builtin_elementwise_fma(d0, d0, acc[r][0]);
          acc[r][1] = __builtin_elementwise_fma(d1, d1, acc[r][1]);
        }
        p = p_next, q = q_next;
      }
      __syncthreads();  // the next step's chunk is stored; this one's readers are done
    }
    float d[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      d[r][0] = sil_sqrt(acc[r][0].x), d[r][1] = sil_sqrt(acc[r][0].y);
      d[r][2] = sil_sqrt(acc[r][1].x), d[r][3] = sil_sqrt(acc[r][1].y);
    }

    // the segments [from, to) of this tile, one per cluster it meets
    const int64_t tile_end = j0 + SIL_TILE < N ? j0 + SIL_TILE : N;
    int64_t from = j0;
    while (from < tile_end) {
      int64_t to = c_end < tile_end ? c_end : tile_end;
      if (to < from) to = from;
      if (to - from == SIL_TILE) {  // the whole tile lies in one cluster
#pragma unroll
        for (int r = 0; r < 4; ++r)
          run[r] += (double)sil_row_sum(((d[r][0] + d[r][1]) + d[r][2]) + d[r][3]);
      } else {  // (adding the + 0 of a column outside the segment changes nothing)
        const int lo = (int)(from - j0) - 4 * tj, hi = (int)(to - j0) - 4 * tj;  // q in [lo, hi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float part = (0 >= lo && 0 < hi) ? d[r][0] : 0.f;
#pragma unroll
          for (int q = 1; q < 4; ++q) part += (q >= lo && q < hi) ? d[r][q] : 0.f;
          run[r] += (double)sil_row_sum(part);
        }
      }
      from = to;
      if (c_end <= from) {  // the cluster ends here
        const double count = (double)(c_end - c_begin);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (tj == 0) {
            const int at = 4 * ti + r;
            if (c == own[at]) a[at] = count > 1.0 ? run[r] / (count - 1.0) : 0.0;
            else if (count > 0.0) b[at] = fmin(b[at], run[r] / count);
          }
          run[r] = 0.0;
        }
        if (c + 1 >= K) break;  // (offsets that do not end at N: nothing further to add)
        ++c;
        c_begin = c_end;
        c_end = c + 1 < K ? offsets[c + 1] : N;
        if (c_end > N) c_end = N;
      }
    }
  }

  if (tj == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = i0 + 4 * ti + r;
      if (row < N) {
        const int k = own[4 * ti + r];
        const int64_t members = (k + 1 < K ? offsets[k + 1] : N) - offsets[k];
        const double ar = a[4 * ti + r], br = b[4 * ti + r];
        const double m = fmax(ar, br);
        const float s = (members == 1 || m == 0.0) ? 0.f : (float)((br - ar) / m);
        if (a_out) a_out[row] = (float)ar;
        if (b_out) b_out[row] = (float)br;
        if (s_out) s_out[row] = s;
        s_keep[row] = s;
      }
    }
  }
}

// *score = sum of s[0 .. N) / N in fp64: thread t adds t, t + 256, ... and a binary tree joins the
// threads
__global__ __launch_bounds__(SIL_THREADS) void silhouette_mean_kernel(const float* __restrict__ s,
                                                                      int64_t N,
                                                                      double* __restrict__ score) {
  __shared__ double red[SIL_THREADS];
  double sum = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += SIL_THREADS) sum += (double)s[i];
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int off = SIL_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *score = red[0] / (double)N;
}

}  // namespace
}  // namespace scvae

#define SCVAE_SILHOUETTE_SIZES(N, L, K)              \
  SCVAE_ARG(L >= 1 && L <= scvae::SIL_MAX_L);        \
  SCVAE_ARG(N >= 3 && N < ((int64_t)1 << 31));       \
  SCVAE_ARG(K >= 2);                                 \
  SCVAE_ARG(K <= N - 1)

extern "C" {

// s of every row, for the mean
int64_t scvae_silhouette_workspace_bytes(int64_t N, int64_t L, int64_t K) {
  SCVAE_SILHOUETTE_SIZES(N, L, K);
  return (4 * N + 7) / 8 * 8;
}

int scvae_silhouette_samples(const float* x, int64_t ldx, int64_t N, int64_t L,
                             const int64_t* offsets, int64_t K, float* a, float* b, float* s,
                             double* score, void* workspace, int64_t workspace_bytes,
                             void* stream) {
  using namespace scvae;
  SCVAE_SILHOUETTE_SIZES(N, L, K);
  SCVAE_ARG(x && offsets && score && workspace && ldx >= L);
  SCVAE_ARG(((uintptr_t)workspace & 7) == 0 &&
            workspace_bytes >= scvae_silhouette_workspace_bytes(N, L, K));
  hipStream_t st = (hipStream_t)stream;
  float* s_keep = static_cast<float*>(workspace);
  const int chunks = ((int)L + SIL_CHUNK - 1) / SIL_CHUNK;
  const size_t lds = (size_t)(chunks + 2) * SIL_CHUNK * SIL_PITCH * 4;
  const int64_t blocks = (N + SIL_TILE - 1) / SIL_TILE;
  SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(silhouette_kernel), (int)lds));
  hipLaunchKernelGGL(silhouette_kernel, dim3((unsigned)blocks), dim3(SIL_THREADS), lds, st, x, ldx,
                     N, (int)L, offsets, (int)K, a, b, s, s_keep);
  SCVAE_LAUNCH_CHECK("silhouette_kernel");
  hipLaunchKernelGGL(silhouette_mean_kernel, dim3(1), dim3(SIL_THREADS), 0, st, s_keep, N, score);
  SCVAE_LAUNCH_CHECK("silhouette_mean_kernel");
  return 0;
}

}  // extern "C"
