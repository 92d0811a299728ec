// k-means over the latent values (scvae/analyses/prediction.py:33-131: the clustering behind
// `scvae evaluate -P k-means`), as exact Lloyd passes on the device.  X is [N, L] fp32 with row
// pitch ldx, the centres are [K, L] fp32, labels int32; 1 <= K <= 256, 1 <= L <= 256,
// K L <= 8192, K <= N < 2^31.  Three passes, each with a C entry at the bottom of this file:
//
//   assign         labels[i] = argmin_k sum_l (x_il - c_kl)^2 in the direct form, fp32, lowest k on
//                  equal distances; optional min_d2[N]; the inertia as one fp64.
//   update         per-cluster counts and fp64 coordinate sums over fixed ranges of KM_RANGE rows,
//                  one workgroup a range, reduced in a fixed order; new centres sum / count rounded
//                  to fp32 once; an empty cluster keeps its centre; counts[K] and the squared
//                  centre shift as one fp64.
//   min_d2_update  min_d2[i] = min(min_d2[i], |x_i - x_j|^2), the pass k-means++ makes per centre.
//
// No floating-point atomics anywhere: every sum has one order, a function of the sizes alone, so
// the same inputs give the same bits on every run.
//
// Shape of assign and min_d2_update: a workgroup of four waves walks tiles of 64 rows.  A tile is
// read from global memory as one contiguous block (coalesced whatever L is) into LDS with an odd
// row pitch, then lane r of every wave owns row r: reading its row from LDS is conflict-free and
// the centre values are one broadcast address per wave.  The four waves split the centres in
// groups of KB (assign) or the coordinates in quarters (min_d2_update); KB centres share each x
// value read.  The centres stay in LDS for the life of the workgroup.
#include <limits.h>

#include "../../include/scvae_hip.h"
#include "common.hpp"

namespace scvae {
namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_TILE = 64;             // rows of a tile: a lane per row
constexpr int KM_MAX_K = 256, KM_MAX_L = 256, KM_MAX_KL = 8192;
constexpr int KM_ASSIGN_BLOCKS = 1024;  // inertia partials: one per workgroup, summed in order
constexpr int KM_TILE_BLOCKS = 2048;
constexpr int KM_RANGE = 1024;          // rows of one update workgroup
constexpr int KM_SLOT_DOUBLES = 8192;   // 64 KB of fp64 accumulators a workgroup
constexpr int KM_ROWS_AHEAD = 16;       // loads in flight per thread in the update
constexpr int KM_LOADS_AHEAD = 16;      // and in the staging of a tile
constexpr int KM_REDUCE_E = 16, KM_REDUCE_Q = 16;

// rows [r0, r0 + nr) of x -> xs[r * LS + l].  Thread t takes elements t, t + 256, ... of the
// block; (row, column) advance by (256 / L, 256 % L) per step, so the loop divides nothing.
// KM_LOADS_AHEAD loads are issued before the first of them is stored to LDS: the pass is
// bound by memory latency, not by instructions.
__device__ __forceinline__ void km_load_tile(const float* __restrict__ x, int64_t ldx, int64_t r0,
                                             int nr, int L, int LS, int r_first, int l_first,
                                             float* xs) {
  const int total = nr * L;
  const int dq = KM_THREADS / L, dm = KM_THREADS - dq * L;
  const float* xb = x + r0 * ldx;
  int r = r_first, l = l_first;
  for (int base = threadIdx.x; base < total; base += KM_THREADS * KM_LOADS_AHEAD) {
    float v[KM_LOADS_AHEAD];
    int at[KM_LOADS_AHEAD];
#pragma unroll
    for (int u = 0; u < KM_LOADS_AHEAD; ++u) {
      const bool on = base + u * KM_THREADS < total;
      v[u] = on ? xb[(int64_t)r * ldx + l] : 0.f;
      at[u] = on ? r * LS + l : -1;
      l += dm;
      r += dq;
      if (l >= L) {
        l -= L;
        ++r;
      }
    }
#pragma unroll
    for (int u = 0; u < KM_LOADS_AHEAD; ++u)
      if (at[u] >= 0) xs[at[u]] = v[u];
  }
}

__device__ __forceinline__ double km_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// LDS: centres [G][L][KS] (group g, slot j = centre g KB + j; unused slots 0), the tile
// [64][L | 1], and the four waves' best (distance, centre) per row.
template <int KB>
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, int L, const float* __restrict__ centres,
    int K, int G, int32_t* __restrict__ labels, float* __restrict__ min_d2,
    double* __restrict__ partial) {
  constexpr int KS = KB <= 4 ? 4 : 8;
  extern __shared__ __align__(16) float km_lds[];
  const int LS = L | 1;
  float* cs = km_lds;
  float* xs = cs + (size_t)G * L * KS;
  float* bd = xs + KM_TILE * LS;
  int* bk = reinterpret_cast<int*>(bd + 4 * KM_TILE);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r_first = threadIdx.x / L, l_first = threadIdx.x - r_first * L;

  for (int idx = threadIdx.x; idx < G * L * KS; idx += KM_THREADS) {
    const int j = idx % KS, gl = idx / KS;
    const int l = gl % L, k = (gl / L) * KB + j;
    cs[idx] = (j < KB && k < K) ? centres[k * L + l] : 0.f;
  }

  const int64_t tiles = (N + KM_TILE - 1) / KM_TILE;
  double inertia = 0.0;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r0 = t * KM_TILE;
    const int nr = (int)((N - r0) < KM_TILE ? (N - r0) : KM_TILE);
    __syncthreads();  // the centres (first tile); the last tile's readers
    km_load_tile(x, ldx, r0, nr, L, LS, r_first, l_first, xs);
    __syncthreads();
    float best = INFINITY;
    int best_k = INT_MAX;
    if (lane < nr) {
      const float* xr = xs + lane * LS;
      for (int g = w; g < G; g += 4) {
        float acc[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) acc[j] = 0.f;
        const float4* cg = reinterpret_cast<const float4*>(cs + (size_t)g * L * KS);
#pragma unroll 4
        for (int l = 0; l < L; ++l) {
          const float xv = xr[l];
          float c[KS];
#pragma unroll
          for (int q = 0; q < KS / 4; ++q) {
            const float4 v = cg[l * (KS / 4) + q];
            c[4 * q] = v.x, c[4 * q + 1] = v.y, c[4 * q + 2] = v.z, c[4 * q + 3] = v.w;
          }
#pragma unroll
          for (int j = 0; j < KB; ++j) {
            const float d = xv - c[j];
            acc[j] = fmaf(d, d, acc[j]);
          }
        }
        // ascending k, strict <: the lowest index of equal distances within this wave
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          const int k = g * KB + j;
          if (k < K && (best_k == INT_MAX || acc[j] < best)) best = acc[j], best_k = k;
        }
      }
    }
    bd[w * KM_TILE + lane] = best;
    bk[w * KM_TILE + lane] = best_k;
    __syncthreads();
    if (w == 0 && lane < nr) {  // (wave 0 holds centre 0: best_k is a centre)
#pragma unroll
      for (int o = 1; o < 4; ++o) {
        const float d = bd[o * KM_TILE + lane];
        const int k = bk[o * KM_TILE + lane];
        if (k != INT_MAX && (d < best || (d == best && k < best_k))) best = d, best_k = k;
      }
      labels[r0 + lane] = best_k;
      if (min_d2) min_d2[r0 + lane] = best;
      inertia += (double)best;
    }
  }
  if (w == 0) {
    inertia = km_wave_sum(inertia);
    if (lane == 0) partial[blockIdx.x] = inertia;
  }
}

// *out = sum of partial[0 .. n): thread t adds t, t + 256, ... and a binary tree joins the threads
__global__ __launch_bounds__(KM_THREADS) void kmeans_sum_kernel(const double* __restrict__ partial,
                                                                int n, double* __restrict__ out) {
  __shared__ double red[KM_THREADS];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += KM_THREADS) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = KM_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
}

// LDS: x_j [L], the tile [64][L | 1], the four waves' partial sums per row
__global__ __launch_bounds__(KM_THREADS) void kmeans_min_d2_kernel(const float* __restrict__ x,
                                                                   int64_t ldx, int64_t N, int L,
                                                                   int64_t row_j,
                                                                   float* __restrict__ min_d2) {
  extern __shared__ __align__(16) float km_lds[];
  const int LS = L | 1;
  float* xj = km_lds;
  float* xs = xj + LS;
  float* part = xs + KM_TILE * LS;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r_first = threadIdx.x / L, l_first = threadIdx.x - r_first * L;
  for (int l = threadIdx.x; l < L; l += KM_THREADS) xj[l] = x[row_j * ldx + l];
  const int lc = (L + 3) / 4;
  const int l0 = w * lc < L ? w * lc : L, l1 = l0 + lc < L ? l0 + lc : L;
  const int64_t tiles = (N + KM_TILE - 1) / KM_TILE;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r0 = t * KM_TILE;
    const int nr = (int)((N - r0) < KM_TILE ? (N - r0) : KM_TILE);
    __syncthreads();
    km_load_tile(x, ldx, r0, nr, L, LS, r_first, l_first, xs);
    __syncthreads();
    float acc = 0.f;
    if (lane < nr) {
      const float* xr = xs + lane * LS;
#pragma unroll 4
      for (int l = l0; l < l1; ++l) {
        const float d = xr[l] - xj[l];
        acc = fmaf(d, d, acc);
      }
    }
    part[w * KM_TILE + lane] = acc;
    __syncthreads();
    if (w == 0 && lane < nr) {
      const float d = ((part[lane] + part[KM_TILE + lane]) + part[2 * KM_TILE + lane]) +
                      part[3 * KM_TILE + lane];
      min_d2[r0 + lane] = fminf(min_d2[r0 + lane], d);
    }
  }
}

// One workgroup a range of KM_RANGE rows.  Thread (s, l) = (t / L, t % L), s < S, adds column l
// of rows s, s + S, ... of the range, in that order, into its own fp64 cells acc[s][label][l]:
// no two threads share a cell, so nothing needs an atomic.  The S slots are then added in order.
// psums[range][K L + K]: the coordinate sums, then the counts (exact as fp64).  A label outside
// [0, K) contributes nothing.
__global__ __launch_bounds__(KM_THREADS) void kmeans_partial_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, int L, const int32_t* __restrict__ labels,
    int K, int S, double* __restrict__ psums) {
  extern __shared__ __align__(16) double km_acc[];
  const int KL = K * L;
  double* acc = km_acc;
  int* lbl = reinterpret_cast<int*>(acc + (size_t)S * KL);
  int* cnt = lbl + KM_RANGE;
  for (int i = threadIdx.x; i < S * KL; i += KM_THREADS) acc[i] = 0.0;
  for (int i = threadIdx.x; i < K; i += KM_THREADS) cnt[i] = 0;
  const int64_t r0 = (int64_t)blockIdx.x * KM_RANGE;
  const int nr = (int)((N - r0) < KM_RANGE ? (N - r0) : KM_RANGE);
  for (int i = threadIdx.x; i < nr; i += KM_THREADS) lbl[i] = labels[r0 + i];
  __syncthreads();
  for (int i = threadIdx.x; i < nr; i += KM_THREADS) {  // integer adds: exact in any order
    const int k = lbl[i];
    if ((unsigned)k < (unsigned)K) atomicAdd(&cnt[k], 1);
  }
  const int s = threadIdx.x / L, l = threadIdx.x - s * L;
  if (s < S) {
    double* a = acc + (size_t)s * KL + l;
    const float* xp = x + r0 * ldx + l;
    // the loads of the next KM_ROWS_AHEAD rows are in flight while this batch is added
    float v[KM_ROWS_AHEAD], v_next[KM_ROWS_AHEAD];
    int kk[KM_ROWS_AHEAD], kk_next[KM_ROWS_AHEAD];
    auto fetch = [&](int j, float* vv, int* kv) {
#pragma unroll
      for (int u = 0; u < KM_ROWS_AHEAD; ++u) {
        const int r = j + u * S;
        const bool on = r < nr;
        vv[u] = on ? xp[(int64_t)r * ldx] : 0.f;
        kv[u] = on ? lbl[r] : -1;
      }
    };
    fetch(s, v, kk);
    for (int j = s; j < nr; j += KM_ROWS_AHEAD * S) {
      fetch(j + KM_ROWS_AHEAD * S, v_next, kk_next);
#pragma unroll
      for (int u = 0; u < KM_ROWS_AHEAD; ++u)
        if ((unsigned)kk[u] < (unsigned)K) a[kk[u] * L] += (double)v[u];
#pragma unroll
      for (int u = 0; u < KM_ROWS_AHEAD; ++u) v[u] = v_next[u], kk[u] = kk_next[u];
    }
  }
  __syncthreads();
  double* out = psums + (size_t)blockIdx.x * (KL + K);
  for (int e = threadIdx.x; e < KL; e += KM_THREADS) {
    double t = acc[e];
    for (int o = 1; o < S; ++o) t += acc[(size_t)o * KL + e];
    out[e] = t;
  }
  for (int k = threadIdx.x; k < K; k += KM_THREADS) out[KL + k] = (double)cnt[k];
}

// sums[e] = sum over the ranges of psums[range][e], E = K L + K elements.  Thread (q, e) adds
// ranges q, q + 16, ... in order; the 16 q of an element are then added in order.
__global__ __launch_bounds__(KM_THREADS) void kmeans_reduce_kernel(
    const double* __restrict__ psums, int ranges, int E, double* __restrict__ sums) {
  __shared__ double red[KM_REDUCE_Q][KM_REDUCE_E];
  const int el = threadIdx.x % KM_REDUCE_E, q = threadIdx.x / KM_REDUCE_E;
  const int e = blockIdx.x * KM_REDUCE_E + el;
  double s = 0.0;
  if (e < E) {
#pragma unroll 4
    for (int r = q; r < ranges; r += KM_REDUCE_Q) s += psums[(size_t)r * E + e];
  }
  red[q][el] = s;
  __syncthreads();
  if (q == 0 && e < E) {
    double t = red[0][el];
#pragma unroll
    for (int o = 1; o < KM_REDUCE_Q; ++o) t += red[o][el];
    sums[e] = t;
  }
}

// new centre = fp32(sum / count), the old one where count = 0; counts; the squared shift.
// `centres` and `new_centres` may be the same array (every element is read, then written, by
// one thread).
__global__ __launch_bounds__(KM_THREADS) void kmeans_finish_kernel(
    const double* __restrict__ sums, const float* centres, int K, int L, float* new_centres,
    int32_t* __restrict__ counts, double* __restrict__ shift) {
  __shared__ double red[KM_THREADS];
  const int KL = K * L;
  double sh = 0.0;
  for (int e = threadIdx.x; e < KL; e += KM_THREADS) {
    const double n = sums[KL + e / L];
    const float c_old = centres[e];
    const float c_new = n > 0.0 ? (float)(sums[e] / n) : c_old;
    new_centres[e] = c_new;
    const double d = (double)c_new - (double)c_old;
    sh += d * d;
  }
  for (int k = threadIdx.x; k < K; k += KM_THREADS) counts[k] = (int32_t)sums[KL + k];
  red[threadIdx.x] = sh;
  __syncthreads();
  for (int off = KM_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *shift = red[0];
}

// centres of one group: the width that leaves the fewest idle slots over four waves, counting
// 4 KB cycles of arithmetic and 6 of LDS reads per coordinate of a group
int km_group_width(int K) {
  int best = 1, best_cost = INT_MAX;
  for (int kb = 1; kb <= 8; ++kb) {
    const int G = (K + kb - 1) / kb;
    const int cost = ((G + 3) / 4) * (4 * kb + 6);
    if (cost <= best_cost) best = kb, best_cost = cost;
  }
  return best;
}

int64_t km_ranges(int64_t N) { return (N + KM_RANGE - 1) / KM_RANGE; }

template <int KB>
int km_launch_assign(hipStream_t s, const float* x, int64_t ldx, int64_t N, int L,
                     const float* centres, int K, int32_t* labels, float* min_d2,
                     double* partial, int blocks) {
  constexpr int KS = KB <= 4 ? 4 : 8;
  const int G = (K + KB - 1) / KB;
  const size_t lds = ((size_t)G * L * KS + (size_t)KM_TILE * (L | 1) + 8 * KM_TILE) * 4;
  auto kfn = kmeans_assign_kernel<KB>;
  SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(kfn), (int)lds));
  hipLaunchKernelGGL(kfn, dim3(blocks), dim3(KM_THREADS), lds, s, x, ldx, N, L, centres, K, G,
                     labels, min_d2, partial);
  SCVAE_LAUNCH_CHECK("kmeans_assign_kernel");
  return 0;
}

}  // namespace
}  // namespace scvae

#define SCVAE_KMEANS_SIZES(N, L, K)                  \
  SCVAE_ARG(N >= 1 && N < ((int64_t)1 << 31));       \
  SCVAE_ARG(L >= 1 && L <= scvae::KM_MAX_L);         \
  SCVAE_ARG(K >= 1 && K <= scvae::KM_MAX_K);         \
  SCVAE_ARG(K * L <= scvae::KM_MAX_KL);              \
  SCVAE_ARG(K <= N)

extern "C" {

int64_t scvae_kmeans_workspace_bytes(int64_t N, int64_t L, int64_t K) {
  SCVAE_KMEANS_SIZES(N, L, K);
  return 8 * (scvae::KM_ASSIGN_BLOCKS + (scvae::km_ranges(N) + 1) * (K * L + K));
}

int scvae_kmeans_assign(const float* x, int64_t ldx, int64_t N, int64_t L, const float* centres,
                        int64_t K, int32_t* labels, float* min_d2, double* inertia,
                        void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace scvae;
  SCVAE_KMEANS_SIZES(N, L, K);
  SCVAE_ARG(x && centres && labels && inertia && workspace && ldx >= L);
  SCVAE_ARG(((uintptr_t)workspace & 7) == 0 &&
            workspace_bytes >= scvae_kmeans_workspace_bytes(N, L, K));
  hipStream_t s = (hipStream_t)stream;
  double* partial = static_cast<double*>(workspace);
  const int64_t tiles = (N + KM_TILE - 1) / KM_TILE;
  const int blocks = (int)(tiles < KM_ASSIGN_BLOCKS ? tiles : KM_ASSIGN_BLOCKS);
  int rc = 0;
  switch (km_group_width((int)K)) {
#define SCVAE_KM_CASE(KB)                                                                    \
  case KB:                                                                                   \
    rc = km_launch_assign<KB>(s, x, ldx, N, (int)L, centres, (int)K, labels, min_d2, partial, \
                              blocks);                                                       \
    break;
    SCVAE_KM_CASE(1) SCVAE_KM_CASE(2) SCVAE_KM_CASE(3) SCVAE_KM_CASE(4)
    SCVAE_KM_CASE(5) SCVAE_KM_CASE(6) SCVAE_KM_CASE(7) SCVAE_KM_CASE(8)
#undef SCVAE_KM_CASE
  }
  if (rc) return rc;
  hipLaunchKernelGGL(kmeans_sum_kernel, dim3(1), dim3(KM_THREADS), 0, s, partial, blocks, inertia);
  SCVAE_LAUNCH_CHECK("kmeans_sum_kernel");
  return 0;
}

int scvae_kmeans_update(const float* x, int64_t ldx, int64_t N, int64_t L, const int32_t* labels,
                        const float* centres, int64_t K, float* new_centres, int32_t* counts,
                        double* shift, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace scvae;
  SCVAE_KMEANS_SIZES(N, L, K);
  SCVAE_ARG(x && labels && centres && new_centres && counts && shift && workspace && ldx >= L);
  SCVAE_ARG(((uintptr_t)workspace & 7) == 0 &&
            workspace_bytes >= scvae_kmeans_workspace_bytes(N, L, K));
  hipStream_t s = (hipStream_t)stream;
  const int KL = (int)(K * L), E = KL + (int)K;
  const int ranges = (int)km_ranges(N);
  double* psums = static_cast<double*>(workspace) + KM_ASSIGN_BLOCKS;
  double* sums = psums + (size_t)ranges * E;
  // accumulator slots: as many rows at once as 256 threads and 64 KB of fp64 cells hold
  int S = KM_THREADS / (int)L;
  if (S > KM_SLOT_DOUBLES / KL) S = KM_SLOT_DOUBLES / KL;
  const size_t lds = (size_t)S * KL * 8 + (KM_RANGE + (size_t)K) * 4;
  SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(kmeans_partial_kernel), (int)lds));
  hipLaunchKernelGGL(kmeans_partial_kernel, dim3(ranges), dim3(KM_THREADS), lds, s, x, ldx, N,
                     (int)L, labels, (int)K, S, psums);
  SCVAE_LAUNCH_CHECK("kmeans_partial_kernel");
  hipLaunchKernelGGL(kmeans_reduce_kernel, dim3((E + KM_REDUCE_E - 1) / KM_REDUCE_E),
                     dim3(KM_THREADS), 0, s, psums, ranges, E, sums);
  SCVAE_LAUNCH_CHECK("kmeans_reduce_kernel");
  hipLaunchKernelGGL(kmeans_finish_kernel, dim3(1), dim3(KM_THREADS), 0, s, sums, centres, (int)K,
                     (int)L, new_centres, counts, shift);
  SCVAE_LAUNCH_CHECK("kmeans_finish_kernel");
  return 0;
}

int scvae_kmeans_min_d2_update(const float* x, int64_t ldx, int64_t N, int64_t L, int64_t j,
                               float* min_d2, void* stream) {
  using namespace scvae;
  SCVAE_ARG(N >= 1 && N < ((int64_t)1 << 31));
  SCVAE_ARG(L >= 1 && L <= scvae::KM_MAX_L);
  SCVAE_ARG(x && min_d2 && ldx >= L && j >= 0 && j < N);
  const int64_t tiles = (N + KM_TILE - 1) / KM_TILE;
  const int blocks = (int)(tiles < KM_TILE_BLOCKS ? tiles : KM_TILE_BLOCKS);
  const size_t lds = ((size_t)(KM_TILE + 1) * (L | 1) + 4 * KM_TILE) * 4;
  SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(kmeans_min_d2_kernel), (int)lds));
  hipLaunchKernelGGL(kmeans_min_d2_kernel, dim3(blocks), dim3(KM_THREADS), lds,
                     (hipStream_t)stream, x, ldx, N, (int)L, j, min_d2);
  SCVAE_LAUNCH_CHECK("kmeans_min_d2_kernel");
  return 0;
}

}  // extern "C"
