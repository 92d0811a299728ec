// Silhouette values of a clustering in COUNT space (scvae/analyses/metrics/clustering.py:120-142
// hands the cells x genes matrix to scikit-learn's silhouette_samples, Euclidean): exact pairwise
// distances between count rows on the matrix cores, then a, b and s from strips of them.
//
// X is [N, F] uint16 counts with row pitch ldx in the layout of scvae_csr_densify_u16: pitch a
// multiple of 8 and at least Fp = F rounded up to 64, pad columns zero, 16-byte aligned base.
// Rows are grouped by cluster, offsets[K + 1] (device int64) as for scvae_silhouette_samples.
// 1 <= F <= 65 536, 3 <= N <= 2^20, 2 <= K <= N - 1.
//
// Why d2(i, j) = sum_g (x_ig - x_jg)^2 is EXACT.  Shift every count by c = 32 896 = 128 * 257:
// y = x - c lies in [-32 896, 32 639] and y = 256 h + l with the two signed bytes
// h = (x >> 8) - 128 and l = (x & 255) - 128, both in [-128, 127]: the bytes of x with their top
// bit flipped, read as int8.  The shift cancels in a difference, so
//     d2(i, j) = m_i + m_j - 2 G_ij,   m_i = sum_g y_ig^2,   G_ij = sum_g y_ig y_jg
//     G_ij = LL + 256 (LH + HL) + 65 536 HH,   LL = sum_g l_ig l_jg, LH = sum_g l_ig h_jg, ...
// over all Fp genes (a pad column is x = 0, y = -c on both sides: it adds the same to m_i + m_j
// and to 2 G_ij).  The four byte products run on v_mfma_i32_32x32x32_i8 with int32 accumulators:
// |l l'| <= 128^2 = 2^14 and Fp <= 2^16, so every partial sum of LL, LH, HL, HH is at most 2^30 in
// magnitude and no int32 accumulation overflows, in any order.  (LH and HL keep an accumulator
// each: their sum could reach 2^31.)  m_i <= 2^16 * 32 896^2 < 2^47 and |G_ij| < 2^47 are put
// together in int64.  Integer arithmetic throughout: no rounding anywhere before the root, no
// atomics, the same bits on every run, and d2(i, j) = d2(j, i) = 0 exactly for equal rows.
//
// d(i, j) = (float)sqrt((double)d2): d2 < 2^50 converts exactly, the fp64 root is within 2^-52
// relative and the one rounding to fp32 within 2^-24: |d - sqrt(d2)| <= (2^-24 + 2^-51) sqrt(d2),
// and d = 0 if and only if d2 = 0.  Both d(i, j) and d(j, i) take the same route from the same
// integer: they are equal bit for bit.
//
// Shape of the distance kernel: a workgroup of 512 threads owns a [128 rows i] x [128 columns j]
// tile of the strip and walks the genes in chunks of 64.  Both row blocks of a chunk are read with
// coalesced 16-byte loads (8 lanes per 128-byte row segment), cut into their lo and hi bytes
// (two v_perm_b32 and an xor per four counts) and parked in LDS as int8 planes with rows of
// 64 + 16 bytes (conflict-free ds_read_b128 fragments); two buffers, the loads of the next chunk
// in flight while this one multiplies, one barrier a chunk.  Wave w multiplies rows
// 32 (w & 3) .. + 31 by columns 64 (w >> 2) .. + 63: 2 tiles x 4 products = 8 accumulators of 16
// int32, 16 MFMAs per chunk.  Symmetry is not exploited: every strip computes all N columns.
//
// The reduction kernel reads a strip: one wave per row walks the columns cluster by cluster.
// Summation order (fp64 throughout, no atomics): within a cluster lane l adds the columns
// begin + l, begin + l + 64, ... in increasing order, then a 6-level xor tree (32, 16, ..., 1)
// joins the lanes.  d(i, i) = 0 exactly, so the own row needs no special case.  a and b are the
// fp64 quotients rounded to fp32 once; s is formed in fp64 from the fp64 a and b and rounded once.
// The score is the fp64 mean of the fp32 s (thread t adds t, t + 256, ...; a binary tree).
#include "../../include/scvae_hip.h"
#include "common.hpp"

namespace scvae {
namespace {

typedef int cs_i32x4 __attribute__((ext_vector_type(4)));
typedef int cs_i32x16 __attribute__((ext_vector_type(16)));
typedef unsigned cs_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned cs_u32x2 __attribute__((ext_vector_type(2)));

constexpr int CS_THREADS = 512;
constexpr int CS_TILE = 128;                 // rows and columns of a workgroup's tile
constexpr int CS_CHUNK = 64;                 // genes per chunk (two MFMA k-steps of 32)
constexpr int CS_ROW = CS_CHUNK + 16;        // LDS bytes per row of a plane
constexpr int CS_PLANE = CS_TILE * CS_ROW;   // one byte plane of one row block
constexpr int CS_BUFFER = 4 * CS_PLANE;      // i lo, i hi, j lo, j hi
constexpr int CS_LDS = 2 * CS_BUFFER;        // 81 920 bytes
constexpr int64_t CS_SHIFT = 32896;          // c = 128 * 257
constexpr int64_t CS_MAX_N = (int64_t)1 << 20;
constexpr int64_t CS_MAX_F = 65536;
constexpr int CS_RED_THREADS = 256;          // reduction: four rows (waves) per workgroup

__host__ __device__ constexpr int64_t cs_padded_genes(int64_t F) {
  return (F + CS_CHUNK - 1) / CS_CHUNK * CS_CHUNK;
}

// m[i] = sum over the Fp genes of (x_ig - c)^2: one wave per row, lane l takes the 16-byte pieces
// l, l + 64, ...; integer sums, any order gives the same value
__global__ __launch_bounds__(256) void count_row_moments_kernel(const uint16_t* __restrict__ x,
                                                                int64_t ldx, int64_t N, int Fp,
                                                                int64_t* __restrict__ m) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int lane = threadIdx.x & 63;
  const cs_u32x4* src = reinterpret_cast<const cs_u32x4*>(x + row * ldx);
  unsigned long long sum = 0;
  for (int p = lane; p < Fp / 8; p += 64) {
    const cs_u32x4 v = src[p];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int y0 = (int)(w[k] & 0xFFFFu) - (int)CS_SHIFT;
      const int y1 = (int)(w[k] >> 16) - (int)CS_SHIFT;
      sum += (unsigned long long)(unsigned)(y0 * y0) + (unsigned long long)(unsigned)(y1 * y1);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)sum, off, 64);
    const unsigned hi = __shfl_xor((unsigned)(sum >> 32), off, 64);
    sum += ((unsigned long long)hi << 32) | lo;
  }
  if (lane == 0) m[row] = (int64_t)sum;
}

// One chunk of one row block in registers: thread t holds the 16-byte pieces t and t + 512 of
// the [128 rows][8 pieces] block (row = piece / 8).
struct CsPieces {
  cs_u32x4 v[2];
};

__device__ __forceinline__ void cs_fetch(const uint16_t* const* src, int gene0, CsPieces& p) {
#pragma unroll
  for (int u = 0; u < 2; ++u) p.v[u] = *reinterpret_cast<const cs_u32x4*>(src[u] + gene0);
}

// eight counts -> their eight lo bytes and eight hi bytes, top bits flipped (x - 128 as int8)
__device__ __forceinline__ void cs_park(const CsPieces& p, unsigned char* lo_plane,
                                        unsigned char* hi_plane) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int piece = threadIdx.x + CS_THREADS * u;
    const int at = (piece >> 3) * CS_ROW + (piece & 7) * 8;
    const cs_u32x4 v = p.v[u];
    cs_u32x2 lo, hi;
    lo.x = __builtin_amdgcn_perm(v.y, v.x, 0x06040200u) ^ 0x80808080u;
    lo.y = __builtin_amdgcn_perm(v.w, v.z, 0x06040200u) ^ 0x80808080u;
    hi.x = __builtin_amdgcn_perm(v.y, v.x, 0x07050301u) ^ 0x80808080u;
    hi.y = __builtin_amdgcn_perm(v.w, v.z, 0x07050301u) ^ 0x80808080u;
    *reinterpret_cast<cs_u32x2*>(lo_plane + at) = lo;
    *reinterpret_cast<cs_u32x2*>(hi_plane + at) = hi;
  }
}

// d[r][j] = d(i0 + r, j) for r < rows, j < N.  grid: (column tiles, row tiles of the strip)
__global__ __launch_bounds__(CS_THREADS) void count_distances_kernel(
    const uint16_t* __restrict__ x, int64_t ldx, int64_t N, int Fp, int64_t i0, int64_t rows,
    const int64_t* __restrict__ m, float* __restrict__ d, int64_t ldd) {
  extern __shared__ __align__(16) unsigned char cs_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 31, kg = lane >> 5;
  const int64_t r0 = (int64_t)blockIdx.y * CS_TILE;      // first strip row of the tile
  const int64_t j0 = (int64_t)blockIdx.x * CS_TILE;      // first column of the tile

  // the rows this thread stages (rows past the strip or past N: the last valid row, never written)
  const uint16_t* src_i[2];
  const uint16_t* src_j[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int piece = tid + CS_THREADS * u;
    int64_t ri = r0 + (piece >> 3), rj = j0 + (piece >> 3);
    if (ri > rows - 1) ri = rows - 1;
    if (rj > N - 1) rj = N - 1;
    src_i[u] = x + (i0 + ri) * ldx + (piece & 7) * 8;
    src_j[u] = x + rj * ldx + (piece & 7) * 8;
  }

  cs_i32x16 acc[2][4];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[q][p][e] = 0;

  const int a_frag = (32 * (w & 3) + li) * CS_ROW + 16 * kg;          // + 32 s
  const int b_frag = (64 * (w >> 2) + li) * CS_ROW + 16 * kg;         // + 32 rows q, + 32 s
  const int chunks = Fp / CS_CHUNK;
  CsPieces pi, pj;
  cs_fetch(src_i, 0, pi);
  cs_fetch(src_j, 0, pj);
  cs_park(pi, cs_lds, cs_lds + CS_PLANE);
  cs_park(pj, cs_lds + 2 * CS_PLANE, cs_lds + 3 * CS_PLANE);
  __syncthreads();
  for (int ch = 0; ch < chunks; ++ch) {
    const bool more = ch + 1 < chunks;
    if (more) {
      cs_fetch(src_i, (ch + 1) * CS_CHUNK, pi);
      cs_fetch(src_j, (ch + 1) * CS_CHUNK, pj);
    }
    const unsigned char* buf = cs_lds + (ch & 1) * CS_BUFFER;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const cs_i32x4 al = *reinterpret_cast<const cs_i32x4*>(buf + a_frag + 32 * s);
      const cs_i32x4 ah = *reinterpret_cast<const cs_i32x4*>(buf + CS_PLANE + a_frag + 32 * s);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int at = b_frag + q * 32 * CS_ROW + 32 * s;
        const cs_i32x4 bl = *reinterpret_cast<const cs_i32x4*>(buf + 2 * CS_PLANE + at);
        const cs_i32x4 bh = *reinterpret_cast<const cs_i32x4*>(buf + 3 * CS_PLANE + at);
        acc[q][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(al, bl, acc[q][0], 0, 0, 0);
        acc[q][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(al, bh, acc[q][1], 0, 0, 0);
        acc[q][2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ah, bl, acc[q][2], 0, 0, 0);
        acc[q][3] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ah, bh, acc[q][3], 0, 0, 0);
      }
    }
    if (more) {   // (the other buffer: its readers passed the barrier of the chunk before)
      unsigned char* next = cs_lds + ((ch + 1) & 1) * CS_BUFFER;
      cs_park(pi, next, next + CS_PLANE);
      cs_park(pj, next + 2 * CS_PLANE, next + 3 * CS_PLANE);
    }
    __syncthreads();
  }

  // accumulator element e of lane (li, kg): row (e & 3) + 8 (e >> 2) + 4 kg, column li
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int64_t col = j0 + 64 * (w >> 2) + 32 * q + li;
    if (col >= N) continue;
    const int64_t mj = m[col];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t r = r0 + 32 * (w & 3) + (e & 3) + 8 * (e >> 2) + 4 * kg;
      if (r >= rows) continue;
      const int64_t g = (int64_t)acc[q][0][e] +
                        256 * ((int64_t)acc[q][1][e] + (int64_t)acc[q][2][e]) +
                        65536 * (int64_t)acc[q][3][e];
      const int64_t d2 = m[i0 + r] + mj - 2 * g;
      d[r * ldd + col] = (float)sqrt((double)d2);
    }
  }
}

__device__ __forceinline__ double cs_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the cluster of row i: the c with offsets[c] <= i < offsets[c + 1] (0 <= c < K whatever the
// offsets hold)
__device__ __forceinline__ int64_t cs_cluster_of(const int64_t* __restrict__ offsets, int64_t K,
                                                 int64_t i) {
  int64_t lo = 0, hi = K - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// a, b, s of the strip's rows i0 .. i0 + rows - 1 from d [rows][ldd]: a wave per row
__global__ __launch_bounds__(CS_RED_THREADS) void count_silhouette_strip_kernel(
    const float* __restrict__ d, int64_t ldd, int64_t i0, int64_t rows, int64_t N,
    const int64_t* __restrict__ offsets, int64_t K, float* __restrict__ a_out,
    float* __restrict__ b_out, float* __restrict__ s_out, float* __restrict__ s_keep) {
  const int64_t r = (int64_t)blockIdx.x * (CS_RED_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int lane = threadIdx.x & 63;
  const int64_t row = i0 + r;
  const float* dr = d + r * ldd;
  const int64_t own = cs_cluster_of(offsets, K, row);
  double a = 0.0, b = INFINITY;
  int64_t members = 1;
  for (int64_t c = 0; c < K; ++c) {
    // (clipped to the columns there are, whatever the offsets hold)
    int64_t begin = offsets[c], end = offsets[c + 1];
    if (begin < 0) begin = 0;
    if (end > N) end = N;
    double sum = 0.0;
    for (int64_t j = begin + lane; j < end; j += 64) sum += (double)dr[j];
    sum = cs_wave_sum(sum);
    const double count = end > begin ? (double)(end - begin) : 0.0;
    if (c == own) {
      members = end - begin;
      a = count > 1.0 ? sum / (count - 1.0) : 0.0;
    } else if (count > 0.0) {
      b = fmin(b, sum / count);
    }
  }
  if (lane == 0) {
    const double largest = fmax(a, b);
    const float s = (members == 1 || largest == 0.0) ? 0.f : (float)((b - a) / largest);
    if (a_out) a_out[row] = (float)a;
    if (b_out) b_out[row] = (float)b;
    if (s_out) s_out[row] = s;
    s_keep[row] = s;
  }
}

// *score = sum of s[0 .. N) / N in fp64: thread t adds t, t + 256, ... and a binary tree joins the
// threads
__global__ __launch_bounds__(256) void count_silhouette_mean_kernel(const float* __restrict__ s,
                                                                    int64_t N,
                                                                    double* __restrict__ score) {
  __shared__ double red[256];
  double sum = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 256) sum += (double)s[i];
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *score = red[0] / (double)N;
}

// workspace of the samples entry: m [N] int64 | s [N] fp32 (8-byte padded) | the strip [R][ldd]
inline int64_t cs_strip_pitch(int64_t N) { return (N + 15) / 16 * 16; }
inline int64_t cs_fixed_bytes(int64_t N) { return 8 * N + (4 * N + 7) / 8 * 8; }
constexpr int64_t CS_STRIP_BYTES = (int64_t)256 << 20;   // what workspace_bytes asks for

int cs_launch_moments(hipStream_t st, const uint16_t* x, int64_t ldx, int64_t N, int64_t F,
                      int64_t* m) {
  hipLaunchKernelGGL(count_row_moments_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, x,
                     ldx, N, (int)cs_padded_genes(F), m);
  SCVAE_LAUNCH_CHECK("count_row_moments_kernel");
  return 0;
}

int cs_launch_distances(hipStream_t st, const uint16_t* x, int64_t ldx, int64_t N, int64_t F,
                        int64_t i0, int64_t rows, const int64_t* m, float* d, int64_t ldd) {
  SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(count_distances_kernel), CS_LDS));
  const dim3 grid((unsigned)((N + CS_TILE - 1) / CS_TILE),
                  (unsigned)((rows + CS_TILE - 1) / CS_TILE));
  hipLaunchKernelGGL(count_distances_kernel, grid, dim3(CS_THREADS), CS_LDS, st, x, ldx, N,
                     (int)cs_padded_genes(F), i0, rows, m, d, ldd);
  SCVAE_LAUNCH_CHECK("count_distances_kernel");
  return 0;
}

}  // namespace
}  // namespace scvae

#define SCVAE_COUNT_SILHOUETTE_SIZES(N, F)           \
  SCVAE_ARG(F >= 1 && F <= scvae::CS_MAX_F);         \
  SCVAE_ARG(N >= 3 && N <= scvae::CS_MAX_N)
#define SCVAE_COUNT_SILHOUETTE_CLUSTERS(N, K)        \
  SCVAE_ARG(K >= 2);                                 \
  SCVAE_ARG(K <= N - 1)
// the layout of scvae_csr_densify_u16
#define SCVAE_COUNT_SILHOUETTE_ROWS(x, ldx, F)                               \
  SCVAE_ARG(x != nullptr && ((uintptr_t)x & 15) == 0);                       \
  SCVAE_ARG(ldx % 8 == 0 && ldx >= scvae::cs_padded_genes(F))

extern "C" {

int64_t scvae_count_silhouette_workspace_bytes(int64_t N, int64_t F, int64_t K) {
  using namespace scvae;
  SCVAE_COUNT_SILHOUETTE_SIZES(N, F);
  SCVAE_COUNT_SILHOUETTE_CLUSTERS(N, K);
  const int64_t row_bytes = 4 * cs_strip_pitch(N);
  int64_t rows = CS_STRIP_BYTES / row_bytes / CS_TILE * CS_TILE;
  if (rows < CS_TILE) rows = CS_TILE;
  if (rows > N) rows = N;
  return cs_fixed_bytes(N) + rows * row_bytes;
}

int scvae_count_distances_u16(const uint16_t* x, int64_t ldx, int64_t N, int64_t F, int64_t i0,
                              int64_t rows, float* d, int64_t ldd, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  using namespace scvae;
  SCVAE_COUNT_SILHOUETTE_SIZES(N, F);
  SCVAE_COUNT_SILHOUETTE_ROWS(x, ldx, F);
  SCVAE_ARG(i0 >= 0 && rows >= 1 && i0 <= N - rows);
  SCVAE_ARG(d != nullptr && ldd >= N);
  SCVAE_ARG(workspace != nullptr && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= 8 * N);
  hipStream_t st = (hipStream_t)stream;
  int64_t* m = static_cast<int64_t*>(workspace);
  if (int rc = cs_launch_moments(st, x, ldx, N, F, m)) return rc;
  return cs_launch_distances(st, x, ldx, N, F, i0, rows, m, d, ldd);
}

int scvae_count_silhouette_samples_u16(const uint16_t* x, int64_t ldx, int64_t N, int64_t F,
                                       const int64_t* offsets, int64_t K, float* a, float* b,
                                       float* s, double* score, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  using namespace scvae;
  SCVAE_COUNT_SILHOUETTE_SIZES(N, F);
  SCVAE_COUNT_SILHOUETTE_CLUSTERS(N, K);
  SCVAE_COUNT_SILHOUETTE_ROWS(x, ldx, F);
  SCVAE_ARG(offsets != nullptr && score != nullptr);
  SCVAE_ARG(workspace != nullptr && ((uintptr_t)workspace & 7) == 0);
  // the strip is what the workspace leaves: whole tiles of 128 rows, at least one (or all N rows)
  const int64_t ldd = cs_strip_pitch(N), least = N < CS_TILE ? N : CS_TILE;
  SCVAE_ARG(workspace_bytes >= cs_fixed_bytes(N) + least * 4 * ldd);
  int64_t strip = (workspace_bytes - cs_fixed_bytes(N)) / (4 * ldd);
  if (strip >= N) strip = N;
  else strip = strip / CS_TILE * CS_TILE;
  hipStream_t st = (hipStream_t)stream;
  int64_t* m = static_cast<int64_t*>(workspace);
  float* s_keep = reinterpret_cast<float*>(m + N);
  float* d = reinterpret_cast<float*>(static_cast<char*>(workspace) + cs_fixed_bytes(N));
  if (int rc = cs_launch_moments(st, x, ldx, N, F, m)) return rc;
  for (int64_t i0 = 0; i0 < N; i0 += strip) {
    const int64_t rows = N - i0 < strip ? N - i0 : strip;
    if (int rc = cs_launch_distances(st, x, ldx, N, F, i0, rows, m, d, ldd)) return rc;
    const int64_t blocks = (rows + CS_RED_THREADS / 64 - 1) / (CS_RED_THREADS / 64);
    hipLaunchKernelGGL(count_silhouette_strip_kernel, dim3((unsigned)blocks),
                       dim3(CS_RED_THREADS), 0, st, d, ldd, i0, rows, N, offsets, K, a, b, s,
                       s_keep);
    SCVAE_LAUNCH_CHECK("count_silhouette_strip_kernel");
  }
  hipLaunchKernelGGL(count_silhouette_mean_kernel, dim3(1), dim3(256), 0, st, s_keep, N, score);
  SCVAE_LAUNCH_CHECK("count_silhouette_mean_kernel");
  return 0;
}

}  // extern "C"
