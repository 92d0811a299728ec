// Principal components of a cells x genes matrix by block subspace iteration: the three passes
// over the matrix that the iteration needs (scvae/analyses/decomposition/decomposition.py:65-91,
// where the reference fits IncrementalPCA(batch_size=100) for more than 2000 features; the loop
// itself is scvae_amd/analyses/decomposition.py).  x [rows, F] is fp32 with a row pitch ldx in
// elements and unit column stride, read where it lies; every element is converted to fp64 in
// registers, and with Xc = X - 1 mu^T
//
//   moments       mu[F] = column means,  total = sum_ij (x_ij - mu_j)^2       (two passes)
//   project       Y [rows, b] = Xc Q,    Q [F, b] fp64, b <= 32               (also `transform`)
//   back-project  Z [F, b]    = Xc^T Y
//
// mu_j is subtracted per element in fp64 inside the kernels (no rank-one correction afterwards),
// so the only roundings are that subtraction and the fp64 accumulation.  Every sum has one fixed
// order and there are no atomics: the same input gives the same bits on every run.
//
// Both products run on v_mfma_f64_16x16x4_f64 (D [16 x 16] += A [16 x 4] B [4 x 16]).  Lane l
// gives A[l & 15][l >> 4] and B[l >> 4][l & 15], one fp64 each, and holds D[(l >> 4) + 4 r][l & 15]
// in register r = 0 .. 3 -- not the row map of the other MFMAs of this code base.
//
// project: a workgroup of 4 waves owns 64 rows (4 row tiles of the MFMA).  Lane (i = l & 15,
// g = l >> 4) reads 8 consecutive floats of row i of each tile as two 16-byte loads, columns
// k0 + 8 g .. k0 + 8 g + 7 of a step of 32 columns: the 4 lanes of a row read 128 contiguous
// bytes.  MFMA e = 0 .. 7 of the step takes element e from every lane, so its k index g stands
// for column k0 + 8 g + e -- a permutation of the 32 columns of the step that the B operand
// Q[k0 + 8 g + e][j] follows; no lane gathers with a stride.  Wave w takes steps w, w + 4, ...;
// the 4 partial tiles join through LDS in the order ((w0 + w1) + w2) + w3.
//
// back-project: a wave owns 64 features and a range of rows.  Lane (i, g) reads the 4 consecutive
// floats f0 + 4 i .. f0 + 4 i + 3 of row r + g as one 16-byte load (the 16 lanes of a row read 256
// contiguous bytes); MFMA e = 0 .. 3 takes element e, so row i of its A operand is feature
// f0 + 4 i + e -- the permutation is in the output rows here, undone when Z is stored.  The rows
// are split in `chunks` ranges over gridDim.y; the ranges' partial Z join in range order.
//
// 16-byte loads are issued at 4-byte alignment (the matrix of an evaluation has an odd pitch);
// global memory takes them.  Steps and feature blocks that are not whole read element by element
// inside [0, F); a row index past the end is clamped to the last row and its products are given
// a zero operand.  Nothing outside the rows x F elements is read.
#include "../../include/scvae_hip.h"
#include "common.hpp"

namespace scvae {
namespace {

// every operation as written: a sum's bits do not depend on what the compiler fuses
#pragma clang fp contract(off)

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) F4u {
  f4 v;
};

constexpr int PCA_THREADS = 256;
constexpr int PCA_MAX_BLOCK = 32;          // widest Q
constexpr int PCA_ROWS = 64;               // rows of a project workgroup
constexpr int PCA_STEP = 32;               // columns of a project step
constexpr int PCA_FEATURES = 64;           // features of a back-project wave
constexpr int PCA_MAX_CHUNKS = 64;         // row ranges of moments and back-project
constexpr int64_t PCA_MAX_FEATURES = (int64_t)1 << 20;

// the 4 floats at p (4-byte aligned) as one 16-byte load
__device__ __forceinline__ f4 load4(const float* p) {
  return reinterpret_cast<const F4u*>(p)->v;
}

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------
// moments: part[chunk][f] = sum over the chunk's rows of x (SQ = false) or of (x - mu_f)^2;
// a thread owns a column, four running sums over the rows r = 0, 1, 2, 3 (mod 4) of the chunk
template <bool SQ>
__global__ __launch_bounds__(PCA_THREADS) void pca_column_sums_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t rows, int F, const double* __restrict__ mu,
    double* __restrict__ part, int64_t chunk_rows) {
  const int f = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (f >= F) return;
  const int64_t ra = (int64_t)blockIdx.y * chunk_rows;
  const int64_t rb = ra + chunk_rows < rows ? ra + chunk_rows : rows;
  const double m = SQ ? mu[f] : 0.0;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  const float* p = x + ra * ldx + f;
  int64_t r = ra;
  for (; r + 4 <= rb; r += 4, p += 4 * ldx) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = p[u * ldx];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double d = (double)v[u] - m;
      a[u] = SQ ? fma(d, d, a[u]) : a[u] + d;
    }
  }
  for (int u = 0; r < rb; ++r, ++u, p += ldx) {
    const double d = (double)p[0] - m;
    a[u] = SQ ? fma(d, d, a[u]) : a[u] + d;
  }
  part[(int64_t)blockIdx.y * F + f] = (a[0] + a[1]) + (a[2] + a[3]);
}

__global__ __launch_bounds__(PCA_THREADS) void pca_mean_kernel(
    const double* __restrict__ part, int chunks, int F, int64_t rows, double* __restrict__ mu) {
  const int f = blockIdx.x * PCA_THREADS + threadIdx.x;
  if (f >= F) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[(int64_t)c * F + f];
  mu[f] = s / (double)rows;
}

// one workgroup: thread t adds the columns t, t + 256, ... (each the sum of its chunks in
// order), then lane l takes lane l + off for off = 32 .. 1 and thread 0 the waves in order
__global__ __launch_bounds__(PCA_THREADS) void pca_total_kernel(
    const double* __restrict__ part, int chunks, int F, double* __restrict__ total) {
  __shared__ double red[PCA_THREADS / WAVE];
  double s = 0.0;
  for (int f = threadIdx.x; f < F; f += PCA_THREADS) {
    double c = 0.0;
    for (int k = 0; k < chunks; ++k) c += part[(int64_t)k * F + f];
    s += c;
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < PCA_THREADS / WAVE; ++i) s += red[i];
    *total = s;
  }
}

// ---------------------------------------------------------------------------------------------
// project.  CT: column tiles of 16 (b <= 16 CT)
template <int CT>
__global__ __launch_bounds__(PCA_THREADS) void pca_project_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t rows, int F, const double* __restrict__ mu,
    const double* __restrict__ q, int b, double* __restrict__ y) {
  __shared__ double red[PCA_THREADS / WAVE - 1][PCA_ROWS][16 * CT];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const int i = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * PCA_ROWS;
  const float* xrow[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    int64_t row = r0 + 16 * t + i;
    if (row > rows - 1) row = rows - 1;          // its results are not stored
    xrow[t] = x + row * ldx;
  }
  d4 acc[4][CT];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[t][c] = d4{0.0, 0.0, 0.0, 0.0};

  const int steps = (F + PCA_STEP - 1) / PCA_STEP;
  for (int s = w; s < steps; s += PCA_THREADS / WAVE) {
    const int k0 = s * PCA_STEP + 8 * g;         // this lane's first column of the step
    float xa[4][8];
    double m[8], qv[CT][8];
    if ((s + 1) * PCA_STEP <= F) {               // a whole step (the same test in every lane)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f4 lo = load4(xrow[t] + k0), hi = load4(xrow[t] + k0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) xa[t][e] = lo[e], xa[t][4 + e] = hi[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        m[e] = mu[k0 + e];
#pragma unroll
        for (int c = 0; c < CT; ++c)
          qv[c][e] = 16 * c + i < b ? q[(int64_t)(k0 + e) * b + 16 * c + i] : 0.0;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool in = k0 + e < F;
        m[e] = in ? mu[k0 + e] : 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) xa[t][e] = in ? xrow[t][k0 + e] : 0.f;
#pragma unroll
        for (int c = 0; c < CT; ++c)
          qv[c][e] = (in && 16 * c + i < b) ? q[(int64_t)(k0 + e) * b + 16 * c + i] : 0.0;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double a = (double)xa[t][e] - m[e];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[t][c] = mfma(a, qv[c][e], acc[t][c]);
      }
    }
  }

  // register r of tile t is row 16 t + g + 4 r of the workgroup, column 16 c + i
  if (w > 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[w - 1][16 * t + g + 4 * r][16 * c + i] = acc[t][c][r];
  }
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int lr = 16 * t + g + 4 * r, col = 16 * c + i;
          double v = acc[t][c][r];
#pragma unroll
          for (int k = 0; k < PCA_THREADS / WAVE - 1; ++k) v += red[k][lr][col];
          const int64_t row = r0 + lr;
          if (row < rows && col < b) y[row * b + col] = v;
        }
  }
}

// ---------------------------------------------------------------------------------------------
// back-project: out [chunks][F][b] (or z itself for one chunk)
template <int CT>
__global__ __launch_bounds__(PCA_THREADS) void pca_back_project_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t rows, int F, const double* __restrict__ mu,
    const double* __restrict__ y, int b, double* __restrict__ out, int64_t chunk_rows) {
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const int i = lane & 15, g = lane >> 4;
  const int fb = (blockIdx.x * (PCA_THREADS / WAVE) + w) * PCA_FEATURES;
  if (fb >= F) return;                           // (no barrier in this kernel)
  const int f0 = fb + 4 * i;                     // this lane's 4 features
  const bool whole = fb + PCA_FEATURES <= F;     // the same in every lane of the wave
  double m[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) m[e] = f0 + e < F ? mu[f0 + e] : 0.0;
  const int64_t ra = (int64_t)blockIdx.y * chunk_rows;
  const int64_t rb = ra + chunk_rows < rows ? ra + chunk_rows : rows;
  d4 acc[4][CT];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[e][c] = d4{0.0, 0.0, 0.0, 0.0};

  for (int64_t r = ra; r < rb; r += 16) {
    float xa[4][4];
    double yv[4][CT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t row = r + 4 * u + g;
      const bool valid = row < rb;
      const int64_t rc = valid ? row : rb - 1;
      const float* p = x + rc * ldx + f0;
      if (whole) {
        const f4 v = load4(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) xa[u][e] = v[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) xa[u][e] = f0 + e < F ? p[e] : 0.f;
      }
#pragma unroll
      for (int c = 0; c < CT; ++c)
        yv[u][c] = (valid && 16 * c + i < b) ? y[rc * b + 16 * c + i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double a = (double)xa[u][e] - m[e];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[e][c] = mfma(a, yv[u][c], acc[e][c]);
      }
  }

  // register r of tile e is row g + 4 r of its A operand: feature fb + 4 (g + 4 r) + e
  double* o = out + (int64_t)blockIdx.y * F * b;
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = fb + 4 * (g + 4 * r) + e, col = 16 * c + i;
        if (f < F && col < b) o[(int64_t)f * b + col] = acc[e][c][r];
      }
}

__global__ __launch_bounds__(PCA_THREADS) void pca_join_kernel(
    const double* __restrict__ part, int chunks, int64_t n, double* __restrict__ z) {
  const int64_t k = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
  if (k >= n) return;
  double s = part[k];
  for (int c = 1; c < chunks; ++c) s += part[(int64_t)c * n + k];
  z[k] = s;
}

// the rows of a range (a multiple of 16) and the number of ranges: enough workgroups to fill
// the chip where the features alone do not, never more than PCA_MAX_CHUNKS
void row_chunks(int64_t rows, int64_t F, int64_t* chunk_rows, int* chunks) {
  const int64_t feature_groups = (F + PCA_THREADS - 1) / PCA_THREADS;
  int64_t want = 2048 / feature_groups;
  if (want > PCA_MAX_CHUNKS) want = PCA_MAX_CHUNKS;
  if (want < 1) want = 1;
  int64_t per = (rows + want - 1) / want;
  per = (per + 15) / 16 * 16;
  *chunk_rows = per;
  *chunks = (int)((rows + per - 1) / per);
}

}  // namespace
}  // namespace scvae

#define SCVAE_PCA_MATRIX(x, ldx, rows, F)                                   \
  SCVAE_ARG(x && ((uintptr_t)x & 3) == 0);                                  \
  SCVAE_ARG(rows >= 1 && rows <= INT32_MAX);                                \
  SCVAE_ARG(F >= 1 && F <= scvae::PCA_MAX_FEATURES);                        \
  SCVAE_ARG(ldx >= F && ldx <= INT64_MAX / 4 / rows)

extern "C" {

int64_t scvae_pca_workspace_bytes(int64_t rows, int64_t F, int64_t b) {
  using namespace scvae;
  if (rows < 1 || rows > INT32_MAX || F < 1 || F > PCA_MAX_FEATURES || b < 1 ||
      b > PCA_MAX_BLOCK) {
    set_error("bad argument: scvae_pca_workspace_bytes(%lld, %lld, %lld)", (long long)rows,
              (long long)F, (long long)b);
    return -1;
  }
  int64_t chunk_rows;
  int chunks;
  row_chunks(rows, F, &chunk_rows, &chunks);
  return (int64_t)sizeof(double) * chunks * F * b;
}

int scvae_pca_moments(const float* x, int64_t ldx, int64_t rows, int64_t F, double* mu,
                      double* total, void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace scvae;
  SCVAE_PCA_MATRIX(x, ldx, rows, F);
  SCVAE_ARG(mu && total && ((uintptr_t)mu & 7) == 0 && ((uintptr_t)total & 7) == 0);
  int64_t chunk_rows;
  int chunks;
  row_chunks(rows, F, &chunk_rows, &chunks);
  SCVAE_ARG(workspace && ((uintptr_t)workspace & 7) == 0);
  SCVAE_ARG(workspace_bytes >= (int64_t)sizeof(double) * chunks * F);
  hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  const int groups = (int)((F + PCA_THREADS - 1) / PCA_THREADS);
  const dim3 grid(groups, chunks);
  hipLaunchKernelGGL(pca_column_sums_kernel<false>, grid, dim3(PCA_THREADS), 0, st, x, ldx, rows,
                     (int)F, (const double*)nullptr, part, chunk_rows);
  SCVAE_LAUNCH_CHECK("pca_column_sums_kernel");
  hipLaunchKernelGGL(pca_mean_kernel, dim3(groups), dim3(PCA_THREADS), 0, st, part, chunks,
                     (int)F, rows, mu);
  SCVAE_LAUNCH_CHECK("pca_mean_kernel");
  hipLaunchKernelGGL(pca_column_sums_kernel<true>, grid, dim3(PCA_THREADS), 0, st, x, ldx, rows,
                     (int)F, (const double*)mu, part, chunk_rows);
  SCVAE_LAUNCH_CHECK("pca_column_sums_kernel");
  hipLaunchKernelGGL(pca_total_kernel, dim3(1), dim3(PCA_THREADS), 0, st, part, chunks, (int)F,
                     total);
  SCVAE_LAUNCH_CHECK("pca_total_kernel");
  return 0;
}

int scvae_pca_project(const float* x, int64_t ldx, int64_t rows, int64_t F, const double* mu,
                      const double* q, int64_t b, double* y, void* stream) {
  using namespace scvae;
  SCVAE_PCA_MATRIX(x, ldx, rows, F);
  SCVAE_ARG(b >= 1 && b <= PCA_MAX_BLOCK);
  SCVAE_ARG(mu && q && y);
  SCVAE_ARG(((uintptr_t)mu & 7) == 0 && ((uintptr_t)q & 7) == 0 && ((uintptr_t)y & 7) == 0);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + PCA_ROWS - 1) / PCA_ROWS));
  if (b <= 16)
    hipLaunchKernelGGL(pca_project_kernel<1>, grid, dim3(PCA_THREADS), 0, st, x, ldx, rows,
                       (int)F, mu, q, (int)b, y);
  else
    hipLaunchKernelGGL(pca_project_kernel<2>, grid, dim3(PCA_THREADS), 0, st, x, ldx, rows,
                       (int)F, mu, q, (int)b, y);
  SCVAE_LAUNCH_CHECK("pca_project_kernel");
  return 0;
}

int scvae_pca_back_project(const float* x, int64_t ldx, int64_t rows, int64_t F, const double* mu,
                           const double* y, int64_t b, double* z, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  using namespace scvae;
  SCVAE_PCA_MATRIX(x, ldx, rows, F);
  SCVAE_ARG(b >= 1 && b <= PCA_MAX_BLOCK);
  SCVAE_ARG(mu && y && z);
  SCVAE_ARG(((uintptr_t)mu & 7) == 0 && ((uintptr_t)y & 7) == 0 && ((uintptr_t)z & 7) == 0);
  int64_t chunk_rows;
  int chunks;
  row_chunks(rows, F, &chunk_rows, &chunks);
  if (chunks > 1) {
    SCVAE_ARG(workspace && ((uintptr_t)workspace & 7) == 0);
    SCVAE_ARG(workspace_bytes >= (int64_t)sizeof(double) * chunks * F * b);
  }
  hipStream_t st = (hipStream_t)stream;
  double* out = chunks > 1 ? static_cast<double*>(workspace) : z;
  const int per_group = PCA_FEATURES * (PCA_THREADS / WAVE);
  const dim3 grid((unsigned)((F + per_group - 1) / per_group), chunks);
  if (b <= 16)
    hipLaunchKernelGGL(pca_back_project_kernel<1>, grid, dim3(PCA_THREADS), 0, st, x, ldx, rows,
                       (int)F, mu, y, (int)b, out, chunk_rows);
  else
    hipLaunchKernelGGL(pca_back_project_kernel<2>, grid, dim3(PCA_THREADS), 0, st, x, ldx, rows,
                       (int)F, mu, y, (int)b, out, chunk_rows);
  SCVAE_LAUNCH_CHECK("pca_back_project_kernel");
  if (chunks > 1) {
    const int64_t n = F * b;
    hipLaunchKernelGGL(pca_join_kernel, dim3((unsigned)((n + PCA_THREADS - 1) / PCA_THREADS)),
                       dim3(PCA_THREADS), 0, st, (const double*)out, chunks, n, z);
    SCVAE_LAUNCH_CHECK("pca_join_kernel");
  }
  return 0;
}

}  // extern "C"
