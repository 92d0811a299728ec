// Pairwise distances between the rows of a cells x genes matrix: what the reference hands to
// sklearn.metrics.pairwise_distances for its "Distances" analysis
// (scvae/analyses/figures/matrices.py:124-130, called from scvae/analyses/subanalyses.py:294-468
// with up to 10 000 sampled cells by all genes).  x [total_rows, F] is fp32 with a row pitch ldx
// in elements and unit column stride, read where it lies and through an optional row index: no
// gathered copy is made.  The Gram product g_ij = sum_k x_ik x_jk runs on
// v_mfma_f64_16x16x4_f64; the operands stay fp32 in LDS and are widened when an MFMA takes
// them, so every product is exact and only the fp64 additions round.
//
// Two passes of one kernel body, 128 x 128 output tiles, only tiles (I, J) with I <= J:
//
//   pass 1 (DIAG)  the diagonal tiles (I, I): of their 8 x 8 MFMA tiles only the 8 on the
//                  diagonal are computed, and g_ii goes to an fp64 [n] buffer
//   pass 2         every upper tile; the metric is applied to the fp64 accumulators with g_ii and
//                  g_jj from pass 1, rounded to fp32 once, laid down in LDS (64 rows at a time)
//                  and written twice: as d[I rows][J columns] and, transposed, as
//                  d[J rows][I columns].  A diagonal tile is written once.  The fp64 Gram is
//                  never stored.
//
// The order of the additions.  A workgroup stages 32 columns of its 128 + 128 rows per step; a
// lane (i = l & 15, g = l >> 4) reads the 4 consecutive floats 16 h + 4 g .. + 3 of row i of an
// MFMA tile as one 16-byte LDS read, and MFMA e = 0 .. 3 takes element e from every lane: its k
// index g stands for column k0 + 16 h + 4 g + e, the same permutation in both operands.  Every
// element g_ij -- diagonal or not, whichever tile or pass it is computed in -- is therefore one
// chain of MFMAs over the steps, h = 0, 1 and e = 0 .. 3 in that order, starting from 0.  So
// g_ij and g_ji have the same bits, and two rows with identical values have g_ii = g_jj = g_ij
// bit for bit: g_ii + g_jj - 2 g_ij is exactly 0, and g_ij / sqrt(g_ii g_jj) exactly 1
// (sqrt(fl(g g)) = g for the correctly rounded root).  Columns past F are staged as zeros
// (+0 products do not change a sum); K is not split, so there is no join and no atomic.
//
// A lane holds D[(l >> 4) + 4 r][l & 15] in register r of an f64 MFMA result -- not the row map
// of the other MFMAs (see pca.hip).
//
// 16-byte global loads are issued at 4-byte alignment, as in pca.hip.  A step that is not whole
// reads element by element inside [0, F).  Tile rows past n take row n - 1 (their results are
// not stored) and index values are clamped to [0, total_rows): nothing outside the matrix is read
// and nothing outside [n, n] of the output is written.
#include "../../include/scvae_hip.h"
#include "common.hpp"

namespace scvae {
namespace {

// every operation as written: the bits do not depend on what the compiler fuses
#pragma clang fp contract(off)

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) F4u {
  f4 v;
};

constexpr int PD_THREADS = 256;
constexpr int PD_TILE = 128;                // rows and columns of a workgroup's output tile
constexpr int PD_STEP = 32;                 // columns staged per step
constexpr int PD_PITCH = PD_STEP + 4;       // floats of a staged row in LDS (16-byte aligned)
constexpr int PD_OUT_PITCH = PD_TILE + 1;   // floats of a row of the finished tile in LDS
constexpr int64_t PD_MAX_ROWS = (int64_t)1 << 16;
constexpr int64_t PD_MAX_FEATURES = (int64_t)1 << 20;
constexpr int PD_LDS_FLOATS = 2 * PD_TILE * PD_PITCH;
static_assert(64 * PD_OUT_PITCH <= PD_LDS_FLOATS, "half a finished tile fits the staging buffers");

__device__ __forceinline__ f4 load4(const float* p) {
  return reinterpret_cast<const F4u*>(p)->v;
}

__device__ __forceinline__ d4 mfma(double a, double b, d4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// the distance from the fp64 Gram entries, rounded once; NaN passes through every comparison
__device__ __forceinline__ float distance_of(int metric, double gi, double gj, double gij) {
  double d;
  if (metric == SCVAE_DISTANCE_EUCLIDEAN) {
    const double t = gi + gj;
    double s = t - 2.0 * gij;
    s = s < 0.0 ? 0.0 : s;
    d = sqrt(s);
  } else {
    const double den = sqrt(gi * gj);
    const double sim = den == 0.0 ? 0.0 : gij / den;     // a row of zero norm: similarity 0
    d = 1.0 - sim;
    d = d < 0.0 ? 0.0 : (d > 2.0 ? 2.0 : d);
  }
  return (float)d;
}

// tile t of the upper triangle, column by column: t = J (J + 1) / 2 + I, I <= J
__device__ __forceinline__ void upper_tile(int t, int* I, int* J) {
  int j = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (j * (j + 1) / 2 > t) --j;
  while ((j + 1) * (j + 2) / 2 <= t) ++j;
  *J = j;
  *I = t - j * (j + 1) / 2;
}

template <bool DIAG>
__global__ __launch_bounds__(PD_THREADS) void pairwise_gram_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t total_rows, int F,
    const int64_t* __restrict__ rows, int n, int metric, double* __restrict__ gdiag,
    float* __restrict__ out, int64_t ldo) {
  __shared__ __attribute__((aligned(16))) float lds[PD_LDS_FLOATS];
  float* As = lds;
  float* Bs = lds + PD_TILE * PD_PITCH;

  int I, J;
  if (DIAG) {
    I = J = blockIdx.x;
  } else {
    upper_tile((int)blockIdx.x, &I, &J);
  }
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), w = tid / WAVE;
  const int i = lane & 15, g = lane >> 4;
  const int wr = w >> 1, wc = w & 1;             // the wave's 64 x 64 quarter of the tile

  // staging: thread (sr, sc) loads floats 4 sc .. 4 sc + 3 of the rows sr + 32 u of both tiles
  const int sr = tid >> 3, sc = tid & 7;
  const float* arow[4];
  const float* brow[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    int ra = I * PD_TILE + sr + 32 * u, rb = J * PD_TILE + sr + 32 * u;
    ra = ra < n ? ra : n - 1;
    rb = rb < n ? rb : n - 1;
    int64_t pa = rows ? rows[ra] : (int64_t)ra, pb = rows ? rows[rb] : (int64_t)rb;
    pa = pa < 0 ? 0 : (pa > total_rows - 1 ? total_rows - 1 : pa);
    pb = pb < 0 ? 0 : (pb > total_rows - 1 ? total_rows - 1 : pb);
    arow[u] = x + pa * ldx;
    brow[u] = x + pb * ldx;
  }

  d4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};

  const int steps = (F + PD_STEP - 1) / PD_STEP;
  f4 pa[4], pb[4];
  auto fetch = [&](int s) {
    const int k = s * PD_STEP + 4 * sc;
    if ((s + 1) * PD_STEP <= F) {                // a whole step (the same test in every thread)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        pa[u] = load4(arow[u] + k);
        pb[u] = load4(brow[u] + k);
      }
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool in = k + e < F;
          pa[u][e] = in ? arow[u][k + e] : 0.f;
          pb[u][e] = in ? brow[u][k + e] : 0.f;
        }
    }
  };

  fetch(0);
  for (int s = 0; s < steps; ++s) {
    __syncthreads();                             // the previous step's reads are done
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      *reinterpret_cast<f4*>(As + (sr + 32 * u) * PD_PITCH + 4 * sc) = pa[u];
      *reinterpret_cast<f4*>(Bs + (sr + 32 * u) * PD_PITCH + 4 * sc) = pb[u];
    }
    __syncthreads();
    if (s + 1 < steps) fetch(s + 1);             // in flight while this step multiplies
    if (DIAG && wr != wc) continue;              // no diagonal MFMA tile in this quarter
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f4 av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        av[a] = *reinterpret_cast<const f4*>(As + (wr * 64 + 16 * a + i) * PD_PITCH + 16 * h +
                                             4 * g);
        bv[a] = *reinterpret_cast<const f4*>(Bs + (wc * 64 + 16 * a + i) * PD_PITCH + 16 * h +
                                             4 * g);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            if (DIAG && a != b) continue;
            acc[a][b] = mfma((double)av[a][e], (double)bv[b][e], acc[a][b]);
          }
        }
      }
    }
  }

  // register r of MFMA tile (a, b) is row 64 wr + 16 a + g + 4 r, column 64 wc + 16 b + i of the
  // workgroup's tile
  if (DIAG) {
    if (wr == wc) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = I * PD_TILE + wr * 64 + 16 * a + g + 4 * r;
          if (g + 4 * r == i && row < n) gdiag[row] = acc[a][a][r];
        }
    }
    return;
  }

  // the finished tile goes through LDS in two halves of 64 rows (the staging buffers hold one)
  for (int half = 0; half < 2; ++half) {
    __syncthreads();
    if (wr == half) {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int lc = wc * 64 + 16 * b + i;
          const int col = J * PD_TILE + lc;
          const double gj = gdiag[col < n ? col : n - 1];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int lr = 16 * a + g + 4 * r;
            const int row = I * PD_TILE + half * 64 + lr;
            const double gi = gdiag[row < n ? row : n - 1];
            const float d = row == col ? 0.f : distance_of(metric, gi, gj, acc[a][b][r]);
            lds[lr * PD_OUT_PITCH + lc] = d;
          }
        }
      }
    }
    __syncthreads();
    {
      const int c = tid & (PD_TILE - 1);
      const int col = J * PD_TILE + c;
      for (int r = tid >> 7; r < 64; r += PD_THREADS / PD_TILE) {
        const int row = I * PD_TILE + half * 64 + r;
        if (row < n && col < n) out[(int64_t)row * ldo + col] = lds[r * PD_OUT_PITCH + c];
      }
    }
    if (I != J) {                                // the mirror: d_ji from the same value
      const int r = tid & 63;
      const int col = I * PD_TILE + half * 64 + r;
      for (int c = tid >> 6; c < PD_TILE; c += PD_THREADS / 64) {
        const int row = J * PD_TILE + c;
        if (row < n && col < n) out[(int64_t)row * ldo + col] = lds[r * PD_OUT_PITCH + c];
      }
    }
  }
}

}  // namespace
}  // namespace scvae

extern "C" {

int64_t scvae_pairwise_distances_workspace_bytes(int64_t n, int64_t F) {
  using namespace scvae;
  if (n < 1 || n > PD_MAX_ROWS || F < 1 || F > PD_MAX_FEATURES) {
    set_error("bad argument: scvae_pairwise_distances_workspace_bytes(%lld, %lld)", (long long)n,
              (long long)F);
    return -1;
  }
  return (int64_t)sizeof(double) * ((n + 31) / 32 * 32);
}

int scvae_pairwise_distances(const float* x, int64_t ldx, int64_t total_rows, int64_t F,
                             const int64_t* rows, int64_t n, int32_t metric, float* out,
                             int64_t ldo, void* workspace, int64_t workspace_bytes,
                             void* stream) {
  using namespace scvae;
  SCVAE_ARG(x && ((uintptr_t)x & 3) == 0);
  SCVAE_ARG(F >= 1 && F <= PD_MAX_FEATURES);
  SCVAE_ARG(n >= 1 && n <= PD_MAX_ROWS);
  SCVAE_ARG(total_rows >= 1 && total_rows <= INT32_MAX);
  SCVAE_ARG(ldx >= F && ldx <= INT64_MAX / 4 / total_rows);
  SCVAE_ARG(rows ? ((uintptr_t)rows & 7) == 0 : n <= total_rows);
  SCVAE_ARG(metric == SCVAE_DISTANCE_EUCLIDEAN || metric == SCVAE_DISTANCE_COSINE);
  SCVAE_ARG(out && ((uintptr_t)out & 3) == 0);
  SCVAE_ARG(ldo >= n && ldo <= INT64_MAX / 4 / n);
  SCVAE_ARG(workspace && ((uintptr_t)workspace & 7) == 0);
  SCVAE_ARG(workspace_bytes >= (int64_t)sizeof(double) * ((n + 31) / 32 * 32));
  hipStream_t st = (hipStream_t)stream;
  double* gdiag = static_cast<double*>(workspace);
  const int tiles = (int)((n + PD_TILE - 1) / PD_TILE);
  hipLaunchKernelGGL(pairwise_gram_kernel<true>, dim3(tiles), dim3(PD_THREADS), 0, st, x, ldx,
                     total_rows, (int)F, rows, (int)n, (int)metric, gdiag, out, ldo);
  SCVAE_LAUNCH_CHECK("pairwise_gram_kernel<diagonal>");
  hipLaunchKernelGGL(pairwise_gram_kernel<false>, dim3(tiles * (tiles + 1) / 2),
                     dim3(PD_THREADS), 0, st, x, ldx, total_rows, (int)F, rows, (int)n,
                     (int)metric, gdiag, out, ldo);
  SCVAE_LAUNCH_CHECK("pairwise_gram_kernel");
  return 0;
}

}  // extern "C"
