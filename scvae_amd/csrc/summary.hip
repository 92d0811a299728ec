// Summary statistics of the evaluation set and of its reconstruction
// (scvae/analyses/metrics/summary.py:27-57, the metrics table of analyses/analyses.py:873-895 with
// the comparison arrays of analyses.py:796-802), accumulated in one streaming pass over blocks of
// rows.  recon [rows, F] and orig [rows, F] are fp32 with row pitches ldr and ldo; either may be
// absent.  Four element streams:
//
//   0  orig         x
//   1  recon        x~
//   2  differences  |x~ - x|                    (both inputs, `comparisons` set)
//   3  log-ratios   |log1p x~ - log1p x|        (both inputs, `comparisons` set)
//
// The elements of streams 2 and 3 are formed in fp64 from the fp32 inputs (the reference rounds
// x~ - x and the two log1p to fp32 per element: a deliberate difference).
//
// Per stream a partial result is (n, count of elements >= tolerance, S = sum x, M2 = sum of
// squared deviations from the partial's own mean, minimum, maximum), n and the count int64, the
// rest fp64.  Two partials join by Chan's pairwise formula written on the sums, so that integer
// data keeps an exact S:
//
//   n = na + nb,  S = Sa + Sb,  M2 = M2a + M2b + (nb Sa - na Sb)^2 / (na nb n)
//
// A thread reads a tile as four 16-byte groups per input and holds those up to 16 elements in
// registers: their partial is the two-pass one (m = S / n, M2 = sum (x - m)^2), which has no
// cancellation whatever the mean, and is joined to the thread's running partial.  Threads join by
// a shuffle-down tree over the 64 lanes, the 4 waves in order, the workgroups' partials in a
// second launch (thread t takes t, t + 256, ... in order, then the same tree), and the result
// joins the state the calls add to.  No floating-point atomics, one fixed order: the same
// sequence of calls on the same data gives the same bits on every run.
//
// Addressing: a row is walked in "virtual columns" v = column + phase, phase = the number of
// floats the row's first element lies past a 16-byte boundary, so that a group of 4 virtual
// columns at a multiple of 4 is one aligned 16-byte load wherever all 4 columns lie in [0, F);
// the at most two groups that straddle the row's ends read their valid columns one by one.
// Nothing outside [0, F) of a row is ever read.  The second input takes 16-byte loads where its
// phase is the first's, dword loads otherwise.  Rows and element offsets are int64, columns
// int32 (F < 2^31 - 8192).
//
// NaN: the hardware's minimum and maximum drop a NaN, so a chunk whose sum is NaN is searched
// for one and then hands on NaN extremes, which the joins keep; S and M2 turn NaN by arithmetic,
// as in NumPy.  +-inf: as IEEE arithmetic gives it (S infinite, M2 NaN).
#include "../../include/scvae_hip.h"
#include "common.hpp"

namespace scvae {
namespace {

// every operation as written (no contraction left to the compiler): the instantiations of the
// kernel give a stream the same bits, and integer data its exact sums
#pragma clang fp contract(off)

constexpr int SUM_THREADS = 256;
constexpr int SUM_GROUPS = 4;                                 // 16-byte groups per thread and tile
constexpr int SUM_CHUNK = 4 * SUM_GROUPS;                     // elements a thread holds at a time
constexpr int64_t SUM_TILE = (int64_t)SUM_THREADS * SUM_CHUNK;  // virtual columns of a tile
constexpr int SUM_MAX_BLOCKS = 1024;                          // 4 workgroups a CU
constexpr int SUM_STREAMS = 4;

struct Partial {
  int64_t n, count;
  double sum, m2, lo, hi;
};
static_assert(sizeof(Partial) == 48, "layout of the summary state");

// workspace: the state [4], then the workgroups' partials [SUM_MAX_BLOCKS][4]
constexpr int64_t SUM_WORKSPACE_BYTES =
    (int64_t)sizeof(Partial) * SUM_STREAMS * (1 + SUM_MAX_BLOCKS);

__device__ __forceinline__ double nan_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ Partial empty_partial() {
  return Partial{0, 0, 0.0, 0.0, (double)INFINITY, -(double)INFINITY};
}

__device__ __forceinline__ Partial join(const Partial& a, const Partial& b) {
  if (b.n == 0) return a;
  if (a.n == 0) return b;
  Partial r;
  const double na = (double)a.n, nb = (double)b.n;
  r.n = a.n + b.n;
  r.count = a.count + b.count;
  r.sum = a.sum + b.sum;
  const double d = nb * a.sum - na * b.sum;
  r.m2 = (a.m2 + b.m2) + d * d / (na * nb * (na + nb));
  r.lo = nan_min(a.lo, b.lo);
  r.hi = nan_max(a.hi, b.hi);
  return r;
}

__device__ __forceinline__ Partial shuffle_down(const Partial& p, int off) {
  Partial r;
  r.n = __shfl_down(p.n, off, WAVE);
  r.count = __shfl_down(p.count, off, WAVE);
  r.sum = __shfl_down(p.sum, off, WAVE);
  r.m2 = __shfl_down(p.m2, off, WAVE);
  r.lo = __shfl_down(p.lo, off, WAVE);
  r.hi = __shfl_down(p.hi, off, WAVE);
  return r;
}

// the join of the workgroup's partials, valid in thread 0: lane l takes lane l + off for
// off = 32 .. 1, then thread 0 the waves in order
__device__ __forceinline__ Partial block_join(Partial p, Partial* red) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) p = join(p, shuffle_down(p, off));
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  __syncthreads();
  if (lane == 0) red[w] = p;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < SUM_THREADS / WAVE; ++i) p = join(p, red[i]);
  return p;
}

// the two-pass partial of the elements e[i] with bit i of mask set, joined to acc.  Minimum,
// maximum and the count are taken in the elements' own type T (fp32 for the two input streams):
// the hardware minimum and maximum, which drop a NaN, and a NaN is put back where there was one.
template <bool FULL, bool COUNT, typename T>
__device__ __forceinline__ void add_chunk(Partial& acc, const T (&e)[SUM_CHUNK], unsigned mask,
                                          T tolerance) {
  T lo = (T)INFINITY, hi = -(T)INFINITY;
  int count = 0;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < SUM_CHUNK; ++i) {
    if (FULL || ((mask >> i) & 1u)) {
      const T x = e[i];
      s += (double)x;
      lo = __builtin_elementwise_min(lo, x);
      hi = __builtin_elementwise_max(hi, x);
      if (COUNT) count += x >= tolerance ? 1 : 0;
    }
  }
  // a NaN element makes the sum NaN (so do infinities of both signs): only then look for one
  bool any_nan = false;
  if (s != s) {
#pragma unroll
    for (int i = 0; i < SUM_CHUNK; ++i)
      if (FULL || ((mask >> i) & 1u)) any_nan |= e[i] != e[i];
  }
  const int n = FULL ? SUM_CHUNK : __popc(mask);
  const double m = FULL ? s * (1.0 / SUM_CHUNK) : s / (double)n;
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < SUM_CHUNK; ++i) {
    if (FULL || ((mask >> i) & 1u)) {
      const double d = (double)e[i] - m;
      q = fma(d, d, q);
    }
  }
  Partial c;
  c.n = n, c.count = count, c.sum = s, c.m2 = q;
  c.lo = any_nan ? (double)NAN : (double)lo;
  c.hi = any_nan ? (double)NAN : (double)hi;
  acc = join(acc, c);
}

template <bool COUNT, typename T>
__device__ __forceinline__ void add_elements(Partial& acc, const T (&e)[SUM_CHUNK],
                                             unsigned mask, T tolerance) {
  if (mask == (1u << SUM_CHUNK) - 1u) add_chunk<true, COUNT>(acc, e, mask, tolerance);
  else if (mask) add_chunk<false, COUNT>(acc, e, mask, tolerance);
}

// the columns col0 .. col0 + 3 of a row into v[0 .. 4): one 16-byte load (`aligned`: the address
// is a multiple of 16) or four dword loads
__device__ __forceinline__ void load_group(const float* __restrict__ row, int col0, bool aligned,
                                           float* v) {
  if (aligned) {
    const float4 t = *reinterpret_cast<const float4*>(row + col0);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = row[col0 + k];
  }
}

__device__ __forceinline__ int phase_of(const float* p) {
  return (int)(((uintptr_t)p >> 2) & 3);
}

// HAS_R / HAS_O: the inputs present; CMP: streams 2 and 3 too (both inputs); chunks: the tiles
// of a row, enough for the largest phase a row of this call has
template <bool HAS_R, bool HAS_O, bool CMP>
__global__ __launch_bounds__(SUM_THREADS) void summary_accumulate_kernel(
    const float* __restrict__ recon, int64_t ldr, const float* __restrict__ orig, int64_t ldo,
    int64_t rows, int64_t F, int64_t chunks, float tolerance, Partial* __restrict__ partials) {
  __shared__ Partial red[SUM_THREADS / WAVE];
  const float* first = HAS_R ? recon : orig;      // the input the groups are aligned to
  const int64_t ld1 = HAS_R ? ldr : ldo;
  const int64_t tiles = rows * chunks;
  const int F32 = (int)F;

  Partial acc[SUM_STREAMS];
#pragma unroll
  for (int s = 0; s < SUM_STREAMS; ++s) acc[s] = empty_partial();

  // tile t = blockIdx.x, + gridDim.x, ... as (row, tile of the row), stepped without a division
  const int64_t step_rows = (int64_t)gridDim.x / chunks, step_c = (int64_t)gridDim.x % chunks;
  int64_t row = (int64_t)blockIdx.x / chunks, c = (int64_t)blockIdx.x % chunks;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x, row += step_rows, c += step_c) {
    if (c >= chunks) c -= chunks, ++row;
    const float* row1 = first + row * ld1;
    const float* row2 = (HAS_R && HAS_O) ? orig + row * ldo : nullptr;
    const int phase = phase_of(row1);
    const bool same = (HAS_R && HAS_O) ? phase_of(row2) == phase : false;
    // The 16-byte loads of a tile are issued together, before anything waits for one.  A tile
    // that lies whole inside the row (all but the first and the last of a row, a test on scalars)
    // needs nothing else.  In the others a group that is not whole inside the row loads the
    // row's first whole group instead (the values are not used) and reads its own valid columns
    // one by one afterwards -- at most two groups of a row do; a row without a whole group
    // (F < 7 at the worst phase) is read column by column.  Columns are int32 (F < 2^31 - 8192).
    const int tile0 = (int)c * (int)SUM_TILE - phase;            // column of the tile's start
    const int base = tile0 + (int)threadIdx.x * 4;
    float a[SUM_CHUNK], b[SUM_CHUNK];             // first input; orig where there are two
    unsigned mask;
    if (tile0 >= 0 && tile0 + (int)SUM_TILE <= F32) {
#pragma unroll
      for (int g = 0; g < SUM_GROUPS; ++g)
        load_group(row1, base + g * SUM_THREADS * 4, true, a + 4 * g);
      if (HAS_R && HAS_O) {
#pragma unroll
        for (int g = 0; g < SUM_GROUPS; ++g)
          load_group(row2, base + g * SUM_THREADS * 4, same, b + 4 * g);
      }
      mask = (1u << SUM_CHUNK) - 1u;
    } else {
      const int first_whole = (4 - phase) & 3;
      const bool has_whole = first_whole + 3 < F32;
      int col0[SUM_GROUPS];
      mask = 0;
#pragma unroll
      for (int g = 0; g < SUM_GROUPS; ++g) {
        col0[g] = base + g * SUM_THREADS * 4;
        if (col0[g] >= 0 && col0[g] + 3 < F32) mask |= 0xFu << (4 * g);
      }
      if (has_whole) {
#pragma unroll
        for (int g = 0; g < SUM_GROUPS; ++g)
          load_group(row1, ((mask >> (4 * g)) & 1u) ? col0[g] : first_whole, true, a + 4 * g);
        if (HAS_R && HAS_O) {
#pragma unroll
          for (int g = 0; g < SUM_GROUPS; ++g)
            load_group(row2, ((mask >> (4 * g)) & 1u) ? col0[g] : first_whole, same, b + 4 * g);
        }
      } else {
#pragma unroll
        for (int i = 0; i < SUM_CHUNK; ++i) a[i] = b[i] = 0.f;
      }
#pragma unroll
      for (int g = 0; g < SUM_GROUPS; ++g) {
        if (!((mask >> (4 * g)) & 1u) && col0[g] + 3 >= 0 && col0[g] < F32) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int col = col0[g] + k;
            if (col >= 0 && col < F32) {
              a[4 * g + k] = row1[col];
              if (HAS_R && HAS_O) b[4 * g + k] = row2[col];
              mask |= 1u << (4 * g + k);
            }
          }
        }
      }
    }
    if (mask == 0) continue;
    add_elements<true>(acc[HAS_R ? 1 : 0], a, mask, tolerance);
    if (HAS_R && HAS_O) {
      add_elements<true>(acc[0], b, mask, tolerance);
      if (CMP) {
        double e[SUM_CHUNK];
#pragma unroll
        for (int i = 0; i < SUM_CHUNK; ++i) e[i] = fabs((double)a[i] - (double)b[i]);
        add_elements<false>(acc[2], e, mask, 0.0);
#pragma unroll
        for (int i = 0; i < SUM_CHUNK; ++i)
          e[i] = fabs(log1p((double)a[i]) - log1p((double)b[i]));
        add_elements<false>(acc[3], e, mask, 0.0);
      }
    }
  }

#pragma unroll
  for (int s = 0; s < SUM_STREAMS; ++s) {
    const bool live = s == 0 ? HAS_O : s == 1 ? HAS_R : CMP;
    Partial p = live ? block_join(acc[s], red) : empty_partial();
    if (threadIdx.x == 0) partials[(int64_t)blockIdx.x * SUM_STREAMS + s] = p;
  }
}

// state[s] <- join(state[s], the workgroups' partials of stream s in their fixed order); workgroup
// s of the launch takes stream s
__global__ __launch_bounds__(SUM_THREADS) void summary_merge_kernel(
    Partial* __restrict__ state, const Partial* __restrict__ partials, int blocks) {
  __shared__ Partial red[SUM_THREADS / WAVE];
  const int s = blockIdx.x;
  Partial p = empty_partial();
  for (int i = threadIdx.x; i < blocks; i += SUM_THREADS)
    p = join(p, partials[(int64_t)i * SUM_STREAMS + s]);
  p = block_join(p, red);
  if (threadIdx.x == 0) state[s] = join(state[s], p);
}

__global__ void summary_reset_kernel(Partial* __restrict__ state) {
  if (threadIdx.x < SUM_STREAMS) state[threadIdx.x] = empty_partial();
}

// stats[s] = (mean, standard deviation with ddof 1, minimum, maximum), counts[s] = (n, count)
__global__ void summary_finish_kernel(const Partial* __restrict__ state,
                                      double* __restrict__ stats, int64_t* __restrict__ counts) {
  const int s = threadIdx.x;
  if (s >= SUM_STREAMS) return;
  const Partial p = state[s];
  const double n = (double)p.n;
  const double nan = __builtin_nan("");
  stats[4 * s + 0] = p.n > 0 ? p.sum / n : nan;
  stats[4 * s + 1] = p.n > 1 ? sqrt(p.m2 / (n - 1.0)) : nan;
  stats[4 * s + 2] = p.n > 0 ? p.lo : nan;
  stats[4 * s + 3] = p.n > 0 ? p.hi : nan;
  counts[2 * s + 0] = p.n;
  counts[2 * s + 1] = p.count;
}

}  // namespace
}  // namespace scvae

#define SCVAE_SUMMARY_WORKSPACE(workspace, workspace_bytes)                 \
  SCVAE_ARG(workspace && ((uintptr_t)workspace & 7) == 0);                  \
  SCVAE_ARG(workspace_bytes >= scvae::SUM_WORKSPACE_BYTES)

extern "C" {

int64_t scvae_summary_workspace_bytes(void) { return scvae::SUM_WORKSPACE_BYTES; }

int scvae_summary_reset(void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace scvae;
  SCVAE_SUMMARY_WORKSPACE(workspace, workspace_bytes);
  hipLaunchKernelGGL(summary_reset_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream,
                     static_cast<Partial*>(workspace));
  SCVAE_LAUNCH_CHECK("summary_reset_kernel");
  return 0;
}

int scvae_summary_accumulate(const float* recon, int64_t ldr, const float* orig, int64_t ldo,
                             int64_t rows, int64_t F, double tolerance, int32_t comparisons,
                             void* workspace, int64_t workspace_bytes, void* stream) {
  using namespace scvae;
  SCVAE_ARG(rows >= 1 && F >= 1);
  SCVAE_ARG(tolerance == tolerance);
  SCVAE_ARG(F <= INT32_MAX - 2 * SUM_TILE);
  SCVAE_ARG(recon || orig);
  SCVAE_ARG(!recon || (ldr >= F && ((uintptr_t)recon & 3) == 0));
  SCVAE_ARG(!orig || (ldo >= F && ((uintptr_t)orig & 3) == 0));
  SCVAE_ARG(!comparisons || (recon && orig));
  SCVAE_ARG(rows <= INT64_MAX / 4 / (ldr > ldo ? ldr : ldo));
  SCVAE_SUMMARY_WORKSPACE(workspace, workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  Partial* state = static_cast<Partial*>(workspace);
  Partial* partials = state + SUM_STREAMS;
  // the lowest fp32 value at or above the tolerance: for an fp32 element e, e >= it exactly
  // when (double)e >= tolerance
  float tolerance_f = (float)tolerance;
  if ((double)tolerance_f < tolerance) tolerance_f = nextafterf(tolerance_f, INFINITY);
  // the phase of a row repeats after at most four rows: tiles for the largest one of this call
  const float* first = recon ? recon : orig;
  const int64_t ld1 = recon ? ldr : ldo;
  int64_t phase = 0;
  for (int64_t r = 0; r < rows && r < 4; ++r) {
    const int64_t p = (int64_t)((((uintptr_t)first >> 2) + (uint64_t)(r * ld1)) & 3);
    if (p > phase) phase = p;
  }
  const int64_t chunks = (F + phase + SUM_TILE - 1) / SUM_TILE;
  const int64_t tiles = rows * chunks;
  const int blocks = (int)(tiles < SUM_MAX_BLOCKS ? tiles : SUM_MAX_BLOCKS);
#define SCVAE_SUMMARY_LAUNCH(R, O, C)                                                          \
  hipLaunchKernelGGL((summary_accumulate_kernel<R, O, C>), dim3(blocks), dim3(SUM_THREADS), 0, \
                     st, recon, ldr, orig, ldo, rows, F, chunks, tolerance_f, partials)
  if (recon && orig && comparisons) SCVAE_SUMMARY_LAUNCH(true, true, true);
  else if (recon && orig) SCVAE_SUMMARY_LAUNCH(true, true, false);
  else if (recon) SCVAE_SUMMARY_LAUNCH(true, false, false);
  else SCVAE_SUMMARY_LAUNCH(false, true, false);
#undef SCVAE_SUMMARY_LAUNCH
  SCVAE_LAUNCH_CHECK("summary_accumulate_kernel");
  hipLaunchKernelGGL(summary_merge_kernel, dim3(SUM_STREAMS), dim3(SUM_THREADS), 0, st, state,
                     partials, blocks);
  SCVAE_LAUNCH_CHECK("summary_merge_kernel");
  return 0;
}

int scvae_summary_finish(const void* workspace, int64_t workspace_bytes, double* stats,
                         int64_t* counts, void* stream) {
  using namespace scvae;
  SCVAE_SUMMARY_WORKSPACE(workspace, workspace_bytes);
  SCVAE_ARG(stats && counts);
  SCVAE_ARG(((uintptr_t)stats & 7) == 0 && ((uintptr_t)counts & 7) == 0);
  hipLaunchKernelGGL(summary_finish_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream,
                     static_cast<const Partial*>(workspace), stats, counts);
  SCVAE_LAUNCH_CHECK("summary_finish_kernel");
  return 0;
}

}  // extern "C"
