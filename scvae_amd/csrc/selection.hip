// Feature selection and example filters on a CSR count matrix
// (scvae/data/processing.py:95-166 `select_features`: values.sum(axis=0) / values.var(axis=0) over
// the genes; :169-302 `filter_examples` and the `values[:, indices]` / `values[filter_indices, :]`
// that both end in).
//
// 1. scvae_csr_feature_moments: per gene j the exact integers sum_j = sum_i x_ij,
//    sum_sq_j = sum_i x_ij^2 and the number of stored values != 0, for counts in [0, 65535].
//    The moments of a gene do not depend on which row a stored entry belongs to, so the kernel
//    partitions the stored entries indptr[0] .. indptr[n_rows] - 1 as they lie in memory, not the
//    rows: empty rows cost nothing, a long row is split like any other stretch, and every read of
//    `indices` is a contiguous, coalesced one.
//
//    A workgroup owns one slab of MOM_SLAB genes and one stretch of entries.  It keeps two 64-bit
//    words per gene of the slab in LDS,
//
//      word 0:  bits 0 .. 39  sum of the values,  bits 40 .. 63  number of values != 0
//      word 1:  sum of the squared values
//
//    and adds every entry of its stretch whose column lies in the slab with two 64-bit LDS adds
//    (one global atomic per stored value is what this avoids).  A stretch holds at most
//    MOM_FLUSH = 2^23 entries between two flushes, which is the bound that keeps the fields apart:
//
//      number of values        <= 2^23                      < 2^24  (bits 40 .. 63)
//      sum of the values       <= 2^23 (2^16 - 1)           < 2^39  (bits 0 .. 39)
//      sum of the squares      <= 2^23 (2^16 - 1)^2         < 2^55  (word 1)
//
//    The kernel's loop enforces it (MOM_FLUSH is the largest stretch it takes before a flush).  A
//    flush adds the slab to the results with one 64-bit integer atomic per result and touched
//    gene.  The results hold for a gene with fewer than 2^31 values != 0:
//    sum_sq <= (2^31 - 1)(2^16 - 1)^2 < 2^63; n_rows <= 2^31 - 1 gives that for a matrix without
//    duplicate entries, and the flush sets bit 2 of `bad` where a gene reaches 2^31 all the same.
//    All arithmetic is integer addition: the results are the same bits for every launch geometry
//    and on every run.
//
//    The entries are read once per slab (the 4-byte column index; the value only where the column
//    lies in the slab, which with sorted rows is a contiguous part of the row): F / MOM_SLAB
//    passes over `indices` and one over `values`.
//
// 2. scvae_csr_submatrix_count / _fill: the rows `rows[o]` (all rows in order without a list) and
//    the columns with column_map[c] >= 0 (all without a map) as a new CSR.  One wave per output
//    row; the fill keeps the order of the entries of a row with a wave-level prefix over the keep
//    predicate, so explicitly stored zeros stay and a monotone map keeps sorted rows sorted.
//    Entry offsets are int64 throughout.
#include "../../include/scvae_hip.h"
#include "common.hpp"

namespace scvae {
namespace {

constexpr int MOM_THREADS = 1024;
constexpr int MOM_SLAB = 8192;                       // genes of a slab: 2 x 8 B x 8192 = 128 KiB of LDS
constexpr int MOM_LDS_BYTES = MOM_SLAB * 2 * (int)sizeof(unsigned long long);
constexpr int MOM_UNROLL = 4;                        // column indices a thread has in flight
constexpr int64_t MOM_FLUSH = (int64_t)1 << 23;      // entries between two flushes (bound above)
constexpr int MOM_GROUPS = 512;                      // workgroups of a launch, about: 2 per CU
constexpr int MOM_COUNT_SHIFT = 40;
constexpr unsigned long long MOM_SUM_MASK = (1ull << MOM_COUNT_SHIFT) - 1;
static_assert(MOM_FLUSH * 65535 < (1ll << (MOM_COUNT_SHIFT - 1)), "sum field");
static_assert(MOM_FLUSH < (1ll << (64 - MOM_COUNT_SHIFT)), "count field");
static_assert(MOM_FLUSH % (MOM_THREADS * MOM_UNROLL) == 0, "whole tiles in a stretch");

constexpr int BAD_VALUE = 1, BAD_COLUMN = 2, BAD_OVERFLOW = 4, BAD_ROW = 8, BAD_OFFSETS = 16;

// grid: x = stretch of entries, y = slab of genes
__global__ __launch_bounds__(MOM_THREADS) void feature_moments_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const float* __restrict__ values, int64_t n_rows, int32_t F,
    unsigned long long* __restrict__ sum, unsigned long long* __restrict__ sum_sq,
    unsigned long long* __restrict__ nonzeros, int32_t* __restrict__ bad) {
  extern __shared__ unsigned long long slab[];       // [MOM_SLAB][2]
  const int64_t first = indptr[0], last = indptr[n_rows];
  const int64_t total = last - first;
  if (total <= 0) return;
  // a stretch: the entries split evenly over gridDim.x, in whole tiles, at most MOM_FLUSH
  constexpr int64_t TILE = (int64_t)MOM_THREADS * MOM_UNROLL;
  int64_t span = (total + gridDim.x - 1) / gridDim.x;
  span = (span + TILE - 1) / TILE * TILE;
  if (span > MOM_FLUSH) span = MOM_FLUSH;
  const int32_t gene0 = (int32_t)blockIdx.y * MOM_SLAB;
  const int32_t genes = min(MOM_SLAB, F - gene0);
  const bool checks = blockIdx.y == 0;               // one slab's workgroups judge the columns
  int flags = 0;
  bool clean = false;                                // the slab in LDS is all zero

  for (int64_t begin = first + (int64_t)blockIdx.x * span; begin < last;
       begin += (int64_t)gridDim.x * span) {
    const int64_t end = min(begin + span, last);
    if (!clean) {
      for (int g = threadIdx.x; g < 2 * MOM_SLAB; g += MOM_THREADS) slab[g] = 0ull;
      clean = true;
    }
    __syncthreads();
    for (int64_t tile = begin; tile < end; tile += TILE) {
      int32_t col[MOM_UNROLL];
#pragma unroll
      for (int u = 0; u < MOM_UNROLL; ++u) {
        const int64_t e = tile + u * MOM_THREADS + threadIdx.x;
        col[u] = e < end ? indices[e] : -1;
      }
#pragma unroll
      for (int u = 0; u < MOM_UNROLL; ++u) {
        const int64_t e = tile + u * MOM_THREADS + threadIdx.x;
        if (e >= end) continue;
        if (checks && (col[u] < 0 || col[u] >= F)) flags |= BAD_COLUMN;
        const int32_t g = col[u] - gene0;
        if (g < 0 || g >= genes) continue;
        const float v = values[e];
        if (!(v >= 0.f && v <= 65535.f && v == truncf(v))) {
          flags |= BAD_VALUE;
          continue;
        }
        if (v == 0.f) continue;
        const unsigned long long x = (unsigned long long)v;
        atomicAdd(&slab[2 * g], x | (1ull << MOM_COUNT_SHIFT));
        atomicAdd(&slab[2 * g + 1], x * x);
      }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < genes; g += MOM_THREADS) {
      const unsigned long long packed = slab[2 * g];
      if (packed == 0ull) continue;
      const unsigned long long count = packed >> MOM_COUNT_SHIFT;
      atomicAdd(&sum[gene0 + g], packed & MOM_SUM_MASK);
      atomicAdd(&sum_sq[gene0 + g], slab[2 * g + 1]);
      const unsigned long long before = atomicAdd(&nonzeros[gene0 + g], count);
      if (before + count >= (1ull << 31)) flags |= BAD_OVERFLOW;
      slab[2 * g] = 0ull;
      slab[2 * g + 1] = 0ull;
    }
    // (the zeroed words are this thread's own in the next pass's flush, and other threads add to
    //  them only after the barrier at the top of the pass)
  }
  if (flags) atomicOr(bad, flags);
}

constexpr int SUB_THREADS = 256;
constexpr int SUB_WAVES = SUB_THREADS / WAVE;

// the row of the input that output row o is, or -1 (and the flag) for one outside the matrix
__device__ __forceinline__ int64_t source_row(const int64_t* __restrict__ rows, int64_t o,
                                              int64_t n_rows, int& flags) {
  const int64_t r = rows ? rows[o] : o;
  if (r < 0 || r >= n_rows) {
    flags |= BAD_ROW;
    return -1;
  }
  return r;
}

// the new column of an entry, or -1 for one that is dropped
__device__ __forceinline__ int32_t new_column(const int32_t* __restrict__ column_map, int32_t c,
                                              int32_t F, int& flags) {
  if (c < 0 || c >= F) {
    flags |= BAD_COLUMN;
    return -1;
  }
  return column_map ? column_map[c] : c;
}

__global__ __launch_bounds__(SUB_THREADS) void submatrix_count_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows,
    int32_t F, const int64_t* __restrict__ rows, int64_t n_out,
    const int32_t* __restrict__ column_map, int64_t* __restrict__ counts,
    int32_t* __restrict__ bad) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t o = (int64_t)blockIdx.x * SUB_WAVES + threadIdx.x / WAVE;
  if (o >= n_out) return;
  int flags = 0;
  const int64_t r = source_row(rows, o, n_rows, flags);
  int64_t kept = 0;
  if (r >= 0) {
    const int64_t begin = indptr[r], end = indptr[r + 1];
    for (int64_t e0 = begin; e0 < end; e0 += WAVE) {
      const int64_t e = e0 + lane;
      const bool keep = e < end && new_column(column_map, indices[e], F, flags) >= 0;
      kept += __popcll(__builtin_amdgcn_ballot_w64(keep));
    }
  }
  if (lane == 0) counts[o] = kept;
  if (flags) atomicOr(bad, flags);
}

__global__ __launch_bounds__(SUB_THREADS) void submatrix_fill_kernel(
    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
    const float* __restrict__ values, int64_t n_rows, int32_t F, const int64_t* __restrict__ rows,
    int64_t n_out, const int32_t* __restrict__ column_map, const int64_t* __restrict__ out_indptr,
    int32_t* __restrict__ out_indices, float* __restrict__ out_values, int32_t* __restrict__ bad) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t o = (int64_t)blockIdx.x * SUB_WAVES + threadIdx.x / WAVE;
  if (o >= n_out) return;
  int flags = 0;
  const int64_t r = source_row(rows, o, n_rows, flags);
  if (r >= 0) {
    // the output row's own room: nothing is written outside it, whatever the offsets say
    int64_t out = out_indptr[o];
    const int64_t out_end = out_indptr[o + 1];
    const int64_t begin = indptr[r], end = indptr[r + 1];
    for (int64_t e0 = begin; e0 < end; e0 += WAVE) {
      const int64_t e = e0 + lane;
      const int32_t c = e < end ? new_column(column_map, indices[e], F, flags) : -1;
      const bool keep = c >= 0;
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
      if (keep) {
        const int64_t at = out + __popcll(mask & ((1ull << lane) - 1ull));
        if (at >= out && at < out_end) {
          out_indices[at] = c;
          out_values[at] = values[e];
        } else {
          flags |= BAD_OFFSETS;
        }
      }
      out += __popcll(mask);
    }
    if (out != out_end) flags |= BAD_OFFSETS;
  }
  if (flags) atomicOr(bad, flags);
}

}  // namespace
}  // namespace scvae

extern "C" {

int scvae_csr_feature_moments(const int64_t* indptr, const int32_t* indices, const float* values,
                              int64_t n_rows, int64_t F, uint64_t* sum, uint64_t* sum_sq,
                              int64_t* nonzeros, int32_t* bad, void* stream) {
  using namespace scvae;
  SCVAE_ARG(n_rows >= 1 && n_rows <= INT32_MAX);
  SCVAE_ARG(F >= 1 && F <= ((int64_t)1 << 20));
  SCVAE_ARG(indptr && sum && sum_sq && nonzeros && bad);
  SCVAE_ARG(((uintptr_t)indptr & 7) == 0 && ((uintptr_t)sum & 7) == 0 &&
            ((uintptr_t)sum_sq & 7) == 0 && ((uintptr_t)nonzeros & 7) == 0);
  SCVAE_ARG(((uintptr_t)indices & 3) == 0 && ((uintptr_t)values & 3) == 0 &&
            ((uintptr_t)bad & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  SCVAE_HIP(hipMemsetAsync(sum, 0, (size_t)F * sizeof(uint64_t), st));
  SCVAE_HIP(hipMemsetAsync(sum_sq, 0, (size_t)F * sizeof(uint64_t), st));
  SCVAE_HIP(hipMemsetAsync(nonzeros, 0, (size_t)F * sizeof(int64_t), st));
  const int slabs = (int)((F + MOM_SLAB - 1) / MOM_SLAB);
  const int stretches = slabs >= MOM_GROUPS ? 1 : MOM_GROUPS / slabs;
  SCVAE_HIP(max_dynamic_lds((const void*)feature_moments_kernel, MOM_LDS_BYTES));
  hipLaunchKernelGGL(feature_moments_kernel, dim3(stretches, slabs), dim3(MOM_THREADS),
                     MOM_LDS_BYTES, st, indptr, indices, values, n_rows, (int32_t)F,
                     reinterpret_cast<unsigned long long*>(sum),
                     reinterpret_cast<unsigned long long*>(sum_sq),
                     reinterpret_cast<unsigned long long*>(nonzeros), bad);
  SCVAE_LAUNCH_CHECK("feature_moments_kernel");
  return 0;
}

#define SCVAE_SUBMATRIX_ARGS()                                                               \
  SCVAE_ARG(n_rows >= 1 && n_rows <= INT32_MAX);                                             \
  SCVAE_ARG(F >= 1 && F <= INT32_MAX);                                                       \
  SCVAE_ARG(n_out >= 0 && n_out <= INT32_MAX);                                               \
  SCVAE_ARG(rows || n_out == n_rows);                                                        \
  SCVAE_ARG(indptr && bad);                                                                  \
  SCVAE_ARG(((uintptr_t)indptr & 7) == 0 && ((uintptr_t)rows & 7) == 0);                     \
  SCVAE_ARG(((uintptr_t)indices & 3) == 0 && ((uintptr_t)column_map & 3) == 0 &&             \
            ((uintptr_t)bad & 3) == 0)

int scvae_csr_submatrix_count(const int64_t* indptr, const int32_t* indices, int64_t n_rows,
                              int64_t F, const int64_t* rows, int64_t n_out,
                              const int32_t* column_map, int64_t* out_counts, int32_t* bad,
                              void* stream) {
  using namespace scvae;
  SCVAE_SUBMATRIX_ARGS();
  SCVAE_ARG(out_counts || n_out == 0);
  SCVAE_ARG(((uintptr_t)out_counts & 7) == 0);
  if (n_out == 0) return 0;
  const int64_t blocks = (n_out + SUB_WAVES - 1) / SUB_WAVES;
  hipLaunchKernelGGL(submatrix_count_kernel, dim3((unsigned)blocks), dim3(SUB_THREADS), 0,
                     (hipStream_t)stream, indptr, indices, n_rows, (int32_t)F, rows, n_out,
                     column_map, out_counts, bad);
  SCVAE_LAUNCH_CHECK("submatrix_count_kernel");
  return 0;
}

int scvae_csr_submatrix_fill(const int64_t* indptr, const int32_t* indices, const float* values,
                             int64_t n_rows, int64_t F, const int64_t* rows, int64_t n_out,
                             const int32_t* column_map, const int64_t* out_indptr,
                             int32_t* out_indices, float* out_values, int32_t* bad,
                             void* stream) {
  using namespace scvae;
  SCVAE_SUBMATRIX_ARGS();
  SCVAE_ARG(out_indptr);
  SCVAE_ARG(((uintptr_t)out_indptr & 7) == 0);
  SCVAE_ARG(((uintptr_t)values & 3) == 0 && ((uintptr_t)out_indices & 3) == 0 &&
            ((uintptr_t)out_values & 3) == 0);
  if (n_out == 0) return 0;
  const int64_t blocks = (n_out + SUB_WAVES - 1) / SUB_WAVES;
  hipLaunchKernelGGL(submatrix_fill_kernel, dim3((unsigned)blocks), dim3(SUB_THREADS), 0,
                     (hipStream_t)stream, indptr, indices, values, n_rows, (int32_t)F, rows, n_out,
                     column_map, out_indptr, out_indices, out_values, bad);
  SCVAE_LAUNCH_CHECK("submatrix_fill_kernel");
  return 0;
}

#undef SCVAE_SUBMATRIX_ARGS

}  // extern "C"
