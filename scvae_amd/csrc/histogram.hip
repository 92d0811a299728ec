// Distributions of a resident fp32 matrix (scvae/analyses/subanalyses.py:119-192 "Count
// distribution" and "Count sum distribution", scvae/analyses/figures/histograms.py:142-179, and
// the numpy.histogram / numpy.percentile those call): an exact histogram over given edges, exact
// order statistics without a sort or a copy, and fp64 row sums.
//
// All three read x [rows, F] fp32 with a row pitch ldx >= F and int64 element offsets; a flat
// array is rows = 1 (F up to 2^40).  With `shift` the element is fl32(x + 1.0f), the reference's
// `series += 1` (histograms.py:160).
//
// Addressing, as in summary.hip but with int64 columns: a row is walked in "virtual columns"
// v = column + phase, phase = the number of floats the row's first element lies past a 16-byte
// boundary, so that a group of 4 virtual columns at a multiple of 4 is one aligned 16-byte load
// wherever all 4 columns lie in [0, F); the at most two groups that straddle the row's ends read
// their valid columns one by one.  Nothing outside [0, F) of a row is ever read.  A tile is
// THREADS x 16 virtual columns: a thread holds four 16-byte groups, all issued before the first
// is used.
//
// 1. scvae_histogram_accumulate.  A workgroup owns one slab of up to HIST_SLAB = 8192 bins (grid
//    y) and a share of the tiles (grid x).  It keeps the slab's edges in their own type and one
//    32-bit count per bin in LDS: 4 (w + 1) + 4 w bytes for a slab of w bins with fp32 edges
//    (64 KiB at the most: two workgroups a CU), 8 (w + 1) + 4 w with fp64 edges (96 KiB).  An
//    element belongs to the slab exactly when
//    e[s0] <= x < e[s0 + w] (<= for the last slab, whose last bin is closed): with non-decreasing
//    edges the largest i with e[i] <= x then lies in [s0, s0 + w).  Elements of other slabs cost
//    those two comparisons and nothing else.  Inside the slab the index is estimated as
//    (x - e[0]) n / (e[n] - e[0]) in fp64 and then walked down while x < e[i] and up while
//    x >= e[i + 1], as far as it takes: the definition holds whatever the estimate was (uniform
//    edges end the walk after at most a step or two; repeated edges walk to the last of them).
//    Comparisons are in the edges' type: fp64 against fp64 edges, and fp32 against fp32 edges,
//    where an fp32 element compares as it would in fp64.
//
//    Counting: about 95 % of a reconstruction falls into one or two bins, and 64 lanes adding to
//    one LDS address serialise.  So before the LDS add a wave takes the bin of its first pending
//    lane, ballots the lanes with the same bin, and that lane adds the popcount once; two such
//    rounds (each only while it finds at least two equal lanes), then the lanes still pending
//    add 1 each.  On values spread over many bins the ballots only cost, so the first of a
//    thread's 16 elements of a tile probes: the other 15 aggregate only where its first round
//    found 16 or more lanes equal.  A workgroup flushes its slab every HIST_FLUSH_TILES tiles at the latest
//    (2^17 tiles x 2^14 elements = 2^31 < 2^32, the bound that keeps a 32-bit count from
//    wrapping) and at its end: one 64-bit integer atomic per touched bin.  Elements below e[0],
//    above e[n] and NaN are counted in registers by the workgroups of slab 0 and added to the
//    three cells of `outside`.  Integer additions only: the same bits for every launch geometry
//    and on every run.
//
// 2. scvae_order_statistics: radix select on the order-preserving map of the fp32 bits
//    (negative: all bits flipped; else the sign bit set; so -0.0 < +0.0), three passes of
//    11 / 11 / 10 bits.  Pass p counts, for every rank, the digit of the elements whose key
//    matches the rank's prefix so far (ranks with one prefix share one histogram), in LDS with
//    the same wave aggregation and 32-bit counts, flushed into 64-bit totals.  Between passes a
//    one-workgroup kernel picks each rank's digit (wave k takes rank k: 64 partial sums, a
//    shuffle scan, then the lane whose stretch holds the rank walks it).  NaN elements are
//    counted apart and never selected; a rank past the last non-NaN element gives NaN, which is
//    where a sort puts them.  Minimum and maximum come from integer atomics on the keys of the
//    first pass.  With `shift` the selection is on x and the results are fl32(r + 1): x -> fl32(x
//    + 1) is non-decreasing, so order statistics commute with it.
//
// 3. scvae_row_sums_f64: one workgroup of 256 threads per row; a thread adds its elements in
//    fp64 in the order of the tiles, the lanes join by a shuffle-down tree, the 4 waves in
//    order, and the sum is rounded once to fp32.  One fixed order whatever the launch.
#include "../../include/scvae_hip.h"
#include "common.hpp"

namespace scvae {
namespace {

#pragma clang fp contract(off)

constexpr int HIST_THREADS = 1024;
constexpr int HIST_CHUNK = 16;                         // elements a thread holds: 4 groups of 4
constexpr int HIST_SLAB = 8192;                        // bins of a slab
constexpr int64_t HIST_FLUSH_TILES = (int64_t)1 << 17; // tiles of a workgroup between flushes
constexpr int HIST_GROUPS_TARGET = 512;                // workgroups of a launch, about
constexpr int ROWSUM_THREADS = 256;
constexpr int SEL_RANKS = 4;
constexpr int SEL_DIGITS = 2048;                       // 11 bits, the widest pass
static_assert(HIST_FLUSH_TILES * HIST_THREADS * HIST_CHUNK <= ((int64_t)1 << 31), "32-bit counts");

__device__ __forceinline__ int phase_of(const float* p) {
  return (int)(((uintptr_t)p >> 2) & 3);
}

// tiles of a row, enough for every phase
template <int THREADS>
__host__ __device__ constexpr int64_t tiles_of_row(int64_t F) {
  return (F + 3 + (int64_t)THREADS * HIST_CHUNK - 1) / ((int64_t)THREADS * HIST_CHUNK);
}

// the thread's 16 elements of tile c of a row into v; bit i of the result: v[i] is an element
template <int THREADS>
__device__ __forceinline__ unsigned load_tile(const float* __restrict__ row, int64_t F, int64_t c,
                                              float (&v)[HIST_CHUNK]) {
  constexpr int64_t TILE = (int64_t)THREADS * HIST_CHUNK;
  const int64_t tile0 = c * TILE - phase_of(row);       // column of the tile's start
  const int64_t base = tile0 + (int64_t)threadIdx.x * 4;
  if (tile0 >= 0 && tile0 + TILE <= F) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 t = *reinterpret_cast<const float4*>(row + base + (int64_t)g * THREADS * 4);
      v[4 * g] = t.x, v[4 * g + 1] = t.y, v[4 * g + 2] = t.z, v[4 * g + 3] = t.w;
    }
    return 0xFFFFu;
  }
  unsigned mask = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int64_t col0 = base + (int64_t)g * THREADS * 4;
    if (col0 >= 0 && col0 + 3 < F) {
      const float4 t = *reinterpret_cast<const float4*>(row + col0);
      v[4 * g] = t.x, v[4 * g + 1] = t.y, v[4 * g + 2] = t.z, v[4 * g + 3] = t.w;
      mask |= 0xFu << (4 * g);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t col = col0 + k;
        const bool in = col >= 0 && col < F;
        v[4 * g + k] = in ? row[col] : 0.f;
        if (in) mask |= 1u << (4 * g + k);
      }
    }
  }
  return mask;
}

// cnt[b] += 1 for every lane with b >= 0.  Called by whole waves (it ballots).  With `aggregate`
// (the same for the whole wave) up to two rounds of: the lanes whose bin is the first pending
// lane's add their number once.  Returns how many lanes the first round found equal (0 without
// `aggregate`): the caller's measure of whether aggregating pays for the elements that follow.
__device__ __forceinline__ int lds_count(unsigned* cnt, int b, bool aggregate) {
  int first_equal = 0;
  if (aggregate) {
    const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      const unsigned long long pending = __builtin_amdgcn_ballot_w64(b >= 0);
      if (pending == 0ull) break;
      const int leader = __builtin_ctzll(pending);
      const int lb = __builtin_amdgcn_readlane(b, __builtin_amdgcn_readfirstlane(leader));
      const bool same = b == lb;
      const int equal = __popcll(__builtin_amdgcn_ballot_w64(same));
      if (round == 0) first_equal = equal;
      if (equal < 2) break;
      if (lane == leader) atomicAdd(&cnt[lb], (unsigned)equal);
      if (same) b = -1;
    }
  }
  if (b >= 0) atomicAdd(&cnt[b], 1u);
  return first_equal;
}
// a tile's first element probes; the other 15 aggregate where it found this many lanes equal
constexpr int HIST_AGGREGATE_FROM = 16;

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// the walk over the tiles blockIdx.x, + gridDim.x, ... as (row, tile of the row), stepped without
// a division (summary.hip)
struct TileWalk {
  int64_t row, c, step_rows, step_c, chunks;
  __device__ __forceinline__ TileWalk(int64_t chunks_) : chunks(chunks_) {
    step_rows = (int64_t)gridDim.x / chunks, step_c = (int64_t)gridDim.x % chunks;
    row = (int64_t)blockIdx.x / chunks, c = (int64_t)blockIdx.x % chunks;
  }
  __device__ __forceinline__ void next() {
    row += step_rows, c += step_c;
    if (c >= chunks) c -= chunks, ++row;
  }
};

// grid: x = share of the tiles, y = slab of bins.  E: the type of the edges, and of every
// comparison: fp32 elements against fp32 edges compare in fp32 as they do in fp64
template <typename E, bool SHIFT, bool AGGREGATE>
__global__ __launch_bounds__(HIST_THREADS, 8) void histogram_kernel(
    const float* __restrict__ x, int64_t ld, int64_t rows, int64_t F, int64_t chunks,
    const E* __restrict__ edges, int n_bins, unsigned long long* __restrict__ counts,
    unsigned long long* __restrict__ outside) {
  extern __shared__ double hist_lds[];               // edges [width + 1], then counts u32 [width]
  const int s0 = (int)blockIdx.y * HIST_SLAB;
  const int width = min(HIST_SLAB, n_bins - s0);
  E* led = reinterpret_cast<E*>(hist_lds);
  unsigned* cnt = reinterpret_cast<unsigned*>(led + width + 1);
  for (int i = threadIdx.x; i <= width; i += HIST_THREADS) led[i] = edges[s0 + i];
  for (int i = threadIdx.x; i < width; i += HIST_THREADS) cnt[i] = 0u;
  const E e0 = edges[0], eN = edges[n_bins];
  const E lo = edges[s0], hi = edges[s0 + width];
  const bool last = s0 + width == n_bins, sides = blockIdx.y == 0;
  // (the estimate only: in fp64 for either type, so that it is as near as it can be)
  const double scale = eN > e0 ? (double)n_bins / ((double)eN - (double)e0) : 0.0;
  unsigned n_below = 0, n_above = 0, n_nan = 0;
  __syncthreads();

  const int64_t tiles = rows * chunks;
  TileWalk walk(chunks);
  int64_t since_flush = 0;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x, walk.next()) {
    float v[HIST_CHUNK];
    const unsigned mask = load_tile<HIST_THREADS>(x + walk.row * ld, F, walk.c, v);
    bool aggregate = AGGREGATE;
#pragma unroll
    for (int i = 0; i < HIST_CHUNK; ++i) {
      int b = -1;
      if ((mask >> i) & 1u) {
        const float xf = SHIFT ? v[i] + 1.0f : v[i];
        const E xd = (E)xf;
        if (xd >= lo && (last ? xd <= hi : xd < hi)) {
          int li = (int)(((double)xd - (double)e0) * scale) - s0;
          li = max(0, min(width - 1, li));
          while (li > 0 && xd < led[li]) --li;
          while (li < width - 1 && xd >= led[li + 1]) ++li;
          b = li;
        } else if (sides) {
          if (xd != xd) ++n_nan;
          else if (xd < e0) ++n_below;
          else if (xd > eN) ++n_above;
        }
      }
      const int equal = lds_count(cnt, b, aggregate);
      if (AGGREGATE && i == 0) aggregate = equal >= HIST_AGGREGATE_FROM;
    }
    if (++since_flush == HIST_FLUSH_TILES || t + gridDim.x >= tiles) {
      since_flush = 0;
      __syncthreads();
      for (int i = threadIdx.x; i < width; i += HIST_THREADS) {
        const unsigned c = cnt[i];
        if (c) {
          atomicAdd(&counts[s0 + i], (unsigned long long)c);
          cnt[i] = 0u;
        }
      }
      if (sides) {
        const unsigned b = wave_sum_u32(n_below), a = wave_sum_u32(n_above),
                       n = wave_sum_u32(n_nan);
        if ((threadIdx.x & (WAVE - 1)) == 0) {
          if (b) atomicAdd(&outside[0], (unsigned long long)b);
          if (a) atomicAdd(&outside[1], (unsigned long long)a);
          if (n) atomicAdd(&outside[2], (unsigned long long)n);
        }
        n_below = n_above = n_nan = 0;
      }
      __syncthreads();
    }
  }
}

// ---- order statistics ----

struct SelectState {
  unsigned long long hist[SEL_RANKS][SEL_DIGITS];
  unsigned long long remaining[SEL_RANKS];   // the rank among the elements with the prefix
  unsigned long long n_valid, n_nan;
  unsigned prefix[SEL_RANKS];
  int slot[SEL_RANKS];                        // the histogram of the rank; -1: no such element
  unsigned key_min, key_max;
  int n_ranks, pad;
};

struct SelectRanks {
  int64_t r[SEL_RANKS];
};

__device__ __forceinline__ unsigned key_of(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__global__ __launch_bounds__(HIST_THREADS) void select_init_kernel(SelectState* __restrict__ st,
                                                                   SelectRanks ranks,
                                                                   int n_ranks) {
  unsigned long long* h = &st->hist[0][0];
  for (int i = threadIdx.x; i < SEL_RANKS * SEL_DIGITS; i += HIST_THREADS) h[i] = 0ull;
  if (threadIdx.x < SEL_RANKS) {
    const int k = threadIdx.x;
    st->remaining[k] = k < n_ranks ? (unsigned long long)ranks.r[k] : 0ull;
    st->prefix[k] = 0u;
    st->slot[k] = k < n_ranks ? 0 : -1;       // no prefix yet: one histogram for all
  }
  if (threadIdx.x == 0) {
    st->n_valid = 0ull, st->n_nan = 0ull;
    st->key_min = 0xFFFFFFFFu, st->key_max = 0u;
    st->n_ranks = n_ranks, st->pad = 0;
  }
}

// PASS 0: bits 31..21 of every element; 1: bits 20..10 under an 11-bit prefix; 2: bits 9..0
// under a 22-bit prefix
template <int PASS>
__global__ __launch_bounds__(HIST_THREADS, 8) void select_pass_kernel(
    const float* __restrict__ x, int64_t ld, int64_t rows, int64_t F, int64_t chunks,
    SelectState* __restrict__ st) {
  __shared__ unsigned lh[SEL_RANKS][SEL_DIGITS];
  for (int i = threadIdx.x; i < SEL_RANKS * SEL_DIGITS; i += HIST_THREADS) (&lh[0][0])[i] = 0u;
  bool active[SEL_RANKS];
  unsigned prefix[SEL_RANKS];
#pragma unroll
  for (int j = 0; j < SEL_RANKS; ++j) {
    active[j] = __builtin_amdgcn_readfirstlane(st->slot[j]) == j;
    prefix[j] = __builtin_amdgcn_readfirstlane(st->prefix[j]);
  }
  unsigned n_nan = 0, kmin = 0xFFFFFFFFu, kmax = 0u;
  __syncthreads();

  const int64_t tiles = rows * chunks;
  TileWalk walk(chunks);
  int64_t since_flush = 0;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x, walk.next()) {
    float v[HIST_CHUNK];
    const unsigned mask = load_tile<HIST_THREADS>(x + walk.row * ld, F, walk.c, v);
    bool aggregate[SEL_RANKS] = {true, true, true, true};
#pragma unroll
    for (int i = 0; i < HIST_CHUNK; ++i) {
      const bool is = (mask >> i) & 1u;
      const bool nan = v[i] != v[i];
      const bool valid = is && !nan;
      const unsigned key = key_of(v[i]);
      if (PASS == 0) {
        if (is && nan) ++n_nan;
        if (valid) kmin = min(kmin, key), kmax = max(kmax, key);
        const int equal = lds_count(lh[0], valid ? (int)(key >> 21) : -1, aggregate[0]);
        if (i == 0) aggregate[0] = equal >= HIST_AGGREGATE_FROM;
      } else {
#pragma unroll
        for (int j = 0; j < SEL_RANKS; ++j) {
          if (!active[j]) continue;              // the same for the whole launch
          const bool match = valid && (PASS == 1 ? key >> 21 : key >> 10) == prefix[j];
          const int digit = PASS == 1 ? (int)((key >> 10) & 0x7FFu) : (int)(key & 0x3FFu);
          const int equal = lds_count(lh[j], match ? digit : -1, aggregate[j]);
          if (i == 0) aggregate[j] = equal >= HIST_AGGREGATE_FROM;
        }
      }
    }
    if (++since_flush == HIST_FLUSH_TILES || t + gridDim.x >= tiles) {
      since_flush = 0;
      __syncthreads();
      for (int i = threadIdx.x; i < SEL_RANKS * SEL_DIGITS; i += HIST_THREADS) {
        const unsigned c = (&lh[0][0])[i];
        if (c) {
          atomicAdd(&st->hist[0][0] + i, (unsigned long long)c);
          (&lh[0][0])[i] = 0u;
        }
      }
      __syncthreads();
    }
  }
  if (PASS == 0) {
    // (a thread's own count cannot wrap: the entry's limits leave it fewer than 2^32 elements)
    n_nan = wave_sum_u32(n_nan);
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
      kmin = min(kmin, (unsigned)__shfl_xor(kmin, off, WAVE));
      kmax = max(kmax, (unsigned)__shfl_xor(kmax, off, WAVE));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
      if (n_nan) atomicAdd(&st->n_nan, (unsigned long long)n_nan);
      if (kmin <= kmax) {
        atomicMin(&st->key_min, kmin);
        atomicMax(&st->key_max, kmax);
      }
    }
  }
}

// one workgroup of SEL_RANKS waves: wave k picks the digit of rank k from its histogram; then the
// histograms are zeroed and the ranks that now share a prefix share a histogram.  After the last
// pass the results are written.
template <int PASS, bool SHIFT>
__global__ __launch_bounds__(SEL_RANKS* WAVE) void select_pick_kernel(
    SelectState* __restrict__ st, int64_t n, float* __restrict__ values,
    float* __restrict__ extremes, int64_t* __restrict__ counts) {
  constexpr int BITS = PASS == 2 ? 10 : 11, DIGITS = 1 << BITS, PER = DIGITS / WAVE;
  __shared__ unsigned new_prefix[SEL_RANKS];
  __shared__ unsigned long long new_remaining[SEL_RANKS];
  __shared__ int alive[SEL_RANKS];
  __shared__ unsigned long long valid_total;
  const int k = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  const int n_ranks = st->n_ranks;
  const int slot = st->slot[k];
  if (lane == 0) alive[k] = 0, new_prefix[k] = 0u, new_remaining[k] = 0ull;
  if (k < n_ranks && slot >= 0) {
    const unsigned long long* h = st->hist[slot] + lane * PER;
    unsigned long long sum = 0ull;
    for (int d = 0; d < PER; ++d) sum += h[d];
    unsigned long long incl = sum;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const unsigned long long up = __shfl_up(incl, off, WAVE);
      if (lane >= off) incl += up;
    }
    const unsigned long long total = __shfl(incl, WAVE - 1, WAVE);
    if (PASS == 0 && k == 0 && lane == 0) valid_total = total;
    const unsigned long long r = st->remaining[k];
    unsigned long long cum = incl - sum;
    if (r >= cum && r < incl) {                 // one lane at the most; none: r >= total
      for (int d = 0; d < PER; ++d) {
        const unsigned long long c = h[d];
        if (r < cum + c) {
          const unsigned digit = (unsigned)(lane * PER + d);
          new_prefix[k] = PASS == 0 ? digit : (st->prefix[k] << BITS) | digit;
          new_remaining[k] = r - cum;
          alive[k] = 1;
          break;
        }
        cum += c;
      }
    }
  }
  __syncthreads();
  unsigned long long* hist = &st->hist[0][0];
  for (int i = threadIdx.x; i < SEL_RANKS * SEL_DIGITS; i += SEL_RANKS * WAVE) hist[i] = 0ull;
  if (threadIdx.x == 0) {
    if (PASS == 0) st->n_valid = valid_total;
    for (int j = 0; j < SEL_RANKS; ++j) {
      int s = -1;
      if (alive[j]) {
        s = j;
        for (int i = j - 1; i >= 0; --i)
          if (alive[i] && new_prefix[i] == new_prefix[j]) s = i;
      }
      st->slot[j] = s;
      st->prefix[j] = new_prefix[j];
      st->remaining[j] = new_remaining[j];
    }
    if (PASS == 2) {
      const float nan = __builtin_nanf("");
      for (int j = 0; j < n_ranks; ++j) {
        const float r = value_of(new_prefix[j]);
        values[j] = alive[j] ? (SHIFT ? r + 1.0f : r) : nan;
      }
      const bool any = st->n_valid > 0ull;
      const float lo = value_of(st->key_min), hi = value_of(st->key_max);
      extremes[0] = any ? (SHIFT ? lo + 1.0f : lo) : nan;
      extremes[1] = any ? (SHIFT ? hi + 1.0f : hi) : nan;
      counts[0] = n;
      counts[1] = (int64_t)st->n_nan;
    }
  }
}

// ---- row sums ----

template <bool SHIFT>
__global__ __launch_bounds__(ROWSUM_THREADS) void row_sums_kernel(const float* __restrict__ x,
                                                                  int64_t ld, int64_t rows,
                                                                  int64_t F,
                                                                  float* __restrict__ out) {
  __shared__ double red[ROWSUM_THREADS / WAVE];
  const int64_t chunks = tiles_of_row<ROWSUM_THREADS>(F);
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* p = x + row * ld;
    double acc = 0.0;
    for (int64_t c = 0; c < chunks; ++c) {
      float v[HIST_CHUNK];
      const unsigned mask = load_tile<ROWSUM_THREADS>(p, F, c, v);
#pragma unroll
      for (int i = 0; i < HIST_CHUNK; ++i)
        if ((mask >> i) & 1u) acc += (double)(SHIFT ? v[i] + 1.0f : v[i]);
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, WAVE);
    if (lane == 0) red[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = red[0];
      for (int i = 1; i < ROWSUM_THREADS / WAVE; ++i) s += red[i];
      out[row] = (float)s;
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace scvae

// the limits every entry of this file shares
#define SCVAE_DISTRIBUTION_MATRIX()                                                  \
  SCVAE_ARG(x && ((uintptr_t)x & 3) == 0);                                           \
  SCVAE_ARG(rows >= 1 && F >= 1 && ldx >= F);                                        \
  SCVAE_ARG(F <= (rows == 1 ? (int64_t)1 << 40 : (int64_t)INT32_MAX));               \
  SCVAE_ARG(rows <= ((int64_t)1 << 60) / ldx)

extern "C" {

int scvae_histogram_accumulate(const float* x, int64_t ldx, int64_t rows, int64_t F, int32_t shift,
                               const void* edges, int32_t flags, int64_t n_bins, int64_t* counts,
                               int64_t* outside, void* stream) {
  using namespace scvae;
  SCVAE_DISTRIBUTION_MATRIX();
  SCVAE_ARG(n_bins >= 1 && n_bins <= ((int64_t)1 << 20));
  SCVAE_ARG((flags & ~3) == 0);
  const bool f64 = flags & 1, aggregate = !(flags & 2);
  SCVAE_ARG(edges && ((uintptr_t)edges & (f64 ? 7 : 3)) == 0);
  SCVAE_ARG(counts && outside);
  SCVAE_ARG(((uintptr_t)counts & 7) == 0 && ((uintptr_t)outside & 7) == 0);
  const int64_t chunks = tiles_of_row<HIST_THREADS>(F);
  const int64_t tiles = rows * chunks;
  const int slabs = (int)((n_bins + HIST_SLAB - 1) / HIST_SLAB);
  int64_t shares = slabs >= HIST_GROUPS_TARGET ? 1 : HIST_GROUPS_TARGET / slabs;
  if (shares > tiles) shares = tiles;
  const int width = (int)(n_bins < HIST_SLAB ? n_bins : HIST_SLAB);
  const int lds = (width + 1) * (int)(f64 ? sizeof(double) : sizeof(float)) +
                  width * (int)sizeof(unsigned);
  const dim3 grid((unsigned)shares, (unsigned)slabs);
#define SCVAE_HISTOGRAM_LAUNCH(E, S, A)                                                           \
  do {                                                                                            \
    SCVAE_HIP(max_dynamic_lds((const void*)histogram_kernel<E, S, A>, lds));                      \
    hipLaunchKernelGGL((histogram_kernel<E, S, A>), grid, dim3(HIST_THREADS), lds,                \
                       (hipStream_t)stream, x, ldx, rows, F, chunks, static_cast<const E*>(edges), \
                       (int)n_bins, reinterpret_cast<unsigned long long*>(counts),                \
                       reinterpret_cast<unsigned long long*>(outside));                           \
  } while (0)
#define SCVAE_HISTOGRAM_LAUNCH_E(E)                          \
  do {                                                       \
    if (shift && aggregate) SCVAE_HISTOGRAM_LAUNCH(E, true, true); \
    else if (shift) SCVAE_HISTOGRAM_LAUNCH(E, true, false);  \
    else if (aggregate) SCVAE_HISTOGRAM_LAUNCH(E, false, true); \
    else SCVAE_HISTOGRAM_LAUNCH(E, false, false);            \
  } while (0)
  if (f64) SCVAE_HISTOGRAM_LAUNCH_E(double);
  else SCVAE_HISTOGRAM_LAUNCH_E(float);
#undef SCVAE_HISTOGRAM_LAUNCH_E
#undef SCVAE_HISTOGRAM_LAUNCH
  SCVAE_LAUNCH_CHECK("histogram_kernel");
  return 0;
}

int64_t scvae_order_statistics_workspace_bytes(void) { return (int64_t)sizeof(scvae::SelectState); }

int scvae_order_statistics(const float* x, int64_t ldx, int64_t rows, int64_t F, int32_t shift,
                           const int64_t* ranks, int32_t n_ranks, float* values, float* extremes,
                           int64_t* counts, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  using namespace scvae;
  SCVAE_DISTRIBUTION_MATRIX();
  SCVAE_ARG(ranks && n_ranks >= 1 && n_ranks <= SEL_RANKS);
  const int64_t n = rows * F;
  SCVAE_ARG(n <= ((int64_t)1 << 42));         // a wave's NaN count stays inside 32 bits
  SelectRanks r{};
  for (int k = 0; k < n_ranks; ++k) {
    SCVAE_ARG(ranks[k] >= 0 && ranks[k] < n);
    r.r[k] = ranks[k];
  }
  SCVAE_ARG(values && extremes && counts);
  SCVAE_ARG(((uintptr_t)values & 3) == 0 && ((uintptr_t)extremes & 3) == 0 &&
            ((uintptr_t)counts & 7) == 0);
  SCVAE_ARG(workspace && ((uintptr_t)workspace & 7) == 0);
  SCVAE_ARG(workspace_bytes >= (int64_t)sizeof(SelectState));
  hipStream_t st = (hipStream_t)stream;
  SelectState* state = static_cast<SelectState*>(workspace);
  const int64_t chunks = tiles_of_row<HIST_THREADS>(F);
  const int64_t tiles = rows * chunks;
  const unsigned blocks = (unsigned)(tiles < HIST_GROUPS_TARGET ? tiles : HIST_GROUPS_TARGET);
  hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(HIST_THREADS), 0, st, state, r,
                     (int)n_ranks);
  SCVAE_LAUNCH_CHECK("select_init_kernel");
#define SCVAE_SELECT_PASS(P)                                                                     \
  do {                                                                                           \
    hipLaunchKernelGGL((select_pass_kernel<P>), dim3(blocks), dim3(HIST_THREADS), 0, st, x, ldx, \
                       rows, F, chunks, state);                                                  \
    SCVAE_LAUNCH_CHECK("select_pass_kernel");                                                    \
    if (shift)                                                                                   \
      hipLaunchKernelGGL((select_pick_kernel<P, true>), dim3(1), dim3(SEL_RANKS* WAVE), 0, st,   \
                         state, n, values, extremes, counts);                                    \
    else                                                                                         \
      hipLaunchKernelGGL((select_pick_kernel<P, false>), dim3(1), dim3(SEL_RANKS* WAVE), 0, st,  \
                         state, n, values, extremes, counts);                                    \
    SCVAE_LAUNCH_CHECK("select_pick_kernel");                                                    \
  } while (0)
  SCVAE_SELECT_PASS(0);
  SCVAE_SELECT_PASS(1);
  SCVAE_SELECT_PASS(2);
#undef SCVAE_SELECT_PASS
  return 0;
}

int scvae_row_sums_f64(const float* x, int64_t ldx, int64_t rows, int64_t F, int32_t shift,
                       float* out, void* stream) {
  using namespace scvae;
  SCVAE_DISTRIBUTION_MATRIX();
  SCVAE_ARG(out && ((uintptr_t)out & 3) == 0);
  const unsigned blocks = (unsigned)(rows < 65536 ? rows : 65536);
  if (shift)
    hipLaunchKernelGGL(row_sums_kernel<true>, dim3(blocks), dim3(ROWSUM_THREADS), 0,
                       (hipStream_t)stream, x, ldx, rows, F, out);
  else
    hipLaunchKernelGGL(row_sums_kernel<false>, dim3(blocks), dim3(ROWSUM_THREADS), 0,
                       (hipStream_t)stream, x, ldx, rows, F, out);
  SCVAE_LAUNCH_CHECK("row_sums_kernel");
  return 0;
}

}  // extern "C"
