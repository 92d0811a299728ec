// Fused decoder output layer on the bf16 matrix cores in the exact-product nine-term form
// ("bf16x9"): the same maths, inputs, outputs and per-strip partial buffers as decoder_fused.hip /
// decoder_fused2.hip (X_TILDE heads va:2466-2489, activation + clip + TFP log_prob du:206-305,
// sum over the genes va:2583-2590, and their backward), with the three products
//
//     GEMM1  pre_j[row, gene] = sum_h d[row, h] W_j[h, gene] + b_j[gene]
//     GEMM2  dW_j[h, gene]   += sum_row d[row, h] G_j[row, gene]         (row h == H: db_j)
//     GEMM3  dd[row, h]       = sum_j sum_gene G_j[row, gene] W_j[h, gene]
//
// evaluated as follows.  An fp32 value is cut EXACTLY into three bf16 terms x = x1 + x2 + x3
// (8 + 8 + 8 significant bits, by truncation: x1 = the upper 16 bits of x, x2 = those of x - x1,
// x3 = the rest); a product x y is the sum of the nine products x_a y_b, each of which is exact
// in fp32 (8 x 8 bits), and the matrix core accumulates them in fp32: the result is an fp32 sum
// of exact products -- the error class of an fp32 FMA chain, not of a bf16 GEMM.  Nine
// v_mfma_f32_*_bf16 per 16 k cost 9 x 32 cycles against 8 x 64 for v_mfma_f32_32x32x2_f32:
// 0.56 of the matrix time of the fp32 kernels.  Reported by bench.py as
// "decoder_head_arith": "bf16x9-exact" with the roofline priced at 2500 / 9 TFLOP/s.
//
// Organisation (one workgroup = 8 waves = one 64-gene strip, walking over 64-row tiles):
//   * d reaches the kernel already cut into bf16 planes, in both operand orientations
//     (split3_hidden_kernel: dA [3][rows][128] for GEMM1, dT [3][128][rows] for GEMM2; column /
//     row H holds ones, so b_j and db_j fall out of the same MFMAs); every operand fragment of d
//     is ONE 16-byte load from L2 straight into the registers that feed the MFMAs -- d never
//     passes through LDS;
//   * the strip's weights are cut once per workgroup and stay in LDS as [head][plane][h][gene]
//     bf16 (144-byte rows: conflict-free ds_read_b128 fragments for GEMM3); GEMM1 reads the same
//     image through ds_read_b64_tr_b16, the hardware transpose read, which hands a lane four
//     consecutive h of its gene;
//   * phase A (all waves): wave (gene block of 16, row half of 32) computes the TRANSPOSED head
//     tile pre_j^T[gene, row] with v_mfma_f32_16x16x32_bf16: a lane then holds four consecutive
//     genes of one row for every head, the likelihood and its gradient run on the accumulator
//     registers (no LDS round trip of the pre-activations), the t > 0 corrections of the
//     negative-binomial kinds as a per-lane walk over the lane's non-zeros; G_j is cut into
//     planes and stored to LDS once, row-major;
//   * phase B (all waves): GEMM3 from LDS (ds_read_b128 of G and W) while the dT fragments of
//     GEMM2 are in flight, then GEMM2 (G through the transpose read); dW accumulators persist
//     in registers over the whole launch;
//   * two workgroup barriers per 64 rows.
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"
#include "likelihood.hpp"

namespace scvae {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4m __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// A/B switch (tools/ab_variants.sh): 1 = the global fragment loads of d stay where the source
// issues them -- one k-step ahead -- (a scheduling barrier that only vector-memory reads may not
// cross); 0 = the compiler sinks them to just before their use to save registers, and the wave
// then waits for an L2 round trip in every k-step
#ifndef D3_PIN_LOADS
#define D3_PIN_LOADS 1
#endif
// how many k-steps ahead the fragments of d are requested (1, or 2: 24 more VGPRs and no faster)
#ifndef D3_AHEAD
#define D3_AHEAD 1
#endif
constexpr int D3_NB = D3_AHEAD + 1;      // fragment buffers
__device__ __forceinline__ void d3_pin_loads() {
  if (D3_PIN_LOADS) __builtin_amdgcn_sched_barrier(0x7C6);   // VMEM reads stay above, MFMAs below; the rest may cross
}

constexpr int D3_THREADS = 512;
constexpr int D3_BM = 64;           // rows per tile
constexpr int D3_KP = 128;          // padded hidden width of the planes of d
// genes per strip (= per workgroup): 64 for one / two heads; 32 for three heads, whose weight
// planes (9 x 112 rows) would not fit LDS next to the G tile at 64
__host__ __device__ constexpr int d3_bn(int P) { return P >= 3 ? 32 : 64; }
// bytes per LDS row: the strip's genes as bf16 + 16 bytes of padding (144 / 80: odd multiples of
// 16 bytes, conflict-free ds_read_b128 fragments)
__host__ __device__ constexpr int d3_rowb(int P) { return 2 * d3_bn(P) + 16; }

__host__ __device__ inline int d3_hp1(int H) { return (H + 1 + 15) / 16 * 16; }

int decoder_fused3_strip_genes(int P) { return d3_bn(P); }
size_t decoder_fused3_lds_bytes(int P, int H) {
  return (size_t)P * 3 * d3_hp1(H) * d3_rowb(P) + (size_t)P * 3 * D3_BM * d3_rowb(P) +
         2 * D3_BM * sizeof(float);
}
bool decoder_fused3_supported(int P, int H) {
  return P <= 3 && H >= 2 && H <= 126 && decoder_fused3_lds_bytes(P, H) <= 160 * 1024;
}
// padded hidden width of the planes of d: [d | 1 | 0 ...] in whole 32-wide contraction steps;
// 128 for every H the all-in-one-phase kernel takes, up to 288 for the producer / consumer kernel
__host__ __device__ inline int d3_kp(int H) { return H + 1 <= D3_KP ? D3_KP : (H + 1 + 31) / 32 * 32; }
// one plane set of d: dA [3][Rpad][KP] then dT [3][KP][Rpad], bf16
__host__ __device__ inline size_t d3_set_elems(int Rpad, int KP = D3_KP) {
  return (size_t)2 * 3 * Rpad * KP;
}
// three plane sets (head dropout: one dropped-out copy of d per head) + the heads' mask words
// [3][Rpad][4]; beyond H = 126 (no dropout instantiation there) one set
size_t decoder_fused3_workspace_floats(int rows, int H) {
  const size_t rpad = (size_t)(rows + D3_BM - 1) / D3_BM * D3_BM;
  const int kp = d3_kp(H);
  if (kp > D3_KP) return d3_set_elems((int)rpad, kp) * sizeof(uint16_t) / sizeof(float) + 64;
  return 3 * d3_set_elems((int)rpad) * sizeof(uint16_t) / sizeof(float) + 3 * rpad * 4 + 64;
}

// x = b1 + b2 + b3 exactly, each term's upper 16 bits a bf16 value (lower 16 bits zero).
// The terms are cut by ROUNDING to nearest (v_cvt_pk_bf16_f32), not by truncation: x - bf16(x)
// has at most 16 significant bits and is exact in fp32, the next residual at most 8 -- the
// three terms still add up to x exactly (the nine-term products stay exact), but they are
// smaller, |b2| <= 2^-9 |x| and |b3| <= 2^-18 |x|, and of either sign: the three products the
// six-term arithmetic leaves out (b2 c3, b3 c2, b3 c3) are then <= 2^-26 |x c| together and
// unbiased -- below the rounding of an fp32 multiply-add -- where truncated terms (all of the
// sign of x, up to 2^-8 and 2^-16) left a one-sided 2^-22 (measured against fp64 at 4096 rows:
// 8e-6 of the largest element of dd, ten times the fp32 matrix cores' error).
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {   // RN, lo in bits 0-15
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2v{lo, hi}, bf16x2));
}
__device__ __forceinline__ void split3_rn(float x, unsigned& b1, unsigned& b2, unsigned& b3) {
  b1 = cvt_pk_bf16(0.f, x) & 0xFFFF0000u;
  const float r1 = x - __uint_as_float(b1);
  b2 = cvt_pk_bf16(0.f, r1) & 0xFFFF0000u;
  b3 = __float_as_uint(r1 - __uint_as_float(b2));
}
// (upper half of hi) << 16 | upper half of lo
__device__ __forceinline__ unsigned pack_hi16(unsigned lo, unsigned hi) {
  return __builtin_amdgcn_perm(hi, lo, 0x07060302u);
}
// the same for two values at once, packed as the planes hold them (x0 in bits 0-15)
__device__ __forceinline__ void split3_rn_pair(float x0, float x1, unsigned& p1, unsigned& p2,
                                               unsigned& p3) {
  p1 = cvt_pk_bf16(x0, x1);
  float r0 = x0 - __uint_as_float(p1 << 16), r1 = x1 - __uint_as_float(p1 & 0xFFFF0000u);
  p2 = cvt_pk_bf16(r0, r1);
  r0 -= __uint_as_float(p2 << 16);
  r1 -= __uint_as_float(p2 & 0xFFFF0000u);
  p3 = pack_hi16(__float_as_uint(r0), __float_as_uint(r1));      // (8 bits each: exact)
}

// d [R, H] fp32 -> the bf16 planes of [d | 1 | 0...] (column H = 1: bias / db; zero beyond and
// for rows >= R), laid out FRAGMENT-MAJOR, so that the operand fragment of a wave is one
// contiguous KiB (64 lanes x 16 bytes, eight full cache lines):
//   dA[pl][rb][ks][lane][8]   GEMM1's B operand (16x16x32): row 16 rb + (lane & 15),
//                             k = 32 ks + 8 (lane >> 4) + e    (rb < Rpad / 16, ks < KP / 32)
//   dT[pl][ht][kg][lane][8]   GEMM2's A operand (32x32x16): h = 32 ht + (lane & 31),
//                             row 16 kg + 8 (lane >> 5) + e                  (kg < Rpad / 16)
// One thread = one lane slot of a fragment, all three planes.  blockIdx.y: 0 = dA, 1 = dT.
// (zero, zero16: the XCD-local accumulators of dd the training kernel is about to add into, as
//  16-byte pieces -- cleared by this launch's threads instead of a memset launch of its own)
// pack_ks >= 0 (the launches that go to the producer / consumer kernel at a width whose last
// 32-wide block holds at most 8 live rows -- d4_packed): that block, k-step / h tile pack_ks with
// h0 = 32 pack_ks, in the PACKED arrangement, its slot 8 a + h' standing for term a of row h0 + h':
//   dA[pl][rb][pack_ks]   lane groups 0..2 (lane >> 4) all hold term pl of d[row, h0 + e], group 3
//                         zeros: against a W fragment whose group a holds term a of W, one MFMA
//                         sums over a as well
//   dT[0][pack_ks][kg]    lane li < 24 holds term li >> 3 of d[row .., h0 + (li & 7)], the lanes
//                         beyond zeros; the tile's places in planes 1 and 2 are zero and not read
__global__ __launch_bounds__(256) void split3_hidden_kernel(const float* __restrict__ d, int R,
                                                            int H, int Rpad, int KP,
                                                            uint16_t* __restrict__ dA,
                                                            uint16_t* __restrict__ dT,
                                                            u32x4* __restrict__ zero,
                                                            size_t zero16, int pack_ks) {
  const int slot = blockIdx.x * 256 + threadIdx.x;       // < Rpad * KP / 8
  for (size_t i = (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; i < zero16;
       i += (size_t)gridDim.x * gridDim.y * 256)
    zero[i] = u32x4{0u, 0u, 0u, 0u};
  if (slot >= Rpad * (KP / 8)) return;
  const int ksp = KP / 32;                               // contraction steps per 16-row block
  const int lane = slot & 63, frag = slot >> 6;
  const int nb = Rpad / 16;
  unsigned t1[8], t2[8], t3[8];
  auto value = [&](int r, int k) {
    if (r >= R) return 0.f;
    return k < H ? d[(size_t)r * H + k] : (k == H ? 1.f : 0.f);
  };
  if (blockIdx.y == 0) {
    const int rb = frag / ksp, ks = frag % ksp;
    const int row = 16 * rb + (lane & 15), k0 = 32 * ks + 8 * (lane >> 4);
    if (ks == pack_ks) {
      const bool live = (lane >> 4) < 3;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        split3_rn(live ? value(row, 32 * ks + e) : 0.f, t1[e], t2[e], t3[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) split3_rn(value(row, k0 + e), t1[e], t2[e], t3[e]);
    }
  } else {
    const int ht = frag / nb, kg = frag % nb;
    const int h = 32 * ht + (lane & 31), r0 = 16 * kg + 8 * (lane >> 5);
    if (ht == pack_ks) {
      const int a = (lane & 31) >> 3;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        unsigned s1, s2, s3;
        split3_rn(a < 3 ? value(r0 + e, 32 * ht + (lane & 7)) : 0.f, s1, s2, s3);
        t1[e] = a == 0 ? s1 : (a == 1 ? s2 : s3);
        t2[e] = 0u;
        t3[e] = 0u;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) split3_rn(value(r0 + e, h), t1[e], t2[e], t3[e]);
    }
  }
  auto pack = [](const unsigned* t) {
    u32x4 v;
    v.x = pack_hi16(t[0], t[1]); v.y = pack_hi16(t[2], t[3]);
    v.z = pack_hi16(t[4], t[5]); v.w = pack_hi16(t[6], t[7]);
    return v;
  };
  const size_t plane = (size_t)KP * Rpad;
  uint16_t* dst = (blockIdx.y == 0 ? dA : dT) + (size_t)slot * 8;
  *reinterpret_cast<u32x4*>(dst) = pack(t1);
  *reinterpret_cast<u32x4*>(dst + plane) = pack(t2);
  *reinterpret_cast<u32x4*>(dst + 2 * plane) = pack(t3);
}

// ---- LDS / global operand fragments ----
__device__ __forceinline__ bf16x8 lds_b128(const char* p) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(p));
}
// transpose read: the 16 lanes of a group pass the addresses of a [4 rows][16 columns] block
// (lane i: row i >> 2, columns 4 (i & 3) ..) and lane i receives column i of the four rows
__device__ __forceinline__ s16x4 lds_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(p));
}
template <int ROWB>
__device__ __forceinline__ bf16x8 lds_tr8(const char* p) {    // rows 0-3 and rows 4-7
  const s16x4 lo = lds_tr(p), hi = lds_tr(p + 4 * ROWB);
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ bf16x8 global_b128(const uint16_t* p) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(p));
}

// one of N registers by a per-lane index (lane masks of the index bits; inline asm: written as
// C++ selects the compiler turns the tree into a dynamically indexed array = scratch)
struct IndexMasks3 { unsigned long long m[3]; };
__device__ __forceinline__ IndexMasks3 index_masks3(int idx) {
  IndexMasks3 k;
#pragma unroll
  for (int b = 0; b < 3; ++b) k.m[b] = __builtin_amdgcn_ballot_w64((idx >> b) & 1);
  return k;
}
__device__ __forceinline__ float cnd3(float lo, float hi, unsigned long long mask) {
  float r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(lo), "v"(hi), "s"(mask));
  return r;
}
__device__ __forceinline__ float select_n(const float (&v)[8], const IndexMasks3& k) {
  float a[4], b[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = cnd3(v[2 * i], v[2 * i + 1], k.m[0]);
#pragma unroll
  for (int i = 0; i < 2; ++i) b[i] = cnd3(a[2 * i], a[2 * i + 1], k.m[1]);
  return cnd3(b[0], b[1], k.m[2]);
}
__device__ __forceinline__ float select_n(const float (&v)[4], const IndexMasks3& k) {
  return cnd3(cnd3(v[0], v[1], k.m[0]), cnd3(v[2], v[3], k.m[0]), k.m[1]);
}

// U16 (compile time): the targets are the uint16 minibatch.  As a run-time flag the two load
// paths met in a branch, the compiler waited for the load INSIDE each arm, and the request for the
// next tile's targets -- meant to travel under a whole phase B -- cost a full memory round trip
// (vmcnt(0): everything in flight) per tile.
//
// TRAIN = false: the forward half alone (evaluation passes, the importance-weight pass): GEMM1 +
// likelihood + row sums; no G, no phase B, one barrier per tile (the row-sum buffer alternates
// between two places), the next tile's operands requested under the last k-step of this one.
//
// DROP = true (training only): dropout of the heads' input connections (mu:45-50 inside every
// X_TILDE dense_layer, va:2475-2488): head j reads its OWN dropped-out copy of d -- plane set j,
// d3_set_elems(Rpad) apart -- in GEMM1 and GEMM2 (contraction steps (k-step, head) instead of
// k-steps, the fragments of d two such steps ahead), and its part of dd passes the head's mask
// (drop_bits[j][row][4]: bit h % 32 of word h / 32) times 1 / keep before the heads are summed.
//
// CP > 0 (KIND = LK_CPOISSON only): the constrained Poisson likelihood (du:218-228: lambda =
// clip(softmax over ALL genes), rate = lambda N) in three passes over the strip grid, because an
// element's likelihood needs the row's log-sum-exp and its gradient the row sum S = sum_f gate_f
// (t_f - N lambda_f) (cpoisson_rows_kernel has the formulas):
//   CP = 1 (forward): per strip and row the maximum of the logits -> ll_part, sum exp(a - max)
//          -> cp.out2;
//   CP = 2 (forward, given cp.lse): the strip's part of sum_f log p(t_f) -> ll_part, of S -> cp.out2;
//   CP = 3 (training, given cp.lse and cp.S): G = gw (gate (t - N lambda) - lambda S), phase B.
//
// IDX (decoder_head3_rows_kernel): the targets are rows of a RESIDENT uint16 matrix, cell b of the
// minibatch its row trows[b].  A lane fetches the index of its row of tile i + 2 right behind its
// request for the targets of tile i + 1 (which use the index fetched a tile earlier), so the
// dependent load is off the chain; rows beyond R read the index of row R - 1.
template <int KIND, int KS1, bool U16, bool TRAIN, bool DROP, int CP>
__global__ __launch_bounds__(D3_THREADS) void decoder_head3_kernel(
    const uint16_t* __restrict__ dA, const uint16_t* __restrict__ dT, int R, int Rpad, int H,
    HeadParams hp, int F, Targets tg, int B, const float* __restrict__ gw, int inline_lgamma,
    float* __restrict__ ll_part, float* __restrict__ dd_part,
    const uint32_t* __restrict__ drop_bits, float inv_keep, CpRows cp) {
  constexpr bool IDX = false;
  const int64_t* const trows = nullptr;
#include "decoder_head3_body.inc"
}
// the uint16 targets through a row index (no head dropout, the four count likelihoods)
template <int KIND, int KS1, bool TRAIN>
__global__ __launch_bounds__(D3_THREADS) void decoder_head3_rows_kernel(
    const uint16_t* __restrict__ dA, const uint16_t* __restrict__ dT, int R, int Rpad, int H,
    HeadParams hp, int F, Targets tg, int B, const float* __restrict__ gw, int inline_lgamma,
    float* __restrict__ ll_part, float* __restrict__ dd_part,
    const int64_t* __restrict__ trows) {
  constexpr bool U16 = true, DROP = false, IDX = true;
  constexpr int CP = 0;
  const uint32_t* const drop_bits = nullptr;
  const float inv_keep = 1.f;
  const CpRows cp = CpRows();
#include "decoder_head3_body.inc"
}


// =================================================================================================
// Round 4: the training step above (TRAIN, no dropout, no constrained-Poisson pass) with the two
// waves of every SIMD in DIFFERENT phases.  tools/probe/coexec_bf16.hip: a wave that keeps the
// bf16 matrix pipe of a SIMD saturated does not slow a VALU wave of the same SIMD (and vice
// versa: both == max), while ONE instruction stream hides only ~4 VALU instructions per
// 32x32x16 MFMA and pays the sum beyond -- and in decoder_head3_kernel both waves of a SIMD run
// the same stream between the same workgroup barriers (GEMM1, then the likelihood's VALU stretch,
// then GEMM3 / GEMM2): matrix busy 45 %, everything else serialised behind it.
//
// Here the workgroup's eight waves are four PRODUCERS (waves 0-3, one per SIMD) and four CONSUMERS
// (waves 4-7, the other wave of each SIMD) on 32-row tiles:
//   producer, tile t:      GEMM1 (wave = 32 genes x 16 rows, or 16 x 16 for three heads) ->
//                          likelihood + gradient on the accumulators -> non-zero walk -> row sums
//                          -> G_j cut into planes -> LDS buffer t & 1
//   consumer, tile t - 1:  GEMM3 dd^T (h tile of the wave x the tile's 32 rows) and GEMM2 dW
//                          (h tile x all the strip's genes x every head: the accumulators persist)
//                          from LDS buffer (t - 1) & 1
// one workgroup barrier per 32 rows (the old schedule: two per 64).  The consumer's matrix work
// (two of the three products) runs under the producer's VALU stretch; the producers carry a
// raised priority, since their GEMM1 + likelihood chain is the longer of the two.
// Same inputs, outputs, slab layouts and arithmetic as decoder_head3_kernel: the two are
// interchangeable launch by launch (SCVAE_D3_SCHEDULE=3 selects the old one; A/B + tests).
constexpr int D4_BM = 32;           // rows per tile

#ifndef D4_COMPACT
#define D4_COMPACT 1
#endif
// the non-zeros' corrections through a dense queue (below) up to four contraction steps
// (H <= 126); the wide geometries, whose weight planes leave no LDS for the queues, keep the
// per-lane walk
__host__ __device__ constexpr bool d4_compact(int ks1) { return D4_COMPACT && ks1 <= 4; }
// NPW producer waves (4 or 8) + four consumers per workgroup
__host__ __device__ constexpr int d4_threads(int npw) { return (npw + 4) * 64; }
size_t decoder_fused4_lds_bytes(int P, int H, int npw, int bn = 0) {
  const int rowb = 2 * (bn ? bn : d3_bn(P)) + 16;
  return (size_t)P * 3 * d3_hp1(H) * rowb + (size_t)2 * P * 3 * D4_BM * rowb +
         (size_t)2 * (npw / 2) * 4 * D4_BM * sizeof(float) +
         (d4_compact((H + 1 + 31) / 32) ? npw * 512 : 0);   // (the producers' queues)
}

#ifndef D4_PROF
#define D4_PROF 0
#endif
// s_setprio of the two kinds of waves (A/B: scvae_amd/csrc/build_prof.sh with EXTRA=-D...)
#ifndef D4_PRIO_PRODUCER
#define D4_PRIO_PRODUCER 1
#endif
#ifndef D4_PRIO_CONSUMER
#define D4_PRIO_CONSUMER 0
#endif
#if D4_PROF
// probe build: cycles (s_memtime) per section, summed over the tiles, of the waves of block 0
__device__ unsigned long long d4_prof[12 * 8];
#define D4_STAMP(k)                                            \
  do {                                                         \
    __builtin_amdgcn_sched_barrier(0);                         \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
    pacc[k] += t_ - plast;                                     \
    plast = t_;                                                \
    __builtin_amdgcn_sched_barrier(0);                         \
  } while (0)
#define D4_PROF_BEGIN unsigned long long pacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, plast = __builtin_amdgcn_s_memtime()
#define D4_PROF_END                                                                  \
  do {                                                                               \
    if (blockIdx.x == 0 && lane == 0)                                                \
      for (int k_ = 0; k_ < 8; ++k_) d4_prof[w * 8 + k_] = pacc[k_];                 \
  } while (0)
#else
#define D4_STAMP(k) do {} while (0)
#define D4_PROF_BEGIN do {} while (0)
#define D4_PROF_END do {} while (0)
#endif

// G1: where the producers' GEMM1 sits relative to the workgroup barrier -- 1: at the END of an
// iteration (for the tile after the one whose likelihood the iteration evaluates), 0: at its
// start, 2 (eight producers): the first producer wave of every SIMD at the start, the second at
// the end.  Measured (4096 x 32 738, kernel + reduces, dd atomics): with four producer waves the
// end is better than the start (ZINB 2.35 -> 2.23 ms, Poisson 0.82 -> 0.81); with eight the start
// beats the end (NB 1.42 against 1.50) and the staggered order beats both: with both GEMM1s at
// the start they and the consumer's GEMM2 all want the matrix pipe in the first half of a tile
// (the section probes: GEMM2 6.0 k cycles for 2.3 k of pipe work) and leave it to GEMM3 alone
// and then idle under the atomic adds in the second.
#ifndef D4_G1_EIGHT
#define D4_G1_EIGHT 0
#endif
// KS1 = ceil((H + 1) / 32) contraction steps of GEMM1 = 32-wide h tiles of GEMM2, up to 9
// (H <= 256): beyond four, a consumer wave owns (KS1 + 3) / 4 h tiles (ht, ht + 4, ht + 8) and the
// producers refill their four fragment slots of d inside the loop.  BN_: genes per strip (0: the
// default of the head count; 32 for two heads once the weight planes of 64 genes no longer fit).
// DBP (H a multiple of 32, from 128): the bias gradients db_j = column sums of G_j are summed by
// the PRODUCERS on their registers (one add per element and tile, a cross-lane reduce at the end)
// instead of falling out of GEMM2's ones row -- which at these widths would be an h tile of its
// own (the fifth at H = 128, the ninth at 256) holding nothing but that row.
// FWD: the forward half alone (is_training = False, the first pass of an importance-weighted
// step) for the decoder widths only this kernel takes -- odd ones and everything beyond 126: the
// producers' GEMM1 + likelihood + row sums; the gradient planes are not formed (nothing reads G:
// the compiler drops its arithmetic), the consumers only add up the row sums.
// IDX (decoder_head4_rows_kernel): the targets through the row index of a resident uint16 matrix,
// fetched a tile ahead of the target prefetch that uses it (as in decoder_head3_kernel).
// PACK (d4_packed: two to four contraction steps, the last with at most 8 live rows of [d | 1] --
// H + 1 in 33..40, 65..72, 97..104): the last 32-wide block of h carries the three bf16 terms of
// its live rows side by side, slot 8 a + h' = term a of row h0 + h' (h0 = 32 (KS1 - 1)), so that an
// MFMA over the block sums over the term index of one operand as well and the block costs three
// MFMAs per step, not nine, in all three products -- the same instructions, exact products and
// fp32 accumulation:
//   GEMM1  the W fragment's lane group a reads plane a of rows h0 .. h0 + 7 (group 3: the zero
//          rows h0 + 8 ..), the fragments of d hold term b in groups 0..2 (split3_hidden_kernel):
//          one MFMA per b;
//   GEMM2  the block's consumer wave loads ONE fragment of d^T (row 8 a + h' = term a) and
//          multiplies it with the three planes of G; the accumulator rows of the three terms of
//          an h sit in one lane (registers i, i + 4, i + 8) and are added once, before dW is stored;
//   GEMM3  that wave's W fragment: lane li reads plane li >> 3, row h0 + (li & 7) (the lanes from
//          24: zero rows), times the three planes of G; the same three registers are added before
//          the adds / stores of dd.
// With six-term arithmetic the packed block still carries all nine terms (three MFMAs, cheaper
// than six and no less accurate).
__host__ __device__ constexpr bool d4_packed(int ks1, int H) {
  return ks1 >= 2 && ks1 <= 4 && H + 1 - 32 * (ks1 - 1) >= 1 && H + 1 - 32 * (ks1 - 1) <= 8;
}
template <int KIND, int KS1, bool U16, int NPW, int BN_ = 0, bool DBP = false,
          int G1 = (NPW == 4 ? 1 : D4_G1_EIGHT), int TERMS = 9, bool FWD = false,
          bool PACK = false>
__global__ __launch_bounds__(d4_threads(NPW)) void decoder_head4_kernel(
    const uint16_t* __restrict__ dA, const uint16_t* __restrict__ dT, int R, int Rpad, int H,
    HeadParams hp, int F, Targets tg, int B, const float* __restrict__ gw, int inline_lgamma,
    float* __restrict__ ll_part, float* __restrict__ dd_part, int dd_atomic, int rg_tiles,
    float* __restrict__ rg_slab) {
  constexpr bool IDX = false;
  const int64_t* const trows = nullptr;
#include "decoder_head4_body.inc"
}
// the uint16 targets through a row index (all nine terms)
template <int KIND, int KS1, int NPW, int BN_, bool DBP, int G1, bool FWD, bool PACK>
__global__ __launch_bounds__(d4_threads(NPW)) void decoder_head4_rows_kernel(
    const uint16_t* __restrict__ dA, const uint16_t* __restrict__ dT, int R, int Rpad, int H,
    HeadParams hp, int F, Targets tg, int B, const float* __restrict__ gw, int inline_lgamma,
    float* __restrict__ ll_part, float* __restrict__ dd_part, int dd_atomic, int rg_tiles,
    float* __restrict__ rg_slab, const int64_t* __restrict__ trows) {
  constexpr bool U16 = true, IDX = true;
  constexpr int TERMS = 9;
#include "decoder_head4_body.inc"
}

#if D4_PROF
extern "C" int scvae_d4_prof_dump(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(d4_prof), sizeof(unsigned long long) * 96);
}
#endif

// which schedule runs a plain training launch: 4 producer / consumer waves (decoder_head4_kernel,
// the default), 3 all waves in one phase (decoder_head3_kernel); read once
// (SCVAE_D3_SCHEDULE=3 / 4 forces one for A/B runs and tests.  Measured at 4096 x 32 738, kernel +
//  reduces: NB 1.49 against 1.58 ms, Poisson 0.90-0.92 against 0.90, ZINB 2.60-2.63 against 2.67)
static int d3_schedule_env() {
  static const int v = [] {
    const char* e = getenv("SCVAE_D3_SCHEDULE");
    return (e && (e[0] == '3' || e[0] == '4')) ? e[0] - '0' : 0;
  }();
  return v;
}
// producer waves per workgroup: eight (16 x 16 blocks, three waves per SIMD) for two heads, four
// for one head (measured, 4096 x 32 738: Poisson 0.81-0.83 ms with four, 0.87-0.88 with eight;
// NB 1.49-1.51 with eight, 1.58-1.61 with four); SCVAE_D4_PRODUCERS=4 / 8 overrides (A/B).
// 32-gene strips (four 16 x 16 blocks per tile) have four.
static int d4_producers_env() {
  static const int v = [] {
    const char* e = getenv("SCVAE_D4_PRODUCERS");
    return (e && (e[0] == '4' || e[0] == '8')) ? e[0] - '0' : 0;
  }();
  return v;
}
// The producer / consumer kernel's geometry for P heads and decoder width H: genes per strip,
// producer waves, contraction steps; ok = it fits (LDS: the strip's weight planes + two G tiles)
struct D4Config { int bn, npw, ks1; size_t lds; bool ok; bool dbp; };
static D4Config d4_config(int P, int H) {
  D4Config c;
  c.ks1 = (H + 1 + 31) / 32;
  c.bn = d3_bn(P);
  c.npw = P >= 3 ? 4 : (d4_producers_env() ? d4_producers_env() : (P == 1 ? 4 : 8));
  c.lds = decoder_fused4_lds_bytes(P, H, c.npw, c.bn);
  if (c.lds > 160 * 1024 && c.bn == 64 && P == 2) {
    // two heads beyond H = 110: the planes of 64 genes no longer fit -- 32-gene strips
    c.bn = 32; c.npw = 4;
    c.lds = decoder_fused4_lds_bytes(P, H, c.npw, c.bn);
  }
  if (c.ks1 > 4 && c.npw == 8) {   // (wide decoders: four producers -- the consumers own 2-3 h tiles)
    c.npw = 4;
    c.lds = decoder_fused4_lds_bytes(P, H, c.npw, c.bn);
  }
  // (H = 128, 160, .. 256: the bias gradient by the producers, GEMM2 without the ones row's tile)
  c.dbp = H >= 128 && H % 32 == 0;
  c.ok = P >= 1 && P <= 3 && H >= 2 && c.ks1 <= (c.dbp ? 9 : 8) && c.lds <= 160 * 1024;
  return c;
}
bool decoder_fused4_supported(int P, int H) { return d4_config(P, H).ok; }
// which schedule runs a plain training launch: 4 producer / consumer waves (decoder_head4_kernel,
// the default and the only one beyond H = 126), 3 all waves in one phase (decoder_head3_kernel)
// Up to 128 rows (the reference's default minibatch of 100) the all-in-one-phase kernel is the
// faster one (4 tiles: 69 against 80 us at 100 x 32 738; 512 rows: the other way round).
static int d3_schedule(int P, int H, int rows) {
  if (!decoder_fused3_supported(P, H)) return 4;
  if (!decoder_fused4_supported(P, H)) return 3;
  return d3_schedule_env() ? d3_schedule_env() : (rows <= 128 ? 3 : 4);
}
int d4_strip_genes(int P, int H) { return d4_config(P, H).bn; }   // the producer / consumer kernel's
// genes per workgroup (= per slab of ll_part / dd_part) of a TRAINING launch
int decoder_fused3_train_strip_genes(int P, int H, int rows, bool drop, int cp_pass) {
  if (!drop && cp_pass == 0 && d3_schedule(P, H, rows) == 4) return d4_config(P, H).bn;
  return d3_bn(P);
}

// whether a training launch with these options accumulates dd with XCD-local atomics (the caller
// then reduces eight [H][rows] copies instead of the per-strip slabs): only the producer /
// consumer kernel has that store
bool decoder_fused3_dd_atomics(int kind, int H, int rows, bool drop, int cp_pass, int dd_mode) {
  const int P = likelihood_heads(kind);
  return (dd_mode & 1) && !(dd_mode & 4) && !drop && cp_pass == 0 && d3_schedule(P, H, rows) == 4;
}

// the training instantiation a plain launch (no dropout, no constrained-Poisson pass) takes, as
// rocprofv3 prints it (bench.py matches its HIP-event timing against the kernel trace by name)
int decoder_fused3_train_kernel_name(int kind, int H, int rows, bool u16, char* out, size_t n,
                                     int terms) {
  const int P = likelihood_heads(kind);
  if (d3_schedule(P, H, rows) == 4) {
    const D4Config c = d4_config(P, H);
    const bool six = terms == 6 && c.ks1 <= 4 && c.bn == d3_bn(P) && !c.dbp;
    const bool pack = c.bn == d3_bn(P) && !c.dbp && d4_packed(c.ks1, H);
    return snprintf(out, n, "decoder_head4_kernel<%d, %d, %s, %d, %d, %s, %d, %d, false, %s>", kind,
                    c.ks1, u16 ? "true" : "false", c.npw, c.bn == d3_bn(P) ? 0 : c.bn,
                    c.dbp ? "true" : "false", c.npw == 4 ? 1 : D4_G1_EIGHT, six ? 6 : 9,
                    pack ? "true" : "false");
  }
  return snprintf(out, n, "decoder_head3_kernel<%d, %d, %s, true, false, 0>", kind,
                  (d3_hp1(H) + 31) / 32, u16 ? "true" : "false");
}

// ---- row groups of the producer / consumer kernel ----
// One workgroup per CU (its LDS), so a launch of `strips` workgroups runs in ceil(strips / CUs)
// rounds and the last round may be nearly empty (27 998 genes on 32-gene strips: 875 workgroups
// on 256 CUs, the fourth round on 107 of them -- a seventh of the launch).  Cutting the rows of
// every strip into n groups multiplies the workgroups; n is chosen for the fullest rounds, a
// group keeps at least 256 rows, and every group beyond the first costs a pass over
// [P][H + 1][F] floats (its dW / db slab), so one more group has to buy at least four percent.
constexpr int D4_MAX_ROW_GROUPS = 4;
size_t decoder_fused3_rg_slab_floats(int H, int F) {
  return (size_t)(D4_MAX_ROW_GROUPS - 1) * 3 * (size_t)(H + 1) * F + 64;
}
static int d4_cu_count() {
  static thread_local int cached_device = -1, cached = 0;
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return 256;
  if (device != cached_device) {
    hipDeviceProp_t prop;
    cached = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 256;
    cached_device = device;
  }
  return cached > 0 ? cached : 256;
}
static int d4_row_groups(int strips, int rows) {
  static const int forced = [] {
    const char* e = getenv("SCVAE_D4_ROW_GROUPS");
    return e ? atoi(e) : 0;
  }();
  const int tiles = (rows + D4_BM - 1) / D4_BM;
  int most = tiles / 8;                            // >= 256 rows per group
  if (most > D4_MAX_ROW_GROUPS) most = D4_MAX_ROW_GROUPS;
  if (most < 1) most = 1;
  if (forced >= 1) return forced < most ? forced : most;
  const int cus = d4_cu_count();
  int best = 1;
  double best_score = 0.0;
  for (int n = 1; n <= most; ++n) {
    const long wgs = (long)strips * n;
    const long rounds = (wgs + cus - 1) / cus;
    const double score = (double)wgs / (double)(rounds * cus) - 0.04 * (n - 1);
    if (score > best_score + 1e-9) { best = n; best_score = score; }
  }
  return best;
}
// gradient rows (dW_j[h, :], h < H; db_j, h == H) += the row groups' slabs, in group order
__global__ __launch_bounds__(256) void d4_rg_combine_kernel(HeadParams hp, int P, int H, int F,
                                                            const float* __restrict__ slab,
                                                            int groups) {
  const int jh = blockIdx.y;                       // (head, row)
  const int j = jh / (H + 1), h = jh % (H + 1);
  float* dst = h < H ? hp.dW[j] + (size_t)h * F : hp.db[j];
  const size_t gstride = (size_t)P * (H + 1) * F;
  const float* src = slab + ((size_t)j * (H + 1) + h) * F;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < F; c += gridDim.x * blockDim.x) {
    float v = dst[c];
    for (int g = 0; g < groups; ++g) v += src[(size_t)g * gstride + c];
    dst[c] = v;
  }
}

// ---- launch of the producer / consumer kernel: the instantiation for (kind, steps, strip, waves) ----
struct D4Launch {
  hipStream_t s; const uint16_t* dA; const uint16_t* dT; int rows, Rpad, H; HeadParams hp; int F;
  Targets t; int B; const float* gw; int inline_lgamma; float* ll_part; float* dd_part;
  int dd_atomic; int strips; size_t lds; int terms; int row_groups; float* rg_slab;
  bool fwd = false;      // the forward half alone (decoder_head4_kernel<..., FWD = true>)
  const int64_t* trows = nullptr;   // the uint16 targets through a row index (..._rows_kernel)
};
template <int KIND, int KS1, int NPW, int BN_, bool DBP = false, int TERMS = 9, bool PACK = false>
static int d4_launch_one(const D4Launch& a) {
  constexpr int G1 = NPW == 4 ? 1 : D4_G1_EIGHT;
  // (the packed remainder block: an instantiation of its own, chosen here from H -- d4_packed;
  //  decoder_fused3_launch asks split3_hidden_kernel for the packed planes by the same rule)
  if constexpr (!PACK && KS1 >= 2 && KS1 <= 4 && BN_ == 0 && !DBP) {
    if (d4_packed(KS1, a.H)) return d4_launch_one<KIND, KS1, NPW, BN_, DBP, TERMS, true>(a);
  }
  // (six-term products: instantiated for the default strips up to four contraction steps, i.e.
  //  H <= 126; the wider geometries keep all nine terms)
  if constexpr (TERMS == 9 && KS1 <= 4 && BN_ == 0 && !DBP) {
    if (a.terms == 6) return d4_launch_one<KIND, KS1, NPW, BN_, DBP, 6, PACK>(a);
  }
  const int tiles = (a.rows + D4_BM - 1) / D4_BM;
  const int rg_tiles = (tiles + a.row_groups - 1) / a.row_groups;
  const int groups = (tiles + rg_tiles - 1) / rg_tiles;     // (no empty group)
  if (a.trows) {
    if constexpr (TERMS == 9) {
      if (!a.t.u16 || a.terms != 9) {
        set_error("decoder_head4_kernel: a row index goes with uint16 targets and nine terms");
        return -1;
      }
      auto rfn = a.fwd ? decoder_head4_rows_kernel<KIND, KS1, NPW, BN_, DBP, G1, true, PACK>
                       : decoder_head4_rows_kernel<KIND, KS1, NPW, BN_, DBP, G1, false, PACK>;
      SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(rfn), (int)a.lds));
      hipLaunchKernelGGL(rfn, dim3(a.strips, groups), dim3(d4_threads(NPW)), a.lds, a.s, a.dA,
                         a.dT, a.rows, a.Rpad, a.H, a.hp, a.F, a.t, a.B, a.gw, a.inline_lgamma,
                         a.ll_part, a.dd_part, a.fwd ? 0 : a.dd_atomic, rg_tiles,
                         a.fwd ? nullptr : a.rg_slab, a.trows);
      if (!a.fwd && groups > 1) {
        constexpr int P = likelihood_heads(KIND);
        hipLaunchKernelGGL(d4_rg_combine_kernel, dim3((a.F + 1023) / 1024, P * (a.H + 1)),
                           dim3(256), 0, a.s, a.hp, P, a.H, a.F, a.rg_slab, groups - 1);
      }
      return 0;
    }
  }
  if constexpr (TERMS == 9) {
    if (a.fwd) {
      auto ffn = a.t.u16 ? decoder_head4_kernel<KIND, KS1, true, NPW, BN_, DBP, G1, 9, true, PACK>
                         : decoder_head4_kernel<KIND, KS1, false, NPW, BN_, DBP, G1, 9, true, PACK>;
      SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(ffn), (int)a.lds));
      hipLaunchKernelGGL(ffn, dim3(a.strips, groups), dim3(d4_threads(NPW)), a.lds, a.s, a.dA,
                         a.dT, a.rows, a.Rpad, a.H, a.hp, a.F, a.t, a.B, a.gw, a.inline_lgamma,
                         a.ll_part, a.dd_part, 0, rg_tiles, nullptr);
      return 0;
    }
  }
  auto kfn = a.t.u16 ? decoder_head4_kernel<KIND, KS1, true, NPW, BN_, DBP, G1, TERMS, false, PACK>
                     : decoder_head4_kernel<KIND, KS1, false, NPW, BN_, DBP, G1, TERMS, false, PACK>;
  SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(kfn), (int)a.lds));
  hipLaunchKernelGGL(kfn, dim3(a.strips, groups), dim3(d4_threads(NPW)), a.lds, a.s, a.dA, a.dT,
                     a.rows, a.Rpad, a.H, a.hp, a.F, a.t, a.B, a.gw, a.inline_lgamma, a.ll_part,
                     a.dd_part, a.dd_atomic, rg_tiles, a.rg_slab);
  if (groups > 1) {
    constexpr int P = likelihood_heads(KIND);
    hipLaunchKernelGGL(d4_rg_combine_kernel, dim3((a.F + 1023) / 1024, P * (a.H + 1)), dim3(256), 0,
                       a.s, a.hp, P, a.H, a.F, a.rg_slab, groups - 1);
  }
  return 0;
}
template <int KIND, int KS1>
static int d4_launch_steps(const D4Launch& a, const D4Config& c) {
  constexpr int P = likelihood_heads(KIND);
  // (the combinations d4_config can return for P heads and KS1 steps)
  if constexpr (KS1 >= 5) {
    if (c.dbp) {
      if constexpr (P == 1) return d4_launch_one<KIND, KS1, 4, 0, true>(a);
      else if constexpr (P == 2) return d4_launch_one<KIND, KS1, 4, 32, true>(a);
      else if constexpr (KS1 == 5) return d4_launch_one<KIND, KS1, 4, 0, true>(a);
    }
  }
  if constexpr (KS1 == 9) {
    set_error("decoder_head4_kernel: nine contraction steps only at H = 256");
    return -1;
  } else if constexpr (P == 1) {
    if constexpr (KS1 <= 4) { if (c.npw == 8) return d4_launch_one<KIND, KS1, 8, 0>(a); }
    return d4_launch_one<KIND, KS1, 4, 0>(a);
  } else if constexpr (P == 2) {
    if constexpr (KS1 <= 4) {
      if (c.bn == 64) return c.npw == 8 ? d4_launch_one<KIND, KS1, 8, 0>(a)
                                        : d4_launch_one<KIND, KS1, 4, 0>(a);
    }
    if constexpr (KS1 >= 4) return d4_launch_one<KIND, KS1, 4, 32>(a);
    set_error("decoder_head4_kernel: no instantiation for %d steps on %d-gene strips", KS1, c.bn);
    return -1;
  } else {
    if constexpr (KS1 <= 5) return d4_launch_one<KIND, KS1, 4, 0>(a);
    set_error("decoder_head4_kernel: three heads beyond H = 159");
    return -1;
  }
}
template <int KIND>
static int d4_launch_kind(const D4Launch& a, const D4Config& c) {
  switch (c.ks1) {
    case 1: return d4_launch_steps<KIND, 1>(a, c);
    case 2: return d4_launch_steps<KIND, 2>(a, c);
    case 3: return d4_launch_steps<KIND, 3>(a, c);
    case 4: return d4_launch_steps<KIND, 4>(a, c);
    case 5: return d4_launch_steps<KIND, 5>(a, c);
    case 6: return d4_launch_steps<KIND, 6>(a, c);
    case 7: return d4_launch_steps<KIND, 7>(a, c);
    case 8: return d4_launch_steps<KIND, 8>(a, c);
    case 9: return d4_launch_steps<KIND, 9>(a, c);
    default: set_error("decoder_head4_kernel: %d contraction steps", c.ks1); return -1;
  }
}

int decoder_fused3_launch(hipStream_t s, bool train, int kind, const float* d, int rows, int H,
                          HeadParams hp, int F, Targets t, int B, const float* gw,
                          int inline_lgamma, float* ll_part, float* dd_part, float* planes,
                          const HeadDropout* drop, int cp_pass, const CpRows* cp, int dd_mode,
                          float* rg_slab, const int64_t* t_rows) {
  const int P = likelihood_heads(kind);
  // (a row index: uint16 targets of the four count likelihoods, plain launches)
  SCVAE_ARG(!t_rows || (t.u16 && kind <= LK_ZINB && !drop && cp_pass == 0 && !(dd_mode & 6)));
  // (head4 alone: beyond the all-in-one-phase kernel's LDS budget; forward-only calls also the
  //  widths and head counts that kernel's forward instantiation does not take -- odd widths, three
  //  heads: decoder_fused_forward sends it exactly those)
  // (dd_mode & 8: a forward-only call asks for the producer / consumer kernel's forward half at a
  //  width the all-in-one-phase kernel would take too)
  const bool wide = !decoder_fused3_supported(P, H) ||
                    (!train && cp_pass == 0 &&
                     (P > 2 || !decoder_fused_supported(H) || (dd_mode & 8)));
  // (dd_mode & 4: the all-in-one-phase kernel whatever the row count -- the two launches of the
  //  piecewise categorical likelihood, whose strided heads and shifted targets only it takes)
  SCVAE_ARG(!(dd_mode & 4) || (train && !wide && !drop && cp_pass == 0));
  SCVAE_ARG((hp.gene_stride == 0 && t.shift == 0.f) || (dd_mode & 4));
  SCVAE_ARG(planes && (!wide || (!drop && cp_pass == 0 && decoder_fused4_supported(P, H))));
  SCVAE_ARG(train || !drop);
  SCVAE_ARG((kind == LK_CPOISSON) == (cp_pass >= 1 && cp_pass <= 3 && cp && cp->count_sum));
  SCVAE_ARG(cp_pass == 0 || ((cp_pass == 3) == train && !drop));
  const CpRows cpr = cp ? *cp : CpRows();
  // (forward only: one- and two-head likelihoods; the three-head one, on 32-gene strips, is
  //  no faster than decoder_forward_kernel: 0.92 vs 0.94 ms at 4096 x 32 738, the same step)
  const int Rpad = (rows + D3_BM - 1) / D3_BM * D3_BM;
  const int KP = d3_kp(H);
  uint16_t* dA = reinterpret_cast<uint16_t*>(planes);
  uint16_t* dT = dA + (size_t)3 * Rpad * KP;
  // (head dropout: one plane set per head, cut from that head's dropped-out copy of d, and the
  //  heads' masks as bits behind the three sets)
  uint32_t* bits = reinterpret_cast<uint32_t*>(dA + 3 * d3_set_elems(Rpad));
  // (the producer / consumer kernel with dd through atomics: its eight accumulators [8][H][rows]
  //  are cleared by the plane-cutting launch)
  const bool head4_train = train && !(dd_mode & 4) && !drop && cp_pass == 0 &&
                           d3_schedule(P, H, rows) == 4;
  const size_t acc_bytes = (size_t)8 * H * rows * sizeof(float);
  const bool clear_here = head4_train && (dd_mode & 1) && (acc_bytes & 15) == 0 &&
                          (reinterpret_cast<uintptr_t>(dd_part) & 15) == 0;
  // (the planes' remainder block packed: only for the producer / consumer kernel, and only where
  //  d4_launch_one picks its PACK instantiation; decoder_head3_kernel reads the plain layout)
  const bool to_head4 = cp_pass == 0 && !drop &&
                        (head4_train || (!train && wide));
  int pack_ks = -1;
  if (to_head4) {
    const D4Config c = d4_config(P, H);
    if (c.bn == d3_bn(P) && !c.dbp && d4_packed(c.ks1, H)) pack_ks = c.ks1 - 1;
  }
  for (int j = 0; j < (drop ? P : 1); ++j) {
    hipLaunchKernelGGL(split3_hidden_kernel, dim3((Rpad * (KP / 8) + 255) / 256, train ? 2 : 1),
                       dim3(256), 0, s, drop ? drop->d[j] : d, rows, H, Rpad, KP,
                       dA + j * d3_set_elems(Rpad), dT + j * d3_set_elems(Rpad),
                       clear_here ? reinterpret_cast<u32x4*>(dd_part) : nullptr,
                       clear_here ? acc_bytes / 16 : (size_t)0, pack_ks);
    SCVAE_LAUNCH_CHECK("split3_hidden_kernel");
    if (drop) {
      const int rc = dropout_mask_words(s, bits + (size_t)j * Rpad * 4, rows, Rpad, H, drop->keep,
                                        drop->seed, drop->site[j], drop->map);
      if (rc) return rc;
    }
  }
  const float inv_keep = drop ? 1.f / drop->keep : 1.f;
  const size_t lds = decoder_fused3_lds_bytes(P, H);
  const int strips = (F + d3_bn(P) - 1) / d3_bn(P);
  const int ks1 = (d3_hp1(H) + 31) / 32;
#define SCVAE_D3KC(K_, KS_, T_, D_, C_)                                                          \
  do {                                                                                            \
    auto kfn = t.u16 ? decoder_head3_kernel<K_, KS_, true, T_, D_, C_>                            \
                     : decoder_head3_kernel<K_, KS_, false, T_, D_, C_>;                          \
    SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(kfn), \
                                  (int)lds));         \
    hipLaunchKernelGGL(kfn, dim3(strips), dim3(D3_THREADS), lds, s, dA, dT, rows, Rpad, H, hp, F, \
                       t, B, gw, inline_lgamma, ll_part, dd_part, bits, inv_keep, cpr);           \
  } while (0)
#define SCVAE_D3K(K_, KS_, T_, D_) SCVAE_D3KC(K_, KS_, T_, D_, 0)
#define SCVAE_D3RK(K_, KS_, T_)                                                                   \
  do {                                                                                            \
    auto kfn = decoder_head3_rows_kernel<K_, KS_, T_>;                                            \
    SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(kfn), (int)lds));                     \
    hipLaunchKernelGGL(kfn, dim3(strips), dim3(D3_THREADS), lds, s, dA, dT, rows, Rpad, H, hp, F, \
                       t, B, gw, inline_lgamma, ll_part, dd_part, t_rows);                        \
  } while (0)
#define SCVAE_D3R(K_, T_)                                                                         \
  switch (ks1) {                                                                                  \
    case 1: SCVAE_D3RK(K_, 1, T_); break;                                                         \
    case 2: SCVAE_D3RK(K_, 2, T_); break;                                                         \
    case 3: SCVAE_D3RK(K_, 3, T_); break;                                                         \
    default: SCVAE_D3RK(K_, 4, T_); break;                                                        \
  }
#define SCVAE_D3C(T_, C_)                                                                         \
  switch (ks1) {                                                                                  \
    case 1: SCVAE_D3KC(LK_CPOISSON, 1, T_, false, C_); break;                                     \
    case 2: SCVAE_D3KC(LK_CPOISSON, 2, T_, false, C_); break;                                     \
    case 3: SCVAE_D3KC(LK_CPOISSON, 3, T_, false, C_); break;                                     \
    default: SCVAE_D3KC(LK_CPOISSON, 4, T_, false, C_); break;                                    \
  }
#define SCVAE_D3(K_, T_, D_)                                                                      \
  switch (ks1) {                                                                                  \
    case 1: SCVAE_D3K(K_, 1, T_, D_); break;                                                      \
    case 2: SCVAE_D3K(K_, 2, T_, D_); break;                                                      \
    case 3: SCVAE_D3K(K_, 3, T_, D_); break;                                                      \
    default: SCVAE_D3K(K_, 4, T_, D_); break;                                                     \
  }
  if (train && decoder_fused_probe(0)) SCVAE_HIP(hipEventRecord(decoder_fused_probe(0), s));
  if (cp_pass == 1) {
    SCVAE_D3C(false, 1);
  } else if (cp_pass == 2) {
    SCVAE_D3C(false, 2);
  } else if (cp_pass == 3) {
    SCVAE_D3C(true, 3);
  } else if (train && drop) {
    switch (kind) {
      case LK_POISSON: SCVAE_D3(LK_POISSON, true, true); break;
      case LK_NB: SCVAE_D3(LK_NB, true, true); break;
      case LK_ZIP: SCVAE_D3(LK_ZIP, true, true); break;
      case LK_ZINB: SCVAE_D3(LK_ZINB, true, true); break;
      case LK_BERNOULLI: SCVAE_D3(LK_BERNOULLI, true, true); break;
      default: set_error("decoder_head3_kernel: likelihood kind %d", kind); return -1;
    }
  } else if ((train && !(dd_mode & 4) && d3_schedule(P, H, rows) == 4) || (!train && wide)) {
    const D4Config c = d4_config(P, H);
    D4Launch a{s, dA, dT, rows, Rpad, H, hp, F, t, B, gw, inline_lgamma, ll_part, dd_part,
               (dd_mode & 1) ? 1 : 0, (F + c.bn - 1) / c.bn, c.lds, (dd_mode & 2) ? 6 : 9, 1,
               rg_slab};
    a.fwd = !train;
    a.trows = t_rows;
    if (a.fwd) { a.dd_atomic = 0; a.terms = 9; }
    // (no slab from the caller: one group -- the stand-alone forward-only / probe entries; the
    //  forward half leaves no dW and needs none)
    if (rg_slab || a.fwd) a.row_groups = d4_row_groups(a.strips, rows);
    if (a.dd_atomic && !clear_here)   // eight XCD-local accumulators [8][H][rows], cleared for this launch
      SCVAE_HIP(hipMemsetAsync(dd_part, 0, (size_t)8 * H * rows * sizeof(float), s));
    int rc;
    switch (kind) {
      case LK_POISSON: rc = d4_launch_kind<LK_POISSON>(a, c); break;
      case LK_NB: rc = d4_launch_kind<LK_NB>(a, c); break;
      case LK_ZIP: rc = d4_launch_kind<LK_ZIP>(a, c); break;
      case LK_ZINB: rc = d4_launch_kind<LK_ZINB>(a, c); break;
      case LK_BERNOULLI: rc = d4_launch_kind<LK_BERNOULLI>(a, c); break;   // du:194-204; targets binarised by the caller
      default: set_error("decoder_head4_kernel: likelihood kind %d", kind); return -1;
    }
    if (rc) return rc;
  } else if (t_rows && train) {
    switch (kind) {
      case LK_POISSON: SCVAE_D3R(LK_POISSON, true); break;
      case LK_NB: SCVAE_D3R(LK_NB, true); break;
      case LK_ZIP: SCVAE_D3R(LK_ZIP, true); break;
      default: SCVAE_D3R(LK_ZINB, true); break;
    }
  } else if (t_rows) {
    switch (kind) {
      case LK_POISSON: SCVAE_D3R(LK_POISSON, false); break;
      case LK_NB: SCVAE_D3R(LK_NB, false); break;
      case LK_ZIP: SCVAE_D3R(LK_ZIP, false); break;
      default: set_error("decoder_head3_kernel (forward): likelihood kind %d", kind); return -1;
    }
  } else if (train) {
    switch (kind) {
      case LK_POISSON: SCVAE_D3(LK_POISSON, true, false); break;
      case LK_NB: SCVAE_D3(LK_NB, true, false); break;
      case LK_ZIP: SCVAE_D3(LK_ZIP, true, false); break;
      case LK_ZINB: SCVAE_D3(LK_ZINB, true, false); break;
      case LK_BERNOULLI: SCVAE_D3(LK_BERNOULLI, true, false); break;   // du:194-204; targets binarised by the caller
      case LK_CAT2: SCVAE_D3(LK_CAT2, true, false); break;   // the class logits of -k (decoder_fused_train_cat)
      case LK_CAT3: SCVAE_D3(LK_CAT3, true, false); break;
      default: set_error("decoder_head3_kernel: likelihood kind %d", kind); return -1;
    }
  } else {
    switch (kind) {
      case LK_POISSON: SCVAE_D3(LK_POISSON, false, false); break;
      case LK_NB: SCVAE_D3(LK_NB, false, false); break;
      case LK_ZIP: SCVAE_D3(LK_ZIP, false, false); break;
      case LK_BERNOULLI: SCVAE_D3(LK_BERNOULLI, false, false); break;
      default: set_error("decoder_head3_kernel (forward): likelihood kind %d", kind); return -1;
    }
  }
#undef SCVAE_D3
#undef SCVAE_D3R
#undef SCVAE_D3RK
#undef SCVAE_D3C
#undef SCVAE_D3KC
#undef SCVAE_D3K
  SCVAE_LAUNCH_CHECK("decoder_head3_kernel");
  if (train && decoder_fused_probe(1)) SCVAE_HIP(hipEventRecord(decoder_fused_probe(1), s));
  return 0;
}

}  // namespace scvae
