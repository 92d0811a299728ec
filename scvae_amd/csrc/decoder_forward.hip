// Forward-only decoder output layer: X_TILDE heads + count likelihood + row sum in one kernel,
// for the graph executions with is_training = False (the epoch-end evaluations of train(),
// va:1092-1150 / 1251-1304, evaluate(), va:1969-2055) and the first pass of an importance-
// weighted training step.  Same inputs and per-strip partial buffer as the training kernels
// (decoder_fused.hip), a different organisation, because nothing has to go back to the matrix
// cores after the likelihood:
//
//   * a workgroup owns a 64-gene strip (weights and biases in LDS for the whole kernel); its waves
//     walk over their own 32-row tiles independently -- no workgroup barrier in the loop, and no
//     LDS staging of d: in the k-slot layout chosen below a lane's share of the d tile is one
//     contiguous run of its row, read from L2 with 16-byte loads into the registers that feed the
//     MFMAs (the next tile's run is requested as soon as the last MFMA of the tile is issued);
//   * a wave computes the TRANSPOSED head tile pre_j^T[gene, row] = W_j^T d^T with
//     v_mfma_f32_32x32x2: in the result layout a lane then holds 16 genes of ONE row, so the
//     likelihood of its 16 elements sums into one register, and the row sum of the tile is that
//     register plus the one of lane ^ 32.  The pre-activations never leave the registers;
//   * the bias rides along as an extra contraction step (d gets a ones column, W_j the bias row);
//   * t is read from HBM straight into that register layout (16-byte loads), in flight under
//     the MFMAs;
//   * the t > 0 corrections of the negative-binomial kinds, lgamma(r+t) - lgamma(r), are the
//     expensive part of an element but needed for 5 % of them: each lane walks over its own
//     non-zero elements (bit mask + find-first-set), so the cost follows the largest count of a
//     lane (about 3 of 16) instead of 16.
//
// MFMA work 2 * P * (H + 2) flop per element; algorithmic HBM traffic 4 B per element (t).
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"
#include "likelihood.hpp"

namespace scvae {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int FW_BN = 64;         // genes per workgroup (= the strip width of ll_part)
constexpr int FW_LD = FW_BN + 1;  // odd LDS row stride of the weight strip
constexpr int FW_BM = 32;         // rows per wave tile
constexpr int FW_HMAX = 126;

// contraction length: H, the ones column (bias), zero padding up to a multiple of 8, so that each
// of the two k-slots covers a multiple of 4 positions.  The number of MFMA steps, HK / 2, is a
// template parameter of the kernel (in units of 4 steps): the d operands live in registers, which
// only works with compile-time indices, and a guard per step makes the compiler copy the
// accumulators at every merge point.
__host__ __device__ inline int fw_hk(int H) { return (H + 8) / 8 * 8; }

static size_t fw_lds_bytes(int P, int H) { return (size_t)P * fw_hk(H) * FW_LD * sizeof(float); }
bool decoder_forward_supported(int P, int H) {
  return H >= 2 && H <= FW_HMAX && (H % 2) == 0 && fw_lds_bytes(P, H) <= 160 * 1024;
}

// One of 16 registers by a per-lane index: a binary tree of 15 v_cndmask under the four lane masks
// of the index bits.  (Written with inline asm: as C++ selects the compiler folds the tree into a
// dynamically indexed array, which for a per-lane index means scratch memory.)
struct IndexMasks { unsigned long long m[4]; };
__device__ __forceinline__ IndexMasks index_masks(int idx) {
  IndexMasks k;
#pragma unroll
  for (int b = 0; b < 4; ++b) k.m[b] = __builtin_amdgcn_ballot_w64((idx >> b) & 1);
  return k;
}
__device__ __forceinline__ float cnd(float lo, float hi, unsigned long long mask) {
  float r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(lo), "v"(hi), "s"(mask));
  return r;
}
__device__ __forceinline__ float select16(const float (&v)[16], const IndexMasks& k) {
  float a[8], b[4], c[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = cnd(v[2 * i], v[2 * i + 1], k.m[0]);
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = cnd(a[2 * i], a[2 * i + 1], k.m[1]);
#pragma unroll
  for (int i = 0; i < 2; ++i) c[i] = cnd(b[2 * i], b[2 * i + 1], k.m[2]);
  return cnd(c[0], c[1], k.m[3]);
}

// U16 (compile time): the targets are the uint16 minibatch (as a run-time flag the two load paths
// met in a branch and every target load was waited for inside it, before the products started)
// IDX (decoder_forward_rows_kernel): the uint16 targets are rows of a resident matrix, cell b its
// row trows[b]; a lane fetches the index of its row of the wave's next tile with that tile's d.
template <int KIND, int KS4, bool U16>
__global__ __launch_bounds__(512) void decoder_forward_kernel(
    const float* __restrict__ d, int R, int H, HeadParams hp, int F, Targets tg,
    int B, int inline_lgamma, float* __restrict__ ll_part) {
  constexpr bool IDX = false;
  const int64_t* const trows = nullptr;
#include "decoder_forward_body.inc"
}
template <int KIND, int KS4>
__global__ __launch_bounds__(512) void decoder_forward_rows_kernel(
    const float* __restrict__ d, int R, int H, HeadParams hp, int F, Targets tg,
    int B, int inline_lgamma, float* __restrict__ ll_part, const int64_t* __restrict__ trows) {
  constexpr bool U16 = true, IDX = true;
#include "decoder_forward_body.inc"
}

int decoder_forward_launch(hipStream_t s, int kind, const float* d, int rows, int H, HeadParams hp,
                           int F, Targets t, int B, int inline_lgamma, float* ll_part,
                           const int64_t* t_rows) {
  const int P = likelihood_heads(kind);
  const size_t lds = fw_lds_bytes(P, H);
  const int strips = (F + FW_BN - 1) / FW_BN;
  if (t_rows) {       // the uint16 targets through a row index: the four count likelihoods
    SCVAE_ARG(t.u16 && kind <= LK_ZINB && t.shift == 0.f);
#define SCVAE_FWR(K_, KS_)                                                                      \
  case KS_: {                                                                                   \
    auto kfn = decoder_forward_rows_kernel<K_, KS_>;                                            \
    SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(kfn), (int)lds));                   \
    hipLaunchKernelGGL(kfn, dim3(strips), dim3(512), lds, s, d, rows, H, hp, F, t, B,           \
                       inline_lgamma, ll_part, t_rows);                                         \
  } break
#define SCVAE_FWRK(K_)                                                                          \
  switch (fw_hk(H) / 8) {                                                                       \
    SCVAE_FWR(K_, 1); SCVAE_FWR(K_, 2); SCVAE_FWR(K_, 3); SCVAE_FWR(K_, 4); SCVAE_FWR(K_, 5);   \
    SCVAE_FWR(K_, 6); SCVAE_FWR(K_, 7); SCVAE_FWR(K_, 8); SCVAE_FWR(K_, 9); SCVAE_FWR(K_, 10);  \
    SCVAE_FWR(K_, 11); SCVAE_FWR(K_, 12); SCVAE_FWR(K_, 13); SCVAE_FWR(K_, 14);                 \
    SCVAE_FWR(K_, 15); SCVAE_FWR(K_, 16);                                                       \
    default: set_error("decoder_forward: hidden size %d", H); return -1;                        \
  }
    switch (kind) {
      case LK_POISSON: SCVAE_FWRK(LK_POISSON); break;
      case LK_NB: SCVAE_FWRK(LK_NB); break;
      case LK_ZIP: SCVAE_FWRK(LK_ZIP); break;
      default: SCVAE_FWRK(LK_ZINB); break;
    }
#undef SCVAE_FWRK
#undef SCVAE_FWR
    SCVAE_LAUNCH_CHECK("decoder_forward_rows_kernel");
    return 0;
  }
#define SCVAE_FW(K_, KS_)                                                                       \
  case KS_: {                                                                                   \
    auto kfn = t.u16 ? decoder_forward_kernel<K_, KS_, true>                                    \
                     : decoder_forward_kernel<K_, KS_, false>;                                  \
    SCVAE_HIP(max_dynamic_lds(reinterpret_cast<const void*>(kfn), \
                                  (int)lds));       \
    hipLaunchKernelGGL(kfn, dim3(strips), dim3(512), lds, s, d, rows, H, hp, F, t, B,           \
                       inline_lgamma, ll_part);                                                 \
  } break
#define SCVAE_FWK(K_)                                                                           \
  switch (fw_hk(H) / 8) {                                                                       \
    SCVAE_FW(K_, 1); SCVAE_FW(K_, 2); SCVAE_FW(K_, 3); SCVAE_FW(K_, 4); SCVAE_FW(K_, 5);        \
    SCVAE_FW(K_, 6); SCVAE_FW(K_, 7); SCVAE_FW(K_, 8); SCVAE_FW(K_, 9); SCVAE_FW(K_, 10);       \
    SCVAE_FW(K_, 11); SCVAE_FW(K_, 12); SCVAE_FW(K_, 13); SCVAE_FW(K_, 14); SCVAE_FW(K_, 15);   \
    SCVAE_FW(K_, 16);                                                                           \
    default: set_error("decoder_forward: hidden size %d", H); return -1;                        \
  }
  switch (kind) {
    case LK_POISSON: SCVAE_FWK(LK_POISSON); break;
    case LK_NB: SCVAE_FWK(LK_NB); break;
    case LK_ZIP: SCVAE_FWK(LK_ZIP); break;
    case LK_ZINB: SCVAE_FWK(LK_ZINB); break;
    case LK_BERNOULLI: SCVAE_FWK(LK_BERNOULLI); break;   // du:194-204; targets binarised by the caller
    case LK_CAT2: SCVAE_FWK(LK_CAT2); break;   // the class logits of -k (decoder_fused_forward_cat)
    case LK_CAT3: SCVAE_FWK(LK_CAT3); break;
    default: set_error("unknown likelihood kind %d", kind); return -1;
  }
#undef SCVAE_FWK
#undef SCVAE_FW
  SCVAE_LAUNCH_CHECK("decoder_forward_kernel");
  return 0;
}

}  // namespace scvae
