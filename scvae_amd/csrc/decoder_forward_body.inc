// Body of decoder_forward_kernel / _rows_kernel: included once per kernel, which sets IDX (and, where IDX is false, a null
// index pointer) in front of it -- see there.  Not a translation unit of its own.
  using Traits = LikelihoodTraits<KIND>;
  constexpr int P = Traits::P;
  constexpr int NW = 8;
  constexpr int BN = FW_BN, LD = FW_LD, BM = FW_BM;
  extern __shared__ __attribute__((aligned(16))) float Ws[];   // [P][HK][LD]; row H = bias
  constexpr int HS = 4 * KS4;         // MFMA steps; k-slot kh covers positions [kh*HS, kh*HS+HS)
  constexpr int HK = 2 * HS;          // == fw_hk(H)
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, kh = lane >> 5;
  const int c0 = blockIdx.x * BN;

  // ---- strip weights (rows 0..H-1), biases (row H), zeros (rows H+1..HK-1) -> LDS, once ----
  {
    // (all of a thread's loads in flight together, from clamped -- always valid -- addresses: a
    //  loop with one load per trip pays a global-memory round trip per weight row)
    const int c = tid & (BN - 1), p0 = tid >> 6;
    const bool col_ok = c0 + c < F;
    const int cc = min(c0 + c, F - 1);
    constexpr int NV = HK / NW;                        // rows p0 + NW u < HK of this thread
    float v[P][NV];
    // (the plain [H, F] layout, or -- the class logits of the P_K head of `-k` -- genes
    //  gene_stride apart in rows of row_pitch elements: kernels.hpp, HeadParams)
    const size_t gs = hp.gene_stride ? hp.gene_stride : 1;
    const size_t rp = hp.row_pitch ? hp.row_pitch : F;
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int pos = p0 + u * NW;
        v[j][u] = pos < H ? hp.W[j][(size_t)pos * rp + cc * gs] : hp.b[j][cc * gs];
      }
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int pos = p0 + u * NW;
        Ws[((size_t)j * HK + pos) * LD + c] = (col_ok && pos <= H) ? v[j][u] : 0.f;
      }
  }
  __syncthreads();

  // ---- this lane's share of a d tile: row li, positions [kh*HS, kh*HS + HS), as the B operand
  //      of step s in dB[s].  H is even and HS is even: pairs never straddle H. ----
  float dB[HS];
  auto load_d = [&](int m0) {
    const int row = min(m0 + li, R - 1);             // (rows beyond R: results are not stored)
    const float* src = d + (size_t)row * H + kh * HS;
    const int p0 = kh * HS;
    // HS is a multiple of 4 and H is even: a group of 4 positions is inside the row, or holds
    // its last two elements, or starts at the ones column / in the zero padding
    typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
    typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
#pragma unroll
    for (int q = 0; q < HS / 4; ++q) {
      const int pos = p0 + 4 * q;
      f32x4u v = {0.f, 0.f, 0.f, 0.f};
      if (pos + 3 < H) {
        v = *reinterpret_cast<const f32x4u*>(src + 4 * q);
      } else if (pos + 1 < H) {
        const f32x2u lo = *reinterpret_cast<const f32x2u*>(src + 4 * q);
        v.x = lo.x; v.y = lo.y; v.z = 1.f;       // pos + 2 == H: the ones column
      } else if (pos == H) {
        v.x = 1.f;
      }
      dB[4 * q] = v.x; dB[4 * q + 1] = v.y; dB[4 * q + 2] = v.z; dB[4 * q + 3] = v.w;
    }
  };
  const int n_tiles = (R + BM - 1) / BM;

  auto load_i = [&](int m0) -> size_t { return (size_t)trows[min(m0 + li, R - 1) % B]; };
  load_d(w * BM);
  size_t tidx = IDX ? load_i(w * BM) : 0;
  for (int tile = w; tile < n_tiles; tile += NW) {
    const int m0 = tile * BM;
    const int row = m0 + li;
    const bool row_ok = row < R;
    const size_t trow_off = (IDX ? tidx : (size_t)((row_ok ? row : R - 1) % B)) * tg.ld;
    if (IDX) tidx = load_i(m0 + NW * BM);
    float lane_sum = 0.f;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      // ---- t of this lane's 16 elements: genes cbase + 8*(i>>2) + (i&3), row li ----
      const int cbase = c0 + cb * 32 + 4 * kh;
      float tv[16];
      if (U16) {           // the uint16 minibatch: four counts per 8-byte load (the pitch covers
                           // whole 64-gene strips, pad columns zero: no bound, no branch, and
                           // nothing touches the loaded value before its use -- a select on it
                           // would end the load's flight)
        const uint16_t* trow = static_cast<const uint16_t*>(tg.p) + trow_off;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = cbase + 8 * g;
          typedef unsigned u32x2u __attribute__((ext_vector_type(2), aligned(4)));
          const u32x2u v = *reinterpret_cast<const u32x2u*>(trow + c);
          tv[4 * g] = (float)(v.x & 0xFFFFu); tv[4 * g + 1] = (float)(v.x >> 16);
          tv[4 * g + 2] = (float)(v.y & 0xFFFFu); tv[4 * g + 3] = (float)(v.y >> 16);
        }
      } else {
        const float* trow = static_cast<const float*>(tg.p) + trow_off;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c = cbase + 8 * g;
          if (c + 3 < F) {   // one 16-byte load (global loads need only 4-byte alignment)
            typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
            const f32x4u v = *reinterpret_cast<const f32x4u*>(trow + c);
            tv[4 * g] = v.x; tv[4 * g + 1] = v.y; tv[4 * g + 2] = v.z; tv[4 * g + 3] = v.w;
          } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) tv[4 * g + u] = (c + u < F) ? trow[c + u] : 0.f;
          }
        }
      }
      // ---- pre_j^T[gene, row] = sum_pos Ws_j[pos, gene] * d[row, pos] ----
      f32x16 acc[P];
#pragma unroll
      for (int j = 0; j < P; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
      const float* ap = Ws + (size_t)(kh * HS) * LD + cb * 32 + li;   // A[m = gene][k-slot kh]
#pragma unroll
      for (int s = 0; s < HS; ++s)
#pragma unroll
        for (int j = 0; j < P; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[(j * HK + s) * LD], dB[s], acc[j], 0, 0,
                                                        0);
      // the d registers are free again: request this wave's next tile, it arrives during the
      // likelihood math below
      if (cb == 1) load_d(m0 + NW * BM);
      // ---- likelihood of the 16 elements ----
      unsigned nz = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float a[P], lp, g[P], r, rgate;
#pragma unroll
        for (int j = 0; j < P; ++j) a[j] = acc[j][i];
        // (tg.shift > 0 -- the count part of the piecewise categorical likelihood: the
        //  distribution sees t - shift where t >= shift, nothing elsewhere; 0: every element)
        const bool live = tv[i] >= tg.shift;
        tv[i] = live ? tv[i] - tg.shift : 0.f;
        lik_dense<KIND, false>(tv[i], a, lp, g, r, rgate);
        const int c = cbase + 8 * (i >> 2) + (i & 3);
        lane_sum += (live && c < F) ? lp : 0.f;
        nz |= (live && tv[i] > 0.f) ? (1u << i) : 0u;    // (t of a gene beyond F was loaded as 0)
        // four elements at a time: the 16 are independent, interleaving all of them only
        // costs registers
        if ((i & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
      // ---- t > 0: + lgamma(r+t) - lgamma(r)  [- lgamma(1+t) unless the caller adds it] ----
      if (Traits::HAS_R || inline_lgamma) {
        while (__builtin_amdgcn_ballot_w64(nz != 0) != 0) {
          const bool on = nz != 0;
          const int idx = on ? __builtin_ctz(nz) : 0;
          nz &= nz - 1;
          const IndexMasks km = index_masks(idx);
          const float tt = select16(tv, km);
          float corr = 0.f;
          if (Traits::HAS_R) {
            // total_count = exp(clip(log_r pre-activation)), the last head (du:266-305)
            float lr[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) lr[i] = acc[P - 1][i];
            const float r = __expf(fminf(fmaxf(select16(lr, km), -10.f), 10.f));
            // one form for the whole wave: the product recurrence if every pending count is a
            // small integer, else the general form (exact for those as well)
            const bool small = !on || (tt <= 8.f && tt == __builtin_rintf(tt));
            float A, D;
            if (__builtin_amdgcn_ballot_w64(!small) == 0)
              lgamma_digamma_diff_small<false>(r, on ? tt : 0.f, A, D);
            else
              lgamma_digamma_diff_general<false>(r, on ? tt : 1.f, A, D);
            corr = A;
          }
          if (inline_lgamma) corr -= lgamma1p(tt);
          lane_sum += on ? corr : 0.f;
        }
      }
    }
    // row sum of the strip: this lane's 32 genes + the 32 of lane ^ 32
    lane_sum += __shfl_xor(lane_sum, 32, 64);
    if (kh == 0 && row_ok) ll_part[(size_t)blockIdx.x * R + row] = lane_sum;
  }
