// Body of count_gemm_dw_kernel / _rows_kernel: included once per kernel, which sets IDX (and, where IDX is false, a null
// index pointer) in front of it -- see there.  Not a translation unit of its own.
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2][3 * CG_NP * CD_ROW];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, kg = lane >> 5;
  constexpr int NTHR = 64 * NW, NPC = (768 + NTHR - 1) / NTHR;   // pieces of dA per thread
  const int m_w = blockIdx.x * (NW * CG_TM) + w * CG_TM;       // first gene of this wave
  const int k_begin = blockIdx.y * k_chunk;
  const int k_end = min(K, k_begin + k_chunk);

  f32x16 acc[2][NT];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][q][i] = 0.f;

  // raw[slot][t][j]  <->  cell kc + 8 kg + j of gene tile t; uniform row pointer + per-lane
  // 32-bit element offset (gene + 8 kg rows)
  // PAIR (uint16 counts, M even): a lane reads genes 2 li and 2 li + 1 of the wave's 64 with one
  // 4-byte load -- gene tile 0 takes the even genes, tile 1 the odd ones -- half the load
  // instructions of the lane-per-gene pattern for the same bytes.
  static_assert(!PAIR || sizeof(XT) == 2, "gene pairs: uint16 counts");
  XT raw[2][2][PAIR ? 1 : 8];
  unsigned rawp[2][PAIR ? 8 : 1];
  unsigned xoff[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
    xoff[t] = (IDX ? 0u : (unsigned)(8 * kg) * (unsigned)ldx) +
              (PAIR ? (unsigned)min(m_w + 2 * li, M - 2)
                    : (unsigned)min(m_w + 32 * t + li, M - 1));
  // the count of gene tile t, cell j of the slot, as fp32
  auto value = [&](auto slot_tag, int t, int j) -> float {
    constexpr int SLOT = decltype(slot_tag)::value;
    if constexpr (PAIR) return (float)(t == 0 ? (rawp[SLOT][j] & 0xFFFFu) : (rawp[SLOT][j] >> 16));
    else return count_to_f32(raw[SLOT][t][j]);
  };
  u32x4 breg[USE_STEADY ? 2 : 1][NPC];
  auto load_x = [&](int kc, auto slot_tag) {
    constexpr int SLOT = decltype(slot_tag)::value;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const XT* srow;
      if constexpr (IDX) {
        const int64_t r0 = xrows[kc + j], r1 = xrows[kc + j + 8];   // uniform: scalar loads
        srow = X + (size_t)(kg ? r1 : r0) * (size_t)ldx;
      } else {
        srow = X + (size_t)(kc + j) * ldx;                       // uniform: scalar base
      }
      if constexpr (PAIR) {
        rawp[SLOT][j] = cg_load<(SCVAE_CG_NT & 2) != 0>(
            reinterpret_cast<const unsigned*>(srow + xoff[0]));
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t)
          raw[SLOT][t][j] = cg_load<(SCVAE_CG_NT & 2) != 0>(srow + xoff[t]);
      }
    }
  };
  auto load_b = [&](int kc, int slot = 0) {
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
      const int p = tid + NTHR * i;                // 768 pieces: (term, column, half)
      const int row = p >> 1, part = p & 1;        // row = term * 128 + column
      // (columns beyond N: the last live column's piece again -- a line this wave requests
      //  anyway, no branch around the load; what they multiply into is never stored)
      const int col = row & (CG_NP - 1), rowl = col < N ? row : row - col + (N - 1);
      if (p < 768 && col < NT * 32)
        breg[slot][i] = *reinterpret_cast<const u32x4*>(T + cg_piece<CD_BK>(kc, rowl, part));
    }
  };
  auto store_b = [&](int buf, int slot = 0) {
#pragma unroll
    for (int i = 0; i < NPC; ++i) {
      const int p = tid + NTHR * i;
      const int row = p >> 1, part = p & 1;
      if (p < 768 && (row & (CG_NP - 1)) < NT * 32)
        *reinterpret_cast<u32x4*>(&Bs[buf][row * CD_ROW + part * 16]) = breg[slot][i];
    }
  };
  // (USE_STEADY: every request of the loop is unconditional -- a chunk index beyond the split's
  //  last chunk is clamped to it, its data never used -- so that the compiler can count the
  //  loads in flight; dA travels TWO chunks ahead, like x)
  const int k_last = k_end - CD_BK;
  auto clampk = [&](int k) { return min(k, k_last); };

  if (k_begin < k_end) {
    load_x(k_begin, std::integral_constant<int, 0>{});
    if (USE_STEADY) load_x(clampk(k_begin + CD_BK), std::integral_constant<int, 1>{});
    else if (k_begin + CD_BK < k_end) load_x(k_begin + CD_BK, std::integral_constant<int, 1>{});
    load_b(k_begin);
    store_b(0);
    if (USE_STEADY) load_b(clampk(k_begin + CD_BK), 1);
  }
  __syncthreads();

  const int frag_off = li * CD_ROW + 16 * kg;
  // STEADY (compile time): chunks j + 1 and j + 2 exist -- requests and hand-over unconditional
  // (see count_gemm_fwd_kernel).  Measured on this kernel the unconditional loop is SLOWER (178 vs
  // 155 us at 4096 x 32 738: both x chunks then really stay in flight, the kernel sits at 256
  // VGPRs and the deeper queue does not pay), so USE_STEADY defaults to off here.
  auto chunk = [&](int kc, auto buf_tag, auto steady_tag) {
    constexpr int BUF = decltype(buf_tag)::value;        // LDS buffer and x slot of this chunk
    constexpr bool STEADY = decltype(steady_tag)::value;
    // ---- cut the counts of this chunk into hi / lo bf16 fragments ----
    u32x4 ahi[2], alo[2];
    unsigned low_bits = 0u;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      unsigned h[4];
#pragma unroll
      for (int pr = 0; pr < 4; ++pr) {
        const unsigned u0 = __float_as_uint(value(buf_tag, t, 2 * pr));
        const unsigned u1 = __float_as_uint(value(buf_tag, t, 2 * pr + 1));
        low_bits |= u0 | u1;
        h[pr] = __builtin_amdgcn_perm(u1, u0, 0x07060302u);          // upper halves
      }
      ahi[t] = u32x4{h[0], h[1], h[2], h[3]};
    }
    const bool need_lo =
        __builtin_amdgcn_readfirstlane(__any((int)((low_bits & 0xFFFFu) != 0u)));
    if (need_lo) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        unsigned l[4];
#pragma unroll
        for (int pr = 0; pr < 4; ++pr) {
          const float x0 = value(buf_tag, t, 2 * pr);
          const float x1 = value(buf_tag, t, 2 * pr + 1);
          const float l0 = x0 - __uint_as_float(__float_as_uint(x0) & 0xFFFF0000u);
          const float l1 = x1 - __uint_as_float(__float_as_uint(x1) & 0xFFFF0000u);
          l[pr] = __builtin_amdgcn_perm(__float_as_uint(l1), __float_as_uint(l0), 0x07060302u);
        }
        alo[t] = u32x4{l[0], l[1], l[2], l[3]};
      }
    }
    // ---- requests: dA one chunk ahead, x two chunks ahead (the slot just converted).  dA first:
    //      in the unconditional loop (STEADY) the wait for dA at the end of the chunk (store_b)
    //      is then vmcnt(8) and leaves the eight younger x loads in flight across the barrier;
    //      with x first it was vmcnt(0) -- the counter retires in issue order -- and in the
    //      conditional loop it still is (the compiler cannot count loads under a branch): every
    //      x request lands within the chunk that issued it.  Measured (round 5, SCVAE_CD_STEADY,
    //      tools/ab_cd_steady.sh): with the x requests really in flight the kernel is SLOWER,
    //      138.8-142.2 against 134.7-137.2 us stand-alone, + 7 us in the step -- as round 2
    //      found with the other order; the default stays the conditional loop ----
    const bool has_next = STEADY || kc + CD_BK < k_end;
    if (STEADY) {
      load_b(clampk(kc + 2 * CD_BK), BUF);
      __builtin_amdgcn_sched_barrier(0);
      load_x(clampk(kc + 2 * CD_BK), buf_tag);
    } else {
      if (has_next) load_b(kc + CD_BK);
      __builtin_amdgcn_sched_barrier(0);
      if (kc + 2 * CD_BK < k_end) load_x(kc + 2 * CD_BK, buf_tag);
    }
    __builtin_amdgcn_sched_barrier(0);

    const unsigned char* bcur = Bs[BUF] + frag_off;
#pragma unroll
    for (int term = 2; term >= 0; --term) {              // smallest term first
      bf16x8 fr[NT];
#pragma unroll
      for (int q = 0; q < NT; ++q)
        fr[q] = as_bf16x8(*reinterpret_cast<const u32x4*>(
            bcur + (term * CG_NP + q * 32) * CD_ROW));
      if (need_lo) {
#pragma unroll
        for (int q = 0; q < NT; ++q) {
          acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(alo[0]), fr[q], acc[0][q],
                                                              0, 0, 0);
          acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(alo[1]), fr[q], acc[1][q],
                                                              0, 0, 0);
        }
      }
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(ahi[0]), fr[q], acc[0][q], 0,
                                                            0, 0);
        acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(ahi[1]), fr[q], acc[1][q], 0,
                                                            0, 0);
      }
    }
    if (STEADY) store_b(BUF ^ 1, BUF ^ 1);     // (dA of chunk kc + 1: requested a chunk ago)
    else if (has_next) store_b(BUF ^ 1);
    lds_barrier();       // (LDS only: the x requests stay in flight across it)
  };
  {
    using B0 = std::integral_constant<int, 0>;
    using B1 = std::integral_constant<int, 1>;
    int kc = k_begin;
    if (USE_STEADY) {
      for (; kc + CD_BK < k_end; kc += 2 * CD_BK) {     // pairs of chunks
        chunk(kc, B0{}, std::true_type{});
        chunk(kc + CD_BK, B1{}, std::true_type{});
      }
      if (kc < k_end) chunk(kc, B0{}, std::true_type{});   // an odd last one
    } else
    for (; kc < k_end; kc += 2 * CD_BK) {
      chunk(kc, B0{}, std::false_type{});
      if (kc + CD_BK < k_end) chunk(kc + CD_BK, B1{}, std::false_type{});
    }
  }

  float* dst = out + (size_t)blockIdx.y * M * ldo;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int col = q * 32 + li;
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * kg;         // row of the gene tile
        const int m = PAIR ? m_w + 2 * i + t : m_w + 32 * t + i;
        if (m < M) dst[(size_t)m * ldo + col] = acc[t][q][r];
      }
    }
