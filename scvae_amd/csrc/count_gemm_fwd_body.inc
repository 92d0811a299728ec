// Body of count_gemm_fwd_kernel / _rows_kernel: included once per kernel, which sets IDX (and, where IDX is false, a null
// index pointer) in front of it -- see there.  Not a translation unit of its own.
  extern __shared__ __attribute__((aligned(16))) unsigned char cf_smem[];
  constexpr int NCOL = 64 * NQ;                         // columns staged per term
  constexpr int B_BYTES = 3 * NCOL * CG_ROW;
  unsigned char* Ahi = cf_smem;                         // [2][256][80]
  unsigned char* Alo = Ahi + 2 * CF_A_BYTES;            // [2][256][80]
  unsigned char* Bsm = Alo + 2 * CF_A_BYTES;            // [2][3][NCOL][80]
  int* lo_flag = reinterpret_cast<int*>(Bsm + 2 * B_BYTES);   // [2][8]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, kg = lane >> 5;
  const int rg = w & 3, q0 = (w >> 2) * NQ;
  const int m0 = blockIdx.x * CF_BM;
  const int k_begin = blockIdx.y * k_chunk;
  const int k_end = min(K, k_begin + k_chunk);

  f32x16 acc[2][NQ];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][q][i] = 0.f;

  // zero both lo planes once (a wave only ever rewrites its own rows)
  for (int i = tid; i < 2 * CF_A_BYTES / 16; i += 512)
    reinterpret_cast<u32x4*>(Alo)[i] = u32x4{0u, 0u, 0u, 0u};

  // ---- staging: 16-byte pieces of the [256, 32] tile; fp32: 8 per row, thread -> 4 pieces (row
  // (tid >> 3) + 64 i, floats 4 (tid & 7) .. + 3); uint16: 4 per row, thread -> 2 pieces (row
  // (tid >> 2) + 128 i, counts 8 (tid & 3) .. + 7) ----
  constexpr int EPP = 16 / (int)sizeof(XT);             // elements per piece
  constexpr int PPR = CG_BK / EPP;                      // pieces per row
  constexpr int RPP = 512 / PPR;                        // rows per pass
  constexpr int PCS = CF_BM / RPP;                      // pieces per thread
  const int part = tid & (PPR - 1);
  const XT* xsrc[PCS];
#pragma unroll
  for (int i = 0; i < PCS; ++i) {
    const int m = min(m0 + tid / PPR + RPP * i, M - 1);
    const size_t xr = IDX ? (size_t)xrows[m] : (size_t)m;
    xsrc[i] = X + xr * ldx + EPP * part;
  }
  const int a_off = (tid / PPR) * CG_ROW + part * (2 * EPP);   // + i * RPP rows
  // two chunks of staging registers: chunk c + 2 is requested while chunk c is multiplied and
  // chunk c + 1 (requested one iteration earlier) is converted and parked -- a full iteration
  // plus the MFMA phase of latency tolerance with a single workgroup per CU
  f32x4u raw[2][PCS];
  u32x4 breg[2][3];
  auto load_tiles = [&](int kc, int slot) {
#pragma unroll
    for (int i = 0; i < PCS; ++i) {
      const f32x4u* src = reinterpret_cast<const f32x4u*>(xsrc[i] + kc);
      if constexpr ((SCVAE_CG_NT & 1) != 0) raw[slot][i] = __builtin_nontemporal_load(src);
      else raw[slot][i] = *src;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int p = tid + 512 * i;                      // (term, column, quarter)
      const int row = p >> 2, prt = p & 3;              // row = term * 128 + column
      // (columns beyond N: the last live column's piece again, as in count_gemm_dw_kernel)
      const int col = row & (CG_NP - 1), rowl = col < N ? row : row - col + (N - 1);
      if (col < NCOL)
        breg[slot][i] = *reinterpret_cast<const u32x4*>(T + cg_piece<CG_BK>(kc, rowl, prt));
    }
  };
  bool dirty0 = false, dirty1 = false;                  // this wave's lo rows of buffer b are set
  auto store_tiles = [&](int buf, int slot) {
    unsigned low = 0u;
    // the piece's counts as fp32 bit patterns (uint16: two per loaded dword)
    auto bits_of = [&](int i, unsigned* u) {
      if constexpr (sizeof(XT) == 4) {
        u[0] = __float_as_uint(raw[slot][i].x); u[1] = __float_as_uint(raw[slot][i].y);
        u[2] = __float_as_uint(raw[slot][i].z); u[3] = __float_as_uint(raw[slot][i].w);
      } else {
        const unsigned w[4] = {__float_as_uint(raw[slot][i].x), __float_as_uint(raw[slot][i].y),
                               __float_as_uint(raw[slot][i].z), __float_as_uint(raw[slot][i].w)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          u[2 * j] = __float_as_uint((float)(w[j] & 0xFFFFu));
          u[2 * j + 1] = __float_as_uint((float)(w[j] >> 16));
        }
      }
    };
#pragma unroll
    for (int i = 0; i < PCS; ++i) {
      unsigned u[EPP], h[EPP / 2];
      bits_of(i, u);
#pragma unroll
      for (int j = 0; j < EPP / 2; ++j) {
        low |= u[2 * j] | u[2 * j + 1];
        h[j] = __builtin_amdgcn_perm(u[2 * j + 1], u[2 * j], 0x07060302u);     // upper halves
      }
      unsigned char* dst = Ahi + buf * CF_A_BYTES + a_off + i * RPP * CG_ROW;
      if constexpr (EPP == 4) *reinterpret_cast<uint2*>(dst) = uint2{h[0], h[1]};
      else *reinterpret_cast<u32x4*>(dst) = u32x4{h[0], h[1], h[2], h[3]};
    }
    const bool need = __builtin_amdgcn_readfirstlane(__any((int)((low & 0xFFFFu) != 0u)));
    if (need || (buf ? dirty1 : dirty0)) {
#pragma unroll
      for (int i = 0; i < PCS; ++i) {
        unsigned u[EPP], l[EPP / 2];
        bits_of(i, u);
#pragma unroll
        for (int j = 0; j < EPP / 2; ++j) {
          const float l0 = __uint_as_float(u[2 * j]) - __uint_as_float(u[2 * j] & 0xFFFF0000u);
          const float l1 = __uint_as_float(u[2 * j + 1]) - __uint_as_float(u[2 * j + 1] & 0xFFFF0000u);
          l[j] = __builtin_amdgcn_perm(__float_as_uint(l1), __float_as_uint(l0), 0x07060302u);
        }
        unsigned char* dst = Alo + buf * CF_A_BYTES + a_off + i * RPP * CG_ROW;
        if constexpr (EPP == 4) *reinterpret_cast<uint2*>(dst) = uint2{l[0], l[1]};
        else *reinterpret_cast<u32x4*>(dst) = u32x4{l[0], l[1], l[2], l[3]};
      }
    }
    if (buf) dirty1 = need; else dirty0 = need;
    if (lane == 0) lo_flag[buf * 8 + w] = need ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int p = tid + 512 * i;
      const int row = p >> 2, prt = p & 3;
      const int term = row >> 7, col = row & (CG_NP - 1);
      if (col < NCOL)
        *reinterpret_cast<u32x4*>(Bsm + buf * B_BYTES + (term * NCOL + col) * CG_ROW + prt * 16) =
            breg[slot][i];
    }
  };

  __syncthreads();                                      // lo planes zeroed
  if (k_begin < k_end) {
    load_tiles(k_begin, 0);
    if (k_begin + CG_BK < k_end) load_tiles(k_begin + CG_BK, 1);
    store_tiles(0, 0);
  }
  __syncthreads();

  const int a_frag = (64 * rg + li) * CG_ROW + 32 * kg;      // + 32 rows * t, + 16 s
  const int b_frag = (q0 * 32 + li) * CG_ROW + 32 * kg;      // + term * NCOL rows, + 32 rows * q
  // one chunk; BUF (compile time: the staging registers are indexed statically) = LDS buffer and
  // staging slot of chunk j = j & 1
  // STEADY (compile time): chunks j + 1 and j + 2 exist, so the request and the hand-over are
  // unconditional -- with conditions the compiler cannot pair them up and waits for every
  // outstanding load at the loop header, which cancels the second chunk of latency tolerance
  auto chunk = [&](int kc, auto buf_tag, auto steady_tag) {
    constexpr int BUF = decltype(buf_tag)::value;
    constexpr bool STEADY = decltype(steady_tag)::value;
    // chunk j + 2 -> staging slot BUF (chunk j left it for LDS before this iteration)
    if (STEADY || kc + 2 * CG_BK < k_end) load_tiles(kc + 2 * CG_BK, BUF);
    __builtin_amdgcn_sched_barrier(0);

    const bool need_lo =
        __builtin_amdgcn_readfirstlane(__any(lo_flag[BUF * 8 + (lane & 7)]));
    const unsigned char* ah = Ahi + BUF * CF_A_BYTES + a_frag;
    const unsigned char* al = Alo + BUF * CF_A_BYTES + a_frag;
    const unsigned char* bb = Bsm + BUF * B_BYTES + b_frag;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 fh[2], fl[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
        fh[t] = as_bf16x8(*reinterpret_cast<const u32x4*>(ah + t * 32 * CG_ROW + 16 * s));
      if (need_lo) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
          fl[t] = as_bf16x8(*reinterpret_cast<const u32x4*>(al + t * 32 * CG_ROW + 16 * s));
      }
#pragma unroll
      for (int term = 2; term >= 0; --term) {           // smallest term first
        bf16x8 fb[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          fb[q] = as_bf16x8(*reinterpret_cast<const u32x4*>(
              bb + (term * NCOL + q * 32) * CG_ROW + 16 * s));
        if (need_lo) {
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl[0], fb[q], acc[0][q], 0, 0, 0);
            acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl[1], fb[q], acc[1][q], 0, 0, 0);
          }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          acc[0][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh[0], fb[q], acc[0][q], 0, 0, 0);
          acc[1][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh[1], fb[q], acc[1][q], 0, 0, 0);
        }
      }
    }
    // chunk j + 1 (requested one iteration ago, staging slot BUF ^ 1) -> LDS buffer BUF ^ 1
    // (scheduling fence: the conversion and its wait for the loads stay below the MFMAs)
    __builtin_amdgcn_sched_barrier(0);
    if (STEADY || kc + CG_BK < k_end) store_tiles(BUF ^ 1, BUF ^ 1);
    lds_barrier();       // (LDS only: the requests for chunk j + 2 stay in flight across it)
  };
  {
    using B0 = std::integral_constant<int, 0>;
    using B1 = std::integral_constant<int, 1>;
    int kc = k_begin;
    for (; kc + 3 * CG_BK < k_end; kc += 2 * CG_BK) {   // chunks j, j + 1 with j + 3 in range
      chunk(kc, B0{}, std::true_type{});
      chunk(kc + CG_BK, B1{}, std::true_type{});
    }
    for (; kc < k_end; kc += 2 * CG_BK) {               // the last one to three chunks
      chunk(kc, B0{}, std::false_type{});
      if (kc + CG_BK < k_end) chunk(kc + CG_BK, B1{}, std::false_type{});
    }
  }

  float* dst = direct ? out : out + (size_t)blockIdx.y * M * ldo;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int col = (q0 + q) * 32 + li;
      if (col >= N) continue;
      const float bv = (direct && bias != nullptr) ? bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + 64 * rg + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * kg;
        if (m < M) {
          float v = acc[t][q][r] + bv;
          if (direct && act == ACT_RELU) v = relu_keep_nan(v);
          dst[(size_t)m * ldo + col] = v;
        }
      }
    }
