// Body of decoder_head3_kernel / _rows_kernel: included once per kernel, which sets IDX (and, where IDX is false, a null
// index pointer) in front of it -- see there.  Not a translation unit of its own.
  static_assert(TRAIN || !DROP, "dropout is a training-time operation");
  static_assert((CP > 0) == (KIND == LK_CPOISSON), "CP selects the passes of LK_CPOISSON");
  static_assert(CP == 0 || ((CP == 3) == TRAIN && !DROP), "CP 1 / 2 forward, CP 3 training");
  using Traits = LikelihoodTraits<KIND>;
  constexpr int P = Traits::P;
  constexpr int BN = d3_bn(P), ROWB = d3_rowb(P);
  constexpr int GPLANE = D3_BM * ROWB;      // bytes of one [64 rows][BN genes] plane of G
  constexpr int NSB = BN / 32;              // 16-gene blocks of a wave in phase A (2 / 1)
  constexpr int NE = 4 * NSB;               // elements of a lane
  constexpr bool KSPLIT = P >= 3;           // GEMM2 splits the tile's rows between wave pairs
  constexpr int KS2 = KSPLIT ? 2 : 4;       // 16-row k-steps of GEMM2 per wave
  constexpr int KS3 = BN / 16;              // 16-gene k-steps of GEMM3 per head
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HP1 = d3_hp1(H);
  const int WPLANE = HP1 * ROWB;                    // bytes of one [HP1][BN] plane of W
  char* Wl = smem;                                  // [P][3][HP1][BN + 8] bf16
  char* Gl = smem + (size_t)P * 3 * WPLANE;         // [P][3][64][BN + 8] bf16
  float* llbuf = reinterpret_cast<float*>(Gl + (size_t)P * 3 * GPLANE);   // [2][64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, i16 = lane & 15, li = lane & 31, kh = lane >> 5;
  const int c0 = blockIdx.x * BN;

  // ---- LDS: zero everything (padding and over-read regions must hold finite values), then the
  //      strip's weights and biases, cut into planes.  ALL of a thread's weight loads -- its rows
  //      of every head -- are requested first, from clamped, always valid addresses, and land
  //      under the zero fill: as a plain loop this fill was one dependent global-memory round trip
  //      per weight row, 12 us per workgroup -- a third of the kernel at a 100-cell minibatch ----
  constexpr int HSTEP = D3_THREADS / BN;
  constexpr int NV = (126 + HSTEP) / HSTEP;            // rows 0 .. H <= 126 of a thread
  {
    const int g = tid & (BN - 1), h0 = tid / BN;
    const bool col_ok = c0 + g < F;
    const int gc = min(c0 + g, F - 1);
    float v[P][NV];
    // (the plain [H, F] layout, or -- the class logits of the P_K head -- genes gene_stride apart
    //  in rows of row_pitch elements)
    const size_t gs = hp.gene_stride ? hp.gene_stride : 1;
    const size_t rp = hp.row_pitch ? hp.row_pitch : F;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float* wj = hp.W[j] + gc * gs;
      const float* bj = hp.b[j] + gc * gs;
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int h = h0 + u * HSTEP;
        const float* src = h < H ? wj + (size_t)h * rp : bj;
        v[j][u] = *src;
      }
    }
    {
      const int n16 = (int)(((size_t)P * 3 * WPLANE + (size_t)P * 3 * GPLANE + 2 * D3_BM * 4) / 16);
      u32x4* z = reinterpret_cast<u32x4*>(smem);
      for (int i = tid; i < n16; i += D3_THREADS) z[i] = u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int h = h0 + u * HSTEP;
        if (h <= H) {
          unsigned b1, b2, b3;
          split3_rn(col_ok ? v[j][u] : 0.f, b1, b2, b3);
          char* dst = Wl + (size_t)(j * 3) * WPLANE + h * ROWB + 2 * g;
          *reinterpret_cast<uint16_t*>(dst) = (uint16_t)(b1 >> 16);
          *reinterpret_cast<uint16_t*>(dst + WPLANE) = (uint16_t)(b2 >> 16);
          *reinterpret_cast<uint16_t*>(dst + 2 * WPLANE) = (uint16_t)(b3 >> 16);
        }
      }
  }
  __syncthreads();

  // ---- wave roles ----
  const int gp = w & 1, rq = w >> 1;        // phase A: genes 16 NSB gp .., rows 16 rq .. of the tile
  const int ht = w & 3, hi2 = w >> 2;       // phase B: h tile; GEMM3: row tile hi2; GEMM2: gene
                                            // tile hi2 (all 64 rows), or -- three heads -- rows
                                            // 32 hi2 .. (all 32 genes)
  const int n_ht3 = (H + 31) / 32, n_ht2 = (H + 1 + 31) / 32;
  const int nb16 = Rpad / 16;               // 16-row blocks of the planes of d

  // per-lane byte offsets
  const int gbase = 16 * NSB * gp;
  const int trw = (8 * q + (i16 >> 2)) * ROWB + 2 * (gbase + 4 * (i16 & 3));        // W, GEMM1
  const int gst = (16 * rq + i16) * ROWB + 2 * (gbase + 4 * q);                     // G store
  const int g3a = (32 * hi2 + li) * ROWB + 16 * kh;                                 // G, GEMM3 A
  const int g3b = (32 * ht + li) * ROWB + 16 * kh;                                  // W, GEMM3 B
  const int g2b = ((KSPLIT ? 32 * hi2 : 0) + 8 * (q >> 1) + (i16 >> 2)) * ROWB +
                  2 * ((KSPLIT ? 0 : 32 * hi2) + 16 * (q & 1) + 4 * (i16 & 3));     // G, GEMM2 B

  f32x16 accW[P];                           // dW tile (h tile ht [, gene tile hi2]) of every head
#pragma unroll
  for (int j = 0; j < P; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) accW[j][i] = 0.f;

  const int n_tiles = (R + D3_BM - 1) / D3_BM;
  const size_t dplane = (size_t)Rpad * D3_KP;

  // targets / upstream of a tile, in flight from the previous phase B (returned by value: an
  // array written through a reference capture ends up in scratch memory)
  struct TileIn { f32x4m t[NSB]; float up0; float cpn, cpl, cps; };
  // (IDX) row of the resident matrix behind this lane's row of the tile at m0 / of the tile the
  // next load_t call reads
  size_t tidx = 0;
  auto load_i = [&](int m0) -> size_t {
    const int rc = min(m0 + 16 * rq + i16, R - 1);
    return (size_t)trows[R == B ? rc : rc % B];
  };
  if (IDX) tidx = load_i(0);
  auto load_t = [&](int m0) {
    TileIn in;
    const int row = m0 + 16 * rq + i16;
    const bool rok = row < R;
    in.up0 = (TRAIN && rok) ? gw[row] : 0.f;
    const int rc = rok ? row : R - 1;
    const int cell = R == B ? rc : rc % B;
    in.cpn = in.cpl = in.cps = 0.f;
    if (CP > 0) in.cpn = cp.count_sum[cell];
    if (CP >= 2) in.cpl = cp.lse[rc];
    if (CP == 3) in.cps = cp.S[rc];
    const size_t trow = (IDX ? tidx : (size_t)cell) * tg.ld;
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb) {
      const int c = c0 + gbase + 16 * sb + 4 * q;
      f32x4m v = {0.f, 0.f, 0.f, 0.f};
      if (U16) {        // pitch % 8 == 0, padding columns zero: one 8-byte load
        const uint16_t* tp = static_cast<const uint16_t*>(tg.p) + trow + c;
        const u32x2 u = *reinterpret_cast<const u32x2*>(tp);
        v.x = __uint_as_float(u.x); v.y = __uint_as_float(u.y);
      } else {
        const float* tp = static_cast<const float*>(tg.p) + trow + c;
        if (c + 3 < F) {
          const f32x4u u = *reinterpret_cast<const f32x4u*>(tp);
          v.x = u.x; v.y = u.y; v.z = u.z; v.w = u.w;
        } else {
          v.x = (c < F) ? tp[0] : 0.f;
          v.y = (c + 1 < F) ? tp[1] : 0.f;
          v.z = (c + 2 < F) ? tp[2] : 0.f;
        }
      }
      in.t[sb] = v;
    }
    return in;
  };
  TileIn nxt = load_t(0);
  if (IDX) tidx = load_i(min(D3_BM, Rpad - D3_BM));
  // d fragments of GEMM1 (B[k = h][n = row]): 3 planes per k-step, one contiguous KiB each,
  // requested one k-step ahead of the MFMAs that use them (k-step 0 of a tile during the
  // previous phase B)
  const size_t dset = DROP ? d3_set_elems(Rpad) : 0;     // plane set of head j: + j * dset
  auto load_d1 = [&](int m0, int ks, bf16x8 (&dst)[3], int j = 0) {
    const uint16_t* dbase = dA + j * dset + ((size_t)(m0 / 16 + rq) * 4 + ks) * 512 + lane * 8;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) dst[pl] = global_b128(dbase + pl * dplane);
  };
  // (DROP: contraction steps st = k-step * P + head; steps 0 and 1 of a tile travel under the
  //  previous phase B)
  constexpr int NST1 = KS1 * P;
  bf16x8 bfr0[3], bfr1[3];
  load_d1(0, 0, bfr0);
  if (DROP) { if (NST1 > 1) load_d1(0, 1 / P, bfr1, 1 % P); }
  else if (D3_AHEAD > 1 && KS1 > 1) load_d1(0, 1, bfr1);

  for (int tile = 0; tile < n_tiles; ++tile) {
    const int m0 = tile * D3_BM;
    const TileIn cur = nxt;
    const float up = cur.up0;
    // row sums of the tile (forward only: alternating with the unused G area)
    // (not at the start of the G area: GEMM1's last k-step reads up to 16 rows past the last
    //  weight plane -- times zero columns of d, but a row sum's low half can be a bf16 NaN)
    float* lb = (!TRAIN && (tile & 1)) ? reinterpret_cast<float*>(Gl + 4096) : llbuf;
    float* lb2 = reinterpret_cast<float*>(Gl + ((tile & 1) ? 12288 : 8192));   // (CP 1 / 2)
    // =================== phase A: GEMM1 (transposed) + likelihood + G -> LDS ===================
    f32x4m acc1[P][NSB];
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb) acc1[j][sb] = f32x4m{0.f, 0.f, 0.f, 0.f};
    if constexpr (DROP) {
      // one head per step: its W fragments one step ahead, its d fragments two
      bf16x8 afr[2][NSB][3], bfr[3][3];
      auto load_wj = [&](int st, bf16x8 (&dst)[NSB][3]) {
        const int ks = st / P, j = st % P;
#pragma unroll
        for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            dst[sb][pl] = lds_tr8<ROWB>(Wl + (size_t)(j * 3 + pl) * WPLANE + trw + 32 * sb +
                                        32 * ks * ROWB);
      };
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) { bfr[0][pl] = bfr0[pl]; bfr[1][pl] = bfr1[pl]; }
      load_wj(0, afr[0]);
#pragma unroll
      for (int st = 0; st < NST1; ++st) {
        if (st + 2 < NST1) {
          load_d1(m0, (st + 2) / P, bfr[(st + 2) % 3], (st + 2) % P);
          d3_pin_loads();
        }
        if (st + 1 < NST1) load_wj(st + 1, afr[(st + 1) & 1]);
        const int j = st % P;
#pragma unroll
        for (int a = 2; a >= 0; --a)
#pragma unroll
          for (int b = 2; b >= 0; --b)
#pragma unroll
            for (int sb = 0; sb < NSB; ++sb)
              acc1[j][sb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  afr[st & 1][sb][a], bfr[st % 3][b], acc1[j][sb], 0, 0, 0);
      }
    } else {
      // W fragments (transpose reads) and d fragments one k-step ahead of the MFMAs
      bf16x8 afr[2][P][NSB][3], bfr[D3_NB][3];
      auto load_w = [&](int ks, bf16x8 (&dst)[P][NSB][3]) {
#pragma unroll
        for (int j = 0; j < P; ++j)
#pragma unroll
          for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
              dst[j][sb][pl] = lds_tr8<ROWB>(Wl + (size_t)(j * 3 + pl) * WPLANE + trw + 32 * sb +
                                             32 * ks * ROWB);
      };
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) bfr[0][pl] = bfr0[pl];
      if (D3_AHEAD > 1 && KS1 > 1) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) bfr[1][pl] = bfr1[pl];
      }
      load_w(0, afr[0]);
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks) {
        if (ks + D3_AHEAD < KS1) {
          load_d1(m0, ks + D3_AHEAD, bfr[(ks + D3_AHEAD) % D3_NB]);
          d3_pin_loads();
        }
        if (ks + 1 < KS1) load_w(ks + 1, afr[(ks + 1) & 1]);
        if (!TRAIN && ks == KS1 - 1) {
          // (forward only) the next tile's targets and first d fragments: under this k-step
          // and the likelihood.  Unconditional -- the last tile requests itself again: under
          // a branch the compiler waits for the loads where the arms meet
          const int mn = min(m0 + D3_BM, Rpad - D3_BM);
          nxt = load_t(mn);
          if (IDX) tidx = load_i(min(mn + D3_BM, Rpad - D3_BM));
          load_d1(mn, 0, bfr0);
          if (D3_AHEAD > 1 && KS1 > 1) load_d1(mn, 1, bfr1);
          d3_pin_loads();
        }
        // small terms first; the accumulators (head x gene block) are independent chains
#pragma unroll
        for (int a = 2; a >= 0; --a)
#pragma unroll
          for (int b = 2; b >= 0; --b)
#pragma unroll
            for (int j = 0; j < P; ++j)
#pragma unroll
              for (int sb = 0; sb < NSB; ++sb)
                acc1[j][sb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    afr[ks & 1][j][sb][a], bfr[ks % D3_NB][b], acc1[j][sb], 0, 0, 0);
      }
    }
    // ---- likelihood of this lane's NSB x 4 elements: row 16 rq + i16, genes
    //      16 NSB gp + 16 sb + 4 q + e ----
    float G[P][NE], tval[NE];
    float lsum = 0.f, lsum2 = 0.f;
    unsigned nz = 0;
    if constexpr (CP > 0) {
      // ---- constrained Poisson: this lane's NE logits of ONE row ----
      const float cpn = cur.cpn, cpl = cur.cpl, cps = cur.cps;
      float av[NE];
      bool okv[NE];
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb) {
        if (U16) {
          const unsigned v0 = __float_as_uint(cur.t[sb][0]), v1 = __float_as_uint(cur.t[sb][1]);
          tval[4 * sb] = (float)(v0 & 0xFFFFu); tval[4 * sb + 1] = (float)(v0 >> 16);
          tval[4 * sb + 2] = (float)(v1 & 0xFFFFu); tval[4 * sb + 3] = (float)(v1 >> 16);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) tval[4 * sb + e] = cur.t[sb][e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          av[4 * sb + e] = acc1[0][sb][e];
          okv[4 * sb + e] = c0 + gbase + 16 * sb + 4 * q + e < F;
        }
      }
      if (CP == 1) {
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < NE; ++i) mx = fmaxf(mx, okv[i] ? av[i] : -INFINITY);
        float se = 0.f;
#pragma unroll
        for (int i = 0; i < NE; ++i) se += okv[i] ? __expf(av[i] - mx) : 0.f;
        float m2 = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
        m2 = fmaxf(m2, __shfl_xor(m2, 32, WAVE));
        se = mx > -INFINITY ? se * __expf(mx - m2) : 0.f;
        lsum = m2;
        lsum2 = se;     // (summed over the wave's gene groups below)
      } else {
        const float log_n = __logf(fmaxf(cpn, F32_TINY));
#pragma unroll
        for (int i = 0; i < NE; ++i) {
          const float tv = tval[i];
          const float log_lam = av[i] - cpl;
          const float lam = __expf(log_lam);
          const bool gate = lam >= F32_TINY;
          const float own = gate ? tv - cpn * lam : 0.f;
          if (CP == 2) {
            const float lam_c = gate ? lam : F32_TINY;
            const float log_rate = (gate ? log_lam : LOG_F32_TINY) + log_n;
            lsum += okv[i] ? (tv > 0.f ? tv * log_rate : 0.f) - lam_c * cpn : 0.f;
            lsum2 += okv[i] ? own : 0.f;
            nz |= (okv[i] && tv > 0.f) ? (1u << i) : 0u;
          } else {
            G[0][i] = up * (own - lam * cps);
          }
        }
      }
    } else {
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb) {
      if (U16) {
        const unsigned v0 = __float_as_uint(cur.t[sb][0]), v1 = __float_as_uint(cur.t[sb][1]);
        tval[4 * sb] = (float)(v0 & 0xFFFFu); tval[4 * sb + 1] = (float)(v0 >> 16);
        tval[4 * sb + 2] = (float)(v1 & 0xFFFFu); tval[4 * sb + 3] = (float)(v1 >> 16);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) tval[4 * sb + e] = cur.t[sb][e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float a[P], g[P], lp, r, rgate;
#pragma unroll
        for (int j = 0; j < P; ++j) a[j] = acc1[j][sb][e];
        // (tg.shift > 0 -- the count part of the piecewise categorical likelihood: the
        //  distribution sees t - shift where t >= shift, nothing elsewhere; 0: every element)
        const bool live = tval[4 * sb + e] >= tg.shift;
        tval[4 * sb + e] = live ? tval[4 * sb + e] - tg.shift : 0.f;
        lik_dense<KIND, TRAIN>(tval[4 * sb + e], a, lp, g, r, rgate);
        const bool ok = live && c0 + gbase + 16 * sb + 4 * q + e < F;
        lsum += ok ? lp : 0.f;
        if (TRAIN) {
#pragma unroll
          for (int j = 0; j < P; ++j) G[j][4 * sb + e] = live ? up * g[j] : 0.f;
        }
        nz |= (ok && tval[4 * sb + e] > 0.f) ? (1u << (4 * sb + e)) : 0u;
      }
    }
    }
    // ---- t > 0: + lgamma(r+t) - lgamma(r) [- lgamma(1+t)], and the digamma term of dlog r:
    //      a per-lane walk over the lane's non-zero elements ----
    if (Traits::HAS_R || (inline_lgamma && (CP == 0 || CP == 2))) {
      float lr[NE];
      if (Traits::HAS_R) {
#pragma unroll
        for (int i = 0; i < NE; ++i) lr[i] = acc1[P - 1][i >> 2][i & 3];
      }
      while (__builtin_amdgcn_ballot_w64(nz != 0) != 0) {
        const bool on = nz != 0;
        const int idx = on ? __builtin_ctz(nz) : 0;
        nz &= nz - 1;
        const IndexMasks3 km = index_masks3(idx);
        const float tt = select_n(tval, km);
        float corr = 0.f;
        if (Traits::HAS_R) {
          const float lrv = select_n(lr, km);
          const float r = __expf(fminf(fmaxf(lrv, -10.f), 10.f));
          const float rgate = (lrv >= -10.f && lrv <= 10.f) ? 1.f : 0.f;
          const bool small = !on || (tt <= 8.f && tt == __builtin_rintf(tt));
          float A, D;
          if (__builtin_amdgcn_ballot_w64(!small) == 0)
            lgamma_digamma_diff_small_wave<TRAIN>(r, on ? tt : 0.f, A, D);
          else
            lgamma_digamma_diff_general<TRAIN>(r, on ? tt : 1.f, A, D);
          corr = A;
          // (zero-inflated: at t > 0 the gradient of the base distribution passes unscaled,
          //  zero_inflated.py:194-199 -- the same insertion)
          if (TRAIN) {
            const float delta = on ? up * rgate * r * D : 0.f;
#pragma unroll
            for (int e = 0; e < NE; ++e) G[P - 1][e] += (idx == e) ? delta : 0.f;
          }
        }
        if (inline_lgamma) corr -= lgamma1p(tt);
        lsum += on ? corr : 0.f;
      }
    }
    // ---- row sums over this wave's genes -> llbuf[gp][row] ----
    if (CP == 1) {
      // (maximum already common to the wave's gene groups; the sums of exponentials refer to it)
      float se = lsum2;
      se += __shfl_xor(se, 16, WAVE);
      se += __shfl_xor(se, 32, WAVE);
      if (q == 0) {
        lb[gp * D3_BM + 16 * rq + i16] = lsum;
        lb2[gp * D3_BM + 16 * rq + i16] = se;
      }
    } else if (CP != 3) {
      float sm = lsum;
      sm += __shfl_xor(sm, 16, WAVE);
      sm += __shfl_xor(sm, 32, WAVE);
      if (q == 0) lb[gp * D3_BM + 16 * rq + i16] = sm;
      if (CP == 2) {
        float s2 = lsum2;
        s2 += __shfl_xor(s2, 16, WAVE);
        s2 += __shfl_xor(s2, 32, WAVE);
        if (q == 0) lb2[gp * D3_BM + 16 * rq + i16] = s2;
      }
    }
    // ---- G_j -> three bf16 planes, row-major [row][gene], 8 bytes (4 genes) per store ----
    if (TRAIN) {
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb) {
        unsigned p1[2], p2[2], p3[2];
#pragma unroll
        for (int e = 0; e < 2; ++e)
          split3_rn_pair(G[j][4 * sb + 2 * e], G[j][4 * sb + 2 * e + 1], p1[e], p2[e], p3[e]);
        char* dst = Gl + (size_t)(j * 3) * GPLANE + gst + 32 * sb;
        *reinterpret_cast<u32x2*>(dst) = u32x2{p1[0], p1[1]};
        *reinterpret_cast<u32x2*>(dst + GPLANE) = u32x2{p2[0], p2[1]};
        *reinterpret_cast<u32x2*>(dst + 2 * GPLANE) = u32x2{p3[0], p3[1]};
      }
    }
    lds_barrier();

    // =================== phase B: GEMM3 (LDS operands), then GEMM2 ===================
    // per-row log-likelihood of the strip: the two gene blocks summed in a fixed order
    if (CP == 1) {
      // the two gene halves: common maximum, sums of exponentials rescaled to it
      if (tid < D3_BM && m0 + tid < R) {
        const float ma = lb[tid], mb = lb[D3_BM + tid];
        const float m = fmaxf(ma, mb);
        const float se = (ma > -INFINITY ? lb2[tid] * __expf(ma - m) : 0.f) +
                         (mb > -INFINITY ? lb2[D3_BM + tid] * __expf(mb - m) : 0.f);
        ll_part[(size_t)blockIdx.x * R + m0 + tid] = m;
        cp.out2[(size_t)blockIdx.x * R + m0 + tid] = se;
      }
    } else if (CP != 3) {
      if (tid < D3_BM && m0 + tid < R) {
        ll_part[(size_t)blockIdx.x * R + m0 + tid] = lb[tid] + lb[D3_BM + tid];
        if (CP == 2) cp.out2[(size_t)blockIdx.x * R + m0 + tid] = lb2[tid] + lb2[D3_BM + tid];
      }
    }
    if (!TRAIN) continue;   // (the next tile writes the other row-sum buffer: no second barrier)
    // GEMM2's d fragments (A[i = h][k = row]) come from L2 one k-step ahead; k-step 0 is
    // requested here and lands under GEMM3
    auto load_a2 = [&](int ks, bf16x8 (&dst)[3], int j = 0) {
      const uint16_t* tb = dT + j * dset +
          ((size_t)ht * nb16 + m0 / 16 + (KSPLIT ? 2 * hi2 : 0) + ks) * 512 + lane * 8;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) dst[pl] = global_b128(tb + pl * dplane);
    };
    constexpr int NST2 = KS2 * P;              // (DROP: steps (k-step, head), two ahead)
    bf16x8 a2[DROP ? 3 : D3_NB][3];
    if (ht < n_ht2) {
      load_a2(0, a2[0]);
      if (DROP) { if (NST2 > 1) load_a2(1 / P, a2[1], 1 % P); }
      else if (D3_AHEAD > 1 && KS2 > 1) load_a2(1, a2[1]);
    }
    // (DROP) the heads' mask words of this lane's row and h tile, shifted to its four-h groups
    uint32_t mw[P];
    if (DROP) {
#pragma unroll
      for (int j = 0; j < P; ++j)
        mw[j] = ht < n_ht3
                    ? drop_bits[((size_t)j * Rpad + m0 + 32 * hi2 + li) * 4 + ht] >> (4 * kh)
                    : 0u;
    }
    // next tile's targets
    if (tile + 1 < n_tiles) nxt = load_t(m0 + D3_BM);
    if (IDX) tidx = load_i(min(m0 + 2 * D3_BM, Rpad - D3_BM));
    if (ht < n_ht3) {
      // ---- GEMM3: dd[row, h] = sum_j sum_gene G_j[row, gene] W_j[h, gene] ----
      f32x16 acc3, accS;
#pragma unroll
      for (int i = 0; i < 16; ++i) { acc3[i] = 0.f; accS[i] = 0.f; }
      bf16x8 af[2][3], bf[2][3];
      auto load_3 = [&](int st, bf16x8 (&a)[3], bf16x8 (&b)[3]) {   // step = head * KS3 + k-step
        const int j = st / KS3, ks = st % KS3;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
          a[pl] = lds_b128(Gl + (size_t)(j * 3 + pl) * GPLANE + g3a + 32 * ks);
          b[pl] = lds_b128(Wl + (size_t)(j * 3 + pl) * WPLANE + g3b + 32 * ks);
        }
      };
      load_3(0, af[0], bf[0]);
#pragma unroll
      for (int st = 0; st < KS3 * P; ++st) {
        if (st + 1 < KS3 * P) load_3(st + 1, af[(st + 1) & 1], bf[(st + 1) & 1]);
#pragma unroll
        for (int a = 2; a >= 0; --a)
#pragma unroll
          for (int b = 2; b >= 0; --b)
            acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[st & 1][b], af[st & 1][a], acc3, 0,
                                                           0, 0);
        if (DROP && st % KS3 == KS3 - 1) {
          // head st / KS3 is complete: through its mask (element i = 4 c + e <-> h = 32 ht +
          // 8 c + 4 kh + e), times 1 / keep, into the sum over the heads
          const uint32_t m = mw[st / KS3];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            accS[i] += ((m >> (8 * (i >> 2) + (i & 3))) & 1u) ? acc3[i] * inv_keep : 0.f;
            acc3[i] = 0.f;
          }
        }
      }
      if (DROP) acc3 = accS;
      // (computed transposed, dd^T[h, row]: a lane holds, for each of four groups, FOUR consecutive
      //  h of one row.  The per-strip partial goes to a slab [strip][H / 4][R][4]: one 16-byte
      //  store per group and lane, 32 consecutive rows of an h quad = 512 contiguous bytes per
      //  half wave -- whole lines, a quarter of the store instructions of an [H][R] slab, which
      //  in turn beat the row-major slab with its 100-float rows in partial lines.
      //  Non-temporal: the slabs are read exactly once, by dd_reduce_q_kernel)
      const int row = m0 + 32 * hi2 + li;
      if (row < R) {
        const int HQ = (H + 3) >> 2;
        f32x4m* dst = reinterpret_cast<f32x4m*>(dd_part) +
                      ((size_t)blockIdx.x * HQ + 8 * ht + kh) * R + row;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (4 * (8 * ht + 2 * c + kh) < H)
            __builtin_nontemporal_store(
                f32x4m{acc3[4 * c], acc3[4 * c + 1], acc3[4 * c + 2], acc3[4 * c + 3]},
                dst + (size_t)2 * c * R);
        }
      }
    }
    // the next tile's d fragments of GEMM1: in flight under GEMM2 and the barrier
    if (tile + 1 < n_tiles) {
      load_d1(m0 + D3_BM, 0, bfr0);
      if (DROP) { if (NST1 > 1) load_d1(m0 + D3_BM, 1 / P, bfr1, 1 % P); }
      else if (D3_AHEAD > 1 && KS1 > 1) load_d1(m0 + D3_BM, 1, bfr1);
    }
    if (ht < n_ht2) {
      // ---- GEMM2: dW_j[h, gene] += sum_row d[row, h] G_j[row, gene] ----
      bf16x8 bf[2][3];
      auto load_2 = [&](int st, bf16x8 (&b)[3]) {                    // step = k-step * P + head
        const int ks = st / P, j = st % P;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          b[pl] = lds_tr8<ROWB>(Gl + (size_t)(j * 3 + pl) * GPLANE + g2b + 16 * ks * ROWB);
      };
      load_2(0, bf[0]);
#pragma unroll
      for (int st = 0; st < KS2 * P; ++st) {
        if (st + 1 < KS2 * P) load_2(st + 1, bf[(st + 1) & 1]);
        if (DROP) {
          if (st + 2 < NST2) {
            load_a2((st + 2) / P, a2[(st + 2) % 3], (st + 2) % P);
            d3_pin_loads();
          }
        } else if (st % P == 0 && st / P + D3_AHEAD < KS2) {
          load_a2(st / P + D3_AHEAD, a2[(st / P + D3_AHEAD) % D3_NB]);
          d3_pin_loads();
        }
        const int ks = st / P, j = st % P;
#pragma unroll
        for (int a = 2; a >= 0; --a)
#pragma unroll
          for (int b = 2; b >= 0; --b)
            accW[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2[DROP ? st % 3 : ks % D3_NB][a],
                                                              bf[st & 1][b], accW[j], 0, 0, 0);
      }
    }
    lds_barrier();
  }

  if (!TRAIN) return;
  // ---- dW / db of the strip ----
  if (KSPLIT) {
    // the two waves of an h tile hold partial sums over the two row halves: waves 4-7 park
    // theirs in LDS (the weights are no longer needed), waves 0-3 add and write
    float* park = reinterpret_cast<float*>(smem) + (size_t)ht * P * 16 * 64;
    if (hi2 == 1 && ht < n_ht2) {
#pragma unroll
      for (int j = 0; j < P; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) park[(j * 16 + i) * 64 + lane] = accW[j][i];
    }
    __syncthreads();
    if (hi2 == 0 && ht < n_ht2) {
#pragma unroll
      for (int j = 0; j < P; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) accW[j][i] += park[(j * 16 + i) * 64 + lane];
    }
  }
  if (ht < n_ht2 && (!KSPLIT || hi2 == 0)) {
    const int c = c0 + (KSPLIT ? 0 : 32 * hi2) + li;
    if (c < F) {
      const size_t gs_out = hp.gene_stride ? hp.gene_stride : 1;
      const size_t rp_out = hp.row_pitch ? hp.row_pitch : F;
#pragma unroll
      for (int j = 0; j < P; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int h = 32 * ht + (i & 3) + 8 * (i >> 2) + 4 * kh;
          if (h < H) hp.dW[j][(size_t)h * rp_out + c * gs_out] = accW[j][i];
          else if (h == H) hp.db[j][c * gs_out] = accW[j][i];
        }
    }
  }
