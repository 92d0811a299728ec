// Body of decoder_head4_kernel / _rows_kernel: included once per kernel, which sets IDX (and, where IDX is false, a null
// index pointer) in front of it -- see there.  Not a translation unit of its own.
  using Traits = LikelihoodTraits<KIND>;
  constexpr int P = Traits::P;
  constexpr int NT = d4_threads(NPW);
  constexpr int BN = BN_ ? BN_ : d3_bn(P), ROWB = 2 * BN + 16;
  constexpr int NT2 = DBP ? KS1 - 1 : KS1;  // 32-wide h tiles of GEMM2
  constexpr int NHT = (NT2 + 3) / 4;        // h tiles of a consumer wave
  static_assert(!DBP || (NPW == 4 && KS1 >= 2), "DBP: four producers");
  constexpr int DF = KS1 < 4 ? KS1 : 4;     // fragment slots of d a producer holds
  constexpr int GPLANE = D4_BM * ROWB;      // bytes of one [32 rows][BN genes] plane of G
  constexpr int GBUF = P * 3 * GPLANE;      // one tile's G: [P][3][32][BN + 8] bf16
  constexpr int NGP = NPW / 2;              // producer waves side by side over the strip's genes
  constexpr int NSB = BN / (16 * NGP);      // 16-gene blocks of a producer wave
  static_assert(NSB >= 1 && NSB * 16 * NGP == BN, "producer waves tile the strip");
  constexpr int NE = 4 * NSB;               // elements of a producer lane
  constexpr int KS3 = BN / 16;              // 16-gene k-steps of GEMM3 per head
  constexpr int NGT = BN / 32;              // 32-gene tiles of GEMM2
  constexpr int LLN = NGP * 4 * D4_BM;      // row-sum partials of a tile: [gene group][q][row]
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HP1 = d3_hp1(H);
  const int WPLANE = HP1 * ROWB;                    // bytes of one [HP1][BN] plane of W
  char* Wl = smem;                                  // [P][3][HP1][BN + 8] bf16
  char* Gl = smem + (size_t)P * 3 * WPLANE;         // [2][P][3][32][BN + 8] bf16
  float* llbuf = reinterpret_cast<float*>(Gl + 2 * GBUF);   // [2][LLN]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, i16 = lane & 15, li = lane & 31, kh = lane >> 5;
  const int c0 = blockIdx.x * BN;
  // (probe build only: ablation flags travel in the upper bits of inline_lgamma -- 1 consumers
  //  idle, 2 producers idle, 4 no non-zero walk, 8 no dd stores; tools/d4_probe.sh, d4_prof.py)
  const int dbg = D4_PROF ? inline_lgamma >> 8 : 0;
  inline_lgamma &= 0xFF;

  // ---- LDS: zero fill, then the strip's weights and biases cut into planes (as above) ----
  constexpr int HSTEP = NT / BN;
  constexpr int NV = (32 * KS1 + HSTEP - 1) / HSTEP;    // rows 0 .. H < 32 KS1 of a thread
  {
    const int g = tid & (BN - 1), h0 = tid / BN;
    const bool col_ok = c0 + g < F;
    const int gc = min(c0 + g, F - 1);
    float v[P][NV];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float* wj = hp.W[j] + gc;
      const float* bj = hp.b[j] + gc;
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int h = min(h0 + u * HSTEP, H);
        const float* src = h < H ? wj + (size_t)h * F : bj;
        v[j][u] = *src;
      }
    }
    {
      const int n16 = (int)(((size_t)P * 3 * WPLANE + 2 * GBUF + 2 * LLN * 4) / 16);
      u32x4* z = reinterpret_cast<u32x4*>(smem);
      for (int i = tid; i < n16; i += NT) z[i] = u32x4{0u, 0u, 0u, 0u};
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

  // (strip x ROW GROUP: workgroup (x, y) takes the 32-row tiles y * rg_tiles .. of strip x, so
  //  that the launch fills whole rounds of the CUs whatever the gene count -- d4_row_groups.  ll
  //  and dd are per row; the strip's dW / db of row group 0 go to the gradient buffers, those of
  //  the groups behind it to rg_slab [group - 1][P][H + 1][F], summed by d4_rg_combine_kernel)
  const int tile0 = blockIdx.y * rg_tiles;
  const int n_tiles = min((R + D4_BM - 1) / D4_BM, tile0 + rg_tiles);
  const int mfirst = tile0 * D4_BM;
  auto grad_row = [&](int j, int h) -> float* {       // dW_j[h, :] (h < H) or db_j (h == H)
    if (blockIdx.y == 0) return h < H ? hp.dW[j] + (size_t)h * F : hp.db[j];
    return rg_slab + (((size_t)(blockIdx.y - 1) * P + j) * (H + 1) + h) * F;
  };
  const int KP = d3_kp(H), ksp = KP / 32;   // padded width of the planes of d, in elements / steps
  const size_t dplane = (size_t)Rpad * KP;
  const int nb16 = Rpad / 16;

  if (w < NPW) {
    // =========================== producers: GEMM1 + likelihood + G ===========================
    // (their GEMM1 + likelihood chain is the longer of the two; measured: which producers win the
    //  arbitration changes who waits at the barrier, not the tile time)
    __builtin_amdgcn_s_setprio(D4_PRIO_PRODUCER);
    const int gp = w % NGP, rq = w / NGP;     // genes 16 NSB gp .., rows 16 rq .. of the tile
    const int gbase = 16 * NSB * gp;
    const int trw = (8 * q + (i16 >> 2)) * ROWB + 2 * (gbase + 4 * (i16 & 3));        // W, GEMM1
    const int gst = (16 * rq + i16) * ROWB + 2 * (gbase + 4 * q);                     // G store
    struct TileIn { f32x4m t[NSB]; float up0; };
    // (IDX) row of the resident matrix behind this lane's row of the tile at m0 / of the tile
    // the next load_t call reads
    size_t tidx = 0;
    auto load_i = [&](int m0) -> size_t {
      const int rc = min(m0 + 16 * rq + i16, R - 1);
      return (size_t)trows[R == B ? rc : rc % B];
    };
    if (IDX) tidx = load_i(mfirst);
    auto load_t = [&](int m0) {
      TileIn in;
      const int row = m0 + 16 * rq + i16;
      const bool rok = row < R;
      in.up0 = (rok && !FWD) ? gw[row] : 0.f;
      const int rc = rok ? row : R - 1;
      const int cell = R == B ? rc : rc % B;
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
    // d fragments of GEMM1 (B[k = h][n = row]): 3 planes per k-step, one contiguous KiB each; a
    // whole tile's worth is requested at once, behind the previous tile's GEMM1, and lands under
    // that tile's likelihood
    bf16x8 dfr[DF][3];
    auto load_dk = [&](int m0, int ks, bf16x8 (&dst)[3]) {
      const uint16_t* dbase = dA + ((size_t)(m0 / 16 + rq) * ksp + ks) * 512 + lane * 8;
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) dst[pl] = global_b128(dbase + pl * dplane);
    };
    auto load_d = [&](int m0) {       // the first DF steps of a tile
#pragma unroll
      for (int ks = 0; ks < DF; ++ks) load_dk(m0, ks, dfr[ks]);
    };
    // GEMM1 of a tile from the fragments of d in dfr: pre_j^T[gene, row] on the accumulators
    f32x4m acc1[P][NSB];
    auto gemm1 = [&](int mt) {      // (mt: the tile's first row -- steps beyond DF are requested here)
#pragma unroll
      for (int j = 0; j < P; ++j)
#pragma unroll
        for (int sb = 0; sb < NSB; ++sb) acc1[j][sb] = f32x4m{0.f, 0.f, 0.f, 0.f};
      bf16x8 afr[2][P][NSB][3];
      auto load_w = [&](int ks, bf16x8 (&dst)[P][NSB][3]) {
        if (PACK && ks == KS1 - 1) {
          // (the packed block: lane group a = q reads plane a of rows h0 .. h0 + 7, group 3 the
          //  zero rows h0 + 8 ..; one fragment per head and gene block, in slot 0)
          const int trp = (q < 3 ? q * WPLANE : 8 * ROWB) + (i16 >> 2) * ROWB +
                          2 * (gbase + 4 * (i16 & 3));
#pragma unroll
          for (int j = 0; j < P; ++j)
#pragma unroll
            for (int sb = 0; sb < NSB; ++sb)
              dst[j][sb][0] = lds_tr8<ROWB>(Wl + (size_t)(j * 3) * WPLANE + trp + 32 * sb +
                                            32 * ks * ROWB);
          return;
        }
#pragma unroll
        for (int j = 0; j < P; ++j)
#pragma unroll
          for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
              dst[j][sb][pl] = lds_tr8<ROWB>(Wl + (size_t)(j * 3 + pl) * WPLANE + trw + 32 * sb +
                                             32 * ks * ROWB);
      };
      load_w(0, afr[0]);
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks) {
        if (ks + 1 < KS1) load_w(ks + 1, afr[(ks + 1) & 1]);
        if (PACK && ks == KS1 - 1) {
          // the W fragment holds the three terms side by side: one MFMA per term of d
#pragma unroll
          for (int b = 2; b >= 0; --b)
#pragma unroll
            for (int j = 0; j < P; ++j)
#pragma unroll
              for (int sb = 0; sb < NSB; ++sb)
                acc1[j][sb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    afr[ks & 1][j][sb][0], dfr[ks % DF][b], acc1[j][sb], 0, 0, 0);
          continue;
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
                if (TERMS == 9 || a + b < 3) acc1[j][sb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    afr[ks & 1][j][sb][a], dfr[ks % DF][b], acc1[j][sb], 0, 0, 0);
        if (ks + DF < KS1) {        // this step's slot is free: step ks + DF of the same tile
          load_dk(mt, ks + DF, dfr[ks % DF]);
          d3_pin_loads();
        }
      }
    };
    // (g1last) the barrier sits between GEMM1 of a tile and its likelihood: when it releases, the
    // producers are in their VALU stretch and the consumers' GEMM2 finds the matrix pipe free;
    // the producers' GEMM1 of the NEXT tile runs at the end of the iteration, under the
    // consumers' stores (or atomic adds) of dd, which issue no matrix instructions.
    float dbacc[P][NE];                 // (DBP) this lane's part of db_j: its genes, its rows
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
      for (int e = 0; e < NE; ++e) dbacc[j][e] = 0.f;
    TileIn nxt = load_t(mfirst);
    if (IDX) tidx = load_i(min(mfirst + D4_BM, Rpad - D4_BM));
    load_d(mfirst);
    const bool g1last = G1 == 1 || (G1 == 2 && w >= NPW / 2);    // (wave-uniform)
    if (g1last) {
      gemm1(mfirst);
      load_d(min(mfirst + D4_BM, Rpad - D4_BM));
      d3_pin_loads();
    }
    D4_PROF_BEGIN;
    for (int tile = tile0; tile < n_tiles; ++tile) {
      const int m0 = tile * D4_BM;
      if (dbg & 2) { lds_barrier(); continue; }
      const TileIn cur = nxt;
      const float up = cur.up0;
      char* Gb = Gl + ((tile - tile0) & 1) * GBUF;
      float* lb = llbuf + ((tile - tile0) & 1) * LLN;
      if (!g1last) gemm1(m0);
      {
        // the next tile's targets (and, GEMM1 first, its fragments of d): under the likelihood.
        // Unconditional (the last tile requests a valid tile again): under a branch the compiler
        // waits for the loads where the arms meet
        nxt = load_t(min(m0 + D4_BM, Rpad - D4_BM));
        if (IDX) tidx = load_i(min(m0 + 2 * D4_BM, Rpad - D4_BM));
        if (!g1last) load_d(min(m0 + D4_BM, Rpad - D4_BM));
        d3_pin_loads();
      }
      // ---- likelihood of this lane's NSB x 4 elements: row 16 rq + i16, genes
      //      16 NSB gp + 16 sb + 4 q + e ----
      float G[P][NE], tval[NE];
      float lsum = 0.f;
      unsigned nz = 0;
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
          lik_dense<KIND, true>(tval[4 * sb + e], a, lp, g, r, rgate);
          const bool ok = c0 + gbase + 16 * sb + 4 * q + e < F;
          lsum += ok ? lp : 0.f;
#pragma unroll
          for (int j = 0; j < P; ++j) G[j][4 * sb + e] = up * g[j];
          nz |= (ok && tval[4 * sb + e] > 0.f) ? (1u << (4 * sb + e)) : 0u;
        }
      }
      D4_STAMP(1);
      if constexpr (d4_compact(KS1)) {
      // ---- t > 0: + lgamma(r+t) - lgamma(r) [- lgamma(1+t)], and the digamma term of dlog r.
      //      5 % of the elements: instead of a per-lane walk (as many passes as the fullest lane
      //      holds non-zeros -- 1.6 on average with a fifth of the lanes busy, and the VALU
      //      instructions of these waves are what the tile time is made of), the wave's non-zeros
      //      are queued densely -- (t, log r) at position [elements e' < e of all lanes][lanes
      //      below] from one ballot per element slot -- corrected in ONE pass of full lanes, and
      //      read back by their owners.  The queue is 512 bytes of LDS of the wave's own (64
      //      entries: one pass per 64 non-zeros).  (Kept in the wave's corner of the G buffer
      //      the tile is about to fill, the kernels whose GEMM1 sits at the end of the
      //      iteration were not repeatable from run to run -- 26-40 of 40 launches differed,
      //      in sporadic elements whose log r came out of GEMM1 wrong -- although no other
      //      wave touches that corner between the two barriers; with the queue in LDS of
      //      its own: 0 of 40.  Not strict aliasing (-fno-strict-aliasing: the same), rarer
      //      with dd through slabs (0-2 of 30), and gone with the queue in the buffer's LAST
      //      plane instead of its first.  Not understood; tools/time_head.py TIME_HEAD_STRESS.) ----
      if ((Traits::HAS_R || inline_lgamma) && !(dbg & 4)) {
        int pos[NE];
        int total = 0;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          const unsigned long long bal = __builtin_amdgcn_ballot_w64(((nz >> e) & 1u) != 0u);
          pos[e] = total + (int)__builtin_amdgcn_mbcnt_hi(
                               (unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
          total += __builtin_popcountll(bal);
        }
        char* qb = reinterpret_cast<char*>(llbuf + 2 * LLN) + w * 512;
        auto qaddr = [&](int k) { return qb + 8 * k; };
        for (int q0 = 0; q0 < total; q0 += 64) {
#pragma unroll
          for (int e = 0; e < NE; ++e) {
            const int k = pos[e] - q0;
            if (((nz >> e) & 1u) && (unsigned)k < 64u) {
              const float lrv = Traits::HAS_R ? acc1[P - 1][e >> 2][e & 3] : 0.f;
              *reinterpret_cast<f32x2*>(qaddr(k)) = f32x2{tval[e], lrv};
            }
          }
          __builtin_amdgcn_wave_barrier();
          const bool on = lane < total - q0;
          f32x2 in = *reinterpret_cast<const f32x2*>(qaddr(lane));
          const float tt = on ? in.x : 1.f;
          float corr = 0.f, rd = 0.f;
          if (Traits::HAS_R) {
            const float lrv = on ? in.y : 0.f;
            const float r = __expf(fminf(fmaxf(lrv, -10.f), 10.f));
            const float rgate = (lrv >= -10.f && lrv <= 10.f) ? 1.f : 0.f;
            const bool small = tt <= 8.f && (U16 || tt == __builtin_rintf(tt));
            float A, D;
            if (__builtin_amdgcn_ballot_w64(!small) == 0)
              lgamma_digamma_diff_small_wave<true>(r, tt, A, D);
            else
              lgamma_digamma_diff_general<true>(r, tt, A, D);
            corr = A;
            rd = rgate * r * D;
          }
          if (inline_lgamma) corr -= lgamma1p(tt);
          if (on) *reinterpret_cast<f32x2*>(qaddr(lane)) = f32x2{corr, rd};
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int e = 0; e < NE; ++e) {
            const int k = pos[e] - q0;
            if (((nz >> e) & 1u) && (unsigned)k < 64u) {
              const f32x2 o = *reinterpret_cast<const f32x2*>(qaddr(k));
              lsum += o.x;
              if (Traits::HAS_R) G[P - 1][e] = fmaf(up, o.y, G[P - 1][e]);
            }
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
      } else {
      // ---- t > 0: + lgamma(r+t) - lgamma(r) [- lgamma(1+t)], and the digamma term of dlog r:
      //      a per-lane walk over the lane's non-zero elements ----
      if ((Traits::HAS_R || inline_lgamma) && !(dbg & 4)) {
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
              lgamma_digamma_diff_small_wave<true>(r, on ? tt : 0.f, A, D);
            else
              lgamma_digamma_diff_general<true>(r, on ? tt : 1.f, A, D);
            corr = A;
            const float delta = on ? up * rgate * r * D : 0.f;
#pragma unroll
            for (int e = 0; e < NE; ++e) G[P - 1][e] += (idx == e) ? delta : 0.f;
          }
          if (inline_lgamma) corr -= lgamma1p(tt);
          lsum += on ? corr : 0.f;
        }
      }
      }
      D4_STAMP(2);
      if (DBP && !FWD) {
#pragma unroll
        for (int j = 0; j < P; ++j)
#pragma unroll
          for (int e = 0; e < NE; ++e) dbacc[j][e] += G[j][e];
      }
      // ---- this lane's part of the row sum -> lb[gp][q][row]: the consumers add the parts ----
      lb[(gp * 4 + q) * D4_BM + 16 * rq + i16] = lsum;
      // ---- G_j -> three bf16 planes, row-major [row][gene], 8 bytes (4 genes) per store ----
      if constexpr (!FWD)
#pragma unroll
      for (int j = 0; j < P; ++j)
#pragma unroll
        for (int sb = 0; sb < NSB; ++sb) {
          unsigned p1[2], p2[2], p3[2];
#pragma unroll
          for (int e = 0; e < 2; ++e)
            split3_rn_pair(G[j][4 * sb + 2 * e], G[j][4 * sb + 2 * e + 1], p1[e], p2[e], p3[e]);
          char* dst = Gb + (size_t)(j * 3) * GPLANE + gst + 32 * sb;
          *reinterpret_cast<u32x2*>(dst) = u32x2{p1[0], p1[1]};
          *reinterpret_cast<u32x2*>(dst + GPLANE) = u32x2{p2[0], p2[1]};
          *reinterpret_cast<u32x2*>(dst + 2 * GPLANE) = u32x2{p3[0], p3[1]};
        }
      D4_STAMP(3);
      // GEMM1 of the next tile (the last iteration: a valid tile again, unused), then the request
      // for the fragments of the tile after it
      if (g1last) {
        gemm1(min(m0 + D4_BM, Rpad - D4_BM));
        load_d(min(m0 + 2 * D4_BM, Rpad - D4_BM));
        d3_pin_loads();
      }
      D4_STAMP(0);
      lds_barrier();
      D4_STAMP(4);
    }
    lds_barrier();     // (the consumers' pass over the last tile)
    D4_PROF_END;
    if (DBP && !FWD) {
      // db_j[gene] = sum over the rows: over the 16 lanes of a q group (the tile's rows of this
      // wave), then over the row blocks rq through LDS (the G tiles are free now), fixed order
#pragma unroll
      for (int j = 0; j < P; ++j)
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          float v = dbacc[j][e];
#pragma unroll
          for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, WAVE);
          dbacc[j][e] = v;
        }
      float* park = reinterpret_cast<float*>(Gl);        // [gp][j][e][q]
      if (rq == 1 && i16 == 0) {
#pragma unroll
        for (int j = 0; j < P; ++j)
#pragma unroll
          for (int e = 0; e < NE; ++e) park[((gp * P + j) * NE + e) * 4 + q] = dbacc[j][e];
      }
      lds_barrier();     // (every wave of the workgroup: the consumers pass it before their dW)
      if (rq == 0 && i16 == 0) {
#pragma unroll
        for (int j = 0; j < P; ++j)
#pragma unroll
          for (int e = 0; e < NE; ++e) {
            const int c = c0 + gbase + 16 * (e >> 2) + 4 * q + (e & 3);
            if (c < F) grad_row(j, H)[c] = dbacc[j][e] + park[((gp * P + j) * NE + e) * 4 + q];
          }
      }
    }
    return;
  }

  // =========================== consumers: GEMM3 (dd) and GEMM2 (dW) ===========================
  __builtin_amdgcn_s_setprio(D4_PRIO_CONSUMER);
  if constexpr (FWD) {
    // forward only: the strip's per-row log-likelihood, the producers' parts in a fixed order
    lds_barrier();       // (the producers' first tile)
    for (int tile = tile0; tile < n_tiles; ++tile) {
      const int m0 = tile * D4_BM;
      const float* lb = llbuf + ((tile - tile0) & 1) * LLN;
      if (w == NPW && lane < D4_BM && m0 + lane < R) {
        float sm = 0.f;
#pragma unroll
        for (int u = 0; u < NGP * 4; ++u) sm += lb[u * D4_BM + lane];
        ll_part[(size_t)blockIdx.x * R + m0 + lane] = sm;
      }
      lds_barrier();
    }
    return;
  }
  const int ht = w - NPW;                         // h tile of this wave
  // (dd_atomic) the accumulator copy of the XCD this workgroup actually runs on: its adds are
  // then performed in that XCD's own L2, the only L2 that ever holds lines of that copy --
  // correct whatever the dispatcher's block -> XCD placement is
  unsigned xcc = 0;
  if (dd_atomic) {
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 7u;
    // (probe build, timing only -- the sums are wrong: the workgroups of an XCD spread over the
    //  eight copies, a quarter of the adds per line at a time)
    if (dbg & 16) xcc = (blockIdx.x >> 3) & 7u;
  }
  const int n_ht3 = (H + 31) / 32, n_ht2 = DBP ? H / 32 : (H + 1 + 31) / 32;
  static_assert(!PACK || (KS1 >= 2 && KS1 <= 4 && !DBP), "PACK: two to four steps, one h tile a wave");
  // (PACK) the wave that owns the remainder tile runs the loop below in its packed form (PKW): a
  // copy of the loop of its own, chosen once per wave, not a branch inside the loop
  auto consume = [&](auto pkw_) __attribute__((always_inline)) {
  constexpr bool PKW = decltype(pkw_)::value;
  constexpr int NPL = PKW ? 1 : 3;          // planes of this wave's fragments of d^T and W
  constexpr int NC = PKW ? 1 : 4;           // groups of eight h slots that hold rows of dd / dW
  // this wave's h tiles: ht, ht + 4, ... (NHT of them; one for H <= 126)
  const int g3a = li * ROWB + 16 * kh;                                               // G, GEMM3
  // W, GEMM3 (PKW: lane li reads plane li >> 3, row h0 + (li & 7); from lane 24 the zero rows)
  const int g3b = PKW ? (li < 24 ? (li >> 3) * WPLANE + (32 * ht + (li & 7)) * ROWB
                                 : (32 * ht + 8 + (li & 7)) * ROWB) + 16 * kh
                      : (32 * ht + li) * ROWB + 16 * kh;
  const int g2b = (8 * (q >> 1) + (i16 >> 2)) * ROWB + 2 * (16 * (q & 1) + 4 * (i16 & 3));  // G, GEMM2
  f32x16 accW[NHT][P][NGT];                 // dW tiles (h tile x gene tile) of every head
#pragma unroll
  for (int t = 0; t < NHT; ++t)
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
      for (int gt = 0; gt < NGT; ++gt)
#pragma unroll
        for (int i = 0; i < 16; ++i) accW[t][j][gt][i] = 0.f;
  // GEMM2's d fragments (A[i = h][k = row]): one contiguous KiB per plane and 16-row k-step; the
  // two k-steps of (row tile, h tile) are requested while the wave works on the pair before
  constexpr int NA2 = NHT > 1 ? 2 : 1;
  bf16x8 a2[NA2][2][NPL];
  auto load_a2k = [&](int m0, int t, int ks, bf16x8 (&dst)[NPL]) {
    // (h tile clamped to the planes' last: a wave without a tile t requests a valid one, unused
    //  -- no branch around the loads, at whose end the compiler would wait for them)
    const int htt = min(ht + 4 * t, ksp - 1);
    const uint16_t* tb = dT + ((size_t)htt * nb16 + m0 / 16 + ks) * 512 + lane * 8;
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) dst[pl] = global_b128(tb + pl * dplane);
  };
  auto load_a2 = [&](int m0, int t, bf16x8 (&dst)[2][NPL]) {
    load_a2k(m0, t, 0, dst[0]);
    load_a2k(m0, t, 1, dst[1]);
  };
  // (across the barrier -- and across GEMM3, where the wave's register need peaks -- only the
  //  first k-step of the next row tile travels; the second is requested when its GEMM2 starts,
  //  half a GEMM2 ahead of its use)
  if (ht < n_ht2) load_a2k(mfirst, 0, 0, a2[0][0]);
  lds_barrier();       // (the producers' first tile)
  D4_PROF_BEGIN;
  for (int tile = tile0; tile < n_tiles; ++tile) {
    const int m0 = tile * D4_BM;
    const char* Gb = Gl + ((tile - tile0) & 1) * GBUF;
    const float* lb = llbuf + ((tile - tile0) & 1) * LLN;
    // per-row log-likelihood of the strip: the producers' parts summed in a fixed order
    if (w == NPW && lane < D4_BM && m0 + lane < R) {
      float sm = 0.f;
#pragma unroll
      for (int u = 0; u < NGP * 4; ++u) sm += lb[u * D4_BM + lane];
      ll_part[(size_t)blockIdx.x * R + m0 + lane] = sm;
    }
    D4_STAMP(0);
    // (GEMM2 first: GEMM3's stores -- or atomic adds -- of this tile's part of dd then sit
    //  right before the barrier and drain under the wait and the next tile's GEMM2)
#pragma unroll
    for (int t = 0; t < NHT; ++t) {
      if (ht + 4 * t < n_ht2 && !(dbg & 1)) {
        // ---- GEMM2: dW_j[h, gene] += sum_row d[row, h] G_j[row, gene] ----
        bf16x8 (&a2t)[2][NPL] = a2[t % NA2];
        if (t == 0) {
          load_a2k(m0, 0, 1, a2[0][1]);
          d3_pin_loads();
        }
        if (t + 1 < NHT) {
          load_a2(m0, t + 1, a2[(t + 1) % NA2]);
          d3_pin_loads();
        }
        constexpr int NST = 2 * P * NGT;             // step = (k-step * P + head) * NGT + gene tile
        bf16x8 bf[2][3];
        auto load_2 = [&](int st, bf16x8 (&b)[3]) {
          const int gt = st % NGT, j = (st / NGT) % P, ks = st / (NGT * P);
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            b[pl] = lds_tr8<ROWB>(Gb + (size_t)(j * 3 + pl) * GPLANE + g2b + 64 * gt +
                                  16 * ks * ROWB);
        };
        load_2(0, bf[0]);
#pragma unroll
        for (int st = 0; st < NST; ++st) {
          if (st + 1 < NST) load_2(st + 1, bf[(st + 1) & 1]);
          const int gt = st % NGT, j = (st / NGT) % P, ks = st / (NGT * P);
#pragma unroll
          for (int a = NPL - 1; a >= 0; --a)
#pragma unroll
            for (int b = 2; b >= 0; --b)
              if (PKW || TERMS == 9 || a + b < 3) accW[t][j][gt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2t[ks][a], bf[st & 1][b],
                                                                       accW[t][j][gt], 0, 0, 0);
        }
      }
    }
    if (ht < n_ht2 && !(dbg & 1)) {
      // the next row tile's fragments of this wave's first h tile (the last tile: its own
      // again), in flight over the barrier
      load_a2k(min(m0 + D4_BM, Rpad - D4_BM), 0, 0, a2[0][0]);
      d3_pin_loads();
    }
    D4_STAMP(2);
#pragma unroll
    for (int t = 0; t < NHT; ++t) {
      if (ht + 4 * t < n_ht3 && !(dbg & 1)) {
        // ---- GEMM3: dd^T[h, row] = sum_j sum_gene W_j[h, gene] G_j[row, gene] ----
        const int htt = ht + 4 * t;
        f32x16 acc3;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc3[i] = 0.f;
        bf16x8 af[2][3], bf[2][NPL];
        auto load_3 = [&](int st, bf16x8 (&a)[3], bf16x8 (&b)[NPL]) {   // step = head * KS3 + k-step
          const int j = st / KS3, ks = st % KS3;
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            a[pl] = lds_b128(Gb + (size_t)(j * 3 + pl) * GPLANE + g3a + 32 * ks);
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl)
            b[pl] = lds_b128(Wl + (size_t)(j * 3 + pl) * WPLANE + g3b + 128 * t * ROWB + 32 * ks);
        };
        load_3(0, af[0], bf[0]);
#pragma unroll
        for (int st = 0; st < KS3 * P; ++st) {
          if (st + 1 < KS3 * P) load_3(st + 1, af[(st + 1) & 1], bf[(st + 1) & 1]);
#pragma unroll
          for (int a = 2; a >= 0; --a)
#pragma unroll
            for (int b = NPL - 1; b >= 0; --b)
              if (PKW || TERMS == 9 || a + b < 3) acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf[st & 1][b], af[st & 1][a], acc3,
                                                             0, 0, 0);
        }
        if constexpr (PKW) {
          // the three terms of row h0 + i + 4 kh: registers i, i + 4, i + 8 of this lane
#pragma unroll
          for (int i = 0; i < 4; ++i) acc3[i] += acc3[i + 4] + acc3[i + 8];
        }
        D4_STAMP(1);
        const int row = (dbg & 8) ? R : m0 + li;
        if (dd_atomic) {
          // no-return fp32 adds into this XCD's [H][R] accumulator (h-major: the 32 lanes of a
          // half wave add to 128 contiguous bytes); dd_reduce_xcd_kernel sums the eight copies
          if (row < R) {
            typedef __attribute__((address_space(1))) float gfloat;
            float* base = dd_part + ((size_t)xcc * H + 32 * htt + 4 * kh) * R + row;
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (32 * htt + 8 * c + 4 * kh + e < H)
                  __builtin_amdgcn_global_atomic_fadd_f32(
                      (gfloat*)(base + (size_t)(8 * c + e) * R), acc3[4 * c + e]);
          }
        } else if (row < R) {
          // slab [strip][H / 4][R][4] (see decoder_head3_kernel): one 16-byte store per h quad
          const int HQ = (H + 3) >> 2;
          f32x4m* dst = reinterpret_cast<f32x4m*>(dd_part) +
                        ((size_t)blockIdx.x * HQ + 8 * htt + kh) * R + row;
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            if (4 * (8 * htt + 2 * c + kh) < H)
              __builtin_nontemporal_store(
                  f32x4m{acc3[4 * c], acc3[4 * c + 1], acc3[4 * c + 2], acc3[4 * c + 3]},
                  dst + (size_t)2 * c * R);
          }
        }
      }
    }
    D4_STAMP(3);
    lds_barrier();
    D4_STAMP(4);
  }
  D4_PROF_END;
  if (DBP) lds_barrier();     // (the producers' exchange of their db parts)
  // ---- dW / db of the strip ----
#pragma unroll
  for (int t = 0; t < NHT; ++t) {
    const int htt = ht + 4 * t;
    if (htt < n_ht2) {
#pragma unroll
      for (int gt = 0; gt < NGT; ++gt) {
        const int c = c0 + 32 * gt + li;
        if (c < F) {
#pragma unroll
          for (int j = 0; j < P; ++j)
#pragma unroll
            for (int i = 0; i < 4 * NC; ++i) {
              const int h = 32 * htt + (i & 3) + 8 * (i >> 2) + 4 * kh;
              // (PKW: the three terms of the row, accumulated side by side over the launch)
              const float v = PKW ? accW[t][j][gt][i] + (accW[t][j][gt][i + 4] + accW[t][j][gt][i + 8])
                                  : accW[t][j][gt][i];
              if (h <= H) grad_row(j, h)[c] = v;
            }
        }
      }
    }
  }
  };   // consume
  if constexpr (PACK) {
    if (ht == KS1 - 1) consume(std::true_type{});
    else consume(std::false_type{});
  } else {
    consume(std::false_type{});
  }
