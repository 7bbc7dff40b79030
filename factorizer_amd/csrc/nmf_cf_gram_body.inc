// nmf_cf_gram_body.inc — the body shared by the kernels of nmf_cf_gram.hip (read the comment in front of them first): one tile
// of one window of the row-space backward.  Included inside a __global__ function that has in scope the template
// arguments WPB, HALF, AT, MODE, FORM, the arguments t, v0, ga, gt, q, T, G, eps, xcd_remap, the workspaces gcfac, cofac
// (null for CF_PLAIN) and the dynamic LDS fz_lds_cfg.  Text, not an inlined function: the plain kernels keep their argument
// list and their machine code to the instruction (a body function inlined into them, or two unused trailing arguments, did
// not).
  static_assert(FORM == CF_PLAIN || (WPB == 4 && !HALF), "the factor forms: 4 patches per workgroup, W-axis shifts = 0 (mod 4)");
  using TL = CfTile<WPB>;
  using Raw = typename CfRaw<AT>::T;
  constexpr int NB = MODE == CFG_RAW ? 8 : 4;            // channels per register batch
  constexpr int IMG = 64 * TL::LW;                      // floats of one channel image
  float* S = fz_lds_cfg;
  const CfTileId id = cf_tile_id<WPB>(q, cf_logical_block(xcd_remap));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t base, V;
  unsigned off[2], off2[2];
  int lidx[2];
  cf_tile_decode<WPB>(q, id, tid, base, V, off, lidx, off2);
  const int own0 = cf_owner_lidx<WPB>(lane, wave, 0), own1 = cf_owner_lidx<WPB>(lane, wave, 1);
  float* hist = S + TL::STAGE_FLOATS + wave * gram_hist_floats(G - 1);

  float x[8][8];
#pragma unroll
  for (int dd = 0; dd < 8; ++dd)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float4 v = cf_ld4<HALF>(t + base + dd * V, off[k], off2[k]);
      x[dd][k * 4 + 0] = v.x; x[dd][k * 4 + 1] = v.y; x[dd][k * 4 + 2] = v.z; x[dd][k * 4 + 3] = v.w;
    }
  const int64_t bh = (int64_t)id.b * q.h + id.hh;           // (sample, head): one plane of gcfac, G0·G1·G2 rows of cofac
  const int64_t vol = (int64_t)q.D * q.H * q.W;
  // CF_FROM_FACTORS: this wave's patch seen from window 0's grid.  o = window-0 coordinate of the patch's first voxel; per
  // axis the patch lies in window-0 patch a (= o >> 3) and, where o is no multiple of 8, in its cyclic successor
  const float* co[2];      // LDS: coefficients of the window-0 patch of this lane's chunk jp
  unsigned vcol[2];        // the chunk's first column inside that patch (v0 lookup)
  if constexpr (FORM == CF_FROM_FACTORS) {
    float* stage = S + TL::STAGE_FLOATS + WPB * gram_hist_floats(G - 1) + wave * (8 * CFG_COFAC);
    const int gp[3] = {id.g0, id.g1, id.gq * WPB + wave}, sh[3] = {q.s0, q.s1, q.s2}, ps[3] = {q.ps0, q.ps1, q.ps2};
    const int dim[3] = {q.D, q.H, q.W}, ng[3] = {q.G0, q.G1, q.G2};
    int o[3], pa[3][2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      o[a] = gp[a] * 8 - sh[a] + ps[a];
      if (o[a] < 0) o[a] += dim[a];
      if (o[a] >= dim[a]) o[a] -= dim[a];
      pa[a][0] = o[a] >> 3;
      pa[a][1] = pa[a][0] + 1 == ng[a] ? 0 : pa[a][0] + 1;
    }
    const float* cp = cofac + bh * q.G0 * q.G1 * q.G2 * CFG_COFAC;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int i = lane + 64 * r, lp = i / (CFG_COFAC / 4), c4 = i % (CFG_COFAC / 4);
      if (i < 8 * (CFG_COFAC / 4)) {
        const int pidx = (pa[0][(lp >> 2) & 1] * q.G1 + pa[1][(lp >> 1) & 1]) * q.G2 + pa[2][lp & 1];
        *reinterpret_cast<float4*>(stage + lp * CFG_COFAC + c4 * 4) = ld4(cp + (int64_t)pidx * CFG_COFAC + c4 * 4);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int p12 = (lane >> 1) & 7, p2 = (lane & 1) * 4;
    int c1 = o[1] + p12; if (c1 >= q.H) c1 -= q.H;
    int c2 = o[2] + p2; if (c2 >= q.W) c2 -= q.W;
    const int b1 = (c1 >> 3) != pa[1][0], b2 = (c2 >> 3) != pa[2][0];
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
      int c0 = o[0] + jp * 4 + (lane >> 4); if (c0 >= q.D) c0 -= q.D;
      const int b0 = (c0 >> 3) != pa[0][0];
      co[jp] = stage + (b0 * 4 + b1 * 2 + b2) * CFG_COFAC;
      vcol[jp] = (unsigned)((((c0 & 7) * 8 + (c1 & 7)) * 8) + (c2 & 7));
    }
  }
  cf_to_owner<WPB>(S, lidx, own0, own1, x);

  CfWave w{lane};
  GramBwd<8, CfWave> P;
  Raw gq[NB][2];
  auto request_g = [&]() {
#pragma unroll
    for (int dd = 0; dd < NB; ++dd)
#pragma unroll
      for (int k = 0; k < 2; ++k) gq[dd][k] = cf_ld_raw<HALF>(ga + base + dd * V, off[k], off2[k]);
  };
#ifdef FZ_PROBE_GRAM_NOMATH   // timing probe (tools/probes/gram_floor.sh): loads, exchanges and stores only
  float probe_acc = 0.f;
  request_g();
#else
  P.forward(w, x, v0, 8, 512, T, G, eps, hist, request_g);
#endif
  asm volatile("" : "+s"(base));
  // dL/da: coalesced -> owner through the stage, two rows at a time, consumed at once
#pragma unroll
  for (int bt = 0; bt < 8 / NB; ++bt) {
#pragma unroll
    for (int s = 0; s < NB / 2; ++s) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < 2; ++k) *reinterpret_cast<float4*>(S + c * IMG + lidx[k]) = cf_raw_f4(gq[2 * s + c][k]);
      if (MODE == CFG_HALVES && bt == 0 && s == NB / 2 - 1) {
#pragma unroll
        for (int dd = 0; dd < NB; ++dd)
#pragma unroll
          for (int k = 0; k < 2; ++k) gq[dd][k] = cf_ld_raw<HALF>(ga + base + (NB + dd) * V, off[k], off2[k]);
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float4 a0 = *reinterpret_cast<const float4*>(S + c * IMG + own0);
        const float4 a1 = *reinterpret_cast<const float4*>(S + c * IMG + own1);
        const float grow[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        FZ_GRAM_OUT_ROW(NB * bt + 2 * s + c, grow);
      }
      __syncthreads();
    }
  }
  // The running sum of the earlier windows is requested stage by stage, right in front of the rows it is added to
  // (requested earlier — by DMA when dL/da has been consumed, or inside the reverse sweep — window 1 took 10-25 us longer)
  float4 gcq[2];           // CF_FROM_FACTORS: window 0's gc at this thread's two chunks (coalesced map)
  auto request_gc0 = [&] {
    if constexpr (FORM == CF_FROM_FACTORS) {
#pragma unroll
      for (int k = 0; k < 2; ++k) gcq[k] = ld4(cf_at(gcfac + bh * vol, off[k]));
    }
  };
#ifdef FZ_PROBE_GRAM_NOMATH
  request_gc0();
#else
  P.reverse(w, x, 1.0f / q.gscale_div, request_gc0);
#endif
  if constexpr (FORM == CF_STORE_FACTORS) {
    // gc through one plane of the exchange (the column layout of one row of X), stored with the coalesced map; the
    // distributed coefficients by the first lane of each group: row g of S, u_T[g], gs[g], ga₁[g]
    *reinterpret_cast<float4*>(S + own0) = make_float4(P.gc[0], P.gc[1], P.gc[2], P.gc[3]);
    *reinterpret_cast<float4*>(S + own1) = make_float4(P.gc[4], P.gc[5], P.gc[6], P.gc[7]);
    __syncthreads();
    float* gp = gcfac + bh * vol;
#pragma unroll
    for (int k = 0; k < 2; ++k) st4(cf_at(gp, off[k]), *reinterpret_cast<const float4*>(S + lidx[k]));
    if ((lane & 7) == 0) {
      const int g = lane >> 3;
      float* cp = cofac + ((((bh * q.G0 + id.g0) * q.G1 + id.g1) * q.G2 + id.gq * WPB + wave) * CFG_COFAC);
      cp[g] = P.ud;
      cp[8 + g] = P.gsd;
      cp[16 + g] = P.ga1d;
      st4(cp + 24 + g * 8, make_float4(P.gKd[0], P.gKd[1], P.gKd[2], P.gKd[3]));
      st4(cp + 24 + g * 8 + 4, make_float4(P.gKd[4], P.gKd[5], P.gKd[6], P.gKd[7]));
    }
    return;
  }
  float gc0[8], vs0[8];    // CF_FROM_FACTORS: window 0's gc and v_start of this lane's columns (owner map)
  if constexpr (FORM == CF_FROM_FACTORS) {
#pragma unroll
    for (int k = 0; k < 2; ++k) *reinterpret_cast<float4*>(S + lidx[k]) = gcq[k];
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
#pragma unroll
      for (int e = 0; e < 4; ++e) vs0[jp * 4 + e] = v0[vcol[jp] + e];   // scalar loads, as ld_v0: no alignment asked of v0
    }
    __syncthreads();
    const float4 a0 = *reinterpret_cast<const float4*>(S + own0), a1 = *reinterpret_cast<const float4*>(S + own1);
    gc0[0] = a0.x; gc0[1] = a0.y; gc0[2] = a0.z; gc0[3] = a0.w; gc0[4] = a1.x; gc0[5] = a1.y; gc0[6] = a1.z; gc0[7] = a1.w;
    __syncthreads();
  }
#pragma unroll
  for (int bt = 0; bt < 8 / NB; ++bt) {
#pragma unroll
    for (int s = 0; s < NB / 2; ++s) {
      Raw old[2][2];
      if (FORM == CF_PLAIN && q.accumulate) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int k = 0; k < 2; ++k) old[c][k] = cf_ld_raw<HALF>(gt + base + (NB * bt + 2 * s + c) * V, off[k], off2[k]);
      }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int m = NB * bt + 2 * s + c;
        float o[8];
#ifdef FZ_PROBE_GRAM_NOMATH
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = x[m][e] + probe_acc;
#else
        float srow[8], gsm, ga1m;
        P.row_coeffs(w, m, srow, gsm, ga1m);
        P.gx_row(m, x, srow, gsm, ga1m, o);
#endif
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = x[m][e] > 0.f ? o[e] : 0.f;
        if constexpr (FORM == CF_FROM_FACTORS) {
#pragma unroll
          for (int jp = 0; jp < 2; ++jp) {
            const float4 sa = *reinterpret_cast<const float4*>(co[jp] + 24 + m * 8);
            const float4 sb = *reinterpret_cast<const float4*>(co[jp] + 24 + m * 8 + 4);
            const float prow[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
            const float pu = co[jp][m], pgs = co[jp][8 + m], pga1 = co[jp][16 + m];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int j = jp * 4 + e;
              const float g0 = gram_gx_elem<float, 8>(pu, gc0[j], pgs, pga1, vs0[j], prow, x, j);
              o[j] += cf_as_stored<AT>(x[m][j] > 0.f ? g0 : 0.f);
            }
          }
        }
        *reinterpret_cast<float4*>(S + c * IMG + own0) = make_float4(o[0], o[1], o[2], o[3]);
        *reinterpret_cast<float4*>(S + c * IMG + own1) = make_float4(o[4], o[5], o[6], o[7]);
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          float4 z = *reinterpret_cast<const float4*>(S + c * IMG + lidx[k]);
          if (FORM == CF_PLAIN && q.accumulate) {
            const float4 o = cf_raw_f4(old[c][k]);
            z.x += o.x; z.y += o.y; z.z += o.z; z.w += o.w;
          }
          cf_st4<HALF>(gt + base + (NB * bt + 2 * s + c) * V, off[k], off2[k], z);
        }
      __syncthreads();
    }
  }
