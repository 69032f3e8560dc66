// rg_blend_bwd_body.inc -- the body of the tile-wide blend backward, included INSIDE blend_bwd_packed_kernel and blend_bwd_ordered_kernel
// (radegs_kernels.hip): prologue, staging, the loop over the tile's entries and the in-wave reduction (row_reduce16, then two __shfl_xor
// steps) are these lines for both.  Shared as text, not as an inlined function template: that moved the instruction stream of all eight
// blend_bwd_packed_kernel instantiations.  In scope at the point of inclusion: COORD, DEPTH, PPL (constant expressions), the kernel's
// argument `a`, and the macro RG_BLEND_BWD_SINK(total) -- what lane `lane` does with its component's wave total of the entry at list position
// range.x + pos, Gaussian gid, record length REC.
  constexpr bool NORMAL = COORD || DEPTH;
  constexpr int NP = PPL / 2;  // pairs per lane
  constexpr int WPT = 4 / PPL;
  constexpr int REC = COORD ? 32 : 16;
  __shared__ float4 lds_a[65 * 4];
  __shared__ float4 lds_b[COORD ? 64 * 3 : 1];
  __shared__ uint32_t lds_id[65];
  __shared__ __attribute__((aligned(16))) float lds_red[4 * kRedRowFloats];   // row_reduce16's scratch

  const int item = xcd_band_remap(blockIdx.x, gridDim.x);
  const int tile = item / WPT, sub = item - tile * WPT;
  const int tile_x = tile % a.gx, tile_y = tile / a.gx;
  const int lane = threadIdx.x;
  const StripGeom geo = lane_geometry<PPL>(lane, tile_x, tile_y, sub);
  const int px = geo.px;
  const int py0 = geo.py_first;
  const int W = a.W, H = a.H;
  const float pixfx = (float)px;
  const float reg_x0 = geo.rx0, reg_x1 = geo.rx1, reg_y0 = geo.ry0, reg_y1 = geo.ry1;
  const uint2 range = a.ranges[tile];

  // Q is the ONE "behind" accumulator per pixel.  Upstream keeps one per blended quantity
  // (accum_rec[3], accum_t_rec, accum_normal_rec[3], accum_alpha_rec, accum_coord_rec[3]:
  // backward.cu:870,900,930,949,962), each following  acc <- acc + alpha*(v - acc)  and each entering
  // dL/dalpha as  w*(v - acc)  with a per-pixel constant weight w (the pixel's cotangent).  The recurrence is
  // linear, so Q = sum_k w_k*acc_k obeys  Q <- Q + alpha*(V - Q)  with  V = sum_k w_k*v_k,  and
  // sum_k w_k*(v_k - acc_k) = V - Q: identical mathematics, 1 register and 2 operations instead of 8 and 24.
  f2 pixfy[NP], T[NP], Q[NP], dLa[NP], tb[NP];
  f2 dLc[NP][3];
  f2 dLt[NP], dLmt[NP];
  f2 dLn[NP][3];
  f2 dLco[COORD ? NP : 1][3], dLmco[COORD ? NP : 1][3];
  uint32_t last_c[PPL], max_cm1[PPL];
  uint32_t wave_last = 0;
#pragma unroll
  for (int s = 0; s < PPL; s++) {
    const int q = s >> 1, e = s & 1;
    const int py = py0 + kStripRowStep * s;
    pixfy[q][e] = (float)py;
    const PixelCotangents ct = pixel_cotangents<COORD, DEPTH>(a, px, py);
    T[q][e] = ct.T; Q[q][e] = 0.f; dLa[q][e] = ct.dLa; tb[q][e] = ct.tb;
    dLt[q][e] = ct.dLt; dLmt[q][e] = ct.dLmt;
    last_c[s] = ct.last_c; max_cm1[s] = ct.max_cm1;
    wave_last = max(wave_last, last_c[s]);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      dLc[q][c][e] = ct.dLc[c]; dLn[q][c][e] = ct.dLn[c];
      if constexpr (COORD) { dLco[q][c][e] = ct.dLco[c]; dLmco[q][c][e] = ct.dLmco[c]; }
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) wave_last = max(wave_last, (uint32_t)__shfl_xor((int)wave_last, m));
  const f2 cW = bc2(0.5f * W), cH = bc2(0.5f * H);
  const RowReduceAddr red = row_reduce_addr(lds_red, lane >> 4, lane & 15);

  for (int hi = (int)wave_last; hi > 0; hi -= 64) {
    __syncthreads();
    const int e0 = hi - 1 - lane;
    bool rel_lane = false;
    if (e0 >= 0) {
      const uint32_t g = a.point_list[range.x + e0];
      lds_id[lane] = g;
      rel_lane = stage_record(a.splat_a, g, lds_a, lane, reg_x0, reg_x1, reg_y0, reg_y1);
      if constexpr (COORD) {
        const float4* sb = a.splat_b + 3 * (size_t)g;
        lds_b[lane * 3 + 0] = sb[0]; lds_b[lane * 3 + 1] = sb[1]; lds_b[lane * 3 + 2] = sb[2];
      }
    }
    uint64_t rel = __ballot(rel_lane);
    const int niter = (int)__popcll(rel);
    __syncthreads();
    for (int it = 0; it < niter; it++) {   // scalar trip count
      const int j = __builtin_ctzll(rel);  // LDS slot j holds list position hi-1-j: ascending j = back to front
      rel &= rel - 1;
      const float4 A = lds_a[j * 4 + 0], B = lds_a[j * 4 + 1], C = lds_a[j * 4 + 2], Dq = lds_a[j * 4 + 3];
      const uint32_t gid = lds_id[j];
      const uint32_t pos = (uint32_t)(hi - 1 - j);
      const float dx = A.x - pixfx;
      const float a_x = (A.z * dx) * dx;
      const float b_xy = A.w * dx;
      f2 dy[NP], power[NP];
      bool cand[PPL], anyc = false;
#pragma unroll
      for (int q = 0; q < NP; q++) {
        dy[q] = bc2(A.y) - pixfy[q];
        const f2 sq = bc2(a_x) + (bc2(B.x) * dy[q]) * dy[q];
        const f2 vq = bc2(b_xy) * dy[q];
        power[q] = fma2(bc2(-0.5f), sq, -vq);  // == splat_power(), one rounding (rg_blend.h)
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const float pw = power[q][e];
          cand[2 * q + e] = (pos < last_c[2 * q + e]) && !(pw > 0.0f) && !(pw < B.z);
          anyc = anyc || cand[2 * q + e];
        }
      }
      if (!__any(anyc)) continue;
      float4 E0, E1, E2;
      if constexpr (COORD) { E0 = lds_b[j * 3 + 0]; E1 = lds_b[j * 3 + 1]; E2 = lds_b[j * 3 + 2]; }
      // the lane's sums over its pixel pairs; components 9..14 as RAW MOMENTS of h = opacity G dL/dalpha about the Gaussian's centre, everything
      // "times dx" applied once to the lane's total (all pixels of a lane share dx): the record blend_bwd_streams_kernel writes
      // (rg_streams.inc), turned into the reference's sums once per Gaussian by preprocess_bwd_kernel (RecordKind::raw_moments, rg_per_gaussian.inc)
      f2 s_col[3], s_nrm[3], s_dt = bc2(0.f), s_dty = bc2(0.f), s_u = bc2(0.f), s_h = bc2(0.f), s_uy = bc2(0.f), s_uyy = bc2(0.f), s_ab = bc2(0.f);
      f2 s_co[COORD ? 3 : 1], s_coy[COORD ? 3 : 1];
#pragma unroll
      for (int c = 0; c < 3; c++) { s_col[c] = bc2(0.f); s_nrm[c] = bc2(0.f); }
      if constexpr (COORD) {
#pragma unroll
        for (int c = 0; c < 3; c++) { s_co[c] = bc2(0.f); s_coy[c] = bc2(0.f); }
      }
      bool contributed = false;
      const float dxcx = dx * A.z;
#pragma unroll
      for (int q = 0; q < NP; q++) {
        if (!__any(cand[2 * q] || cand[2 * q + 1])) continue;  // wave-uniform
        // ---- alpha (decision = forward's exp_spec rule; value from the hardware exp) ----
        f2 G = f2{__expf(power[q][0]), __expf(power[q][1])};
        f2 a_raw = bc2(B.y) * G;
        {
          const bool b0 = fabsf(fmaf(a_raw[0], 255.0f, -1.0f)) < 1.0e-4f, b1 = fabsf(fmaf(a_raw[1], 255.0f, -1.0f)) < 1.0e-4f;
          if (__any(b0 || b1)) {  // within 1e-4 of the 1/255 threshold: decide with the specified exponential
            if (b0) { G[0] = exp_spec(power[q][0]); a_raw[0] = B.y * G[0]; }
            if (b1) { G[1] = exp_spec(power[q][1]); a_raw[1] = B.y * G[1]; }
          }
        }
        f2 alpha = f2{fminf(0.99f, a_raw[0]), fminf(0.99f, a_raw[1])};
        const bool act0 = cand[2 * q] && !(alpha[0] < 1.0f / 255.0f), act1 = cand[2 * q + 1] && !(alpha[1] < 1.0f / 255.0f);
        contributed = contributed || act0 || act1;
        alpha = f2{act0 ? alpha[0] : 0.f, act1 ? alpha[1] : 0.f};
        G = f2{act0 ? G[0] : 0.f, act1 ? G[1] : 0.f};
        const f2 one_m_a = bc2(1.f) - alpha;
        const f2 inv1ma = f2{rcp_refined(one_m_a[0]), rcp_refined(one_m_a[1])};
        T[q] = T[q] * inv1ma;
        const f2 dch = alpha * T[q];
        // V = <cotangent of this pixel, blended quantities of this Gaussian>; dL/dalpha's blend part = V - Q
        f2 V = dLa[q];
        {
          const float col[3] = {C.x, C.y, C.z};
#pragma unroll
          for (int c = 0; c < 3; c++) {
            V = fma2(bc2(col[c]), dLc[q][c], V);
            s_col[c] = fma2(dch, dLc[q][c], s_col[c]);
          }
        }
        const bool med0 = act0 && pos == max_cm1[2 * q], med1 = act1 && pos == max_cm1[2 * q + 1];
        if constexpr (COORD) {
          const float cpx[3] = {E0.x, E0.z, E1.x}, cpy[3] = {E0.y, E0.w, E1.y}, vp[3] = {E1.z, E1.w, E2.x};
#pragma unroll
          for (int c = 0; c < 3; c++) {
            const f2 cc = fma2(bc2(cpy[c]), dy[q], bc2(fmaf(cpx[c], dx, vp[c])));
            V = fma2(cc, dLco[q][c], V);
            const f2 msel = f2{med0 ? dLmco[q][c][0] : 0.f, med1 ? dLmco[q][c][1] : 0.f};
            const f2 dco = fma2(dch, dLco[q][c], msel);
            s_co[c] += dco;
            s_coy[c] = fma2(dco, dy[q], s_coy[c]);
          }
        }
        if constexpr (DEPTH) {
          const f2 t = fma2(bc2(Dq.x), dy[q], bc2(fmaf(C.w, dx, B.w)));
          V = fma2(t, dLt[q], V);
          const f2 msel = f2{med0 ? dLmt[q][0] : 0.f, med1 ? dLmt[q][1] : 0.f};
          const f2 dt_ = fma2(dch, dLt[q], msel);
          s_dt += dt_;
          s_dty = fma2(dt_, dy[q], s_dty);
        }
        if constexpr (NORMAL) {
          const float nn[3] = {Dq.y, Dq.z, Dq.w};
#pragma unroll
          for (int c = 0; c < 3; c++) {
            V = fma2(bc2(nn[c]), dLn[q][c], V);
            s_nrm[c] = fma2(dch, dLn[q][c], s_nrm[c]);
          }
        }
        f2 dL_dopa = V - Q[q];
        Q[q] = fma2(alpha, dL_dopa, Q[q]);   // alpha = 0 for a pixel that sits this entry out: Q unchanged
        dL_dopa = dL_dopa * T[q];
        dL_dopa = fma2(inv1ma, tb[q], dL_dopa);

        const f2 u = G * dL_dopa;
        const f2 hq = bc2(B.y) * u;   // h = opacity * u: the moments are h's (rg_streams.inc)
        const f2 uy = hq * dy[q];
        const f2 ex = fma2(dy[q], bc2(A.w), bc2(dxcx));    // the conic applied to (dx, dy)
        const f2 ey = fma2(dy[q], bc2(B.x), bc2(b_xy));
        const f2 tt = fma2(__builtin_elementwise_abs(ey), cH, __builtin_elementwise_abs(ex) * cW);
        s_u += u; s_h += hq; s_uy += uy;
        s_uyy = fma2(uy, dy[q], s_uyy);
        s_ab = fma2(__builtin_elementwise_abs(hq), tt, s_ab);
      }
      const uint64_t contrib_mask = __ballot(contributed);
      if (contrib_mask == 0) continue;
      float gs[REC];
      gs[0] = s_col[0][0] + s_col[0][1]; gs[1] = s_col[1][0] + s_col[1][1]; gs[2] = s_col[2][0] + s_col[2][1];
      gs[3] = s_dt[0] + s_dt[1]; gs[4] = gs[3] * dx; gs[5] = s_dty[0] + s_dty[1];
      gs[6] = s_nrm[0][0] + s_nrm[0][1]; gs[7] = s_nrm[1][0] + s_nrm[1][1]; gs[8] = s_nrm[2][0] + s_nrm[2][1];
      gs[15] = s_u[0] + s_u[1];
      gs[9] = (s_h[0] + s_h[1]) * dx; gs[10] = s_uy[0] + s_uy[1]; gs[11] = s_ab[0] + s_ab[1];
      gs[12] = gs[9] * dx; gs[13] = gs[10] * dx; gs[14] = s_uyy[0] + s_uyy[1];
      if constexpr (COORD) {
#pragma unroll
        for (int c = 0; c < 3; c++) { gs[16 + c] = s_co[c][0] + s_co[c][1]; gs[19 + 2 * c] = gs[16 + c] * dx; gs[20 + 2 * c] = s_coy[c][0] + s_coy[c][1]; }
#pragma unroll
        for (int c = 25; c < 32; c++) gs[c] = 0.f;
      }
      // rows first (one DPP stage + wave-private LDS: row_reduce16), then the four rows' totals of component (lane & 15)
      float tot = row_reduce16(*reinterpret_cast<float (*)[16]>(gs), red);
      tot += __shfl_xor(tot, 16);
      tot += __shfl_xor(tot, 32);
      if constexpr (REC == 32) {
        float tot1 = row_reduce16(*reinterpret_cast<float (*)[16]>(gs + 16), red);
        tot1 += __shfl_xor(tot1, 16);
        tot1 += __shfl_xor(tot1, 32);
        if (lane >= 16 && lane < 25) RG_BLEND_BWD_SINK(tot1);
      }
      if (lane < 16) RG_BLEND_BWD_SINK(tot);
    }
  }
