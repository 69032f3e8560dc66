// rg_integrate.inc -- included by radegs_kernels.hip inside namespace rg (after stage_record / xcd_band_remap, which the blend kernels share).
// ============================================================================ integrate ==
// GaussianRasterizer.integrate (GOF-style point integration used by mesh extraction): for every query point that
// projects into the image, the opacity accumulated along its pixel's ray up to the point.
//   preprocessPointsCUDA  DGR/cuda_rasterizer/forward.cu:855-900   -> points_preprocess_kernel
//   createWithKeys + SortPairs + identifyTileRanges (rasterizer_impl.cu:114-145,784-806)
//                                                                   -> per-PIXEL counting sort (count / scan / scatter)
//   integrateCUDA         forward.cu:938-1372                       -> integrate_kernel
// Re-design: the reference bins points per 16x16 tile and lets every pixel thread scan its tile's whole point list to
// find its own points (two per-thread local arrays of 2048 + 5x256 entries).  A point belongs to exactly one pixel
// (floor of its projection) and points do not interact, so they are binned per pixel here: each lane gets the [start,end)
// range of its own points, the 2048-entry "contributed" list is replaced by the decisions of the 5-sample transmittance test
// (kept as bits, or replayed: identical arithmetic => identical decisions), and no per-thread scratch arrays exist at all.
struct PointsPreArgs {
  int PN; const float* points3D; const float* view; float focal_x, focal_y; int W, H;
  float2* p2d; float* pdepth; uint32_t* ppix; uint32_t* pix_count;
  float* out_alpha_integrated; float* out_color_integrated; float* out_coordinate2d; float* out_sdf;
};

// initial values of rasterize_points.cu:312-320
__device__ __forceinline__ void point_outputs_init(const PointsPreArgs& a, int i) {
  a.out_alpha_integrated[i] = 1.0f;
  a.out_color_integrated[3 * (size_t)i] = 0.f; a.out_color_integrated[3 * (size_t)i + 1] = 0.f; a.out_color_integrated[3 * (size_t)i + 2] = 0.f;
  a.out_coordinate2d[2 * (size_t)i] = 0.f; a.out_coordinate2d[2 * (size_t)i + 1] = 0.f;
  a.out_sdf[i] = -1000.0f;
}
__global__ void __launch_bounds__(256) points_init_kernel(const PointsPreArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < a.PN) point_outputs_init(a, i);
}

__global__ void __launch_bounds__(256) points_preprocess_kernel(const PointsPreArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.PN) return;
  point_outputs_init(a, i);
  a.ppix[i] = 0xFFFFFFFFu;
  const float* p = a.points3D + 3 * (size_t)i;
  const v3 pv = xform43(mk3(p[0], p[1], p[2]), a.view);
  if (pv.z <= 0.2f) return;
  const float ix = (float)((double)(a.focal_x * pv.x / (pv.z + 0.0000001f)) + a.W / 2.);
  const float iy = (float)((double)(a.focal_y * pv.y / (pv.z + 0.0000001f)) + a.H / 2.);
  // written as acceptance: a NaN projection (a NaN coordinate, 0 * inf in the view transform) passes no compare and must not be binned
  if (!(ix >= 0 && ix < a.W && iy >= 0 && iy < a.H)) return;
  a.pdepth[i] = sqrtf(pv.x * pv.x + pv.y * pv.y + pv.z * pv.z);
  a.p2d[i] = make_float2(ix, iy);
  const uint32_t pix = (uint32_t)f2i_sat(floorf(iy)) * (uint32_t)a.W + (uint32_t)f2i_sat(floorf(ix));
  a.ppix[i] = pix;
  atomicAdd(&a.pix_count[pix], 1u);
}

// slot = incl[pix] - (old remaining count): distinct slots inside the pixel's range, no second cursor array
__global__ void __launch_bounds__(256) points_scatter_kernel(int PN, const uint32_t* ppix, uint32_t* pix_count, const uint32_t* pix_incl,
                                                            uint32_t* pt_sorted) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= PN) return;
  const uint32_t pix = ppix[i];
  if (pix == 0xFFFFFFFFu) return;
  const uint32_t rem = atomicSub(&pix_count[pix], 1u);
  pt_sorted[pix_incl[pix] - rem] = (uint32_t)i;
}

struct IntegrateArgs {
  const uint2* ranges; const uint32_t* point_list; const float4* splat_a; const float4* inte_rec;
  int W, H, gx; const float* bg;
  const uint32_t* pix_incl; const uint32_t* pt_sorted; const float2* p2d; const float* pdepth;
  float* out9; float* final_T; uint32_t* n_contrib;
  float* out_alpha_integrated; float* out_color_integrated; float* out_coordinate2d; float* out_sdf;
};

constexpr int kMaxContributors = 512 * 4;  // MAX_NUM_CONTRIBUTORS * 4, auxiliary.h:27 / forward.cu:1003
constexpr int kPointsPerPass = 4;

// The 5-sample (centre + 4 corners) transmittance test of forward.cu:1043-1110 for one list entry; updates cT and
// reports which samples passed.  Returns true when any did ("used").
struct FiveSample { float alpha0, depth0, depth_max; bool pass0; };
__device__ __forceinline__ bool five_sample(const float4 A, const float4 B, float rpx, float rpy, float pixfx, float pixfy, float cT[5],
                                            FiveSample& o) {
  const float offx[5] = {0.0f, -0.5f, 0.5f, -0.5f, 0.5f}, offy[5] = {0.0f, -0.5f, -0.5f, 0.5f, 0.5f};
  bool used = false;
  o.pass0 = false;
  o.depth_max = -INFINITY;
#pragma unroll
  for (int c = 0; c < 5; c++) {
    const float dx = A.x - pixfx - offx[c], dy = A.y - pixfy - offy[c];
    const float depth = B.w + (rpx * dx + rpy * dy);
    const float power = -0.5f * (A.z * dx * dx + B.x * dy * dy) - A.w * dx * dy;
    if (power > 0.0f || power < B.z) continue;  // B.z: conservative exponent threshold for alpha < 1/255
    const float alpha = fminf(0.99f, B.y * exp_spec(power));
    if (alpha < 1.0f / 255.0f) continue;
    const float test_T = cT[c] * (1 - alpha);
    if (test_T < 0.0001f) continue;
    if (c == 0) { o.pass0 = true; o.alpha0 = alpha; o.depth0 = depth; }
    o.depth_max = fmaxf(o.depth_max, depth);
    cT[c] = test_T;
    used = true;
  }
  return used;
}

// The opacity of a list entry (records A, B; ray plane rpx, rpy; inte_rec pair I0, I1) at a query point that projects to (qx, qy) at
// distance qd: forward.cu:1296-1330 with deviations (1) and (3) of DESIGN 10.  A well-conditioned Gaussian (I1.z) is evaluated at the
// nearer of the point and the entry's depth plane; an ill-conditioned one is a step at that plane: nothing in front of it.
__device__ __forceinline__ float point_alpha(const float4 A, const float4 B, float rpx, float rpy, const float4 I0, const float4 I1, float qx,
                                             float qy, float qd) {
  const float dx = A.x - qx, dy = A.y - qy;
  const float depth = B.w + (rpx * dx + rpy * dy);
  float dz = B.w;
  if (I1.z != 0.0f) dz = B.w - fminf(qd, depth);
  else if (qd < depth) return 0.f;
  const m3 inv = mk33(I0.x, I0.y, I0.z, I0.y, I0.w, I1.x, I0.z, I1.x, I1.y);
  const v3 du = mk3(dx, dy, dz);
  const float power = -0.5f * dot(du, mul(inv, du));
  return fminf(0.99f, B.y * exp_spec(fminf(power, 80.0f)));
}

// Phase 2 walks the tile list again for the query points of a pixel and needs, per (pixel, entry), only WHETHER the 5-sample test of
// phase 1 let the entry through ("used": the reference keeps those ids in a 2048-entry per-thread array, forward.cu:1003,1121).  Phase 1
// leaves one bit per (pixel, entry) in wave-private LDS (64 bits per lane and batch of 64 entries, 12 batches = 6 KB) and phase 2 reads
// it: the same decisions by construction, no exponential for them in phase 2.  Tiles with more than 768 entries replay the test instead
// -- five specified exponentials per (pixel, entry) and pass.
constexpr int kUsedBatches = 12;   // 16: 5.26 ms on C2 with 4 M points, 12 / 10: 4.87 (LDS per wave decides the occupancy; + 3 KB of per-pixel staging for the point-major phase 2)

// What phase 1 leaves of a pixel for its query points: the colour over the background and the median contributor's depth plane.
struct PixelPlane { float col0, col1, col2, mid_dc, mid_px, mid_py, mid_mx, mid_my; };

struct IntegrateLds {
  float4 a[64 * 4];                             // the staged batch: splat records
  float4 i[64 * 2];                             //                   inte_rec pairs (phase 2)
  unsigned long long used[kUsedBatches * 64];   // phase 1's decisions, [batch][pixel]
  // point-major phase 2, per pixel of the strip:
  PixelPlane pix[64];
  uint32_t off[64 + 1];                         // exclusive scan of the pixels' point counts
  uint32_t first[64];                           // first index of the pixel's points in pt_sorted
  uint32_t last[64];                            // the pixel's last contributor (bound of its walk)
};

// One wave's 16x4 pixel strip, the tile list it walks and the lane's own pixel.
struct Strip {
  uint32_t first; int n;          // the tile's entries: point_list[first .. first + n)
  int lane;
  float x0, x1, y0, y1;           // sample positions of the strip (pixel centres +- 0.5) for the batch cull
  bool inside; size_t pix, HW;    // the lane's pixel: in the image?  its index, the plane size
  float pixfx, pixfy;
};

// Stages the batch of 64 list entries that starts at `base` (lane k: entry base + k; INTE: also its inte_rec pair) between two barriers
// and returns the set of entries worth visiting (entry_may_touch).
template <bool INTE>
__device__ __forceinline__ uint64_t stage_batch(const IntegrateArgs& a, const Strip& s, int base, IntegrateLds& lds) {
  __syncthreads();
  const int k = base + s.lane;
  bool rel_lane = false;
  if (k < s.n) {
    const uint32_t g = a.point_list[s.first + k];
    rel_lane = stage_record(a.splat_a, g, lds.a, s.lane, s.x0, s.x1, s.y0, s.y1);
    if constexpr (INTE) {
      const float4* si = a.inte_rec + 2 * (size_t)g;
      lds.i[s.lane * 2 + 0] = si[0]; lds.i[s.lane * 2 + 1] = si[1];
    }
  }
  const uint64_t rel = __ballot(rel_lane);
  __syncthreads();
  return rel;
}

// One more visited entry of a query point's walk.
__device__ __forceinline__ void point_blend(float alpha, float& pa, float& pT) {
  if (alpha < 1.0f / 255.0f) return;
  const float test_T = pT * (1 - alpha);
  pa += alpha * pT;
  pT = test_T;
}

// The outputs of query point q (rasterize_points.cu's four point tensors); pp: its pixel.
__device__ __forceinline__ void store_point(const IntegrateArgs& a, size_t q, float pa, float qx, float qy, float qd, const PixelPlane& pp) {
  a.out_alpha_integrated[q] = pa;
  a.out_color_integrated[3 * q] = pp.col0; a.out_color_integrated[3 * q + 1] = pp.col1; a.out_color_integrated[3 * q + 2] = pp.col2;
  a.out_coordinate2d[2 * q] = qx; a.out_coordinate2d[2 * q + 1] = qy;
  if (qd > 0) {
    const float dx = pp.mid_mx - qx, dy = pp.mid_my - qy;
    const float depth = pp.mid_dc + (pp.mid_px * dx + pp.mid_py * dy);
    a.out_sdf[q] = depth - qd;
  }
}

// ---------------------------------------------------------------- phase 1: the image ----
// Blends the lane's pixel, writes its planes of out9 / final_T / n_contrib, leaves the used bits of the first kUsedBatches batches in
// lds.used and returns what phase 2 needs of the pixel.
__device__ __forceinline__ void image_pass(const IntegrateArgs& a, const Strip& s, IntegrateLds& lds, PixelPlane& pl, uint32_t& last_c) {
  float cT[5] = {1.f, 1.f, 1.f, 1.f, 1.f};  // cT[0] is the pixel's T
  float C0 = 0.f, C1 = 0.f, C2 = 0.f, C3 = 0.f, C4 = 0.f, C6 = 0.f, C7 = 0.f;
  pl = PixelPlane{};   // a pixel outside the image, or without a median contributor, keeps zeros
  last_c = 0;
  uint32_t n_local = 0;
  bool done = !s.inside;
  for (int base = 0; base < s.n; base += 64) {
    if (__all(done)) break;
    uint64_t rel = stage_batch<false>(a, s, base, lds);
    unsigned long long used_bits = 0ull;
    while (rel != 0) {
      const int j = __builtin_ctzll(rel);
      rel &= rel - 1;
      if (done) continue;
      const float4 A = lds.a[j * 4 + 0], B = lds.a[j * 4 + 1], Cc = lds.a[j * 4 + 2], D = lds.a[j * 4 + 3];
      const float T = cT[0];
      FiveSample f;
      if (!five_sample(A, B, Cc.w, D.x, s.pixfx, s.pixfy, cT, f)) continue;
      used_bits |= 1ull << j;
      if (f.depth_max > C6) C6 = f.depth_max;
      if (f.pass0) {
        C0 += Cc.x * f.alpha0 * T; C1 += Cc.y * f.alpha0 * T; C2 += Cc.z * f.alpha0 * T;
        C7 += f.alpha0 * T;
        C3 += f.depth0 * f.alpha0 * T;
        if (T > 0.5f) { C4 = f.depth0; pl.mid_dc = B.w; pl.mid_px = Cc.w; pl.mid_py = D.x; pl.mid_mx = A.x; pl.mid_my = A.y; }
      }
      last_c = (uint32_t)(base + j + 1);
      n_local += 1;
      if (n_local >= (uint32_t)kMaxContributors) done = true;  // the reference stops this pixel here (forward.cu:1121-1125)
    }
    if ((base >> 6) < kUsedBatches) lds.used[(base >> 6) * 64 + s.lane] = used_bits;
  }
  const float T = cT[0];
  if (s.inside) {
    const size_t pix = s.pix, HW = s.HW;
    pl.col0 = C0 + T * a.bg[0]; pl.col1 = C1 + T * a.bg[1]; pl.col2 = C2 + T * a.bg[2];
    a.final_T[pix] = T;
    a.n_contrib[pix] = last_c;
    a.out9[0 * HW + pix] = pl.col0; a.out9[1 * HW + pix] = pl.col1; a.out9[2 * HW + pix] = pl.col2;
    a.out9[3 * HW + pix] = C3; a.out9[4 * HW + pix] = C4; a.out9[6 * HW + pix] = C6; a.out9[7 * HW + pix] = C7;
  }
}

// ------------------------------------- phase 2, point-major: one query point per LANE ----
// For tiles whose every batch has its used bits.  The replay form below gives every pixel-lane four point slots per walk of the list; a
// pixel holds 1.6 points on average (C2, 4 M points) and an entry is used by a quarter of a strip's pixels, so ~one lane-slot in ten
// would do work.  Here the strip's points (sorted by pixel: four runs of pt_sorted, [cur, pe) per lane) are dealt to the lanes 64 at a
// time; a point-lane reads ITS pixel's used bits and per-pixel results from LDS and carries one point through the walk.
__device__ __forceinline__ void points_by_lane(const IntegrateArgs& a, const Strip& s, IntegrateLds& lds, const PixelPlane& pl, uint32_t last_c,
                                               uint32_t cur, uint32_t pe) {
  const int lane = s.lane;
  const uint32_t cnt = pe - cur;
  uint32_t incl = cnt;                   // inclusive wave scan of the counts
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)incl, d);
    if (lane >= d) incl += y;
  }
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  __syncthreads();
  lds.off[lane] = incl - cnt;
  if (lane == 63) lds.off[64] = total;
  lds.first[lane] = cur;
  lds.last[lane] = last_c;
  lds.pix[lane] = pl;
  __syncthreads();
  for (uint32_t r0 = 0; r0 < total; r0 += 64) {
    const uint32_t q = r0 + (uint32_t)lane;
    const bool have = q < total;
    // the pixel this point belongs to: the last p with off[p] <= q (binary search over the 64 offsets)
    int p = 0;
    uint32_t pid = 0;
    float qx = 0.f, qy = 0.f, qd = 0.f, pa = 0.f, pT = 1.f;
    if (have) {
#pragma unroll
      for (int step = 32; step > 0; step >>= 1)
        if (lds.off[p + step] <= q) p += step;
      pid = a.pt_sorted[lds.first[p] + (q - lds.off[p])];
      const float2 qq = a.p2d[pid];
      qx = qq.x; qy = qq.y; qd = a.pdepth[pid];
    }
    const uint32_t my_last = have ? lds.last[p] : 0u;
    for (int base = 0; base < s.n; base += 64) {
      if (__all((uint32_t)base >= my_last)) break;
      uint64_t rel = stage_batch<true>(a, s, base, lds);
      const unsigned long long my_bits = have ? lds.used[(base >> 6) * 64 + p] : 0ull;
      while (rel != 0) {
        const int j = __builtin_ctzll(rel);
        rel &= rel - 1;
        const bool mine = ((my_bits >> j) & 1ull) != 0ull;     // phase 1's decision for (this point's pixel, entry)
        if (!__any(mine)) continue;
        if (!mine) continue;
        const float4 A = lds.a[j * 4 + 0], B = lds.a[j * 4 + 1], Cc = lds.a[j * 4 + 2], D = lds.a[j * 4 + 3];
        point_blend(point_alpha(A, B, Cc.w, D.x, lds.i[j * 2 + 0], lds.i[j * 2 + 1], qx, qy, qd), pa, pT);
      }
    }
    if (have) store_point(a, pid, pa, qx, qy, qd, lds.pix[p]);
  }
}

// ------------------------------- phase 2, replay: the lane's pixel, four points per walk ----
// For tiles longer than the used bits reach: every walk repeats the 5-sample test of phase 1 (rT: identical arithmetic => identical
// decisions) up to the pixel's last contributor.
__device__ __forceinline__ void points_by_pixel_replay(const IntegrateArgs& a, const Strip& s, IntegrateLds& lds, const PixelPlane& pl,
                                                       uint32_t last_c, uint32_t cur, uint32_t pe) {
  while (__any(cur < pe)) {
    const int np = (int)min((uint32_t)kPointsPerPass, pe - cur);
    uint32_t pid[kPointsPerPass];
    float qx[kPointsPerPass], qy[kPointsPerPass], qd[kPointsPerPass], pa[kPointsPerPass], pT[kPointsPerPass];
#pragma unroll
    for (int i = 0; i < kPointsPerPass; i++) {
      pid[i] = 0; qx[i] = qy[i] = qd[i] = 0.f; pa[i] = 0.f; pT[i] = 1.f;
      if (i < np) {
        pid[i] = a.pt_sorted[cur + i];
        const float2 q = a.p2d[pid[i]];
        qx[i] = q.x; qy[i] = q.y; qd[i] = a.pdepth[pid[i]];
      }
    }
    float rT[5] = {1.f, 1.f, 1.f, 1.f, 1.f};
    const uint32_t my_last = np > 0 ? last_c : 0u;
    for (int base = 0; base < s.n; base += 64) {
      if (__all((uint32_t)base >= my_last)) break;
      uint64_t rel = stage_batch<true>(a, s, base, lds);
      while (rel != 0) {
        const int j = __builtin_ctzll(rel);
        rel &= rel - 1;
        if ((uint32_t)(base + j + 1) > my_last) continue;
        const float4 A = lds.a[j * 4 + 0], B = lds.a[j * 4 + 1], Cc = lds.a[j * 4 + 2], D = lds.a[j * 4 + 3];
        FiveSample f;
        if (!five_sample(A, B, Cc.w, D.x, s.pixfx, s.pixfy, rT, f)) continue;
        const float4 I0 = lds.i[j * 2 + 0], I1 = lds.i[j * 2 + 1];
#pragma unroll
        for (int i = 0; i < kPointsPerPass; i++)
          if (i < np) point_blend(point_alpha(A, B, Cc.w, D.x, I0, I1, qx[i], qy[i], qd[i]), pa[i], pT[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < kPointsPerPass; i++)
      if (i < np) store_point(a, pid[i], pa[i], qx[i], qy[i], qd[i], pl);
    cur += (uint32_t)np;
  }
}

__global__ void __launch_bounds__(64) integrate_kernel(const IntegrateArgs a) {
  __shared__ IntegrateLds lds;
  const int item = xcd_band_remap(blockIdx.x, gridDim.x);
  const int tile = item >> 2, sub = item & 3;
  const int tile_x = tile % a.gx, tile_y = tile / a.gx;
  const int lane = threadIdx.x, lx = lane & 15, lr = lane >> 4;
  const int px = tile_x * 16 + lx, py = tile_y * 16 + sub * 4 + lr;
  const uint2 range = a.ranges[tile];
  Strip s;
  s.first = range.x; s.n = (int)(range.y - range.x);
  s.lane = lane;
  s.x0 = (float)(tile_x * 16); s.x1 = s.x0 + 16.0f;
  s.y0 = (float)(tile_y * 16 + sub * 4); s.y1 = s.y0 + 4.0f;
  s.inside = px < a.W && py < a.H;
  s.pix = (size_t)py * a.W + px; s.HW = (size_t)a.H * a.W;
  s.pixfx = (float)px + 0.5f; s.pixfy = (float)py + 0.5f;

  PixelPlane pl;
  uint32_t last_c;
  image_pass(a, s, lds, pl, last_c);

  uint32_t cur = 0, pe = 0;   // this pixel's query points: pt_sorted[cur .. pe)
  if (s.inside) {
    cur = s.pix == 0 ? 0u : a.pix_incl[s.pix - 1];
    pe = a.pix_incl[s.pix];
    a.out9[8 * s.HW + s.pix] = (float)(pe - cur);
  }
  // wave-uniform: does every batch of this tile have its used bits?
  if (s.n <= kUsedBatches * 64) points_by_lane(a, s, lds, pl, last_c, cur, pe);
  else points_by_pixel_replay(a, s, lds, pl, last_c, cur, pe);
}
