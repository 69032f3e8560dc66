// radegs_kernels.hip -- gfx950 kernels of the differentiable splat rasterizer.
//
// Stage map (reference kernel -> this translation unit); DGR = submodules/diff-gaussian-rasterization:
//   preprocessCUDA<3,false>   DGR/cuda_rasterizer/forward.cu:307-423        -> preprocess_fwd_kernel        (rg_per_gaussian.inc)
//   duplicateWithKeys         DGR/cuda_rasterizer/rasterizer_impl.cu:70-111 -> emit_instances_kernel
//   identifyTileRanges        rasterizer_impl.cu:151-173                    -> tile_ranges_kernel
//   renderCUDA fwd            forward.cu:428-693                            -> blend_fwd_kernel             (entry streams: rg_streams.inc)
//   renderCUDA bwd            DGR/cuda_rasterizer/backward.cu:631-1016      -> blend_bwd_packed_kernel, blend_bwd_ordered_kernel (rg_blend_bwd_body.inc; entry streams: rg_streams.inc)
//   computeCov2DCUDA + preprocessCUDA bwd  backward.cu:145-488,560-628      -> preprocess_bwd_kernel        (rg_per_gaussian.inc)
//   checkFrustum              rasterizer_impl.cu:54-66                      -> mark_visible_kernel          (rg_per_gaussian.inc)
//   integrateCUDA             forward.cu:938-1372                           -> integrate_kernel             (rg_integrate.inc)
// This file keeps what the binning and blend code share (CamArgs, the record staging, the in-wave reduction), the binning kernels and the
// tile-wide blend kernels; the host side is rg_launch.inc.
//
// Design for CDNA4 (not a translation of the CUDA block structure):
//   * Blend kernels: ONE wave64 owns a 16 x (4*PPL) pixel strip of a 16x16 tile; each lane keeps
//     PPL pixels (same column, rows 4 apart) in registers.  No cross-wave sharing, no barriers in
//     the hot loop.  Per-Gaussian attributes are wave-uniform: they are staged 64 entries at a
//     time into wave-private LDS (each lane gathers one 64-B record = one cache line) and read
//     back as broadcast ds_read_b128 -- amortised over PPL pixels per lane, which keeps the
//     LDS pipe (one b128 per 4 clk per CU) off the critical path.
//   * The skip test needs no transcendental: a per-Gaussian exponent threshold (computed once in
//     preprocess) rejects alpha < 1/255 pairs from the quadratic form alone; exp is evaluated
//     only for surviving pairs, with the specified exp_spec() so that every thresholded decision
//     matches the CPU oracle bit-for-bit.
//   * Backward: per-lane partial gradients of one Gaussian are reduced over all 16 (or 32) gradient
//     components at once (row_reduce16), which leaves component c in lane c, so ONE 16/25-lane
//     global_atomic_add_f32 instruction updates one 64-B accumulator line.
//   * blockIdx -> tile mapping gives each XCD a contiguous band of tiles (neighbouring tiles
//     share splat records -> per-XCD L2 reuse).
// No MFMA: there is no dense contraction on this path.
#include <hip/hip_runtime.h>
#include <type_traits>

#include "rg_blend.h"
#include "rg_layout.h"
#include "rg_preprocess.h"
#include "rg_preprocess_bwd.h"

namespace rg {

// ------------------------------------------------------------------ launch arguments ----
struct CamArgs {
  const float* view;    // device [16]
  const float* proj;    // device [16]
  const float* campos;  // device [3]
  float focal_x, focal_y, tan_fovx, tan_fovy, kernel_size, scale_modifier;
  int W, H, gx, gy;
};

__device__ __forceinline__ Camera load_camera(const CamArgs& a) {
  Camera c;
#pragma unroll
  for (int i = 0; i < 16; i++) { c.view[i] = a.view[i]; c.proj[i] = a.proj[i]; }
#pragma unroll
  for (int i = 0; i < 3; i++) c.campos[i] = a.campos[i];
  c.focal_x = a.focal_x; c.focal_y = a.focal_y; c.tan_fovx = a.tan_fovx; c.tan_fovy = a.tan_fovy;
  c.kernel_size = a.kernel_size; c.scale_modifier = a.scale_modifier;
  c.W = a.W; c.H = a.H; c.gx = a.gx; c.gy = a.gy;
  return c;
}

// The depth keys of the visible Gaussians start here: preprocess_fwd_kernel tests a key against it, the 3-pass depth sort subtracts it.
constexpr uint32_t kDepthKeyBase = 0x3E4CCCCDu;   // bits(0.2f): every visible Gaussian lies beyond the near plane (auxiliary.h:166)

#include "rg_per_gaussian.inc"   // one thread per Gaussian: preprocess forward / backward, mark_visible, the view-parallel SH gradient

// ============================================================================== binning ==
// One thread per Gaussian IN DEPTH ORDER; writes (tile id, gaussian idx) for every tile of its rect, rows outer /
// columns inner -- the emission order of rasterizer_impl.cu:98-109.  Splats with few tiles are written by their own
// lane; a splat with many tiles (heavy-overdraw scenes: hundreds per splat) is handed to the whole wave, which writes
// its instances 64 at a time to consecutive addresses -- coalesced, and no lane serialises a 300-iteration loop.
constexpr int kEmitCoopThreshold = 16;
// rect != nullptr (tile grid at most 255x255): rect[i] is the packed tile rectangle of the i-th Gaussian IN DEPTH ORDER (the scan's
// gather wrote it): no random access at all here, instead of recomputing the rectangle from three gathers.
// MASKS (sub-tile entry streams, rg_streams.inc): the instance value also carries, in its top byte, which of the tile's eight 8x4
// blocks the splat can reach (ellipse_tile_mask, rg_blend.h).  Here the splat's record is in registers once for all its tiles; after
// the sort the same question costs a dependent gather per list entry.  block_lists_kernel strips the byte again.
template <bool MASKS>
__global__ void __launch_bounds__(256) emit_instances_kernel(int P, const uint32_t* idx_sorted, const uint32_t* offsets,
                                                            const uint32_t* tiles_touched, const float4* splat_a, const int* radii,
                                                            const uint32_t* rect, int gx, int gy, uint32_t* tile_keys, uint32_t* vals,
                                                            uint32_t cap, uint32_t* ranges_to_clear, uint32_t* count_mirror, uint32_t seq, uint32_t* stream_tag, int key16,
                                                            int mask_in_key, const unsigned long long* tile_sq_sum) {
  // key16: tile ids leave as 16-bit keys (grids of at most 65 536 tiles): the tile sort then moves a third less (radegs_sort.hip)
  // mask_in_key (MASKS, scenes of 2^24 Gaussians and more, 32-bit keys): the block mask rides in the top byte of the KEY -- the tile sort
  // only looks at the low tile bits -- and the value is the plain Gaussian index
  uint16_t* const tile_keys16 = reinterpret_cast<uint16_t*>(tile_keys);
  // cap: capacity of tile_keys/vals.  With exact allocation it equals num_rendered; in the speculative path (rg_launch.inc)
  // it is a prediction and instances beyond it are dropped here (the host detects the overflow and redoes the binning).
  const int i = blockIdx.x * 256 + threadIdx.x;
  // Two chores that used to be kernels of their own (a 5 us copy and a 5 us fill per forward): the tile ranges start at (0,0)
  // (rasterizer_impl.cu:383's memset; tile_ranges_kernel runs two sorts later), and num_rendered goes to the host's pinned words
  // without a copy engine command or an event: the count, then this forward's sequence number with release order (the host polls the
  // sequence word once everything else of the forward is queued, rg_launch.inc::finish_speculative).
  if (ranges_to_clear) {
    for (int k = i; k < 2 * gx * gy; k += (int)gridDim.x * 256) ranges_to_clear[k] = 0u;
  }
  if (count_mirror && i == 0) {
    __hip_atomic_store(count_mirror, offsets[P - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long sq = tile_sq_sum ? *tile_sq_sum : 0ull;   // PIN_SQ_LO / PIN_SQ_HI (rg_launch.inc)
    __hip_atomic_store(count_mirror + 6, (uint32_t)sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(count_mirror + 7, (uint32_t)(sq >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // PIN_SEQ; a stream forward publishes it later, together with the chunks its lists took (block_lists_kernel)
    if (!MASKS) __hip_atomic_store(count_mirror + 2, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (i == 0) {   // does this image state hold entry streams?  (ImageState::stream_tag; the chunk allocator and its overflow flag start at 0)
    stream_tag[0] = MASKS ? kStreamTag : 0u; stream_tag[1] = 0u; stream_tag[3] = 0u;
  }
  const int lane = threadIdx.x & 63;
  uint32_t idx = 0, ntiles = 0, off = 0;
  int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
  if (i < P) {
    idx = idx_sorted[i];
    if (rect) {
      const uint32_t r = rect[i];   // already in depth order (the scan gathered it)
      x0 = (int)(r & 255u); y0 = (int)((r >> 8) & 255u); x1 = x0 + (int)((r >> 16) & 255u); y1 = y0 + (int)(r >> 24);
      ntiles = (uint32_t)((x1 - x0) * (y1 - y0));
      if (ntiles) off = (i == 0) ? 0u : offsets[i - 1];
      if (MASKS && ntiles) { q0 = splat_a[4 * (size_t)idx]; q1 = splat_a[4 * (size_t)idx + 1]; }
    } else {
      ntiles = tiles_touched[idx];
      if (ntiles) {
        off = (i == 0) ? 0u : offsets[i - 1];
        q0 = splat_a[4 * (size_t)idx];
        if (MASKS) q1 = splat_a[4 * (size_t)idx + 1];
        tile_rect(q0.x, q0.y, radii[idx], gx, gy, x0, y0, x1, y1);
      }
    }
  }
  if constexpr (MASKS) {
    // Entry streams: every INSTANCE gets a block mask (~150 instructions), and a lane that walks its own splat's tiles leaves most of
    // the wave idle (a wave costs its LARGEST splat: 2x2 tiles next to 4x4).  The wave therefore expands its 64 splats into their
    // instances and deals those to the lanes 64 at a time: exclusive prefix of the tile counts, lane t of a chunk finds its splat by a
    // binary search over the prefixes (6 ds_bpermute steps), fetches that splat's rectangle and its ellipse set-up (computed once, by
    // the owning lane, for the whole rectangle) and evaluates ONE tile: 4 slabs, 2 columns each.  Same instances at the same positions
    // (offset of the splat + row-major position in its rectangle).
    uint32_t incl = ntiles;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(incl, d);
      if (lane >= d) incl += y;
    }
    const uint32_t excl = incl - ntiles;
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    const int w_own = x1 - x0;
    EllipseSetup e_own;
    e_own.kind = 0; e_own.cy = 0.f; e_own.det = 0.f; e_own.cxM = 0.f; e_own.icx = 0.f; e_own.hx = 0.f; e_own.hy = 0.f; e_own.tstar = 0.f; e_own.eps = 0.f;
    if (ntiles) e_own = ellipse_setup_rect(q0.x, q0.y, q0.z, q0.w, q1.x, q1.z, x0, y0, x1, y1);
    for (uint32_t base = 0; base < total; base += 64) {
      const uint32_t t = base + (uint32_t)lane;
      int g = 0;                                   // largest lane k with excl_k <= t (excl is non-decreasing, excl_0 = 0)
#pragma unroll
      for (int step = 32; step > 0; step >>= 1) {
        const uint32_t pm = __shfl(excl, g + step);
        if (pm <= t) g += step;
      }
      const uint32_t local = t - __shfl(excl, g);
      const uint32_t g_idx = __shfl(idx, g), g_off = __shfl(off, g);
      const int g_x0 = __shfl(x0, g), g_y0 = __shfl(y0, g), g_w = __shfl(w_own, g);
      const float g_mx = __shfl(q0.x, g), g_my = __shfl(q0.y, g);
      EllipseSetup e;
      e.kind = __shfl(e_own.kind, g); e.cy = __shfl(e_own.cy, g); e.det = __shfl(e_own.det, g); e.cxM = __shfl(e_own.cxM, g);
      e.icx = __shfl(e_own.icx, g); e.hx = __shfl(e_own.hx, g); e.hy = __shfl(e_own.hy, g); e.tstar = __shfl(e_own.tstar, g);
      e.eps = __shfl(e_own.eps, g);
      if (t < total) {
        // row-major position in the splat's rectangle: local = ty * w + tx (rg_blend.h)
        RG_RECT_TILE_OF(local, g_w, tx, ty)
        const uint32_t pos = g_off + local;
        if (pos < cap) {
          const uint32_t mask = ellipse_rect_tile_mask(e, g_mx, g_my, g_x0, g_y0, tx, (int)ty) << kMaskShift;
          const uint32_t tile = (uint32_t)((g_y0 + (int)ty) * gx + (g_x0 + tx));
          if (key16) tile_keys16[pos] = (uint16_t)tile; else tile_keys[pos] = tile | (mask_in_key ? mask : 0u);
          vals[pos] = mask_in_key ? g_idx : (g_idx | mask);
        }
      }
    }
    return;
  }
  // tile-wide kernels: no masks.  Splats with few tiles are written by their own lane; a splat with many tiles (heavy-overdraw scenes:
  // hundreds per splat) is handed to the whole wave, which writes its instances 64 at a time to consecutive addresses.
  const bool big = ntiles > (uint32_t)kEmitCoopThreshold;
  if (ntiles && !big) {
    for (int y = y0; y < y1; y++) {
      for (int x = x0; x < x1; x++) {
        if (off < cap) {
          if (key16) tile_keys16[off] = (uint16_t)(y * gx + x); else tile_keys[off] = (uint32_t)(y * gx + x);
          vals[off] = idx;
        }
        off++;
      }
    }
  }
  uint64_t todo = __ballot(big);
  while (todo) {
    const int src = __builtin_ctzll(todo);
    todo &= todo - 1;
    const uint32_t g_idx = __shfl(idx, src), g_n = __shfl(ntiles, src), g_off = __shfl(off, src);
    const int g_x0 = __shfl(x0, src), g_y0 = __shfl(y0, src), g_w = __shfl(x1, src) - g_x0;
    for (uint32_t t = lane; t < g_n; t += 64) {
      const int ty = (int)(t / (uint32_t)g_w), tx = (int)(t - (uint32_t)ty * (uint32_t)g_w);
      if (g_off + t < cap) {
        if (key16) tile_keys16[g_off + t] = (uint16_t)((g_y0 + ty) * gx + (g_x0 + tx)); else tile_keys[g_off + t] = (uint32_t)((g_y0 + ty) * gx + (g_x0 + tx));
        vals[g_off + t] = g_idx;
      }
    }
  }
}

// key_mask: the bits of a key that are the tile id (32-bit keys of a scene of 2^24 Gaussians and more carry the block mask above them)
// One 16-byte load of consecutive keys per thread (8 of the 16-bit ones) and the key before them (rounds 1-5: one key and its predecessor
// per thread, two 2-byte loads: 107 us for C5's 50 M keys); `cap` = items the buffer holds (a vector that would reach past it goes key by key).
constexpr int kRangeThreads = 256;
template <class K>
__global__ void __launch_bounds__(kRangeThreads) tile_ranges_kernel(int L, const K* keys, uint2* ranges, const uint32_t* L_dev, uint32_t key_mask, int cap) {
  constexpr int V = 16 / (int)sizeof(K);
  if (L_dev) L = (int)min((uint32_t)L, *L_dev);  // capacity launch, see emit_instances_kernel
  const long long base = ((long long)blockIdx.x * kRangeThreads + threadIdx.x) * V;
  if (base >= L) return;
  K v[V];
  if (base + V <= cap) {
    const uint4 w = *reinterpret_cast<const uint4*>(keys + base);
    __builtin_memcpy(v, &w, 16);
  } else {
#pragma unroll
    for (int k = 0; k < V; k++) v[k] = base + k < cap ? keys[base + k] : (K)0;
  }
  uint32_t prev = base > 0 ? ((uint32_t)keys[base - 1] & key_mask) : 0u;
#pragma unroll
  for (int k = 0; k < V; k++) {
    const long long i = base + k;
    if (i >= L) break;
    const uint32_t cur = (uint32_t)v[k] & key_mask;
    if (i == 0) ranges[cur].x = 0;
    else if (cur != prev) { ranges[prev].y = (uint32_t)i; ranges[cur].x = (uint32_t)i; }
    if (i == L - 1) ranges[cur].y = (uint32_t)L;
    prev = cur;
  }
}

// Batch-level culling.  While a batch of 64 list entries is staged, lane k still has entry k's
// record in registers; it tests the axis-aligned bounding box of the entry's {power >= thr} ellipse
// (the only region where alpha can reach 1/255) against the pixel rectangle this wave owns.  One
// ballot then gives the 64-bit set of entries worth visiting; the serial walk only touches those.
// The ellipse  1/2 (cx dx^2 + 2 cy dx dy + cz dy^2) <= -thr  has half extents
// hx = sqrt(m cz / det), hy = sqrt(m cx / det), m = -2 thr, det = cx cz - cy^2.  They are inflated by
// 0.1 % + 0.01 px so fp32 rounding of `power` at a pixel can never disagree; any NaN makes the
// comparisons false, i.e. keeps the entry (conservative).  thr > 0 (opacity so low that even the
// centre fails) means the entry can never blend.
__device__ __forceinline__ bool entry_may_touch(const float4 q0, const float4 q1, float x_lo, float x_hi, float y_lo, float y_hi) {
  const float mx = q0.x, my = q0.y, cx = q0.z, cy = q0.w, cz = q1.x, thr = q1.z;
  const float det = cx * cz - cy * cy;
  const float m = -2.0f * thr;
  const float r = m / det;
  const float hx = sqrtf(r * cz) * 1.001f + 0.01f;
  const float hy = sqrtf(r * cx) * 1.001f + 0.01f;
  const bool off = (mx + hx < x_lo) || (mx - hx > x_hi) || (my + hy < y_lo) || (my - hy > y_hi);
  // The extents only mean something for a positive-definite conic.  A needle-thin splat's determinant can round to <= 0 (the
  // preprocess only rejects det == 0, forward.cu:127): such an entry is kept and the exact per-pixel rule decides, as for NaN.
  const bool definite = (det > 0.0f) && (cx > 0.0f) && (cz > 0.0f);
  return !(thr > 0.0f) && !(off && definite);
}

// One lane stages one list entry: the 64-byte record (one cache line) of Gaussian g goes into LDS slot `slot`, and the answer is
// whether the entry can touch the wave's pixel rectangle (entry_may_touch).
__device__ __forceinline__ bool stage_record(const float4* splat_a, uint32_t g, float4* lds_a, int slot, float x_lo, float x_hi, float y_lo,
                                             float y_hi) {
  const float4* src = splat_a + 4 * (size_t)g;
  const float4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
  lds_a[slot * 4 + 0] = q0; lds_a[slot * 4 + 1] = q1; lds_a[slot * 4 + 2] = q2; lds_a[slot * 4 + 3] = q3;
  return entry_may_touch(q0, q1, x_lo, x_hi, y_lo, y_hi);
}

// blockIdx -> work item such that each XCD (block b runs on XCD b % 8) owns a contiguous band.
__device__ __forceinline__ int xcd_band_remap(int b, int n) {
  const int q = n >> 3, r = n & 7, xcd = b & 7, loc = b >> 3;
  return xcd * q + (xcd < r ? xcd : r) + loc;
}

#include "rg_integrate.inc"   // GaussianRasterizer.integrate: the query-point kernels and integrate_kernel

// =========================================================================== blend, fwd ==
struct BlendFwdArgs {
  const uint2* ranges; const uint32_t* point_list; const float4* splat_a; const float4* splat_b;
  int W, H, gx, ntiles; float focal_x, focal_y;
  const float* bg;
  float* out_color; float* out_coord; float* out_mcoord; float* out_depth; float* out_mdepth; float* out_alpha; float* out_normal;
  uint32_t* n_contrib; float* accum_coord; float* accum_depth; float* normal_length;
  const uint32_t* blk_count; const uint32_t* blk_base; uint32_t* blk_consumed; uint32_t* blk_chunks; const uint32_t* blk_order;   // sub-tile entry streams (rg_streams.inc)
};

// The maps a mode does NOT produce are all-zero in the reference, whatever the flags (torch::full(0), rasterize_points.cu:71-77).  A
// caller that hands their pointers over gets them zeroed here, by the pixel's own lane in the forward's epilogue -- the stores ride along
// in a VALU-bound kernel; a separate fill of the 6 unproduced planes of a depth-mode 1080p view was a 9-us kernel + its launch gap per
// forward.  (NULL: the caller does not want them, or provides zeros itself.)
template <bool COORD, bool DEPTH>
__device__ __forceinline__ void zero_unproduced_maps(const BlendFwdArgs& a, size_t pix, size_t HW) {
  // non-temporal: nothing on this path reads these planes again, and 50 MB of ordinary stores would push the entry streams and records the
  // backward is about to re-read out of the L2 / Infinity Cache
  auto z = [](float* p) { __builtin_nontemporal_store(0.0f, p); };
  if constexpr (!COORD) {
    if (a.out_coord) { z(a.out_coord + pix); z(a.out_coord + HW + pix); z(a.out_coord + 2 * HW + pix); }
    if (a.out_mcoord) { z(a.out_mcoord + pix); z(a.out_mcoord + HW + pix); z(a.out_mcoord + 2 * HW + pix); }
  }
  if constexpr (!DEPTH) {
    if (a.out_depth) z(a.out_depth + pix);
    if (a.out_mdepth) z(a.out_mdepth + pix);
  }
  if constexpr (!COORD && !DEPTH) {
    if (a.out_normal) { z(a.out_normal + pix); z(a.out_normal + HW + pix); z(a.out_normal + 2 * HW + pix); }
  }
}

// One pixel's epilogue (forward.cu:631-692): the last and the median contributor, colour over the background, alpha, the maps the mode
// produces, what the backward re-reads (accum_*, normal_length), zeros for the other maps.  T_final: the transmittance left behind the
// last entry -- each formulation passes its own (see the two call sites).  Co / mCo are only read in coord mode.
template <bool COORD, bool DEPTH>
__device__ __forceinline__ void blend_fwd_epilogue(const BlendFwdArgs& a, int px, int py, float T_final, uint32_t last_c, uint32_t max_c,
                                                   float Cr, float Cg, float Cb, float weight, const float (&Co)[3], const float (&mCo)[3],
                                                   float Dep, float mDep, float Nx, float Ny, float Nz) {
  constexpr bool NORMAL = COORD || DEPTH;
  const int W = a.W, H = a.H;
  const size_t HW = (size_t)H * W;
  const size_t pix = (size_t)W * py + px;
  const float pnx = ((float)px - W / 2.f) / a.focal_x;
  const float pny = ((float)py - H / 2.f) / a.focal_y;
  const float ln = sqrtf(pnx * pnx + pny * pny + 1);
  a.n_contrib[pix] = last_c;
  a.n_contrib[pix + HW] = max_c;
  a.out_color[pix] = fmaf(T_final, a.bg[0], Cr);
  a.out_color[HW + pix] = fmaf(T_final, a.bg[1], Cg);
  a.out_color[2 * HW + pix] = fmaf(T_final, a.bg[2], Cb);
  a.out_alpha[pix] = weight;
  zero_unproduced_maps<COORD, DEPTH>(a, pix, HW);
  if constexpr (COORD) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      a.out_coord[c * HW + pix] = last_c ? Co[c] / weight : 0.f;
      a.accum_coord[c * HW + pix] = Co[c];
      a.out_mcoord[c * HW + pix] = mCo[c];
    }
  }
  if constexpr (DEPTH) {
    const float depth_ln = Dep / ln;
    a.accum_depth[pix] = depth_ln;
    a.out_depth[pix] = last_c ? depth_ln / weight : 0.f;
    a.out_mdepth[pix] = mDep / ln;
  }
  if constexpr (NORMAL) {
    if (last_c) {
      float len_n = sqrtf(Nx * Nx + Ny * Ny + Nz * Nz);
      a.normal_length[pix] = len_n;
      len_n = fmaxf(len_n, 1.0E-12F);
      a.out_normal[pix] = Nx / len_n;
      a.out_normal[HW + pix] = Ny / len_n;
      a.out_normal[2 * HW + pix] = Nz / len_n;
    } else {
      a.normal_length[pix] = 1;
      a.out_normal[pix] = 0; a.out_normal[HW + pix] = 0; a.out_normal[2 * HW + pix] = 0;
    }
  }
}

// One wave64 owns a 16 x (4*PPL) strip of the tile: lane -> column (lane & 15), rows (lane >> 4) + 4 s.
struct StripGeom { int px, py_first; float rx0, rx1, ry0, ry1; };
template <int PPL>
__device__ __forceinline__ StripGeom lane_geometry(int lane, int tile_x, int tile_y, int sub) {
  StripGeom g;
  g.px = tile_x * 16 + (lane & 15); g.py_first = tile_y * 16 + sub * (4 * PPL) + (lane >> 4);
  g.rx0 = (float)(tile_x * 16); g.rx1 = g.rx0 + 15.0f; g.ry0 = (float)(tile_y * 16 + sub * (4 * PPL)); g.ry1 = g.ry0 + (float)(4 * PPL - 1);
  return g;
}
constexpr int kStripRowStep = 4;   // rows between the pixels of one lane

template <bool COORD, bool DEPTH, int PPL>
__global__ void __launch_bounds__(64) blend_fwd_kernel(const BlendFwdArgs a) {
  constexpr bool NORMAL = COORD || DEPTH;
  constexpr int WPT = 4 / PPL;  // waves per tile
  __shared__ float4 lds_a[65 * 4];
  __shared__ float4 lds_b[COORD ? 64 * 3 : 1];

  const int item = xcd_band_remap(blockIdx.x, gridDim.x);
  const int tile = item / WPT, sub = item - tile * WPT;
  const int tile_x = tile % a.gx, tile_y = tile / a.gx;
  const int lane = threadIdx.x;
  const StripGeom geo = lane_geometry<PPL>(lane, tile_x, tile_y, sub);
  const int px = geo.px;
  const int py0 = geo.py_first;  // slot s -> row py0 + 4 s
  const int W = a.W, H = a.H;
  const float pixfx = (float)px;
  // pixel rectangle owned by this wave (for batch culling)
  const float reg_x0 = geo.rx0, reg_x1 = geo.rx1, reg_y0 = geo.ry0, reg_y1 = geo.ry1;

  const uint2 range = a.ranges[tile];
  const int n = (int)(range.y - range.x);

  // Tw is the working transmittance: it equals T until the pixel terminates, then it is forced to
  // 0 -- any later candidate then fails `T*(1-alpha) >= 1e-4` by itself, which is exactly "done".
  float pixfy[PPL], T[PPL], Tw[PPL], Cr[PPL], Cg[PPL], Cb[PPL], weight[PPL];
  float Dep[PPL], mDep[PPL], Nx[PPL], Ny[PPL], Nz[PPL];
  float Co[COORD ? PPL : 1][3], mCo[COORD ? PPL : 1][3];
  uint32_t last_c[PPL], max_c[PPL];
  bool inside[PPL];
#pragma unroll
  for (int s = 0; s < PPL; s++) {
    const int py = py0 + kStripRowStep * s;
    pixfy[s] = (float)py;
    inside[s] = px < W && py < H;
    T[s] = 1.0f; Tw[s] = inside[s] ? 1.0f : 0.0f; Cr[s] = Cg[s] = Cb[s] = 0.f; weight[s] = 0.f;
    Dep[s] = mDep[s] = 0.f; Nx[s] = Ny[s] = Nz[s] = 0.f;
    last_c[s] = 0; max_c[s] = 0xFFFFFFFFu;
    if constexpr (COORD) {
#pragma unroll
      for (int c = 0; c < 3; c++) { Co[s][c] = 0.f; mCo[s][c] = 0.f; }
    }
  }
  bool all_done;
  {
    bool d = true;
#pragma unroll
    for (int s = 0; s < PPL; s++) d = d && (Tw[s] == 0.0f);
    all_done = __all(d);
  }

  for (int base = 0; base < n && !all_done; base += 64) {
    // ---- stage up to 64 list entries: one 64-B record (one cache line) per lane ----
    __syncthreads();
    const int k = base + lane;
    bool rel_lane = false;
    if (k < n) {
      const uint32_t g = a.point_list[range.x + k];
      rel_lane = stage_record(a.splat_a, g, lds_a, lane, reg_x0, reg_x1, reg_y0, reg_y1);
      if constexpr (COORD) {
        const float4* sb = a.splat_b + 3 * (size_t)g;
        lds_b[lane * 3 + 0] = sb[0]; lds_b[lane * 3 + 1] = sb[1]; lds_b[lane * 3 + 2] = sb[2];
      }
    }
    uint64_t rel = __ballot(rel_lane);
    const int niter = (int)__popcll(rel);
    __syncthreads();
    for (int it = 0; it < niter && !all_done; it++) {   // scalar trip count
      const int j = __builtin_ctzll(rel);
      rel &= rel - 1;
      const float4 A = lds_a[j * 4 + 0], B = lds_a[j * 4 + 1];  // {mx,my,cx,cy} {cz,op,thr,ts}
      const float dx = A.x - pixfx;
      const float a_x = (A.z * dx) * dx;
      const float b_xy = A.w * dx;
      float power[PPL];
      bool cand[PPL], anyc = false;
#pragma unroll
      for (int s = 0; s < PPL; s++) {
        const float dy = A.y - pixfy[s];
        power[s] = splat_power(a_x, b_xy, B.x, dy);
        cand[s] = !(power[s] > 0.0f) && !(power[s] < B.z);
        anyc = anyc || cand[s];
      }
      if (__any(anyc)) {  // (no `continue`: a single loop back-edge keeps the per-pixel state in place, no PHI copies)
      const float4 C = lds_a[j * 4 + 2], Dq = lds_a[j * 4 + 3];  // {r,g,b,rpx} {rpy,nx,ny,nz}
      float4 E0, E1, E2;
      if constexpr (COORD) { E0 = lds_b[j * 3 + 0]; E1 = lds_b[j * 3 + 1]; E2 = lds_b[j * 3 + 2]; }
      const uint32_t contributor = (uint32_t)(base + j + 1);
      bool newly_done = false;
#pragma unroll
      for (int s = 0; s < PPL; s++) {
        if (cand[s]) {
          const float G = exp_spec(power[s]);
          const float alpha = fminf(0.99f, B.y * G);
          if (!(alpha < 1.0f / 255.0f)) {
            const float test_T = Tw[s] * (1 - alpha);
            if (test_T < 0.0001f) {
              newly_done = newly_done || (Tw[s] != 0.0f);
              Tw[s] = 0.0f;
            } else {
              const float aT = alpha * T[s];
              const float dy = A.y - pixfy[s];
              Cr[s] = fmaf(C.x, aT, Cr[s]); Cg[s] = fmaf(C.y, aT, Cg[s]); Cb[s] = fmaf(C.z, aT, Cb[s]);
              const bool before_median = T[s] > 0.5f;
              if constexpr (COORD) {
                float c[3];
                coord_planes(E0, E1, E2, dx, dy, c);
                Co[s][0] = fmaf(c[0], aT, Co[s][0]); Co[s][1] = fmaf(c[1], aT, Co[s][1]); Co[s][2] = fmaf(c[2], aT, Co[s][2]);
                if (before_median) { mCo[s][0] = c[0]; mCo[s][1] = c[1]; mCo[s][2] = c[2]; }
              }
              if constexpr (DEPTH) {
                const float t = B.w + fmaf(C.w, dx, Dq.x * dy);
                Dep[s] = fmaf(t, aT, Dep[s]);
                if (before_median) mDep[s] = t;
              }
              if constexpr (NORMAL) {
                Nx[s] = fmaf(Dq.y, aT, Nx[s]); Ny[s] = fmaf(Dq.z, aT, Ny[s]); Nz[s] = fmaf(Dq.w, aT, Nz[s]);
                if (before_median) max_c[s] = contributor;
              }
              weight[s] += aT;
              T[s] = test_T;
              Tw[s] = test_T;
              last_c[s] = contributor;
            }
          }
        }
      }
      if (__any(newly_done)) {
        bool d = true;
#pragma unroll
        for (int s = 0; s < PPL; s++) d = d && (Tw[s] == 0.0f);
        all_done = __all(d);
      }
      }
    }
  }

  // ---- epilogue ----
#pragma unroll
  for (int s = 0; s < PPL; s++) {
    if (!inside[s]) continue;
    // final transmittance: T[s], the running product itself (the stream kernel keeps none and passes 1 - weight: rg_streams.inc)
    blend_fwd_epilogue<COORD, DEPTH>(a, px, py0 + kStripRowStep * s, T[s], last_c[s], max_c[s], Cr[s], Cg[s], Cb[s], weight[s],
                                     Co[COORD ? s : 0], mCo[COORD ? s : 0], Dep[s], mDep[s], Nx[s], Ny[s], Nz[s]);
  }
}

// =========================================================================== blend, bwd ==
// 1/x for x in [0.01, 1]: hardware reciprocal (1 ulp) + one Newton step.  T is recovered back to front as T <- T / (1 - alpha)
// over hundreds of entries (backward.cu:843), so the per-step error compounds; the reference divides exactly (no fast-math in
// its build).  With the refinement the chain is as accurate as an IEEE division at 3 instructions instead of ~10.
__device__ __forceinline__ float rcp_refined(float x) {
  const float r = __builtin_amdgcn_rcpf(x);
  return fmaf(fmaf(-x, r, 1.0f), r, r);
}

struct BlendBwdArgs {
  const uint2* ranges; const uint32_t* point_list; const float4* splat_a; const float4* splat_b;
  int W, H, gx, ntiles; float focal_x, focal_y;
  const float* bg;
  const float* alphas; const float* normalmap;
  const uint32_t* n_contrib; const float* accum_coord; const float* accum_depth; const float* normal_length;
  const float* dL_dpix; const float* dL_dcoord; const float* dL_dmcoord; const float* dL_ddepth; const float* dL_dmdepth;
  const float* dL_dalpha; const float* dL_dnormal;
  float* acc;  // [P][REC] per-Gaussian sums, SplatAcc order
  int P;       // Gaussians (rows of acc)
  const uint32_t* stream_tag;   // ImageState::stream_tag (stream kernels only)
  uint32_t* stream_err;         // mapped host word: set when stream_tag says this buffer holds no entry streams (may be nullptr)
  const uint32_t* blk_base; const uint32_t* blk_consumed; const uint32_t* blk_chunks; const uint32_t* blk_order;   // sub-tile entry streams (rg_streams.inc)
};

typedef float v4f __attribute__((ext_vector_type(4)));

// ---- per-(block, entry) reduction of the 16 per-Gaussian sums over the 16 lanes of a DPP row (round 6) ----
// Rounds 2-5 ran all four butterfly stages on the VALU (24 bank-masked DPP adds + 13 selects / adds = 37 half-rate instructions,
// ~165 of the loop's ~530 issue cycles).  Now only the first stage does: a DPP add with a bank mask only writes the lanes of the
// enabled banks (4 lanes each), so "lanes 0..7 keep components 0..7, lanes 8..15 keep 8..15" is two masked adds per component
// (row_ror:8 pairs lane l with l ^ 8).  The remaining 8 x 8 transposition goes through wave-private LDS: every lane stores its 8
// partial sums (two ds_write_b128), lane l reads component l & 7 of the 8 lanes of its half row (four ds_read2_b32) and adds them
// up with 7 full-rate adds: 16 DPP + 7 adds on the VALU (~90 cycles), 6 LDS instructions that other waves' VALU work covers.
// (All sixteen components through LDS would need 4 KB per wave -- with the staged records 8.7 KB, four waves per SIMD.)
// Layout of a row's 576-byte scratch (144 floats): lane j's 8 sums at float offset (j >> 3) * 72 + (j & 7) * 8, its two 16-byte
// halves swapped when bit 2 of j is set; the +32 bytes per half row and +64 per row put the two half rows and the two rows that share
// an LDS cycle on different banks for the reads, the swap does the same for the eight lanes of a ds_write_b128 group.
constexpr int kRedRowFloats = 144;
__device__ __forceinline__ void row_reduce16_first_stage(float (&v)[16]) {
  asm volatile(
      "s_nop 1\n\t"
      "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %0, %8, %8 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %1, %9, %9 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %2, %10, %10 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %3, %3, %3 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %3, %11, %11 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %4, %4, %4 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %4, %12, %12 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %5, %5, %5 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %5, %13, %13 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %6, %6, %6 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %6, %14, %14 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %7, %7, %7 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %7, %15, %15 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
      "s_nop 1"
      : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])
      : "v"(v[8]), "v"(v[9]), "v"(v[10]), "v"(v[11]), "v"(v[12]), "v"(v[13]), "v"(v[14]), "v"(v[15]));
}
struct RowReduceAddr {   // per lane, set up once per kernel
  float* w0; float* w1;         // where this lane's two 16-byte halves go
  const float* r0; const float* r1;   // component (lane & 7) of source lanes 0..3 / 4..7 of the half row (+ 8 k floats for source k)
};
__device__ __forceinline__ RowReduceAddr row_reduce_addr(float* scratch, int grp, int l) {
  RowReduceAddr a;
  float* row = scratch + grp * kRedRowFloats;
  const int sw = (l >> 2) & 1, c8 = l & 7, half = l >> 3;
  a.w0 = row + half * 72 + c8 * 8 + sw * 4;
  a.w1 = row + half * 72 + c8 * 8 + (sw ^ 1) * 4;
  a.r0 = row + half * 72 + (c8 >> 2) * 4 + (c8 & 3);
  a.r1 = row + half * 72 + ((c8 >> 2) ^ 1) * 4 + (c8 & 3);
  return a;
}
// In: v[c] = this lane's partial sum of component c.  Returns the row total of component (lane & 15).
__device__ __forceinline__ float row_reduce16(float (&v)[16], const RowReduceAddr& ad) {
  row_reduce16_first_stage(v);
  *reinterpret_cast<v4f*>(ad.w0) = v4f{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<v4f*>(ad.w1) = v4f{v[4], v[5], v[6], v[7]};
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float t0 = ad.r0[0], t1 = ad.r0[8], t2 = ad.r0[16], t3 = ad.r0[24];
  const float t4 = ad.r1[32], t5 = ad.r1[40], t6 = ad.r1[48], t7 = ad.r1[56];
  __builtin_amdgcn_wave_barrier();   // the next call's stores stay behind these loads
  return ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7));
}

// One pixel's cotangents as both blend backwards start from them (backward.cu:706-781): the transmittance behind the last entry, the
// cotangent of alpha (dLa, with the normalised maps' 1/alpha^2 terms folded in), the background term tb, and the cotangents of colour
// (dLc), depth and median depth (dLt, dLmt), normal (dLn), coord and median coord (dLco, dLmco), each already divided by what the
// forward's epilogue divided by.  last_c: entries of the list the pixel consumed; max_cm1: 0-based position of its median contributor
// (0xFFFFFFFF, "none", never matches).  Each kernel copies the fields into its own register layout.
struct PixelCotangents {
  float T, dLa, tb, dLc[3], dLt, dLmt, dLn[3], dLco[3], dLmco[3];
  uint32_t last_c, max_cm1;
};
template <bool COORD, bool DEPTH>
__device__ __forceinline__ PixelCotangents pixel_cotangents(const BlendBwdArgs& a, int px, int py) {
  constexpr bool NORMAL = COORD || DEPTH;
  const int W = a.W, H = a.H;
  const size_t HW = (size_t)H * W;
  PixelCotangents o;
  const bool inside = px < W && py < H;
  const size_t pix = inside ? (size_t)W * py + px : 0;
  const float alpha_px = inside ? a.alphas[pix] : 0.f;
  const float T_final = inside ? (1 - alpha_px) : 0.f;
  const float w_final = alpha_px;
  o.T = T_final;
  o.last_c = inside ? a.n_contrib[pix] : 0u;
  o.max_cm1 = (inside ? a.n_contrib[pix + HW] : 0u) - 1u;
  o.dLt = 0.f; o.dLmt = 0.f;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    o.dLc[c] = inside ? a.dL_dpix[c * HW + pix] : 0.f;
    o.dLn[c] = 0.f; o.dLco[c] = 0.f; o.dLmco[c] = 0.f;
  }
  float dla = inside ? a.dL_dalpha[pix] : 0.f;
  o.tb = -T_final * (a.bg[0] * o.dLc[0] + a.bg[1] * o.dLc[1] + a.bg[2] * o.dLc[2]);
  // Pixels nothing blended into (alpha = 0) cannot pass a gradient to any Gaussian; their 1/alpha factors would be inf/NaN and
  // poison the wave-wide sums through the multiplicative masks, so their geometry cotangents stay zero.
  if (NORMAL && inside && o.last_c > 0) {
    const float ww = w_final * w_final;
    const float pnx = ((float)px - W / 2.f) / a.focal_x;
    const float pny = ((float)py - H / 2.f) / a.focal_y;
    const float ln = sqrtf(pnx * pnx + pny * pny + 1);
    if constexpr (COORD) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float gw = a.dL_dcoord[c * HW + pix];
        dla -= gw * a.accum_coord[c * HW + pix] / ww;
        o.dLco[c] = gw / w_final;
        o.dLmco[c] = a.dL_dmcoord[c * HW + pix];
      }
    }
    if constexpr (DEPTH) {
      const float gw = a.dL_ddepth[pix];
      dla -= gw * a.accum_depth[pix] / ww;
      o.dLt = gw / w_final / ln;
      o.dLmt = a.dL_dmdepth[pix] / ln;
    }
    {
      const float g0 = a.dL_dnormal[pix], g1 = a.dL_dnormal[HW + pix], g2 = a.dL_dnormal[2 * HW + pix];
      const float n0 = a.normalmap[pix], n1 = a.normalmap[HW + pix], n2 = a.normalmap[2 * HW + pix];
      const float nlen = a.normal_length[pix];
      if (nlen < 1.0E-12F) {
        o.dLn[0] = g0 / 1.0E-12F; o.dLn[1] = g1 / 1.0E-12F; o.dLn[2] = g2 / 1.0E-12F;
      } else {
        const float dt = g0 * n0 + g1 * n1 + g2 * n2;
        o.dLn[0] = (g0 - dt * n0) / nlen; o.dLn[1] = (g1 - dt * n1) / nlen; o.dLn[2] = (g2 - dt * n2) / nlen;
      }
    }
  }
  o.dLa = dla;
  return o;
}

// ------------------------------------------------------------------ blend, bwd (packed) ----
// Second formulation of the same backward: the pixels of one lane are handled in PAIRS as 2-wide
// fp32 vectors (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 do two pixels per issue slot), and a
// pixel that does not take part in an entry is switched off with two selects (alpha := 0, G := 0)
// instead of a divergent branch: with alpha = 0 every recurrence below is an exact no-op
// (T*rcp(1) = T, acc + 0*d = acc) and every gradient term is 0.  The only branches left are
// wave-uniform, so the pair bodies are straight-line code the scheduler can interleave.
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 bc2(float v) { return f2{v, v}; }

// second launch-bound = waves per SIMD the register allocator must leave room for
template <bool COORD, bool DEPTH, int PPL>
__global__ void __launch_bounds__(64, (COORD ? (PPL == 4 ? 1 : 2) : (PPL == 4 ? 2 : 5))) blend_bwd_packed_kernel(const BlendBwdArgs a) {
  static_assert(PPL == 2 || PPL == 4, "pairs of pixels per lane");
  // the wave's totals of an entry are ADDED to the Gaussian's record: the order in which the tiles' waves arrive is the scheduler's
#define RG_BLEND_BWD_SINK(total_) unsafeAtomicAdd(a.acc + (size_t)gid * REC + lane, total_)
#include "rg_blend_bwd_body.inc"
#undef RG_BLEND_BWD_SINK
}

// The deterministic backward's blend (radegs_backward_ordered, include/radegs.h): one wave per tile (the PPL == 4 geometry), and a.acc is the
// PARTIAL-record array [R][REC], not the accumulator -- the wave's totals of an entry are STORED as the record of the entry's position in
// point_list.  One writer per record; the records of entries a wave skips or never reaches keep the zeros the launcher filled in.
// ordered_sums_kernel then adds every Gaussian's partial records in ascending position.
template <bool COORD, bool DEPTH>
__global__ void __launch_bounds__(64, (COORD ? 1 : 2)) blend_bwd_ordered_kernel(const BlendBwdArgs a) {
  constexpr int PPL = 4;
#define RG_BLEND_BWD_SINK(total_) a.acc[((size_t)range.x + pos) * REC + lane] = (total_)
#include "rg_blend_bwd_body.inc"
#undef RG_BLEND_BWD_SINK
}

// Fixed-order segment sum: one group of REC lanes per Gaussian finds its run [lo, hi) in the sorted keys (lower / upper bound), lane c adds
// component c of the run's partial records in ascending k -- ascending position in point_list, i.e. tile order, then depth order, because the
// sort is stable -- with plain fp32 adds from 0.0f, and stores the record.  The order is a function of point_list alone.
template <int REC>
__global__ void __launch_bounds__(256) ordered_sums_kernel(int P, uint32_t R, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ pos,
                                                          const float* __restrict__ part, float* __restrict__ acc) {
  const size_t gi = ((size_t)blockIdx.x * 256u + threadIdx.x) / REC;
  if (gi >= (size_t)P) return;
  const uint32_t g = (uint32_t)gi, c = threadIdx.x % REC;
  uint32_t lo = 0, n = R;
  while (n > 0) {  // first k with keys[k] >= g
    const uint32_t h = n >> 1;
    if (keys[lo + h] < g) { lo += h + 1; n -= h + 1; } else n = h;
  }
  uint32_t hi = lo;
  n = R - lo;
  while (n > 0) {  // first k with keys[k] > g
    const uint32_t h = n >> 1;
    if (keys[hi + h] <= g) { hi += h + 1; n -= h + 1; } else n = h;
  }
  float s = 0.0f;
  for (uint32_t k = lo; k < hi; k++) s += part[(size_t)pos[k] * REC + c];
  acc[(size_t)g * REC + c] = s;
}

}  // namespace rg

// The blend kernels over sub-tile entry streams use the helpers above.
#include "rg_streams.inc"

// The host-side orchestration and the C ABI (include/radegs.h) follow; they need the kernels above in scope.
#include "rg_launch.inc"
