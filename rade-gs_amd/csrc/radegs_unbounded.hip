// radegs_unbounded.hip -- unbounded mesh extraction: the reference's GaussianExtractor.extract_mesh_unbounded
// (utils/mesh_utils.py:162-270 with utils/mcube_utils.py), which upstream runs as ~20 eager kernels per view and chunk plus a marching
// cubes on the host.
//     fuse                 fuse_kernel<CONTRACT, RGB, BRICK>: one thread per sample, all views in one launch, the running average in registers
//     after the weld       uncontract_kernel
//     dense marching cubes densemc_count_kernel -> two scans -> densemc_emit_kernel
//
// The specification is include/radegs.h, "Unbounded mesh extraction"; tests/unbounded_restatement.py restates it in NumPy float32 and the
// kernels are held to that bit for bit.  -ffp-contract=off: one rounding per operation, products before sums, as numpy evaluates them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_mc_tables.h"
#include "rg_prims.h"
#include "rg_workspace.h"

namespace rgub {

using rg::blocks_of;

struct Frame {   // contraction: x = uncontract(y) radius + center
  float radius, cx, cy, cz;
};

__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

__device__ __forceinline__ void uncontract(float& x, float& y, float& z, const Frame& f) {
  const float mag = norm3(x, y, z);
  if (!(mag < 1.0f)) {
    const float inv = 1.0f / (2.0f - mag);
    x = inv * (x / mag);
    y = inv * (y / mag);
    z = inv * (z / mag);
  }
  x = x * f.radius + f.cx;
  y = y * f.radius + f.cy;
  z = z * f.radius + f.cz;
}

// bilinear, align_corners, border padding, at the clamped pixel coordinates (ix, iy): the order of torch's grid_sample
__device__ __forceinline__ float gather(const float* __restrict__ img, int W, int H, float ix, float iy) {
  const float x0f = floorf(ix), y0f = floorf(iy), x1f = x0f + 1.0f, y1f = y0f + 1.0f;
  int x0 = (int)x0f, y0 = (int)y0f;
  x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0);   // already so for every finite (ix, iy); keeps the address inside the map whatever comes
  y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
  const float nw = (x1f - ix) * (y1f - iy), ne = (ix - x0f) * (y1f - iy), sw = (x1f - ix) * (iy - y0f), se = (ix - x0f) * (iy - y0f);
  const bool xin = x0 + 1 < W, yin = y0 + 1 < H;
  const float* row0 = img + (size_t)y0 * W;
  float out = 0.0f;
  out = out + row0[x0] * nw;
  if (xin) out = out + row0[x0 + 1] * ne;
  if (yin) {
    const float* row1 = row0 + W;
    out = out + row1[x0] * sw;
    if (xin) out = out + row1[x0 + 1] * se;
  }
  return out;
}

// Explicit mode (samples != nullptr): thread = sample.  Lattice mode: sample (lx * ny + ly) * nz + lz at (ax[lx], ay[ly], az[lz]);
// BRICK false: thread = sample index (a wave is a run along z: full-line stores); BRICK true: a wave is a 4 x 4 x 4 brick (its projections
// form a compact patch of each map; 16-byte store segments).  The results do not depend on the mapping.
template <bool CONTRACT, bool RGB, bool BRICK>
__global__ void __launch_bounds__(256) fuse_kernel(long long M, const float* __restrict__ samples, const float* __restrict__ ax, const float* __restrict__ ay,
                                                   const float* __restrict__ az, int nx, int ny, int nz, int V,
                                                   const RadegsUnboundedView* __restrict__ views, Frame frame, float trunc5,
                                                   float* __restrict__ out_tsdf, float* __restrict__ out_rgb) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  long long m;
  float x, y, z;
  bool live;
  if (samples) {
    m = t;
    live = m < M;
    if (live) {
      x = samples[3 * m];
      y = samples[3 * m + 1];
      z = samples[3 * m + 2];
    }
  } else {
    int lx, ly, lz;
    if (BRICK) {
      const int bz = (nz + 3) >> 2, by = (ny + 3) >> 2;
      const long long brick = t >> 6;
      const int lane = (int)(t & 63);
      lz = (int)(brick % bz) * 4 + (lane & 3);
      ly = (int)((brick / bz) % by) * 4 + ((lane >> 2) & 3);
      lx = (int)(brick / ((long long)bz * by)) * 4 + (lane >> 4);
      live = lx < nx && ly < ny && lz < nz;
    } else {
      lz = (int)(t % nz);
      ly = (int)((t / nz) % ny);
      lx = (int)(t / ((long long)nz * ny));
      live = t < M;
    }
    m = ((long long)lx * ny + ly) * nz + lz;
    if (live) {
      x = ax[lx];
      y = ay[ly];
      z = az[lz];
    }
  }
  if (!live) x = y = z = __builtin_nanf("");   // never in view: the lane only takes part in the ballots
  float trunc = trunc5;
  if (CONTRACT) {
    uncontract(x, y, z, frame);
    const float n = norm3(x, y, z);
    if (n > 1.0f) trunc = trunc5 * (1.0f / (2.0f - fminf(n, 1.9f)));
  }
  float tsdf = 1.0f, w = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f;
  for (int v = 0; v < V; v++) {
    const RadegsUnboundedView& vw = views[v];   // wave-uniform: scalar loads
    const int W = vw.W, H = vw.H;
    const float* __restrict__ depth = vw.depth;
    if (W < 1 || H < 1 || !depth) continue;
    const float qx = ((x * vw.m[0] + y * vw.m[4]) + z * vw.m[8]) + vw.m[12];
    const float qy = ((x * vw.m[1] + y * vw.m[5]) + z * vw.m[9]) + vw.m[13];
    const float qw = ((x * vw.m[3] + y * vw.m[7]) + z * vw.m[11]) + vw.m[15];
    const float px = qx / qw, py = qy / qw;
    const bool inview = px > -1.0f && px < 1.0f && py > -1.0f && py < 1.0f && qw > 0.0f;
    if (__ballot(inview) == 0ull) continue;     // no lane of the wave sees this view: none of its lines is touched
    if (!inview) continue;
    const float ix = fminf(fmaxf(((px + 1.0f) / 2.0f) * (float)(W - 1), 0.0f), (float)(W - 1));
    const float iy = fminf(fmaxf(((py + 1.0f) / 2.0f) * (float)(H - 1), 0.0f), (float)(H - 1));
    const float sdf = gather(depth, W, H, ix, iy) - qw;
    if (!(sdf > -trunc)) continue;
    const float s = fminf(fmaxf(sdf / trunc, -1.0f), 1.0f);
    const float wp = w + 1.0f;
    tsdf = (tsdf * w + s) / wp;
    if (RGB) {
      const float* __restrict__ rgb = vw.rgb;
      if (rgb) {
        const size_t plane = (size_t)W * H;
        r = (r * w + gather(rgb, W, H, ix, iy)) / wp;
        g = (g * w + gather(rgb + plane, W, H, ix, iy)) / wp;
        b = (b * w + gather(rgb + 2 * plane, W, H, ix, iy)) / wp;
      }
    }
    w = wp;
  }
  if (!live) return;
  out_tsdf[m] = tsdf;
  if (RGB) {
    out_rgb[3 * m] = r;
    out_rgb[3 * m + 1] = g;
    out_rgb[3 * m + 2] = b;
  }
}

__global__ void __launch_bounds__(256) uncontract_kernel(long long M, const float* __restrict__ in, Frame frame, float max_range, float* __restrict__ out) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float p[3] = {in[3 * m], in[3 * m + 1], in[3 * m + 2]};
  uncontract(p[0], p[1], p[2], frame);
#pragma unroll
  for (int k = 0; k < 3; k++) out[3 * m + k] = p[k] < -max_range ? -max_range : (p[k] > max_range ? max_range : p[k]);   // NaN stays NaN
}

// ------------------------------------------------------------------- dense marching cubes -------------------------------------------------------------------
// One thread per lattice point m = (lx * ny + ly) * nz + lz.  info[m]: which of the point's owned edges (+x, +y, +z) are cut (bits 0-2) and how
// many triangles the cell with this lowest corner yields (bits 3-5).
__device__ __forceinline__ int case_of(const float* __restrict__ v, long long m, int ny, int nz) {
  int cs = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) cs |= (v[m + ((long long)(k & 1) * ny + ((k >> 1) & 1)) * nz + (k >> 2)] < 0.0f ? 1 : 0) << k;
  return cs;
}

__global__ void __launch_bounds__(256) densemc_count_kernel(const float* __restrict__ values, int nx, int ny, int nz, uint8_t* __restrict__ info,
                                                            uint32_t* __restrict__ nv, uint32_t* __restrict__ nt) {
  const long long n = (long long)nx * ny * nz, m = (long long)blockIdx.x * 256 + threadIdx.x;
  if (m >= n) return;
  const int lz = (int)(m % nz), ly = (int)((m / nz) % ny), lx = (int)(m / ((long long)nz * ny));
  const bool o = values[m] < 0.0f;
  uint32_t mask = 0;
  if (lx + 1 < nx && o != (values[m + (long long)ny * nz] < 0.0f)) mask |= 1u;
  if (ly + 1 < ny && o != (values[m + nz] < 0.0f)) mask |= 2u;
  if (lz + 1 < nz && o != (values[m + 1] < 0.0f)) mask |= 4u;
  uint32_t tris = 0;
  if (lx + 1 < nx && ly + 1 < ny && lz + 1 < nz) tris = kMcNumTris[case_of(values, m, ny, nz)];
  info[m] = (uint8_t)(mask | (tris << 3));
  nv[m] = __popc(mask);
  nt[m] = tris;
}

__global__ void densemc_totals_kernel(long long n, const uint32_t* __restrict__ nv_incl, const uint32_t* __restrict__ nt_incl, long long* __restrict__ counts2) {
  counts2[0] = nv_incl[n - 1];
  counts2[1] = nt_incl[n - 1];
}

__global__ void __launch_bounds__(256) densemc_emit_kernel(const float* __restrict__ values, const float* __restrict__ ax, const float* __restrict__ ay,
                                                           const float* __restrict__ az, int nx, int ny, int nz, int ox, int oy, int oz, long long G,
                                                           const uint8_t* __restrict__ info, const uint32_t* __restrict__ nv_incl,
                                                           const uint32_t* __restrict__ nt_incl, uint32_t V, uint32_t F, float* __restrict__ vertices,
                                                           long long* __restrict__ keys, long long* __restrict__ faces) {
  const long long n = (long long)nx * ny * nz, m = (long long)blockIdx.x * 256 + threadIdx.x;
  if (m >= n) return;
  const int lz = (int)(m % nz), ly = (int)((m / nz) % ny), lx = (int)(m / ((long long)nz * ny));
  const uint32_t inf = info[m], mask = inf & 7u, tris = inf >> 3;
  if (mask) {
    uint32_t id = nv_incl[m] - __popc(mask);
    const float v_o = values[m];
    const float c[3] = {ax[lx], ay[ly], az[lz]};
    const long long key0 = ((((long long)(ox + lx)) * G + (oy + ly)) * G + (oz + lz)) * 3;
    for (int a = 0; a < 3; a++) {
      if (!(mask >> a & 1u)) continue;
      if (id >= V) break;
      const float v_e = values[m + (a == 0 ? (long long)ny * nz : (a == 1 ? nz : 1))];
      const float c_e = a == 0 ? ax[lx + 1] : (a == 1 ? ay[ly + 1] : az[lz + 1]);
      const float t = (0.0f - v_o) / (v_e - v_o);
#pragma unroll
      for (int k = 0; k < 3; k++) vertices[3 * (size_t)id + k] = k == a ? c[k] + t * (c_e - c[k]) : c[k];
      keys[id] = key0 + a;
      id++;
    }
  }
  if (tris) {
    const int cs = case_of(values, m, ny, nz);
    uint32_t fid = nt_incl[m] - tris;
    for (uint32_t t = 0; t < tris && t < RG_MC_MAX_TRIS; t++, fid++) {
      if (fid >= F) break;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int e = kMcTriTable[cs][3 * t + k];
        long long id = -1;
        if (e >= 0) {
          const long long om = m + ((long long)kMcEdgeInfo[e][0] * ny + kMcEdgeInfo[e][1]) * nz + kMcEdgeInfo[e][2];   // a corner of this cell
          const uint32_t oi = info[om] & 7u, axis = kMcEdgeInfo[e][3];
          id = (long long)(nv_incl[om] - __popc(oi)) + __popc(oi & ((1u << axis) - 1u));
        }
        faces[3 * (size_t)fid + k] = id;
      }
    }
  }
}

struct McView {
  uint8_t* info;
  uint32_t *nv, *nt, *nv_incl, *nt_incl;
  void* temp;
  size_t temp_bytes, bytes;
};
static McView mc_carve(long long N, void* base) {
  const size_t n = (size_t)N;
  rg::Carver c(base);
  McView v;
  v.temp_bytes = rg::scan_temp_bytes(n);
  v.info = c.take<uint8_t>(n);
  for (uint32_t** a : {&v.nv, &v.nt, &v.nv_incl, &v.nt_incl}) *a = c.take<uint32_t>(n);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}
// the number of lattice points, 0 when the lattice is refused: an axis shorter than 2, or more points than the scans address
static long long mc_points(int nx, int ny, int nz) {
  if (nx < 2 || ny < 2 || nz < 2) return 0;
  const long long n = (long long)nx * ny * nz;   // < 2^93 cannot be: three ints below 2^31 -- checked in steps
  if ((long long)nx * ny >= (1ll << 31) || n >= (1ll << 31)) return 0;
  return n;
}
static bool finite_positive(float v) { return v > 0.0f && isfinite(v); }

template <bool CONTRACT, bool RGB>
static void launch_fuse(bool brick, unsigned blocks, hipStream_t s, long long M, const float* samples, const float* ax, const float* ay, const float* az, int nx,
                        int ny, int nz, int V, const RadegsUnboundedView* views, Frame frame, float trunc5, float* tsdf, float* rgb) {
  if (brick)
    hipLaunchKernelGGL((fuse_kernel<CONTRACT, RGB, true>), dim3(blocks), dim3(256), 0, s, M, samples, ax, ay, az, nx, ny, nz, V, views, frame, trunc5, tsdf, rgb);
  else
    hipLaunchKernelGGL((fuse_kernel<CONTRACT, RGB, false>), dim3(blocks), dim3(256), 0, s, M, samples, ax, ay, az, nx, ny, nz, V, views, frame, trunc5, tsdf, rgb);
}

}  // namespace rgub

extern "C" {

int radegs_unbounded_fuse(long long M, const float* samples, const float* ax, const float* ay, const float* az, int nx, int ny, int nz, int mapping, int V,
                          const RadegsUnboundedView* views, int contract, float radius, const float* center3, float trunc5, float* tsdf, float* rgb,
                          void* stream) {
  if (M < 0 || V < 0 || (V && !views) || !center3 || !rgub::finite_positive(trunc5) || (mapping != RADEGS_UNBOUNDED_ZRUN && mapping != RADEGS_UNBOUNDED_BRICK))
    return RADEGS_ERR_INVALID_ARG;
  if (contract && !rgub::finite_positive(radius)) return RADEGS_ERR_INVALID_ARG;
  const bool lattice = samples == nullptr;
  if (lattice) {
    if (nx < 1 || ny < 1 || nz < 1 || !ax || !ay || !az) return RADEGS_ERR_INVALID_ARG;
    if ((long long)nx * ny >= (1ll << 31) || (long long)nx * ny * nz >= (1ll << 31)) return RADEGS_ERR_TOO_LARGE;
    if (M != (long long)nx * ny * nz) return RADEGS_ERR_INVALID_ARG;
  }
  if (M >= (1ll << 31)) return RADEGS_ERR_TOO_LARGE;
  if (M == 0) return 0;
  if (!tsdf) return RADEGS_ERR_INVALID_ARG;
  const bool brick = lattice && mapping == RADEGS_UNBOUNDED_BRICK;
  const long long threads = brick ? 64ll * ((nx + 3) / 4) * ((ny + 3) / 4) * ((nz + 3) / 4) : M;
  const unsigned blocks = rg::blocks_of((size_t)threads);
  const rgub::Frame f = {radius, center3[0], center3[1], center3[2]};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (contract) {
    if (rgb) rgub::launch_fuse<true, true>(brick, blocks, s, M, samples, ax, ay, az, nx, ny, nz, V, views, f, trunc5, tsdf, rgb);
    else rgub::launch_fuse<true, false>(brick, blocks, s, M, samples, ax, ay, az, nx, ny, nz, V, views, f, trunc5, tsdf, rgb);
  } else {
    if (rgb) rgub::launch_fuse<false, true>(brick, blocks, s, M, samples, ax, ay, az, nx, ny, nz, V, views, f, trunc5, tsdf, rgb);
    else rgub::launch_fuse<false, false>(brick, blocks, s, M, samples, ax, ay, az, nx, ny, nz, V, views, f, trunc5, tsdf, rgb);
  }
  return rg::launch_status();
}

int radegs_unbounded_uncontract(long long M, const float* contracted, float radius, const float* center3, float max_range, float* world, void* stream) {
  if (M < 0 || !center3 || !rgub::finite_positive(radius) || !(max_range > 0.0f)) return RADEGS_ERR_INVALID_ARG;
  if (M >= (1ll << 31)) return RADEGS_ERR_TOO_LARGE;
  if (M == 0) return 0;
  if (!contracted || !world) return RADEGS_ERR_INVALID_ARG;
  const rgub::Frame f = {radius, center3[0], center3[1], center3[2]};
  hipLaunchKernelGGL(rgub::uncontract_kernel, dim3(rg::blocks_of((size_t)M)), dim3(256), 0, static_cast<hipStream_t>(stream), M, contracted, f, max_range, world);
  return rg::launch_status();
}

size_t radegs_densemc_bytes(int nx, int ny, int nz) {
  const long long n = rgub::mc_points(nx, ny, nz);
  return n ? rgub::mc_carve(n, nullptr).bytes : 0;
}

int radegs_densemc_plan(const float* values, int nx, int ny, int nz, void* workspace, size_t workspace_bytes, long long* counts2, void* stream_v) {
  const long long n = rgub::mc_points(nx, ny, nz);
  if (!n || !values || !counts2 || !workspace || workspace_bytes < radegs_densemc_bytes(nx, ny, nz) || !rg::aligned16(workspace)) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const rgub::McView w = rgub::mc_carve(n, workspace);
  hipLaunchKernelGGL(rgub::densemc_count_kernel, dim3(rg::blocks_of((size_t)n)), dim3(256), 0, s, values, nx, ny, nz, w.info, w.nv, w.nt);
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, w.nv, nullptr, w.nv_incl, (size_t)n, s) != hipSuccess) return RADEGS_ERR_HIP;
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, w.nt, nullptr, w.nt_incl, (size_t)n, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgub::densemc_totals_kernel, dim3(1), dim3(1), 0, s, n, w.nv_incl, w.nt_incl, counts2);
  return rg::launch_status();
}

int radegs_densemc_emit(const float* values, const float* ax, const float* ay, const float* az, int nx, int ny, int nz, const int* offset3, long long G,
                        const void* workspace, long long V, long long F, float* vertices, long long* keys, long long* faces, void* stream) {
  const long long n = rgub::mc_points(nx, ny, nz);
  if (!n || V < 0 || F < 0 || !offset3 || G < 1 || G > (1ll << 20)) return RADEGS_ERR_INVALID_ARG;
  if (offset3[0] < 0 || offset3[1] < 0 || offset3[2] < 0 || offset3[0] + (long long)nx > G || offset3[1] + (long long)ny > G || offset3[2] + (long long)nz > G)
    return RADEGS_ERR_INVALID_ARG;
  if (V >= 0xFFFFFFFFll || F >= 0xFFFFFFFFll) return RADEGS_ERR_TOO_LARGE;
  if (V == 0 && F == 0) return 0;
  if (!values || !ax || !ay || !az || !workspace || (V && (!vertices || !keys)) || (F && !faces)) return RADEGS_ERR_INVALID_ARG;
  const rgub::McView w = rgub::mc_carve(n, const_cast<void*>(workspace));
  hipLaunchKernelGGL(rgub::densemc_emit_kernel, dim3(rg::blocks_of((size_t)n)), dim3(256), 0, static_cast<hipStream_t>(stream), values, ax, ay, az, nx, ny, nz,
                     offset3[0], offset3[1], offset3[2], G, w.info, w.nv_incl, w.nt_incl, (uint32_t)V, (uint32_t)F, vertices, keys, faces);
  return rg::launch_status();
}

}  // extern "C"
