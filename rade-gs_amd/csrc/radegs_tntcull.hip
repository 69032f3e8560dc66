// radegs_tntcull.hip -- Tanks-and-Temples mesh culling: eval_tnt/cull_mesh.py, the step between the marching-tetrahedra mesh
// and eval_tnt/run.py, which upstream hands to pyrender / EGL and to eager torch.
//     cull_mesh.py:17-66     extract_depth_from_mesh: one depth map per camera      setup_kernel (one lane per triangle and view: transform,
//                                                                                   near clip, reject, walk a small box in place, queue a large
//                                                                                   one in chunks), drain_kernel (one workgroup per chunk),
//                                                                                   resolve_kernel (untouched pixels read 0)
//     cull_mesh.py:96-183    Mesher.point_masks at forecast_radius = 0              count_views_kernel (one lane per point, all cameras of a batch)
// Face filtering and renumbering are radegs_tetmesh_filter_plan_flags / _apply.
//
// The specification is include/radegs.h, "Tanks-and-Temples mesh culling", and DESIGN.md 11 N11; tests/tntcull_restatement.py restates it in
// NumPy.  The rasterizer is fp64 and -ffp-contract=off: every coverage decision is the sign of a difference of two rounded products, evaluated
// from the same end point of an edge whichever triangle owns it, so two triangles that share an edge see exactly opposite values and no pixel
// centre falls between them.  Depth is merged with a 32-bit unsigned atomic minimum on the float's bits (positive floats order as their bits
// do): the map does not depend on the order of the faces, bit for bit.  The vertex test is fp32, as upstream's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_workspace.h"

namespace rgtc {

using rg::blocks_of;
constexpr int kSmallBox = 256;           // boxes of at most this many pixel centres are walked by the lane that set the triangle up
constexpr int kChunk = 1024;             // pixel centres of a queued box one workgroup of drain_kernel covers
constexpr int kDrainBlocks = 8192;
constexpr int kMaxViews = 65535;         // gridDim.y
constexpr int kMaxSide = 32768;          // H, W: a box holds at most 2^30 pixel centres
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr size_t kDefaultQueue = size_t(1) << 20;

struct Raster {
  int H, W;
  double fx, fy, cx, cy, znear, zfar;
};

struct Entry {
  uint32_t face, view_sub, chunk, pad;   // view_sub = view << 1 | which triangle of the clipped polygon's fan
};

// header words of the workspace: the queue's counter, then the statistics the bench reads
enum { kCount = 0, kSmall = 1, kQueued = 2, kOverflow = 3, kHeaderWords = 8 };

struct View {
  unsigned long long* header;
  Entry* queue;
  size_t bytes;
};

inline View carve(size_t entries, void* base) {
  rg::Carver c(base);
  View v;
  v.header = c.take<unsigned long long>(kHeaderWords);
  v.queue = c.take<Entry>(entries);
  v.bytes = c.off;
  return v;
}

// ------------------------------------------------------------------ triangle set-up ------------------------------------------------------------------
struct Vtx {
  double X, Y, d;   // camera space, d = -z
};

struct Edge {
  double ax, ay, dx, dy;   // from the end point that is smaller in (x, then y)
  bool flip;               // the triangle walks the edge the other way: negate
};

struct Tri {
  Edge e0, e1, e2;         // opposite vertex 0, 1, 2
  double d0, d1, d2;
  bool neg;                // clockwise in window space: negate all three
  int jlo, ilo, bw, bh;    // the box of pixel centres; bw <= 0: nothing to draw
};

__device__ __forceinline__ bool lex_less(const Vtx& a, const Vtx& b) {
  if (a.X != b.X) return a.X < b.X;
  if (a.Y != b.Y) return a.Y < b.Y;
  return a.d < b.d;
}

// where the edge meets d = znear, always from the lexicographically smaller end
__device__ __forceinline__ Vtx meet(Vtx a, Vtx b, double znear) {
  if (lex_less(b, a)) {
    const Vtx t = a;
    a = b;
    b = t;
  }
  const double t = (znear - a.d) / (b.d - a.d);
  Vtx r;
  r.X = a.X + t * (b.X - a.X);
  r.Y = a.Y + t * (b.Y - a.Y);
  r.d = znear;
  return r;
}

// Sutherland-Hodgman against d >= znear, vertex order kept, written out per case (no indexed array: nothing in scratch); returns the polygon's
// vertex count: 0, 3 or 4.  Walking 0 -> 1 -> 2 -> 0, a kept vertex is emitted, then the meeting point of an edge that changes side.
__device__ __forceinline__ int clip_near(const Vtx& v0, const Vtx& v1, const Vtx& v2, double znear, Vtx& q0, Vtx& q1, Vtx& q2, Vtx& q3) {
  const int mask = (v0.d >= znear ? 1 : 0) | (v1.d >= znear ? 2 : 0) | (v2.d >= znear ? 4 : 0);
  q0 = v0, q1 = v1, q2 = v2, q3 = v2;
  if (mask == 7) return 3;
  if (mask == 0) return 0;
  const Vtx m01 = meet(v0, v1, znear), m12 = meet(v1, v2, znear), m20 = meet(v2, v0, znear);   // the one between two ends of one side is not used
  switch (mask) {
    case 1: q1 = m01, q2 = m20; return 3;                       // v0, 01, 20
    case 2: q0 = m01, q2 = m12; return 3;                       // 01, v1, 12
    case 4: q0 = m12, q1 = v2, q2 = m20; return 3;              // 12, v2, 20
    case 6: q0 = m01, q1 = v1, q2 = v2, q3 = m20; return 4;     // 01, v1, v2, 20
    case 5: q1 = m01, q2 = m12, q3 = v2; return 4;              // v0, 01, 12, v2
    default: q2 = m12, q3 = m20; return 4;                      // 3: v0, v1, 12, 20
  }
}

__device__ __forceinline__ Edge make_edge(double ax, double ay, double bx, double by) {
  Edge e;
  e.flip = bx < ax || (bx == ax && by < ay);
  if (e.flip) {
    e.ax = bx, e.ay = by, e.dx = ax - bx, e.dy = ay - by;
  } else {
    e.ax = ax, e.ay = ay, e.dx = bx - ax, e.dy = by - ay;
  }
  return e;
}

__device__ __forceinline__ double edge_value(const Edge& e, double px, double py) {
  const double v = e.dx * (py - e.ay) - e.dy * (px - e.ax);
  return e.flip ? -v : v;
}

__device__ __forceinline__ Tri make_tri(const Raster& R, const Vtx& a, const Vtx& b, const Vtx& c) {
  Tri t;
  const double x0 = R.fx * a.X / a.d + R.cx, y0 = R.cy - R.fy * a.Y / a.d;
  const double x1 = R.fx * b.X / b.d + R.cx, y1 = R.cy - R.fy * b.Y / b.d;
  const double x2 = R.fx * c.X / c.d + R.cx, y2 = R.cy - R.fy * c.Y / c.d;
  t.e0 = make_edge(x1, y1, x2, y2);
  t.e1 = make_edge(x2, y2, x0, y0);
  t.e2 = make_edge(x0, y0, x1, y1);
  t.d0 = a.d, t.d1 = b.d, t.d2 = c.d;
  const double area = edge_value(t.e2, x2, y2);
  t.neg = area < 0.0;
  // the pixel centres (j + 0.5, i + 0.5) inside the closed bounding box; every comparison is false for NaN, which leaves the box empty
  const double jlo = fmax(ceil(fmin(fmin(x0, x1), x2) - 0.5), 0.0), jhi = fmin(floor(fmax(fmax(x0, x1), x2) - 0.5), (double)(R.W - 1));
  const double ilo = fmax(ceil(fmin(fmin(y0, y1), y2) - 0.5), 0.0), ihi = fmin(floor(fmax(fmax(y0, y1), y2) - 0.5), (double)(R.H - 1));
  const bool draw = (area < 0.0 || area > 0.0) && jlo <= jhi && ilo <= ihi;
  t.jlo = draw ? (int)jlo : 0;
  t.ilo = draw ? (int)ilo : 0;
  t.bw = draw ? (int)jhi - t.jlo + 1 : 0;
  t.bh = draw ? (int)ihi - t.ilo + 1 : 0;
  return t;
}

// one pixel centre: covered iff the three oriented edge values are >= 0; 1/d is affine in window space
__device__ __forceinline__ void shade(const Raster& R, const Tri& t, int i, int j, uint32_t* __restrict__ map) {
  const double px = (double)j + 0.5, py = (double)i + 0.5;
  double E0 = edge_value(t.e0, px, py), E1 = edge_value(t.e1, px, py), E2 = edge_value(t.e2, px, py);
  if (t.neg) E0 = -E0, E1 = -E1, E2 = -E2;
  if (!(E0 >= 0.0 && E1 >= 0.0 && E2 >= 0.0)) return;
  const double sum = (E0 + E1) + E2;
  if (!(sum > 0.0)) return;
  const double d = sum / ((E0 / t.d0 + E1 / t.d1) + E2 / t.d2);
  if (!(d >= R.znear && d <= R.zfar)) return;
  const uint32_t bits = __float_as_uint((float)d);
  uint32_t* cell = map + (size_t)i * R.W + j;
  if (bits < *cell) atomicMin(cell, bits);   // a stale read is only ever too large: the minimum is never skipped
}

// the triangle `sub` of the fan of face f's clipped polygon, as view `cam` sees it; false: there is none
__device__ __forceinline__ bool face_tri(const Raster& R, long long V, const double* __restrict__ vertices, const long long* __restrict__ faces,
                                         const double* __restrict__ cam, long long f, int sub, Tri& t, int& n_out) {
  const long long ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  n_out = 0;
  if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) return false;   // the Python layer refuses such input; a C caller gets no wild read
  const long long idx[3] = {ia, ib, ic};
  Vtx p[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double x = vertices[3 * idx[k]], y = vertices[3 * idx[k] + 1], z = vertices[3 * idx[k] + 2];
    p[k].X = ((cam[0] * x + cam[1] * y) + cam[2] * z) + cam[3];
    p[k].Y = ((cam[4] * x + cam[5] * y) + cam[6] * z) + cam[7];
    p[k].d = -(((cam[8] * x + cam[9] * y) + cam[10] * z) + cam[11]);
  }
  Vtx q0, q1, q2, q3;
  const int n = clip_near(p[0], p[1], p[2], R.znear, q0, q1, q2, q3);
  n_out = n;
  if (n < 3 || (sub == 1 && n < 4)) return false;
  t = sub == 0 ? make_tri(R, q0, q1, q2) : make_tri(R, q0, q2, q3);
  return t.bw > 0;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(256) clear_kernel(size_t n, uint32_t* __restrict__ map) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) map[i] = kEmpty;
}

__global__ void __launch_bounds__(256) resolve_kernel(size_t n, uint32_t* __restrict__ map) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && map[i] == kEmpty) map[i] = 0u;
}

// One lane per (face, view).  No lane leaves early: the statistics are summed over the wave at the end.
__global__ void __launch_bounds__(256) setup_kernel(Raster R, long long V, long long F, const double* __restrict__ vertices,
                                                    const long long* __restrict__ faces, const double* __restrict__ cams, uint32_t* __restrict__ maps,
                                                    unsigned long long* __restrict__ header, Entry* __restrict__ queue, unsigned long long capacity) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  const int view = blockIdx.y;
  uint32_t* map = maps + (size_t)view * R.H * R.W;
  unsigned long long n_small = 0, n_queued = 0, n_over = 0;
  if (f < F) {
    for (int sub = 0; sub < 2; sub++) {
      Tri t;
      int n;
      const bool draw = face_tri(R, V, vertices, faces, cams + 12 * view, f, sub, t, n);
      if (draw) {
        const int npix = t.bw * t.bh;
        if (npix <= kSmallBox) {
          n_small++;
          for (int k = 0; k < npix; k++) shade(R, t, t.ilo + k / t.bw, t.jlo + k % t.bw, map);
        } else {
          n_queued++;
          const unsigned long long chunks = (unsigned long long)((npix + kChunk - 1) / kChunk);
          const unsigned long long base = atomicAdd(&header[kCount], chunks);
          for (unsigned long long c = 0; c < chunks; c++) {
            if (base + c < capacity) {
              Entry e;
              e.face = (uint32_t)f, e.view_sub = (uint32_t)view << 1 | (uint32_t)sub, e.chunk = (uint32_t)c, e.pad = 0u;
              queue[base + c] = e;
            } else {   // the queue is full: this lane walks the chunk itself (slow, and the same map)
              n_over++;
              const int end = min(npix, (int)(c + 1) * kChunk);
              for (int k = (int)c * kChunk; k < end; k++) shade(R, t, t.ilo + k / t.bw, t.jlo + k % t.bw, map);
            }
          }
        }
      }
      if (n < 4) break;
    }
  }
  n_small = wave_sum(n_small), n_queued = wave_sum(n_queued), n_over = wave_sum(n_over);
  if ((threadIdx.x & 63) == 0) {
    if (n_small) atomicAdd(&header[kSmall], n_small);
    if (n_queued) atomicAdd(&header[kQueued], n_queued);
    if (n_over) atomicAdd(&header[kOverflow], n_over);
  }
}

// One workgroup per queued chunk: every thread repeats the set-up (the same code, hence the same numbers), then takes every 256th pixel centre.
__global__ void __launch_bounds__(256) drain_kernel(Raster R, long long V, long long F, const double* __restrict__ vertices,
                                                    const long long* __restrict__ faces, const double* __restrict__ cams, uint32_t* __restrict__ maps,
                                                    const unsigned long long* __restrict__ header, const Entry* __restrict__ queue,
                                                    unsigned long long capacity, int views) {
  const unsigned long long filled = header[kCount] < capacity ? header[kCount] : capacity;
  for (unsigned long long q = blockIdx.x; q < filled; q += gridDim.x) {
    const Entry e = queue[q];
    const int view = (int)(e.view_sub >> 1), sub = (int)(e.view_sub & 1u);
    if (view >= views || (long long)e.face >= F) continue;
    Tri t;
    int n;
    if (!face_tri(R, V, vertices, faces, cams + 12 * view, (long long)e.face, sub, t, n)) continue;
    uint32_t* map = maps + (size_t)view * R.H * R.W;
    const long long npix = (long long)t.bw * t.bh, first = (long long)e.chunk * kChunk;
    const long long end = first + kChunk < npix ? first + kChunk : npix;
    for (long long k = first + threadIdx.x; k < end; k += 256) shade(R, t, t.ilo + (int)(k / t.bw), t.jlo + (int)(k % t.bw), map);
  }
}

// ------------------------------------------------------------------ vertex visibility ------------------------------------------------------------------
struct Pinhole {
  int H, W, B;
  float fx, fy, cx, cy, eps;
};

// grid_sample's coordinate: normalised as vgrid is, unnormalised as align_corners = True does, clamped as border padding does
__device__ __forceinline__ float sample_coord(float u, int size) {
  const float s = (float)(size - 1);
  const float g = u / s * 2.0f - 1.0f;
  const float x = (g + 1.0f) / 2.0f * s;
  return fminf(s, fmaxf(x, 0.0f));
}

__global__ void __launch_bounds__(256) count_views_kernel(Pinhole P, long long N, const float* __restrict__ points, const float* __restrict__ cams,
                                                          const float* __restrict__ depths, int* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
  int seen = 0;
  for (int b = 0; b < P.B; b++) {
    const float* m = cams + 12 * b;   // the same address in every lane: scalar loads
    const float xc = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const float yc = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const float zc = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    const float zz = zc + 1e-8f;
    const float u = (P.fx * xc + P.cx * zc) / zz, v = (P.fy * yc + P.cy * zc) / zz;
    if (!(u >= 0.0f && u <= (float)(P.W - 1) && v >= 0.0f && v <= (float)(P.H - 1) && zz > 0.0f)) continue;   // false for NaN
    const float ix = sample_coord(u, P.W), iy = sample_coord(v, P.H);
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float nw = ((fx0 + 1.0f) - ix) * ((fy0 + 1.0f) - iy), ne = (ix - fx0) * ((fy0 + 1.0f) - iy);
    const float sw = ((fx0 + 1.0f) - ix) * (iy - fy0), se = (ix - fx0) * (iy - fy0);
    const float* map = depths + (size_t)b * P.H * P.W;
    const bool right = x0 + 1 < P.W, below = y0 + 1 < P.H;   // a neighbour outside the image is left out (its weight is 0)
    float s = 0.0f;
    s += map[(size_t)y0 * P.W + x0] * nw;
    if (right) s += map[(size_t)y0 * P.W + x0 + 1] * ne;
    if (below) s += map[(size_t)(y0 + 1) * P.W + x0] * sw;
    if (right && below) s += map[(size_t)(y0 + 1) * P.W + x0 + 1] * se;
    seen += s > 0.0f ? (zz < s + P.eps ? 1 : 0) : 1;
  }
  counts[i] += seen;
}

inline bool raster_ok(int H, int W, double fx, double fy, double cx, double cy, double znear, double zfar) {
  return H >= 2 && W >= 2 && H <= kMaxSide && W <= kMaxSide && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy) && isfinite(znear) &&
         isfinite(zfar) && znear > 0.0 && zfar > znear;
}

}  // namespace rgtc

extern "C" {

size_t radegs_tntcull_render_bytes(long long F, int B) {
  if (F < 0 || B < 0) return 0;
  const unsigned long long worst = 2ull * (unsigned long long)F * (unsigned long long)B;   // one chunk per drawn triangle; larger boxes share the rest
  const size_t entries = worst < rgtc::kDefaultQueue ? (size_t)worst : rgtc::kDefaultQueue;
  return rgtc::carve(entries, nullptr).bytes;
}

int radegs_tntcull_render_begin(long long V, long long F, const double* vertices, const long long* faces, int B, const double* w2c, int H, int W, double fx,
                                double fy, double cx, double cy, double znear, double zfar, void* workspace, size_t workspace_bytes, float* depth,
                                void* stream_v) {
  if (V < 0 || F < 0 || B < 0 || !rgtc::raster_ok(H, W, fx, fy, cx, cy, znear, zfar)) return RADEGS_ERR_INVALID_ARG;
  if (V >= (1ll << 31) || F >= (1ll << 31) || B > rgtc::kMaxViews || (unsigned long long)B * H * W >= (1ull << 39)) return RADEGS_ERR_TOO_LARGE;
  const size_t header_bytes = rgtc::carve(0, nullptr).bytes;
  if (!workspace || workspace_bytes < header_bytes || !rg::aligned16(workspace)) return RADEGS_ERR_INVALID_ARG;
  if (B == 0) return 0;
  if (!depth || !w2c || (F && (!vertices || !faces))) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const size_t capacity = (workspace_bytes - header_bytes) / sizeof(rgtc::Entry);
  const rgtc::View w = rgtc::carve(capacity, workspace);
  const rgtc::Raster R = {H, W, fx, fy, cx, cy, znear, zfar};
  const size_t pixels = (size_t)B * H * W;
  if (hipMemsetAsync(w.header, 0, rgtc::kHeaderWords * sizeof(unsigned long long), s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgtc::clear_kernel, dim3(rg::blocks_of(pixels)), dim3(256), 0, s, pixels, reinterpret_cast<uint32_t*>(depth));
  if (F)
    hipLaunchKernelGGL(rgtc::setup_kernel, dim3(rg::blocks_of((size_t)F), B), dim3(256), 0, s, R, V, F, vertices, faces, w2c, reinterpret_cast<uint32_t*>(depth),
                       w.header, w.queue, (unsigned long long)capacity);
  return rg::launch_status();
}

int radegs_tntcull_render_finish(long long V, long long F, const double* vertices, const long long* faces, int B, const double* w2c, int H, int W, double fx,
                                 double fy, double cx, double cy, double znear, double zfar, const void* workspace, size_t workspace_bytes, float* depth,
                                 long long* stats4, void* stream_v) {
  if (V < 0 || F < 0 || B < 0 || !rgtc::raster_ok(H, W, fx, fy, cx, cy, znear, zfar)) return RADEGS_ERR_INVALID_ARG;
  if (V >= (1ll << 31) || F >= (1ll << 31) || B > rgtc::kMaxViews || (unsigned long long)B * H * W >= (1ull << 39)) return RADEGS_ERR_TOO_LARGE;
  const size_t header_bytes = rgtc::carve(0, nullptr).bytes;
  if (!workspace || workspace_bytes < header_bytes || !rg::aligned16(workspace)) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (B == 0) return stats4 && hipMemsetAsync(stats4, 0, 4 * sizeof(long long), s) != hipSuccess ? RADEGS_ERR_HIP : 0;
  if (!depth || !w2c || (F && (!vertices || !faces))) return RADEGS_ERR_INVALID_ARG;
  const size_t capacity = (workspace_bytes - header_bytes) / sizeof(rgtc::Entry);
  const rgtc::View w = rgtc::carve(capacity, const_cast<void*>(workspace));
  const rgtc::Raster R = {H, W, fx, fy, cx, cy, znear, zfar};
  const size_t pixels = (size_t)B * H * W;
  if (F && capacity) {
    const unsigned nb = (unsigned)(capacity < (size_t)rgtc::kDrainBlocks ? capacity : (size_t)rgtc::kDrainBlocks);
    hipLaunchKernelGGL(rgtc::drain_kernel, dim3(nb), dim3(256), 0, s, R, V, F, vertices, faces, w2c, reinterpret_cast<uint32_t*>(depth), w.header, w.queue,
                       (unsigned long long)capacity, B);
  }
  hipLaunchKernelGGL(rgtc::resolve_kernel, dim3(rg::blocks_of(pixels)), dim3(256), 0, s, pixels, reinterpret_cast<uint32_t*>(depth));
  if (stats4 && hipMemcpyAsync(stats4, w.header, 4 * sizeof(long long), hipMemcpyDeviceToDevice, s) != hipSuccess) return RADEGS_ERR_HIP;
  return rg::launch_status();
}

int radegs_tntcull_count_views(long long N, const float* points, int B, int H, int W, const float* depths, const float* w2c, float fx, float fy, float cx,
                               float cy, float eps, int* counts, void* stream) {
  if (N < 0 || B < 0 || H < 2 || W < 2 || H > rgtc::kMaxSide || W > rgtc::kMaxSide || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy) ||
      !isfinite(eps))
    return RADEGS_ERR_INVALID_ARG;
  if (N == 0 || B == 0) return 0;
  if (!points || !depths || !w2c || !counts) return RADEGS_ERR_INVALID_ARG;
  const rgtc::Pinhole P = {H, W, B, fx, fy, cx, cy, eps};
  hipLaunchKernelGGL(rgtc::count_views_kernel, dim3(rg::blocks_of((size_t)N)), dim3(256), 0, static_cast<hipStream_t>(stream), P, N, points, w2c, depths,
                     counts);
  return rg::launch_status();
}

}  // extern "C"
