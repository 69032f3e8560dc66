// radegs_tetmesh.hip -- mesh extraction: the consumer of radegs_integrate, mesh_extract_tetrahedra.py.
//     utils/tetmesh.py:97-138                 marching tetrahedra over one chunk      plan + emit around the one host read (NV, NF)
//     scene/gaussian_model.py:400-429         get_tetra_points                        tetra_points_kernel
//     mesh_extract_tetrahedra.py:42-55        one view of evaluage_cull_alpha         cull_alpha_kernel / cull_finish_kernel
//     mesh_extract_tetrahedra.py:93-102       one bisection step                      bisect_kernel
//     mesh_extract_tetrahedra.py:107-110      the vertex / face filter                filter plan + apply around one host read
//
// Marching tetrahedra.  Upstream runs torch.unique over the six edges of every surface-crossing tetrahedron and throws the
// non-crossing ones away afterwards.  Here only CROSSING edges (occ[lo] != occ[hi], 3 or 4 per crossing tet) become instances; a
// mesh vertex is one distinct (lo, hi), numbered in ascending lexicographic order, which is what unique + the crossing mask give.
//   plan  occ_pack_kernel       occ = sdf > 0 as a V-bit mask (classification gathers bits, not sdf dwords)
//         classify_kernel       per tet: case code, #crossing edges, one- / two-triangle flag        -> flags[3 T], code[T]
//         rg::inclusive_scan_gather_u32 over the 3 T flags: instance offsets and the two face numberings in one scan
//         emit_edges_kernel     (lo, hi) of every crossing edge at offset[tet] + rank of the edge inside the tet
//         rg::radix_sort_order_2xu32: the stable order of the (lo, hi) pairs, hi the minor word.  The instance count E stays on the
//                               device (n_dev); the grids are sized by the capacity 4 T.
//         head_kernel           first instance of every distinct (lo, hi)   -> scan -> vertex id of every sorted instance
//         scatter_ids_kernel    vertex id back to the instance's emission slot + the two counts
//   emit  vertex_kernel         interp_v and the three gathers, one thread per head instance
//         face_kernel           one thread per tet: the six edge slots through the triangle table
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_filter.h"
#include "rg_prims.h"
#include "rg_workspace.h"

namespace rgt {

using rg::blocks_of;
using rg::kMaxItems;

// rows of upstream's 16 x 6 triangle table (utils/tetmesh.py:23-40), one nibble per entry, entry 0 lowest; 0xF = none
__constant__ uint32_t kTriTable[16] = {0xFFFFFFu, 0xFFF201u, 0xFFF304u, 0x431241u, 0xFFF513u, 0x352032u, 0x451041u, 0xFFF524u,
                                       0xFFF254u, 0x154014u, 0x253023u, 0xFFF531u, 0x134214u, 0xFFF403u, 0xFFF102u, 0xFFFFFFu};
// edge e of base_tet_edges joins corners kEdgeA[e], kEdgeB[e]; crossing-edge mask of case code c (bit e set: corners differ in occ)
__device__ __forceinline__ uint32_t cross_mask(uint32_t c) {
  const uint32_t o0 = c & 1u, o1 = (c >> 1) & 1u, o2 = (c >> 2) & 1u, o3 = (c >> 3) & 1u;
  return (o0 ^ o1) | ((o0 ^ o2) << 1) | ((o0 ^ o3) << 2) | ((o1 ^ o2) << 3) | ((o1 ^ o3) << 4) | ((o2 ^ o3) << 5);
}
__device__ __forceinline__ uint32_t num_triangles(uint32_t c) {   // num_triangles_table: 1 for one or three corners inside, 2 for two
  const uint32_t k = __popc(c);
  return k == 2u ? 2u : ((k == 1u || k == 3u) ? 1u : 0u);
}

__global__ void __launch_bounds__(256) occ_pack_kernel(uint32_t V, const float* __restrict__ sdf, unsigned long long* __restrict__ bits) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;   // V < 2^31: no wrap
  const unsigned long long b = __ballot(i < V && sdf[i] > 0.0f);
  if ((threadIdx.x & 63u) == 0u && i < V) bits[i >> 6] = b;
}

__device__ __forceinline__ uint32_t occ_of(const uint32_t* __restrict__ bits, int v) { return (bits[(uint32_t)v >> 5] >> ((uint32_t)v & 31u)) & 1u; }

// flags[t] = number of crossing edges, flags[T + t] = one-triangle tet, flags[2 T + t] = two-triangle tet.  A tet with an index outside
// [0, V) is treated as not crossing (the Python layer refuses such input; a C caller gets no out-of-bounds read).
__global__ void __launch_bounds__(256) classify_kernel(long long T, uint32_t V, const int4* __restrict__ tets, const uint32_t* __restrict__ bits,
                                                       uint32_t* __restrict__ flags, uint8_t* __restrict__ code) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int4 q = tets[t];
  uint32_t c = 0;
  if ((uint32_t)q.x < V && (uint32_t)q.y < V && (uint32_t)q.z < V && (uint32_t)q.w < V)
    c = occ_of(bits, q.x) | (occ_of(bits, q.y) << 1) | (occ_of(bits, q.z) << 2) | (occ_of(bits, q.w) << 3);
  const uint32_t nt = num_triangles(c);
  code[t] = (uint8_t)c;
  flags[t] = __popc(cross_mask(c));
  flags[T + t] = nt == 1u;
  flags[2 * T + t] = nt == 2u;
}

__global__ void __launch_bounds__(256) emit_edges_kernel(long long T, const int4* __restrict__ tets, const uint8_t* __restrict__ code,
                                                         const uint32_t* __restrict__ incl, uint32_t* __restrict__ lo, uint32_t* __restrict__ hi) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const uint32_t m = cross_mask(code[t]);
  if (m == 0u) return;
  const int4 q = tets[t];
  const uint32_t v[4] = {(uint32_t)q.x, (uint32_t)q.y, (uint32_t)q.z, (uint32_t)q.w};
  uint32_t at = incl[t] - __popc(m);
  constexpr int ea[6] = {0, 0, 0, 1, 1, 2}, eb[6] = {1, 2, 3, 2, 3, 3};
#pragma unroll
  for (int e = 0; e < 6; e++)
    if ((m >> e) & 1u) {
      const uint32_t a = v[ea[e]], b = v[eb[e]];
      lo[at] = a < b ? a : b;
      hi[at] = a < b ? b : a;
      at++;
    }
}

// head[i] = 1 where sorted instance i opens a new (lo, hi); 0 elsewhere, up to the capacity (the scan runs over all of it)
__global__ void __launch_bounds__(256) head_kernel(uint32_t cap, const uint32_t* __restrict__ n_dev, const uint32_t* __restrict__ lo_sorted,
                                                   const uint32_t* __restrict__ hi, const uint32_t* __restrict__ perm, uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= cap) return;
  uint32_t h = 0;
  if (i < *n_dev) h = i == 0u || lo_sorted[i] != lo_sorted[i - 1] || hi[perm[i]] != hi[perm[i - 1]];
  head[i] = h;
}

// vid_of[emission slot] = vertex id; thread 0 also writes counts2 = {n_verts, n_faces}
__global__ void __launch_bounds__(256) scatter_ids_kernel(uint32_t cap, long long T, const uint32_t* __restrict__ incl, const uint32_t* __restrict__ perm,
                                                          const uint32_t* __restrict__ vid_incl, uint32_t* __restrict__ vid_of,
                                                          long long* __restrict__ counts2) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t E = incl[T - 1];
  if (i == 0u) {
    const uint32_t n1 = incl[2 * T - 1] - E, n2 = incl[3 * T - 1] - incl[2 * T - 1];
    counts2[0] = E ? (long long)vid_incl[E - 1] : 0ll;
    counts2[1] = (long long)n1 + 2ll * (long long)n2;
  }
  if (i >= cap || i >= E) return;
  vid_of[perm[i]] = vid_incl[i] - 1u;
}

__global__ void __launch_bounds__(256) vertex_kernel(uint32_t cap, const uint32_t* __restrict__ n_dev, long long n_verts, const uint32_t* __restrict__ head,
                                                     const uint32_t* __restrict__ vid_incl, const uint32_t* __restrict__ lo_sorted,
                                                     const uint32_t* __restrict__ hi, const uint32_t* __restrict__ perm,
                                                     const float* __restrict__ vertices, const float* __restrict__ sdf, const float* __restrict__ scales,
                                                     float* __restrict__ end_points, float* __restrict__ end_sdf, float* __restrict__ end_scales,
                                                     long long* __restrict__ interp_v) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= cap || i >= *n_dev || !head[i]) return;
  const size_t v = vid_incl[i] - 1u;
  if ((long long)v >= n_verts) return;   // a caller that passed other counts than plan's gets no out-of-bounds write
  const uint32_t a = lo_sorted[i], b = hi[perm[i]];
  interp_v[2 * v] = (long long)a;
  interp_v[2 * v + 1] = (long long)b;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    end_points[6 * v + k] = vertices[3 * (size_t)a + k];
    end_points[6 * v + 3 + k] = vertices[3 * (size_t)b + k];
  }
  end_sdf[2 * v] = sdf[a];
  end_sdf[2 * v + 1] = sdf[b];
  end_scales[2 * v] = scales[a];
  end_scales[2 * v + 1] = scales[b];
}

__global__ void __launch_bounds__(256) face_kernel(long long T, long long n_faces, const uint8_t* __restrict__ code, const uint32_t* __restrict__ incl,
                                                   const uint32_t* __restrict__ vid_of, long long* __restrict__ faces) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const uint32_t c = code[t], nt = num_triangles(c);
  if (nt == 0u) return;
  const uint32_t m = cross_mask(c), at = incl[t] - __popc(m), row = kTriTable[c];
  const uint32_t E = incl[T - 1], n1 = incl[2 * T - 1] - E;
  long long f = nt == 1u ? (long long)(incl[T + t] - E) - 1 : (long long)n1 + 2ll * ((long long)(incl[2 * T + t] - incl[2 * T - 1]) - 1);
  if (f < 0 || f + (long long)nt > n_faces) return;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    if (k == 3 && nt == 1u) break;
    const uint32_t e = (row >> (4 * k)) & 15u;
    faces[3 * f + k] = (long long)vid_of[at + __popc(m & ((1u << e) - 1u))];
  }
}

struct Workspace {
  uint32_t *bits, *flags, *incl;
  uint8_t* code;
  uint32_t *lo, *hi, *b1, *perm1, *lo_g, *lo_sorted, *perm2;   // b1, perm1, lo_g: the sort's scratch
  void* temp;
  size_t temp_bytes, bytes;
  // after the sort: head flags live in lo_g, the scanned vertex ids in perm1, the per-slot ids in b1
};

static size_t capacity(long long T) { return 4 * (size_t)T; }
static Workspace carve(int V, long long T, void* base) {
  const size_t n = (size_t)T, cap = capacity(T);
  rg::Carver c(base);
  Workspace v;
  v.temp_bytes = rg::sort_temp_bytes(cap);
  if (rg::scan_temp_bytes(cap) > v.temp_bytes) v.temp_bytes = rg::scan_temp_bytes(cap);
  if (rg::scan_temp_bytes(3 * n) > v.temp_bytes) v.temp_bytes = rg::scan_temp_bytes(3 * n);
  v.bits = c.take<uint32_t>(2 * (((size_t)V + 63) / 64));   // whole 64-bit words: occ_pack_kernel writes one per wave
  v.flags = c.take<uint32_t>(3 * n);
  v.incl = c.take<uint32_t>(3 * n);
  v.code = c.take<uint8_t>(n);
  for (uint32_t** a : {&v.lo, &v.hi, &v.b1, &v.perm1, &v.lo_g, &v.lo_sorted, &v.perm2}) *a = c.take<uint32_t>(cap);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

static bool sizes_ok(int V, long long T) { return V >= 0 && T >= 0 && 5ull * (unsigned long long)T < kMaxItems; }   // V < 2^31: it is an int

// ------------------------------------------------------------- per-point kernels -------------------------------------------------------------
// One thread per Gaussian: its eight box corners (24 consecutive floats: six 16-byte stores) and its centre.
__global__ void __launch_bounds__(256) tetra_points_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ scales3,
                                                           const float* __restrict__ rotation, float* __restrict__ out_points,
                                                           float* __restrict__ out_scale) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float4 q4 = *reinterpret_cast<const float4*>(rotation + 4 * (size_t)i);
  const float norm = sqrtf(q4.x * q4.x + q4.y * q4.y + q4.z * q4.z + q4.w * q4.w);
  const float r = q4.x / norm, x = q4.y / norm, y = q4.z / norm, z = q4.w / norm;
  const float R[3][3] = {{1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - r * z), 2.0f * (x * z + r * y)},
                         {2.0f * (x * y + r * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - r * x)},
                         {2.0f * (x * z - r * y), 2.0f * (y * z + r * x), 1.0f - 2.0f * (x * x + y * y)}};
  float s[3], c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    s[k] = scales3[3 * (size_t)i + k] * 3.0f;
    c[k] = xyz[3 * (size_t)i + k];
  }
  float o[24];
#pragma unroll
  for (int j = 0; j < 8; j++) {   // corner j: binary counting, x the most significant bit
    const float bx = (j & 4) ? s[0] : -s[0], by = (j & 2) ? s[1] : -s[1], bz = (j & 1) ? s[2] : -s[2];
#pragma unroll
    for (int k = 0; k < 3; k++) o[3 * j + k] = ((R[k][0] * bx + R[k][1] * by) + R[k][2] * bz) + c[k];
  }
  float* dst = out_points + 24 * (size_t)i;   // 96 bytes per Gaussian: 16-byte aligned where out_points is (checked by the launcher)
#pragma unroll
  for (int g = 0; g < 6; g++) *reinterpret_cast<float4*>(dst + 4 * g) = make_float4(o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]);
  float* ctr = out_points + 24 * (size_t)P + 3 * (size_t)i;
  ctr[0] = c[0]; ctr[1] = c[1]; ctr[2] = c[2];
  const float smax = fmaxf(fmaxf(s[0], s[1]), s[2]);
  float* sc = out_scale + 8 * (size_t)i;
  *reinterpret_cast<float4*>(sc) = make_float4(smax, smax, smax, smax);
  *reinterpret_cast<float4*>(sc + 4) = make_float4(smax, smax, smax, smax);
  out_scale[8 * (size_t)P + i] = smax;
}

// product of the masks at one pixel; outside the image: grid_sample's zero padding
__device__ __forceinline__ float mask_at(int x, int y, int W, int H, const float* __restrict__ mask, const float* __restrict__ gt,
                                         const float* __restrict__ extra) {
  if (x < 0 || y < 0 || x >= W || y >= H) return 0.0f;
  const size_t at = (size_t)y * W + x;
  float m = mask[at];
  if (gt) m = m * gt[at];
  if (extra) m = m * extra[at];
  return m;
}

// One view of evaluage_cull_alpha (mesh_extract_tetrahedra.py:42-54) per point: the coordinate normalisation, grid_sample (bilinear,
// align_corners=False, zero padding; the corner weights in the order of torch's GPU kernel), the 0.5 test and the two updates.
__global__ void __launch_bounds__(256) cull_alpha_kernel(long long PN, const float* __restrict__ alpha, const float2* __restrict__ coord,
                                                         const float* __restrict__ mask, const float* __restrict__ gt, const float* __restrict__ extra,
                                                         int W, int H, float* __restrict__ final_sdf, int* __restrict__ weight) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= PN) return;
  const float2 p = coord[i];
  const float gx = (p.x * 2.0f + 1.0f) / (float)(W - 1) - 1.0f, gy = (p.y * 2.0f + 1.0f) / (float)(H - 1) - 1.0f;
  const float ix = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f, iy = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
  const float fx = floorf(ix), fy = floorf(iy);
  float prob = 0.0f;
  // a coordinate far outside the image (or NaN) has no in-bounds corner; the range test also keeps the int conversion defined
  if (fx >= -1.0f && fy >= -1.0f && fx <= (float)W && fy <= (float)H) {
    const int x0 = (int)fx, y0 = (int)fy;
    const float x1f = fx + 1.0f, y1f = fy + 1.0f;
    const float nw = (x1f - ix) * (y1f - iy), ne = (ix - fx) * (y1f - iy), sw = (x1f - ix) * (iy - fy), se = (ix - fx) * (iy - fy);
    prob = mask_at(x0, y0, W, H, mask, gt, extra) * nw;
    prob += mask_at(x0 + 1, y0, W, H, mask, gt, extra) * ne;
    prob += mask_at(x0, y0 + 1, W, H, mask, gt, extra) * sw;
    prob += mask_at(x0 + 1, y0 + 1, W, H, mask, gt, extra) * se;
  }
  if (prob > 0.5f) {
    const float a = alpha[i], f = final_sdf[i];
    final_sdf[i] = (a != a) ? a : (a < f ? a : f);   // torch.min propagates NaN
    weight[i] += 1;
  }
}

__global__ void __launch_bounds__(256) cull_finish_kernel(long long PN, const float* __restrict__ final_sdf, const int* __restrict__ weight,
                                                          float* __restrict__ sdf_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= PN) return;
  sdf_out[i] = weight[i] > 0 ? 0.5f - final_sdf[i] : -100.0f;
}

// One bisection step (mesh_extract_tetrahedra.py:93-102), in place: mid = (left + right) / 2 is what the caller evaluated mid_sdf at.
__global__ void __launch_bounds__(256) bisect_kernel(long long N, float* __restrict__ left_pts, float* __restrict__ right_pts, float* __restrict__ left_sdf,
                                                     float* __restrict__ right_sdf, const float* __restrict__ mid_sdf, float* __restrict__ mid_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float m = mid_sdf[i], l = left_sdf[i];
  const bool low = (m < 0.0f && l < 0.0f) || (m > 0.0f && l > 0.0f);   // mid_sdf == 0: false, the right end moves
  if (low) left_sdf[i] = m; else right_sdf[i] = m;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    float a = left_pts[3 * i + k], b = right_pts[3 * i + k];
    const float mid = (a + b) / 2.0f;
    if (low) { a = mid; left_pts[3 * i + k] = mid; } else { b = mid; right_pts[3 * i + k] = mid; }
    mid_out[3 * i + k] = (a + b) / 2.0f;
  }
}

// ---------------------------------------------------------------- the filter ----------------------------------------------------------------
__global__ void __launch_bounds__(256) keep_vertex_kernel(long long NV, const float* __restrict__ end_points, const float* __restrict__ end_scales,
                                                          uint32_t* __restrict__ flags) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= NV) return;
  const float* e = end_points + 6 * v;
  const float dx = e[0] - e[3], dy = e[1] - e[4], dz = e[2] - e[5];
  flags[v] = sqrtf((dx * dx + dy * dy) + dz * dz) <= end_scales[2 * v] + end_scales[2 * v + 1];
}

__global__ void __launch_bounds__(256) keep_face_kernel(long long NV, long long NF, const long long* __restrict__ faces, uint32_t* __restrict__ flags) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= NF) return;
  uint32_t keep = 1;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const long long v = faces[3 * f + k];
    keep &= (v >= 0 && v < NV) ? flags[v] : 0u;
  }
  flags[NV + f] = keep;
}

__global__ void filter_counts_kernel(long long NV, long long NF, const uint32_t* __restrict__ incl, long long* __restrict__ counts2) {
  const uint32_t nv = NV ? incl[NV - 1] : 0u;
  counts2[0] = nv;
  counts2[1] = NF ? (long long)(incl[NV + NF - 1] - nv) : 0ll;
}

__global__ void __launch_bounds__(256) filter_apply_kernel(long long NV, long long NF, long long nv_out, long long nf_out, const float* __restrict__ points,
                                                           const long long* __restrict__ faces, const uint32_t* __restrict__ flags,
                                                           const uint32_t* __restrict__ incl, float* __restrict__ out_v, long long* __restrict__ out_f) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= NV + NF || !flags[j]) return;
  if (j < NV) {
    const long long r = (long long)incl[j] - 1;
    if (r >= nv_out) return;
#pragma unroll
    for (int k = 0; k < 3; k++) out_v[3 * r + k] = points[3 * j + k];
  } else {
    const uint32_t nv = NV ? incl[NV - 1] : 0u;
    const long long r = (long long)(incl[j] - nv) - 1;
    if (r >= nf_out) return;
#pragma unroll
    for (int k = 0; k < 3; k++) out_f[3 * r + k] = (long long)incl[faces[3 * (j - NV) + k]] - 1;   // all three kept: flags[j]
  }
}

using rg::FilterView;

// The part of the two filter plans after the vertex flags w.flags[0, NV) are on their way: the face flags, the scan, the counts.
static int filter_plan_faces(long long NV, long long NF, const long long* faces, const FilterView& w, long long* counts2, hipStream_t s) {
  if (NF) hipLaunchKernelGGL(keep_face_kernel, dim3(blocks_of((size_t)NF)), dim3(256), 0, s, NV, NF, faces, w.flags);
  return rg::filter_scan_counts(NV, NF, w, counts2, s);
}

}  // namespace rgt

// rg_filter.h: the half of the filter radegs_meshclean.hip shares
namespace rg {

FilterView filter_carve(long long NV, long long NF, void* base) {
  const size_t n = (size_t)(NV + NF);
  Carver c(base);
  FilterView v;
  v.temp_bytes = scan_temp_bytes(n);
  v.flags = c.take<uint32_t>(n);
  v.incl = c.take<uint32_t>(n);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}
bool filter_sizes_ok(long long NV, long long NF) {
  return NV >= 0 && NF >= 0 && (unsigned long long)NV < kMaxItems && (unsigned long long)NF < kMaxItems && (unsigned long long)(NV + NF) < kMaxItems;
}
int filter_scan_counts(long long NV, long long NF, const FilterView& w, long long* counts2, hipStream_t s) {
  if (inclusive_scan_gather_u32(w.temp, w.temp_bytes, w.flags, nullptr, w.incl, (size_t)(NV + NF), s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgt::filter_counts_kernel, dim3(1), dim3(1), 0, s, NV, NF, w.incl, counts2);
  return launch_status();
}

}  // namespace rg

extern "C" {

size_t radegs_tetmesh_plan_bytes(int V, long long T) {
  if (!rgt::sizes_ok(V, T) || V == 0 || T == 0) return 0;
  return rgt::carve(V, T, nullptr).bytes;
}

int radegs_tetmesh_plan(int V, long long T, const int* tets, const float* sdf, void* workspace, size_t workspace_bytes, long long* counts2,
                        void* stream_v) {
  if (V < 0 || T < 0 || !counts2) return RADEGS_ERR_INVALID_ARG;
  if (!rgt::sizes_ok(V, T)) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (V == 0 || T == 0) return hipMemsetAsync(counts2, 0, 2 * sizeof(long long), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if (!tets || !sdf || !workspace || workspace_bytes < radegs_tetmesh_plan_bytes(V, T) || !rg::aligned16(workspace) ||
      !rg::aligned16(tets))
    return RADEGS_ERR_INVALID_ARG;
  const rgt::Workspace w = rgt::carve(V, T, workspace);
  const uint32_t cap = (uint32_t)rgt::capacity(T);
  const int4* tets4 = reinterpret_cast<const int4*>(tets);
  int end_bit = 1;
  while (end_bit < 31 && ((unsigned)(V - 1) >> end_bit)) end_bit++;
  hipLaunchKernelGGL(rgt::occ_pack_kernel, dim3(rg::blocks_of((size_t)V)), dim3(256), 0, s, (uint32_t)V, sdf, reinterpret_cast<unsigned long long*>(w.bits));
  hipLaunchKernelGGL(rgt::classify_kernel, dim3(rg::blocks_of((size_t)T)), dim3(256), 0, s, T, (uint32_t)V, tets4, w.bits, w.flags, w.code);
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, w.flags, nullptr, w.incl, 3 * (size_t)T, s) != hipSuccess) return RADEGS_ERR_HIP;
  const uint32_t* n_dev = w.incl + (T - 1);   // E, the number of crossing-edge instances: never read by the host
  hipLaunchKernelGGL(rgt::emit_edges_kernel, dim3(rg::blocks_of((size_t)T)), dim3(256), 0, s, T, tets4, w.code, w.incl, w.lo, w.hi);
  if (rg::radix_sort_order_2xu32(w.temp, w.temp_bytes, w.hi, w.lo, w.lo_sorted, w.perm2, w.b1, w.perm1, w.lo_g, cap, end_bit, end_bit, s, n_dev) !=
      hipSuccess)
    return RADEGS_ERR_HIP;
  uint32_t *head = w.lo_g, *vid_incl = w.perm1, *vid_of = w.b1;
  hipLaunchKernelGGL(rgt::head_kernel, dim3(rg::blocks_of(cap)), dim3(256), 0, s, cap, n_dev, w.lo_sorted, w.hi, w.perm2, head);
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, head, nullptr, vid_incl, cap, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgt::scatter_ids_kernel, dim3(rg::blocks_of(cap)), dim3(256), 0, s, cap, T, w.incl, w.perm2, vid_incl, vid_of, counts2);
  return rg::launch_status();
}

int radegs_tetmesh_emit(int V, long long T, const int* tets, const float* sdf, const float* vertices, const float* scales, const void* workspace,
                        long long n_verts, long long n_faces, float* end_points, float* end_sdf, float* end_scales, long long* faces,
                        long long* interp_v, void* stream_v) {
  if (V < 0 || T < 0 || n_verts < 0 || n_faces < 0) return RADEGS_ERR_INVALID_ARG;
  if (!rgt::sizes_ok(V, T)) return RADEGS_ERR_TOO_LARGE;
  if (V == 0 || T == 0 || (n_verts == 0 && n_faces == 0)) return 0;
  if (!tets || !sdf || !vertices || !scales || !workspace || (n_verts && (!end_points || !end_sdf || !end_scales || !interp_v)) || (n_faces && !faces))
    return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const rgt::Workspace w = rgt::carve(V, T, const_cast<void*>(workspace));
  const uint32_t cap = (uint32_t)rgt::capacity(T);
  const uint32_t* n_dev = w.incl + (T - 1);
  if (n_verts)
    hipLaunchKernelGGL(rgt::vertex_kernel, dim3(rg::blocks_of(cap)), dim3(256), 0, s, cap, n_dev, n_verts, w.lo_g, w.perm1, w.lo_sorted, w.hi, w.perm2,
                       vertices, sdf, scales, end_points, end_sdf, end_scales, interp_v);
  if (n_faces)
    hipLaunchKernelGGL(rgt::face_kernel, dim3(rg::blocks_of((size_t)T)), dim3(256), 0, s, T, n_faces, w.code, w.incl, w.b1, faces);
  return rg::launch_status();
}

int radegs_tetra_points(int P, const float* xyz, const float* scales3, const float* rotation_raw, float* out_points, float* out_scale, void* stream) {
  if (P < 0 || P > (1 << 27)) return RADEGS_ERR_INVALID_ARG;
  if (P == 0) return 0;
  if (!xyz || !scales3 || !rotation_raw || !out_points || !out_scale ||
      ((reinterpret_cast<uintptr_t>(rotation_raw) | reinterpret_cast<uintptr_t>(out_points) | reinterpret_cast<uintptr_t>(out_scale)) & 15))
    return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgt::tetra_points_kernel, dim3((P + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), P, xyz, scales3, rotation_raw,
                     out_points, out_scale);
  return rg::launch_status();
}

int radegs_cull_alpha_accumulate(long long PN, const float* alpha_integrated, const float* point_coordinate, const float* mask, const float* gt_mask,
                                 const float* masks_extra, int W, int H, float* final_sdf, int* weight, void* stream) {
  if (PN < 0 || PN >= (1ll << 39) || W < 1 || H < 1) return RADEGS_ERR_INVALID_ARG;
  if (PN == 0) return 0;
  if (!alpha_integrated || !point_coordinate || !mask || !final_sdf || !weight || (reinterpret_cast<uintptr_t>(point_coordinate) & 7)) return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgt::cull_alpha_kernel, dim3(rg::blocks_of((size_t)PN)), dim3(256), 0, static_cast<hipStream_t>(stream), PN, alpha_integrated,
                     reinterpret_cast<const float2*>(point_coordinate), mask, gt_mask, masks_extra, W, H, final_sdf, weight);
  return rg::launch_status();
}

int radegs_cull_alpha_finish(long long PN, const float* final_sdf, const int* weight, float* sdf_out, void* stream) {
  if (PN < 0 || PN >= (1ll << 39)) return RADEGS_ERR_INVALID_ARG;
  if (PN == 0) return 0;
  if (!final_sdf || !weight || !sdf_out) return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgt::cull_finish_kernel, dim3(rg::blocks_of((size_t)PN)), dim3(256), 0, static_cast<hipStream_t>(stream), PN, final_sdf, weight, sdf_out);
  return rg::launch_status();
}

int radegs_tetmesh_bisect(long long N, float* left_pts, float* right_pts, float* left_sdf, float* right_sdf, const float* mid_sdf, float* mid_pts_out,
                          void* stream) {
  if (N < 0 || N >= (1ll << 39)) return RADEGS_ERR_INVALID_ARG;
  if (N == 0) return 0;
  if (!left_pts || !right_pts || !left_sdf || !right_sdf || !mid_sdf || !mid_pts_out) return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgt::bisect_kernel, dim3(rg::blocks_of((size_t)N)), dim3(256), 0, static_cast<hipStream_t>(stream), N, left_pts, right_pts, left_sdf,
                     right_sdf, mid_sdf, mid_pts_out);
  return rg::launch_status();
}

size_t radegs_tetmesh_filter_plan_bytes(long long NV, long long NF) {
  if (!rg::filter_sizes_ok(NV, NF) || NV + NF == 0) return 0;
  return rg::filter_carve(NV, NF, nullptr).bytes;
}

int radegs_tetmesh_filter_plan(long long NV, long long NF, const float* end_points, const float* end_scales, const long long* faces, void* workspace,
                               size_t workspace_bytes, long long* counts2, void* stream_v) {
  if (NV < 0 || NF < 0 || !counts2) return RADEGS_ERR_INVALID_ARG;
  if (!rg::filter_sizes_ok(NV, NF)) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (NV == 0) return hipMemsetAsync(counts2, 0, 2 * sizeof(long long), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;   // no vertex: no face survives
  if (!end_points || !end_scales || (NF && !faces) || !workspace || workspace_bytes < radegs_tetmesh_filter_plan_bytes(NV, NF) ||
      !rg::aligned16(workspace))
    return RADEGS_ERR_INVALID_ARG;
  const rg::FilterView w = rg::filter_carve(NV, NF, workspace);
  hipLaunchKernelGGL(rgt::keep_vertex_kernel, dim3(rg::blocks_of((size_t)NV)), dim3(256), 0, s, NV, end_points, end_scales, w.flags);
  return rgt::filter_plan_faces(NV, NF, faces, w, counts2, s);
}

int radegs_tetmesh_filter_plan_flags(long long NV, long long NF, const unsigned* vertex_flags, const long long* faces, void* workspace,
                                     size_t workspace_bytes, long long* counts2, void* stream_v) {
  if (NV < 0 || NF < 0 || !counts2) return RADEGS_ERR_INVALID_ARG;
  if (!rg::filter_sizes_ok(NV, NF)) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (NV == 0) return hipMemsetAsync(counts2, 0, 2 * sizeof(long long), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if (!vertex_flags || (NF && !faces) || !workspace || workspace_bytes < radegs_tetmesh_filter_plan_bytes(NV, NF) ||
      !rg::aligned16(workspace))
    return RADEGS_ERR_INVALID_ARG;
  const rg::FilterView w = rg::filter_carve(NV, NF, workspace);
  if (hipMemcpyAsync(w.flags, vertex_flags, (size_t)NV * sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess) return RADEGS_ERR_HIP;
  return rgt::filter_plan_faces(NV, NF, faces, w, counts2, s);
}

int radegs_tetmesh_filter_apply(long long NV, long long NF, const float* points, const long long* faces, const void* workspace, long long nv_out,
                                long long nf_out, float* out_vertices, long long* out_faces, void* stream) {
  if (NV < 0 || NF < 0 || nv_out < 0 || nf_out < 0 || nv_out > NV || nf_out > NF) return RADEGS_ERR_INVALID_ARG;
  if (!rg::filter_sizes_ok(NV, NF)) return RADEGS_ERR_TOO_LARGE;
  if (NV == 0 || nv_out == 0) return 0;
  if (!points || (NF && !faces) || !workspace || !out_vertices || (nf_out && !out_faces)) return RADEGS_ERR_INVALID_ARG;
  const rg::FilterView w = rg::filter_carve(NV, NF, const_cast<void*>(workspace));
  hipLaunchKernelGGL(rgt::filter_apply_kernel, dim3(rg::blocks_of((size_t)(NV + (nf_out ? NF : 0)))), dim3(256), 0, static_cast<hipStream_t>(stream), NV,
                     nf_out ? NF : 0, nv_out, nf_out, points, faces, w.flags, w.incl, out_vertices, out_faces);
  return rg::launch_status();
}

}  // extern "C"
