// radegs_meshsimplify.hip -- mesh simplification: vertex clustering with quadric error (Lindstrom 2000; Open3D's
// simplify_vertex_clustering with SimplificationContraction.Quadric or .Average), the step upstream's users take in Open3D or MeshLab after
// post_process_mesh.  The specification is include/radegs.h, "Mesh simplification", and DESIGN.md 11 N21; tests/simplify_restatement.py
// restates it in NumPy.
//
// Cells.  Every vertex gets the 63-bit key cx << 42 | cy << 21 | cz of its cell; rg::radix_sort_order_2xu32 puts the vertices in (key, vertex)
// order and hands back the joined key; the heads of the runs are flagged and scanned, which numbers the cells by ascending key.
// Vertices.  A cell's average walks its run of the sorted vertices (ascending vertex index).  The 3 F corner records are put in stable order of
// their corner's cell; a cell adds the quadrics of its run, ascending (triangle, corner), plainly from 0.0 -- the order is a function of the run
// alone, no float atomics.  One wave per cell: the 64 lanes compute 64 records' quadrics side by side into LDS, ten lanes then add one entry
// each in record order, so that only the additions are serial (one lane per cell, the same additions, took 2.5 to 10 times as long at 10x to
// 1000x fewer faces: DESIGN.md 11 N21).  The quadric of a record is recomputed from its triangle where it is needed: 3 F x 10 doubles are
// never stored.  solve_kernel: cyclic Jacobi on the 3x3 block, one lane per cell.
// Faces.  Corners -> cell numbers, collapsed faces flagged, survivors rotated smallest first; duplicates: the rotated triples are sorted LSD (the
// third number, then stable by (second, first) with the two-word sort) and every triple equal to its predecessor is flagged.  The compaction of
// faces and cells is radegs_meshclean_compact_plan / _apply on the flags; face_source reads the face half of that plan.
// fp64, -ffp-contract=off, IEEE divide and sqrt.  Every loop is bounded by an argument of the launch and no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_filter.h"
#include "rg_prims.h"
#include "rg_workspace.h"

namespace rgms {

using rg::blocks_of;
constexpr long long kMaxVertices = 1ll << 31;   // V < 2^31
constexpr long long kMaxFaces = 1ll << 30;      // F <= 2^30: the 3 F corner records stay in the sort's u32 words
constexpr long long kMaxAttributes = 1 << 16;
constexpr int kCellBits = RADEGS_SIMPLIFY_CELL_BITS;
constexpr long long kCellMask = (1ll << kCellBits) - 1;
constexpr int kSweeps = RADEGS_SIMPLIFY_JACOBI_SWEEPS;

inline int bits_for(unsigned long long max_value) {   // the sort's end bit for keys in [0, max_value]
  int b = 1;
  while (b < 32 && (max_value >> b)) b++;
  return b;
}
inline bool sizes_ok(long long V, long long F) { return V < kMaxVertices && F <= kMaxFaces; }
inline bool grid_ok(double ox, double oy, double oz, double h) { return isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(h) && h > 0.0; }

// -------------------------------------------------------------------------- cells --------------------------------------------------------------------------
struct CellsView {
  uint32_t *lo, *hi, *hi_sorted, *s0, *s1, *s2;
  unsigned long long* joined;
  void* temp;
  size_t temp_bytes, bytes;
};
inline CellsView cells_carve(long long V, void* base) {
  const size_t n = (size_t)V;
  rg::Carver c(base);
  CellsView v;
  const size_t a = rg::sort_temp_bytes(n), b = rg::scan_temp_bytes(n);
  v.temp_bytes = a > b ? a : b;
  v.lo = c.take<uint32_t>(n), v.hi = c.take<uint32_t>(n), v.hi_sorted = c.take<uint32_t>(n);
  v.s0 = c.take<uint32_t>(n), v.s1 = c.take<uint32_t>(n), v.s2 = c.take<uint32_t>(n);
  v.joined = c.take<unsigned long long>(n);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

// floor((x - o) / h), one rounding per operation.  The host refuses a mesh with a cell outside [0, 2^21); the clamp keeps the key's fields apart
// whatever arrives (NaN: 0).
__device__ __forceinline__ unsigned long long cell_of(double x, double o, double h) {
  const double c = floor((x - o) / h);
  return c >= 0.0 ? (c <= (double)kCellMask ? (unsigned long long)c : (unsigned long long)kCellMask) : 0ull;
}

__global__ void __launch_bounds__(256) cell_keys_kernel(long long V, const double* __restrict__ vertices, double ox, double oy, double oz, double h,
                                                        uint32_t* __restrict__ lo, uint32_t* __restrict__ hi) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const unsigned long long key = cell_of(vertices[3 * v], ox, h) << (2 * kCellBits) | cell_of(vertices[3 * v + 1], oy, h) << kCellBits |
                                 cell_of(vertices[3 * v + 2], oz, h);
  lo[v] = (uint32_t)key, hi[v] = (uint32_t)(key >> 32);
}

__global__ void __launch_bounds__(256) heads_kernel(uint32_t n, const unsigned long long* __restrict__ joined, uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) head[i] = i == 0u || joined[i] != joined[i - 1u];
}

// position i of the sorted vertices: its vertex gets the cell's number; a head also writes the cell's first position and key.  cell_start has
// V + 1 entries and cell_key V, and incl[i] <= i + 1 <= V: no write leaves them.
__global__ void __launch_bounds__(256) number_cells_kernel(uint32_t n, const unsigned long long* __restrict__ joined, const uint32_t* __restrict__ order,
                                                           const uint32_t* __restrict__ head, const uint32_t* __restrict__ incl,
                                                           long long* __restrict__ vertex_cell, uint32_t* __restrict__ cell_start,
                                                           long long* __restrict__ cell_key, long long* __restrict__ n_cells) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = incl[i] - 1u;
  vertex_cell[order[i]] = r;
  if (head[i]) cell_start[r] = i, cell_key[r] = (long long)joined[i];
  if (i == n - 1u) cell_start[r + 1u] = n, *n_cells = (long long)r + 1;
}

// ------------------------------------------------------------------------- vertices -------------------------------------------------------------------------
struct VerticesView {
  uint32_t *key, *key_sorted, *rec_sorted;
  void* temp;
  size_t temp_bytes, bytes;
};
inline VerticesView vertices_carve(long long F, void* base) {
  const size_t n = 3 * (size_t)F;
  rg::Carver c(base);
  VerticesView v;
  v.temp_bytes = rg::sort_temp_bytes(n);
  v.key = c.take<uint32_t>(n), v.key_sorted = c.take<uint32_t>(n), v.rec_sorted = c.take<uint32_t>(n);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

// One thread per (cell, component): component < 3 a coordinate, the rest the attributes.  The members of the cell in ascending vertex index,
// added to 0.0, divided by their number.
__global__ void __launch_bounds__(256) average_kernel(long long V, long long K, int A, const double* __restrict__ vertices, const double* __restrict__ attributes,
                                                      const uint32_t* __restrict__ order, const uint32_t* __restrict__ cell_start,
                                                      double* __restrict__ averages, double* __restrict__ attr_out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int C = 3 + A;
  if (t >= K * C) return;
  const long long cell = t / C;
  const int e = (int)(t - cell * C);
  const uint32_t first = cell_start[cell], last = min(cell_start[cell + 1], (uint32_t)V);
  const double* src = e < 3 ? vertices + e : attributes + (e - 3);
  const long long stride = e < 3 ? 3 : A;
  double s = 0.0;
  for (uint32_t i = first; i < last; i++) {
    const uint32_t v = order[i];
    if (v < (uint32_t)V) s += src[(long long)v * stride];
  }
  s = s / (double)(last - first);
  if (e < 3) averages[3 * cell + e] = s; else attr_out[cell * A + (e - 3)] = s;
}

// the cell of every corner record; K for an index or a cell out of range: no cell walks that run
__global__ void __launch_bounds__(256) corner_cells_kernel(long long V, long long K, size_t n, const long long* __restrict__ faces,
                                                           const long long* __restrict__ vertex_cell, uint32_t* __restrict__ key) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long v = faces[i];
  long long c = K;
  if (v >= 0 && v < V) c = vertex_cell[v];
  key[i] = (c >= 0 && c < K) ? (uint32_t)c : (uint32_t)K;
}

// The ten entries w [n; d][n; d]^T of triangle f, in the order xx xy xz xd yy yz yd zz zd dd; all 0.0 where the triangle contributes nothing
// (an index outside [0, V), or a length that is not positive and finite) -- adding 0.0 leaves every bit of a sum that started at 0.0.
__device__ __forceinline__ void face_quadric(long long V, long long F, const double* __restrict__ vertices, const long long* __restrict__ faces, long long f,
                                             double (&q)[10]) {
#pragma unroll
  for (int e = 0; e < 10; e++) q[e] = 0.0;
  if (f < 0 || f >= F) return;
  const long long ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) return;
  const double ax = vertices[3 * ia], ay = vertices[3 * ia + 1], az = vertices[3 * ia + 2];
  const double ux = vertices[3 * ib] - ax, uy = vertices[3 * ib + 1] - ay, uz = vertices[3 * ib + 2] - az;
  const double vx = vertices[3 * ic] - ax, vy = vertices[3 * ic + 1] - ay, vz = vertices[3 * ic + 2] - az;
  const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  if (!(len > 0.0 && isfinite(len))) return;
  const double w = 0.5 * len, hx = nx / len, hy = ny / len, hz = nz / len;
  const double d = -((hx * ax + hy * ay) + hz * az);
  const double wx = w * hx, wy = w * hy, wz = w * hz, wd = w * d;
  q[0] = wx * hx, q[1] = wx * hy, q[2] = wx * hz, q[3] = wx * d;
  q[4] = wy * hy, q[5] = wy * hz, q[6] = wy * d;
  q[7] = wz * hz, q[8] = wz * d;
  q[9] = wd * d;
}

// One wave (a workgroup of 64) per cell, which walks the cell's run of the sorted corner records.  Per 64 records the lanes compute one quadric
// each into LDS (row stride 11 doubles: odd, so the ten adding lanes and the 64 writers spread over the banks), then lane e < 10 adds entry e
// of the rows in record order.  first / last are the same for all lanes, so every lane meets the same barriers.
__global__ void __launch_bounds__(64) quadric_kernel(long long V, long long F, long long K, uint32_t n, const double* __restrict__ vertices,
                                                     const long long* __restrict__ faces, const uint32_t* __restrict__ key_sorted,
                                                     const uint32_t* __restrict__ rec_sorted, double* __restrict__ quadrics) {
  __shared__ double sh[64 * 11];
  const long long cell = blockIdx.x;
  if (cell >= K) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t first = rg::lower_bound(key_sorted, n, (uint32_t)cell), last = rg::lower_bound(key_sorted, n, (uint32_t)cell + 1u);
  double acc = 0.0;
  for (uint32_t base = first; base < last; base += 64u) {
    const uint32_t i = base + lane;
    double q[10];
    face_quadric(V, F, vertices, faces, i < last ? (long long)(rec_sorted[i] / 3u) : -1ll, q);
#pragma unroll
    for (int e = 0; e < 10; e++) sh[lane * 11u + e] = q[e];
    __syncthreads();
    const uint32_t m = min(64u, last - base);
    if (lane < 10u)
      for (uint32_t j = 0; j < m; j++) acc += sh[j * 11u + lane];
    __syncthreads();
  }
  if (lane < 10u) quadrics[10 * cell + lane] = acc;
}

// one rotation of the cyclic Jacobi method on the symmetric 3x3 (app, aqq, apq and the two entries arp, arq of the third index r), applied to
// the columns p and q of R too; a zero apq is left alone
__device__ __forceinline__ void rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double (&R)[3][3], int p, int q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double tp = t * apq;
  app = app - tp, aqq = aqq + tp, apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp, arq = rq;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double kp = c * R[k][p] - s * R[k][q], kq = s * R[k][p] + c * R[k][q];
    R[k][p] = kp, R[k][q] = kq;
  }
}

// one lane per cell: x = m - sum over the eigenvalues above 1e-3 of the largest of ((r . g) / lambda) r, g = A m + b; m where that fails
__global__ void __launch_bounds__(256) solve_kernel(long long K, const double* __restrict__ quadrics, const double* __restrict__ averages,
                                                    const long long* __restrict__ cell_key, double ox, double oy, double oz, double h,
                                                    double* __restrict__ positions) {
  const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
  if (cell >= K) return;
  const double* Q = quadrics + 10 * cell;
  const double q00 = Q[0], q01 = Q[1], q02 = Q[2], b0 = Q[3], q11 = Q[4], q12 = Q[5], b1 = Q[6], q22 = Q[7], b2 = Q[8];
  const double m0 = averages[3 * cell], m1 = averages[3 * cell + 1], m2 = averages[3 * cell + 2];
  const double g0 = ((q00 * m0 + q01 * m1) + q02 * m2) + b0;
  const double g1 = ((q01 * m0 + q11 * m1) + q12 * m2) + b1;
  const double g2 = ((q02 * m0 + q12 * m1) + q22 * m2) + b2;
  double a00 = q00, a01 = q01, a02 = q02, a11 = q11, a12 = q12, a22 = q22;
  double R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < kSweeps; sweep++) {
    if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
    rotate(a00, a11, a01, a02, a12, R, 0, 1);
    rotate(a00, a22, a02, a01, a12, R, 0, 2);
    rotate(a11, a22, a12, a01, a02, R, 1, 2);
  }
  double lmax = a00;
  if (a11 > lmax) lmax = a11;
  if (a22 > lmax) lmax = a22;
  double x0 = m0, x1 = m1, x2 = m2;
  if (lmax > 0.0 && isfinite(lmax)) {
    const double cut = 1e-3 * lmax;
    const double lam[3] = {a00, a11, a22};
#pragma unroll
    for (int i = 0; i < 3; i++) {
      if (lam[i] > cut) {
        const double coef = ((R[0][i] * g0 + R[1][i] * g1) + R[2][i] * g2) / lam[i];
        x0 = x0 - coef * R[0][i], x1 = x1 - coef * R[1][i], x2 = x2 - coef * R[2][i];
      }
    }
    const unsigned long long key = (unsigned long long)cell_key[cell];
    const double cx = (double)((key >> (2 * kCellBits)) & (unsigned long long)kCellMask), cy = (double)((key >> kCellBits) & (unsigned long long)kCellMask),
                 cz = (double)(key & (unsigned long long)kCellMask);
    const bool inside = isfinite(x0) && isfinite(x1) && isfinite(x2) && x0 >= ox + cx * h && x0 <= ox + (cx + 1.0) * h && x1 >= oy + cy * h &&
                        x1 <= oy + (cy + 1.0) * h && x2 >= oz + cz * h && x2 <= oz + (cz + 1.0) * h;
    if (!inside) x0 = m0, x1 = m1, x2 = m2;
  }
  positions[3 * cell] = x0, positions[3 * cell + 1] = x1, positions[3 * cell + 2] = x2;
}

// --------------------------------------------------------------------------- faces ---------------------------------------------------------------------------
struct FacesView {
  uint32_t *k1, *k2, *k3, *k3_sorted, *p1, *m2, *m1_sorted, *p2, *s0, *s1, *s2;
  unsigned long long* joined;
  void* temp;
  size_t temp_bytes, bytes;
};
inline FacesView faces_carve(long long F, void* base) {
  const size_t n = (size_t)F;
  rg::Carver c(base);
  FacesView v;
  v.temp_bytes = rg::sort_temp_bytes(n);
  v.k1 = c.take<uint32_t>(n), v.k2 = c.take<uint32_t>(n), v.k3 = c.take<uint32_t>(n), v.k3_sorted = c.take<uint32_t>(n), v.p1 = c.take<uint32_t>(n);
  v.m2 = c.take<uint32_t>(n), v.m1_sorted = c.take<uint32_t>(n), v.p2 = c.take<uint32_t>(n);
  v.s0 = c.take<uint32_t>(n), v.s1 = c.take<uint32_t>(n), v.s2 = c.take<uint32_t>(n);
  v.joined = c.take<unsigned long long>(n);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

// Face f in cell numbers, rotated so that the smallest comes first (the orientation stays); remove[f] = 1 where two corners share a cell or an
// index is out of range, and the row is then (0, 0, 0).  With keys: the triple for the duplicate search, (K, K, K) for a removed face.
__global__ void __launch_bounds__(256) face_cells_kernel(long long V, long long F, long long K, const long long* __restrict__ faces,
                                                         const long long* __restrict__ vertex_cell, long long* __restrict__ cell_faces,
                                                         unsigned char* __restrict__ remove, uint32_t* __restrict__ k1, uint32_t* __restrict__ k2,
                                                         uint32_t* __restrict__ k3) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const long long ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  long long a = 0, b = 0, c = 0;
  bool dead = ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V;
  if (!dead) {
    a = vertex_cell[ia], b = vertex_cell[ib], c = vertex_cell[ic];
    dead = a < 0 || b < 0 || c < 0 || a >= K || b >= K || c >= K || a == b || b == c || c == a;
  }
  if (dead) {
    a = b = c = 0;
  } else if (b < a && b < c) {
    const long long t = a; a = b, b = c, c = t;
  } else if (c < a && c < b) {
    const long long t = c; c = b, b = a, a = t;
  }
  cell_faces[3 * f] = a, cell_faces[3 * f + 1] = b, cell_faces[3 * f + 2] = c;
  remove[f] = dead;
  if (k1) k1[f] = dead ? (uint32_t)K : (uint32_t)a, k2[f] = dead ? (uint32_t)K : (uint32_t)b, k3[f] = dead ? (uint32_t)K : (uint32_t)c;
}

__global__ void __launch_bounds__(256) gather2_kernel(uint32_t n, const uint32_t* __restrict__ p1, const uint32_t* __restrict__ k1,
                                                      const uint32_t* __restrict__ k2, uint32_t* __restrict__ m1, uint32_t* __restrict__ m2) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t f = p1[i] < n ? p1[i] : 0u;
  m1[i] = k1[f], m2[i] = k2[f];
}

// position i of the faces sorted by (first, second, third, face): a live face whose triple equals its predecessor's is a duplicate of a face of
// lower index.  Every writer of remove[] writes 1.
__global__ void __launch_bounds__(256) duplicates_kernel(uint32_t n, uint32_t K, const unsigned long long* __restrict__ joined, const uint32_t* __restrict__ p1,
                                                         const uint32_t* __restrict__ p2, const uint32_t* __restrict__ k3, unsigned char* __restrict__ remove) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0u || i >= n) return;
  const unsigned long long key = joined[i];
  if (joined[i - 1u] != key || (uint32_t)(key >> 32) == K) return;
  const uint32_t a = p2[i], b = p2[i - 1u];
  if (a >= n || b >= n) return;
  const uint32_t f = p1[a], g = p1[b];
  if (f >= n || g >= n) return;
  if (k3[f] == k3[g]) remove[f] = 1;
}

// the input face of every output face, from the face half of the compaction plan (rg_filter.h)
__global__ void __launch_bounds__(256) face_source_kernel(long long K, long long F, long long nf_out, const uint32_t* __restrict__ flags,
                                                          const uint32_t* __restrict__ incl, long long* __restrict__ face_source) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F || !flags[K + f]) return;
  const long long r = (long long)(incl[K + f] - (K ? incl[K - 1] : 0u)) - 1;
  if (r >= 0 && r < nf_out) face_source[r] = f;
}

}  // namespace rgms

extern "C" {

size_t radegs_simplify_cells_bytes(long long V) {
  if (V <= 0 || V >= rgms::kMaxVertices) return 0;
  return rgms::cells_carve(V, nullptr).bytes;
}

int radegs_simplify_cells(long long V, const double* vertices, double ox, double oy, double oz, double h, long long max_key, void* workspace,
                          size_t workspace_bytes, long long* vertex_cell, int* order, int* cell_start, long long* cell_key, long long* n_cells,
                          void* stream_v) {
  if (V < 0 || !n_cells || max_key < 0 || !rgms::grid_ok(ox, oy, oz, h)) return RADEGS_ERR_INVALID_ARG;
  if (V >= rgms::kMaxVertices) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (V == 0) return hipMemsetAsync(n_cells, 0, sizeof(long long), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if (!vertices || !vertex_cell || !order || !cell_start || !cell_key || !workspace || workspace_bytes < radegs_simplify_cells_bytes(V) ||
      !rg::aligned16(workspace))
    return RADEGS_ERR_INVALID_ARG;
  const rgms::CellsView w = rgms::cells_carve(V, workspace);
  const uint32_t n = (uint32_t)V;
  const unsigned long long mk = (unsigned long long)max_key;
  const int hi_bits = rgms::bits_for(mk >> 32), lo_bits = (mk >> 32) ? 32 : rgms::bits_for(mk);
  uint32_t* perm = reinterpret_cast<uint32_t*>(order);
  hipLaunchKernelGGL(rgms::cell_keys_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, V, vertices, ox, oy, oz, h, w.lo, w.hi);
  if (rg::radix_sort_order_2xu32(w.temp, w.temp_bytes, w.lo, w.hi, w.hi_sorted, perm, w.s0, w.s1, w.s2, n, lo_bits, hi_bits, s, nullptr, w.joined) != hipSuccess)
    return RADEGS_ERR_HIP;
  uint32_t *head = w.s0, *incl = w.s1;   // the sort's scratch is free again
  hipLaunchKernelGGL(rgms::heads_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, n, w.joined, head);
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, head, nullptr, incl, n, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgms::number_cells_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, n, w.joined, perm, head, incl, vertex_cell,
                     reinterpret_cast<uint32_t*>(cell_start), cell_key, n_cells);
  return rg::launch_status();
}

size_t radegs_simplify_vertices_bytes(long long F) {
  if (F <= 0 || F > rgms::kMaxFaces) return 0;
  return rgms::vertices_carve(F, nullptr).bytes;
}

int radegs_simplify_vertices(long long V, long long F, long long K, int A, const double* vertices, const long long* faces, const double* attributes,
                             const long long* vertex_cell, const int* order, const int* cell_start, const long long* cell_key, double ox, double oy,
                             double oz, double h, int quadric, void* workspace, size_t workspace_bytes, double* averages,
                             double* attributes_out, double* quadrics, double* positions, void* stream_v) {
  if (V < 0 || F < 0 || K < 0 || K > V || A < 0 || A > rgms::kMaxAttributes || (quadric != 0 && quadric != 1) || !rgms::grid_ok(ox, oy, oz, h))
    return RADEGS_ERR_INVALID_ARG;
  if (!rgms::sizes_ok(V, F) || (unsigned long long)K * (unsigned long long)(3 + A) > (1ull << 38)) return RADEGS_ERR_TOO_LARGE;   // average_kernel's grid
  if (K == 0) return 0;
  if (!vertices || !order || !cell_start || !averages || (A && (!attributes || !attributes_out))) return RADEGS_ERR_INVALID_ARG;
  if (quadric && (!quadrics || !positions || !cell_key || (F && (!faces || !vertex_cell || !workspace ||
                                                                  workspace_bytes < radegs_simplify_vertices_bytes(F) || !rg::aligned16(workspace)))))
    return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const uint32_t* ord = reinterpret_cast<const uint32_t*>(order);
  const uint32_t* start = reinterpret_cast<const uint32_t*>(cell_start);
  hipLaunchKernelGGL(rgms::average_kernel, dim3(rg::blocks_of((size_t)K * (size_t)(3 + A))), dim3(256), 0, s, V, K, A, vertices, attributes, ord, start, averages,
                     attributes_out);
  if (!quadric) return rg::launch_status();
  if (F) {
    const rgms::VerticesView w = rgms::vertices_carve(F, workspace);
    const size_t n = 3 * (size_t)F;
    hipLaunchKernelGGL(rgms::corner_cells_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, V, K, n, faces, vertex_cell, w.key);
    if (rg::radix_sort_pairs_u32(w.temp, w.temp_bytes, w.key, w.key_sorted, nullptr, w.rec_sorted, n, rgms::bits_for((unsigned long long)K), s) != hipSuccess)
      return RADEGS_ERR_HIP;
    hipLaunchKernelGGL(rgms::quadric_kernel, dim3((unsigned)K), dim3(64), 0, s, V, F, K, (uint32_t)n, vertices, faces, w.key_sorted, w.rec_sorted, quadrics);
  } else if (hipMemsetAsync(quadrics, 0, (size_t)K * 10 * sizeof(double), s) != hipSuccess) {
    return RADEGS_ERR_HIP;
  }
  hipLaunchKernelGGL(rgms::solve_kernel, dim3(rg::blocks_of((size_t)K)), dim3(256), 0, s, K, quadrics, averages, cell_key, ox, oy, oz, h, positions);
  return rg::launch_status();
}

size_t radegs_simplify_faces_bytes(long long F) {
  if (F <= 0 || F > rgms::kMaxFaces) return 0;
  return rgms::faces_carve(F, nullptr).bytes;
}

int radegs_simplify_faces(long long V, long long F, long long K, const long long* faces, const long long* vertex_cell, int remove_duplicates, void* workspace,
                          size_t workspace_bytes, long long* cell_faces, unsigned char* remove, void* stream_v) {
  if (V < 0 || F < 0 || K < 0 || K > V || (remove_duplicates != 0 && remove_duplicates != 1)) return RADEGS_ERR_INVALID_ARG;
  if (!rgms::sizes_ok(V, F)) return RADEGS_ERR_TOO_LARGE;
  if (F == 0) return 0;
  if (!faces || !vertex_cell || !cell_faces || !remove ||
      (remove_duplicates && (!workspace || workspace_bytes < radegs_simplify_faces_bytes(F) || !rg::aligned16(workspace))))
    return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const uint32_t n = (uint32_t)F;
  if (!remove_duplicates) {
    hipLaunchKernelGGL(rgms::face_cells_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, V, F, K, faces, vertex_cell, cell_faces, remove, (uint32_t*)nullptr,
                       (uint32_t*)nullptr, (uint32_t*)nullptr);
    return rg::launch_status();
  }
  const rgms::FacesView w = rgms::faces_carve(F, workspace);
  const int bits = rgms::bits_for((unsigned long long)K);
  hipLaunchKernelGGL(rgms::face_cells_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, V, F, K, faces, vertex_cell, cell_faces, remove, w.k1, w.k2, w.k3);
  if (rg::radix_sort_pairs_u32(w.temp, w.temp_bytes, w.k3, w.k3_sorted, nullptr, w.p1, n, bits, s) != hipSuccess) return RADEGS_ERR_HIP;
  uint32_t* m1 = w.k3_sorted;   // the sorted third numbers are not read again
  hipLaunchKernelGGL(rgms::gather2_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, n, w.p1, w.k1, w.k2, m1, w.m2);
  if (rg::radix_sort_order_2xu32(w.temp, w.temp_bytes, w.m2, m1, w.m1_sorted, w.p2, w.s0, w.s1, w.s2, n, bits, bits, s, nullptr, w.joined) != hipSuccess)
    return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgms::duplicates_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, n, (uint32_t)K, w.joined, w.p1, w.p2, w.k3, remove);
  return rg::launch_status();
}

int radegs_simplify_face_source(long long K, long long F, const void* compact_workspace, long long nf_out, long long* face_source, void* stream) {
  if (K < 0 || F < 0 || nf_out < 0 || nf_out > F) return RADEGS_ERR_INVALID_ARG;
  if (!rgms::sizes_ok(K, F)) return RADEGS_ERR_TOO_LARGE;
  if (nf_out == 0) return 0;
  if (!compact_workspace || !face_source) return RADEGS_ERR_INVALID_ARG;
  const rg::FilterView w = rg::filter_carve(K, F, const_cast<void*>(compact_workspace));
  hipLaunchKernelGGL(rgms::face_source_kernel, dim3(rg::blocks_of((size_t)F)), dim3(256), 0, static_cast<hipStream_t>(stream), K, F, nf_out, w.flags, w.incl,
                     face_source);
  return rg::launch_status();
}

}  // extern "C"
