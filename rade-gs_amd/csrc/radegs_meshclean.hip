// radegs_meshclean.hip -- mesh clean-up: the steps of the reference that treat the mesh as a graph, which upstream hands
// to Open3D and trimesh.
//     utils/mesh_utils.py:23-44      post_process_mesh: cluster_connected_triangles, remove_*     cluster, stats, compact plan + apply
//     eval_tnt/cull_mesh.py:186-202  Mesher.get_connected_mesh: mesh.split, areas                 the same, adjacency "manifold_edge"
//     mesh_extract.py:104            mesh.compute_vertex_normals                                  vertex_normals
// The specification is include/radegs.h, "Mesh clean-up", and DESIGN.md 11 N12; tests/meshclean_restatement.py restates it in NumPy.
//
// Clusters.  The 3 F undirected edge records (lo, hi) are put in order by rg::radix_sort_order_2xu32 with the joined key; equal neighbours in
// that order are the triangles on one edge, and link_kernel joins them in a union-find over the triangles.
//   parent[x] <= x holds at every moment: it starts as parent[x] = x, a link is a compare-and-swap that replaces a root's own index by a
//   SMALLER root, and path halving only ever lowers an entry (atomicMin) to one of x's ancestors.  Hence
//   - a find walks strictly downwards in index until it meets parent[r] == r: it terminates, and no cycle can form;
//   - the root of a set is its smallest member (true of singletons; a link keeps the smaller of two roots, the minimum of the union), so
//     after all links the root of every triangle is the smallest triangle index of its component whatever the interleaving of the atomics.
//   A failed compare-and-swap means the root was hung elsewhere meanwhile, by a link that succeeded: the loop finds the new roots and tries
//   again.  Nothing spins on a flag and no workgroup waits for another; flattening is a second launch (roots_kernel), not a grid barrier.
// Numbering: roots flagged, scanned, gathered -- ascending smallest triangle index.  Counts: integer atomics.  Areas: the triangles in stable
// cluster-sorted order, consecutive groups of 256 of a cluster through rg::block_sum, the group sums of a cluster added in ascending order by
// one thread: the order of every addition is a function of the cluster's triangle count alone.  fp64, -ffp-contract=off.
// Vertex normals: the 3 F corner records in stable order of their vertex; a vertex walks its run, ascending (triangle, corner): np.add.at's
// order, no float atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_filter.h"
#include "rg_prims.h"
#include "rg_reduce.h"
#include "rg_workspace.h"

namespace rgmc {

using rg::blocks_of;
constexpr long long kMaxVertices = 1ll << 31;   // V < 2^31
constexpr long long kMaxFaces = 1ll << 30;      // F <= 2^30: 3 F records and their indices stay in the sort's u32 words

inline int bits_for(unsigned long long max_value) {   // the sort's end bit for keys in [0, max_value]
  int b = 1;
  while (b < 32 && (max_value >> b)) b++;
  return b;
}
inline bool sizes_ok(long long V, long long F) { return V < kMaxVertices && F <= kMaxFaces; }

// ------------------------------------------------------------------------ clusters ------------------------------------------------------------------------
struct ClusterView {
  uint32_t *lo, *hi, *lo_sorted, *perm, *s0, *s1, *s2;
  unsigned long long* joined;
  void* temp;
  size_t temp_bytes, bytes;
};
inline ClusterView cluster_carve(long long F, void* base) {
  const size_t n = 3 * (size_t)F;
  rg::Carver c(base);
  ClusterView v;
  const size_t a = rg::sort_temp_bytes(n), b = rg::scan_temp_bytes((size_t)F);
  v.temp_bytes = a > b ? a : b;
  v.lo = c.take<uint32_t>(n), v.hi = c.take<uint32_t>(n), v.lo_sorted = c.take<uint32_t>(n), v.perm = c.take<uint32_t>(n);
  v.s0 = c.take<uint32_t>(n), v.s1 = c.take<uint32_t>(n), v.s2 = c.take<uint32_t>(n);
  v.joined = c.take<unsigned long long>(n);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

// record 3 f + k: the edge from corner k to corner k + 1.  An index outside [0, V) (the Python layer refuses such input) makes the record
// a self-edge, which joins nothing.
__global__ void __launch_bounds__(256) edge_records_kernel(long long V, long long F, const long long* __restrict__ faces, uint32_t* __restrict__ lo,
                                                           uint32_t* __restrict__ hi) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const long long a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  const bool ok = a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;
  const uint32_t v0 = ok ? (uint32_t)a : 0u, v1 = ok ? (uint32_t)b : 0u, v2 = ok ? (uint32_t)c : 0u;
  lo[3 * f] = min(v0, v1), hi[3 * f] = max(v0, v1);
  lo[3 * f + 1] = min(v1, v2), hi[3 * f + 1] = max(v1, v2);
  lo[3 * f + 2] = min(v2, v0), hi[3 * f + 2] = max(v2, v0);
}

__global__ void __launch_bounds__(256) iota_kernel(uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = i;
}

__device__ __forceinline__ uint32_t load_parent(const uint32_t* parent, uint32_t x) { return __atomic_load_n(parent + x, __ATOMIC_RELAXED); }

// the root of x, halving the path on the way: parent[x] is lowered to its grandparent, an ancestor of x and not above parent[x]
__device__ __forceinline__ uint32_t find_root(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = load_parent(parent, x);
    if (p == x) return x;
    const uint32_t g = load_parent(parent, p);
    if (g != p) atomicMin(parent + x, g);
    x = p;
  }
}

__device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root(parent, a), b = find_root(parent, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }      // a is the larger root: it goes under b
    if (atomicCAS(parent + a, a, b) == a) return;           // failed: a was hung under another root meanwhile -- find again
  }
}

// One thread per position of the sorted records.  "edge": a record equal to its predecessor joins the two triangles, which chains a whole run.
// "manifold_edge": only a run of exactly two records joins.
__global__ void __launch_bounds__(256) link_kernel(uint32_t n, int manifold, const unsigned long long* __restrict__ joined,
                                                   const uint32_t* __restrict__ perm, uint32_t* parent) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0u || i >= n) return;
  const unsigned long long key = joined[i];
  if (joined[i - 1] != key || (uint32_t)(key >> 32) == (uint32_t)key) return;
  if (manifold && ((i >= 2u && joined[i - 2] == key) || (i + 1u < n && joined[i + 1] == key))) return;
  unite(parent, perm[i - 1] / 3u, perm[i] / 3u);
}

// after every link: root[f], and whether f is one
__global__ void __launch_bounds__(256) roots_kernel(uint32_t F, uint32_t* parent, uint32_t* __restrict__ root, uint32_t* __restrict__ is_root) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  if (f >= F) return;
  const uint32_t r = find_root(parent, f);
  root[f] = r;
  is_root[f] = r == f;
}

__global__ void __launch_bounds__(256) number_kernel(uint32_t F, const uint32_t* __restrict__ root, const uint32_t* __restrict__ incl,
                                                     long long* __restrict__ triangle_clusters, long long* __restrict__ n_clusters) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  if (f >= F) return;
  triangle_clusters[f] = (long long)incl[root[f]] - 1;
  if (f == F - 1u) *n_clusters = incl[f];
}

// ------------------------------------------------------------------- counts and areas -------------------------------------------------------------------
struct StatsView {
  uint32_t *key, *key_sorted, *tri_sorted, *cnt, *cnt_incl, *grp, *grp_incl;
  double *group_sum, *partial;
  void* temp;
  size_t temp_bytes, bytes;
};
inline size_t max_groups(long long F, long long C) { return (size_t)(F / 256 + C); }   // sum of ceil(n_c / 256) <= floor(F / 256) + C
inline StatsView stats_carve(long long F, long long C, void* base) {
  rg::Carver c(base);
  StatsView v;
  const size_t a = rg::sort_temp_bytes((size_t)F), b = rg::scan_temp_bytes((size_t)C);
  v.temp_bytes = a > b ? a : b;
  v.key = c.take<uint32_t>((size_t)F), v.key_sorted = c.take<uint32_t>((size_t)F), v.tri_sorted = c.take<uint32_t>((size_t)F);
  v.cnt = c.take<uint32_t>((size_t)C), v.cnt_incl = c.take<uint32_t>((size_t)C), v.grp = c.take<uint32_t>((size_t)C), v.grp_incl = c.take<uint32_t>((size_t)C);
  v.group_sum = c.take<double>(max_groups(F, C));
  v.partial = c.take<double>(rg::kSumBlocks);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

// a label outside [0, C) (the Python layer passes the labels radegs_meshclean_cluster wrote) counts as cluster 0: no wild write
__global__ void __launch_bounds__(256) count_kernel(long long F, long long C, const long long* __restrict__ triangle_clusters, uint32_t* __restrict__ key,
                                                    uint32_t* __restrict__ cnt) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const long long c = triangle_clusters[f];
  const uint32_t k = (c >= 0 && c < C) ? (uint32_t)c : 0u;
  key[f] = k;
  atomicAdd(cnt + k, 1u);
}

__global__ void __launch_bounds__(256) counts_out_kernel(long long C, const uint32_t* __restrict__ cnt, uint32_t* __restrict__ grp,
                                                         long long* __restrict__ cluster_n) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  cluster_n[c] = cnt[c];
  grp[c] = (cnt[c] + 255u) >> 8;
}

// 0.5 |(b - a) x (c - a)|, one rounding per operation, in the order written; an index outside [0, V): 0
__device__ __forceinline__ void face_normal(long long V, const double* __restrict__ vertices, const long long* __restrict__ faces, long long f, double& nx,
                                            double& ny, double& nz) {
  const long long ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  nx = ny = nz = 0.0;
  if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) return;
  const double ax = vertices[3 * ia], ay = vertices[3 * ia + 1], az = vertices[3 * ia + 2];
  const double ux = vertices[3 * ib] - ax, uy = vertices[3 * ib + 1] - ay, uz = vertices[3 * ib + 2] - az;
  const double vx = vertices[3 * ic] - ax, vy = vertices[3 * ic + 1] - ay, vz = vertices[3 * ic + 2] - az;
  nx = uy * vz - uz * vy;
  ny = uz * vx - ux * vz;
  nz = ux * vy - uy * vx;
}
__device__ __forceinline__ double face_area(long long V, const double* __restrict__ vertices, const long long* __restrict__ faces, long long f) {
  double nx, ny, nz;
  face_normal(V, vertices, faces, f, nx, ny, nz);
  return 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
}

// One workgroup per group of 256 consecutive triangles of one cluster in cluster-sorted order; a group's missing tail adds 0.0.
__global__ void __launch_bounds__(256) group_area_kernel(long long V, uint32_t C, const double* __restrict__ vertices, const long long* __restrict__ faces,
                                                         const uint32_t* __restrict__ tri_sorted, const uint32_t* __restrict__ cnt,
                                                         const uint32_t* __restrict__ cnt_incl, const uint32_t* __restrict__ grp,
                                                         const uint32_t* __restrict__ grp_incl, double* __restrict__ group_sum) {
  __shared__ double sh[256];
  const uint32_t j = blockIdx.x;
  if (j >= grp_incl[C - 1u]) return;                                  // the same for the whole workgroup: before any barrier
  const uint32_t c = rg::lower_bound(grp_incl, C, j + 1u);            // the first cluster whose groups end past j
  const uint32_t within = (j - (grp_incl[c] - grp[c])) * 256u + threadIdx.x;
  double v[1] = {0.0};
  if (within < cnt[c]) v[0] = face_area(V, vertices, faces, (long long)tri_sorted[(cnt_incl[c] - cnt[c]) + within]);
  rg::block_sum(v, sh);
  if (threadIdx.x == 0) group_sum[j] = v[0];
}

__global__ void __launch_bounds__(256) cluster_area_kernel(uint32_t C, const uint32_t* __restrict__ grp, const uint32_t* __restrict__ grp_incl,
                                                           const double* __restrict__ group_sum, double* __restrict__ cluster_area) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= C) return;
  const uint32_t first = grp_incl[c] - grp[c];
  double s = 0.0;
  for (uint32_t g = 0; g < grp[c]; g++) s += group_sum[first + g];
  cluster_area[c] = s;
}

// the total over all triangles in their own order: rg_reduce.h's two stages
__global__ void __launch_bounds__(256) total_partial_kernel(long long V, long long F, const double* __restrict__ vertices, const long long* __restrict__ faces,
                                                            double* __restrict__ partial) {
  __shared__ double sh[256];
  double v[1] = {0.0};
  for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < F; f += (long long)gridDim.x * 256) v[0] += face_area(V, vertices, faces, f);
  rg::block_sum(v, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = v[0];
}
__global__ void __launch_bounds__(256) total_final_kernel(int nblocks, const double* __restrict__ partial, double* __restrict__ out) {
  __shared__ double sh[256];
  double v[1] = {0.0};
  rg::add_partials(partial, nblocks, v);
  rg::block_sum(v, sh);
  if (threadIdx.x == 0) out[0] = v[0];
}

// ----------------------------------------------------------------------- compaction -----------------------------------------------------------------------
// face f survives `remove` / `cluster_keep` (either may be null); an out-of-range label or index removes the face
__device__ __forceinline__ bool face_selected(long long V, long long f, long long C, const long long* __restrict__ faces, const unsigned char* __restrict__ remove,
                                              const long long* __restrict__ triangle_clusters, const unsigned char* __restrict__ cluster_keep) {
  if (remove && remove[f]) return false;
  if (cluster_keep) {
    const long long c = triangle_clusters[f];
    if (c < 0 || c >= C || !cluster_keep[c]) return false;
  }
  const long long a = faces[3 * f], b = faces[3 * f + 1], c3 = faces[3 * f + 2];
  return a >= 0 && b >= 0 && c3 >= 0 && a < V && b < V && c3 < V;
}

__global__ void __launch_bounds__(256) fill_kernel(size_t n, uint32_t value, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = value;
}

// flags[V + f]: the face stays; flags[v] = 1 for the corners of the selected faces (degenerate ones included: a vertex only such a face
// references stays, as in the reference's order of calls).  Every writer of flags[v] writes 1.
__global__ void __launch_bounds__(256) face_flags_kernel(long long V, long long F, long long C, const long long* __restrict__ faces,
                                                         const unsigned char* __restrict__ remove, const long long* __restrict__ triangle_clusters,
                                                         const unsigned char* __restrict__ cluster_keep, int drop_degenerate, int mark_vertices,
                                                         uint32_t* __restrict__ flags) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const bool sel = face_selected(V, f, C, faces, remove, triangle_clusters, cluster_keep);
  bool keep = sel;
  if (sel) {
    const long long a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (mark_vertices) flags[a] = 1u, flags[b] = 1u, flags[c] = 1u;
    if (drop_degenerate && (a == b || b == c || c == a)) keep = false;
  }
  flags[V + f] = keep;
}

__global__ void __launch_bounds__(256) compact_apply_kernel(long long V, long long F, long long nv_out, long long nf_out, const long long* __restrict__ faces,
                                                            const uint32_t* __restrict__ flags, const uint32_t* __restrict__ incl,
                                                            long long* __restrict__ kept_vertices, long long* __restrict__ out_faces) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= V + F || !flags[j]) return;
  if (j < V) {
    const long long r = (long long)incl[j] - 1;
    if (r < nv_out) kept_vertices[r] = j;
  } else {
    const uint32_t nv = V ? incl[V - 1] : 0u;
    const long long r = (long long)(incl[j] - nv) - 1;
    if (r >= nf_out) return;
#pragma unroll
    for (int k = 0; k < 3; k++) out_faces[3 * r + k] = (long long)incl[faces[3 * (j - V) + k]] - 1;   // in range and kept: flags[j]
  }
}

// --------------------------------------------------------------------- vertex normals ---------------------------------------------------------------------
struct NormalsView {
  uint32_t *key, *key_sorted, *rec_sorted;
  void* temp;
  size_t temp_bytes, bytes;
};
inline NormalsView normals_carve(long long F, void* base) {
  const size_t n = 3 * (size_t)F;
  rg::Carver c(base);
  NormalsView v;
  v.temp_bytes = rg::sort_temp_bytes(n);
  v.key = c.take<uint32_t>(n), v.key_sorted = c.take<uint32_t>(n), v.rec_sorted = c.take<uint32_t>(n);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

// the vertex of every corner record; V for an index outside [0, V): no vertex walks that run
__global__ void __launch_bounds__(256) corner_keys_kernel(long long V, size_t n, const long long* __restrict__ faces, uint32_t* __restrict__ key) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long v = faces[i];
  key[i] = (v >= 0 && v < V) ? (uint32_t)v : (uint32_t)V;
}

__global__ void __launch_bounds__(256) vertex_normals_kernel(long long V, uint32_t n, const double* __restrict__ vertices, const long long* __restrict__ faces,
                                                             const uint32_t* __restrict__ key_sorted, const uint32_t* __restrict__ rec_sorted,
                                                             int normalized, double* __restrict__ normals) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (uint32_t i = rg::lower_bound(key_sorted, n, (uint32_t)v); i < n && key_sorted[i] == (uint32_t)v; i++) {
    double nx, ny, nz;
    face_normal(V, vertices, faces, (long long)(rec_sorted[i] / 3u), nx, ny, nz);
    sx += nx, sy += ny, sz += nz;
  }
  if (normalized) {
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    if (len > 0.0 && isfinite(len)) {
      sx /= len, sy /= len, sz /= len;
    } else {
      sx = 0.0, sy = 0.0, sz = 1.0;
    }
  }
  normals[3 * v] = sx, normals[3 * v + 1] = sy, normals[3 * v + 2] = sz;
}

}  // namespace rgmc

extern "C" {

size_t radegs_meshclean_cluster_bytes(long long F) {
  if (F <= 0 || F > rgmc::kMaxFaces) return 0;
  return rgmc::cluster_carve(F, nullptr).bytes;
}

int radegs_meshclean_cluster(long long V, long long F, const long long* faces, int manifold, void* workspace, size_t workspace_bytes,
                             long long* triangle_clusters, long long* n_clusters, void* stream_v) {
  if (V < 0 || F < 0 || !n_clusters || (manifold != 0 && manifold != 1)) return RADEGS_ERR_INVALID_ARG;
  if (!rgmc::sizes_ok(V, F)) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (F == 0) return hipMemsetAsync(n_clusters, 0, sizeof(long long), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if (!faces || !triangle_clusters || !workspace || workspace_bytes < radegs_meshclean_cluster_bytes(F) || !rg::aligned16(workspace))
    return RADEGS_ERR_INVALID_ARG;
  const rgmc::ClusterView w = rgmc::cluster_carve(F, workspace);
  const uint32_t n = (uint32_t)(3 * F);
  const int end_bit = rgmc::bits_for(V ? (unsigned long long)(V - 1) : 0ull);
  hipLaunchKernelGGL(rgmc::edge_records_kernel, dim3(rg::blocks_of((size_t)F)), dim3(256), 0, s, V, F, faces, w.lo, w.hi);
  if (rg::radix_sort_order_2xu32(w.temp, w.temp_bytes, w.hi, w.lo, w.lo_sorted, w.perm, w.s0, w.s1, w.s2, n, end_bit, end_bit, s, nullptr, w.joined) !=
      hipSuccess)
    return RADEGS_ERR_HIP;
  uint32_t *parent = w.s0, *root = w.s1, *is_root = w.s2, *incl = w.lo;   // the sort's scratch and its inputs are free again
  hipLaunchKernelGGL(rgmc::iota_kernel, dim3(rg::blocks_of((size_t)F)), dim3(256), 0, s, (uint32_t)F, parent);
  hipLaunchKernelGGL(rgmc::link_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, n, manifold, w.joined, w.perm, parent);
  hipLaunchKernelGGL(rgmc::roots_kernel, dim3(rg::blocks_of((size_t)F)), dim3(256), 0, s, (uint32_t)F, parent, root, is_root);
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, is_root, nullptr, incl, (size_t)F, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgmc::number_kernel, dim3(rg::blocks_of((size_t)F)), dim3(256), 0, s, (uint32_t)F, root, incl, triangle_clusters, n_clusters);
  return rg::launch_status();
}

size_t radegs_meshclean_stats_bytes(long long F, long long C) {
  if (F <= 0 || F > rgmc::kMaxFaces || C <= 0 || C > F) return 0;
  return rgmc::stats_carve(F, C, nullptr).bytes;
}

int radegs_meshclean_stats(long long V, long long F, long long C, const double* vertices, const long long* faces, const long long* triangle_clusters,
                           void* workspace, size_t workspace_bytes, long long* cluster_n_triangles, double* cluster_area, double* total_area,
                           void* stream_v) {
  if (V < 0 || F < 0 || C < 0 || C > F || (F > 0 && C == 0)) return RADEGS_ERR_INVALID_ARG;
  if (!rgmc::sizes_ok(V, F)) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (F == 0) return total_area && hipMemsetAsync(total_area, 0, sizeof(double), s) != hipSuccess ? RADEGS_ERR_HIP : 0;
  const bool areas = cluster_area || total_area;
  if (!triangle_clusters || !cluster_n_triangles || (areas && (!vertices || !faces)) || !workspace ||
      workspace_bytes < radegs_meshclean_stats_bytes(F, C) || !rg::aligned16(workspace))
    return RADEGS_ERR_INVALID_ARG;
  const rgmc::StatsView w = rgmc::stats_carve(F, C, workspace);
  if (hipMemsetAsync(w.cnt, 0, (size_t)C * sizeof(uint32_t), s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgmc::count_kernel, dim3(rg::blocks_of((size_t)F)), dim3(256), 0, s, F, C, triangle_clusters, w.key, w.cnt);
  hipLaunchKernelGGL(rgmc::counts_out_kernel, dim3(rg::blocks_of((size_t)C)), dim3(256), 0, s, C, w.cnt, w.grp, cluster_n_triangles);
  if (cluster_area) {
    if (rg::radix_sort_pairs_u32(w.temp, w.temp_bytes, w.key, w.key_sorted, nullptr, w.tri_sorted, (size_t)F, rgmc::bits_for((unsigned long long)(C - 1)), s) !=
            hipSuccess ||
        rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, w.cnt, nullptr, w.cnt_incl, (size_t)C, s) != hipSuccess ||
        rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, w.grp, nullptr, w.grp_incl, (size_t)C, s) != hipSuccess)
      return RADEGS_ERR_HIP;
    hipLaunchKernelGGL(rgmc::group_area_kernel, dim3((unsigned)rgmc::max_groups(F, C)), dim3(256), 0, s, V, (uint32_t)C, vertices, faces, w.tri_sorted, w.cnt,
                       w.cnt_incl, w.grp, w.grp_incl, w.group_sum);
    hipLaunchKernelGGL(rgmc::cluster_area_kernel, dim3(rg::blocks_of((size_t)C)), dim3(256), 0, s, (uint32_t)C, w.grp, w.grp_incl, w.group_sum, cluster_area);
  }
  if (total_area) {
    const int nb = rg::sum_blocks(F);
    hipLaunchKernelGGL(rgmc::total_partial_kernel, dim3(nb), dim3(256), 0, s, V, F, vertices, faces, w.partial);
    hipLaunchKernelGGL(rgmc::total_final_kernel, dim3(1), dim3(256), 0, s, nb, w.partial, total_area);
  }
  return rg::launch_status();
}

size_t radegs_meshclean_compact_bytes(long long V, long long F) {
  if (V < 0 || F < 0 || !rgmc::sizes_ok(V, F) || V + F == 0) return 0;
  return rg::filter_carve(V, F, nullptr).bytes;
}

int radegs_meshclean_compact_plan(long long V, long long F, long long C, const long long* faces, const unsigned char* remove,
                                  const long long* triangle_clusters, const unsigned char* cluster_keep, int drop_degenerate, int drop_unreferenced,
                                  void* workspace, size_t workspace_bytes, long long* counts2, void* stream_v) {
  if (V < 0 || F < 0 || C < 0 || !counts2 || (cluster_keep && !triangle_clusters)) return RADEGS_ERR_INVALID_ARG;
  if (!rgmc::sizes_ok(V, F)) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (V + F == 0) return hipMemsetAsync(counts2, 0, 2 * sizeof(long long), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if ((F && !faces) || !workspace || workspace_bytes < radegs_meshclean_compact_bytes(V, F) || !rg::aligned16(workspace)) return RADEGS_ERR_INVALID_ARG;
  const rg::FilterView w = rg::filter_carve(V, F, workspace);
  if (V) hipLaunchKernelGGL(rgmc::fill_kernel, dim3(rg::blocks_of((size_t)V)), dim3(256), 0, s, (size_t)V, drop_unreferenced ? 0u : 1u, w.flags);
  if (F)
    hipLaunchKernelGGL(rgmc::face_flags_kernel, dim3(rg::blocks_of((size_t)F)), dim3(256), 0, s, V, F, C, faces, remove, triangle_clusters, cluster_keep,
                       drop_degenerate, drop_unreferenced, w.flags);
  return rg::filter_scan_counts(V, F, w, counts2, s);
}

int radegs_meshclean_compact_apply(long long V, long long F, const long long* faces, const void* workspace, long long nv_out, long long nf_out,
                                   long long* kept_vertices, long long* out_faces, void* stream) {
  if (V < 0 || F < 0 || nv_out < 0 || nf_out < 0 || nv_out > V || nf_out > F) return RADEGS_ERR_INVALID_ARG;
  if (!rgmc::sizes_ok(V, F)) return RADEGS_ERR_TOO_LARGE;
  if (nv_out == 0 && nf_out == 0) return 0;
  if ((nf_out && (!faces || !out_faces)) || !workspace || (nv_out && !kept_vertices)) return RADEGS_ERR_INVALID_ARG;
  const rg::FilterView w = rg::filter_carve(V, F, const_cast<void*>(workspace));
  hipLaunchKernelGGL(rgmc::compact_apply_kernel, dim3(rg::blocks_of((size_t)(V + (nf_out ? F : 0)))), dim3(256), 0, static_cast<hipStream_t>(stream), V,
                     nf_out ? F : 0, nv_out, nf_out, faces, w.flags, w.incl, kept_vertices, out_faces);
  return rg::launch_status();
}

size_t radegs_meshclean_normals_bytes(long long F) {
  if (F <= 0 || F > rgmc::kMaxFaces) return 0;
  return rgmc::normals_carve(F, nullptr).bytes;
}

int radegs_meshclean_vertex_normals(long long V, long long F, const double* vertices, const long long* faces, int normalized, void* workspace,
                                    size_t workspace_bytes, double* normals, void* stream_v) {
  if (V < 0 || F < 0) return RADEGS_ERR_INVALID_ARG;
  if (!rgmc::sizes_ok(V, F)) return RADEGS_ERR_TOO_LARGE;
  if (V == 0) return 0;
  if (!normals || !vertices || (F && (!faces || !workspace || workspace_bytes < radegs_meshclean_normals_bytes(F) || !rg::aligned16(workspace))))
    return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  rgmc::NormalsView w = rgmc::normals_carve(F ? F : 1, F ? workspace : nullptr);
  const size_t n = 3 * (size_t)F;
  if (F) {
    hipLaunchKernelGGL(rgmc::corner_keys_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, V, n, faces, w.key);
    if (rg::radix_sort_pairs_u32(w.temp, w.temp_bytes, w.key, w.key_sorted, nullptr, w.rec_sorted, n, rgmc::bits_for((unsigned long long)V), s) != hipSuccess)
      return RADEGS_ERR_HIP;
  }
  hipLaunchKernelGGL(rgmc::vertex_normals_kernel, dim3(rg::blocks_of((size_t)V)), dim3(256), 0, s, V, (uint32_t)n, vertices, faces, w.key_sorted, w.rec_sorted,
                     normalized, normals);
  return rg::launch_status();
}

}  // extern "C"
