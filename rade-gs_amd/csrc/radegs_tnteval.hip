// radegs_tnteval.hip -- Tanks-and-Temples mesh evaluation: the consumer of the marching-tetrahedra mesh, eval_tnt/run.py with
// registration.py and evaluation.py, which upstream hands to Open3D on the CPU.
//     run.py:94-108                        vertices + face centroids                centroid_kernel
//     registration.py:113-131              transform, crop, voxel / uniform thinning transform_kernel, crop_kernel, voxel_key_kernel -> the two-word
//                                                                                   sort (with the joined key) -> first -> scan -> voxel_emit_kernel
//     registration.py:154-161, 193-200     ICP, point to point with scaling         transform_kernel, (mesh_eval's grid), pair_sums / pair_moments
//     evaluation.py:96-98, 173-196         distances, histogram, F-score            (mesh_eval's grid), histogram_kernel
//
// The specification is include/radegs.h, "Tanks-and-Temples evaluation"; tests/tnteval_restatement.py restates it in NumPy.  Geometry is fp64
// as in radegs_mesheval.hip, and for the same reason: every step is a decision on an exact coordinate or distance.  -ffp-contract=off: one
// rounding per operation, products before sums in the order written.  The only atomics are integer ones (the histogram and its counter):
// their result does not depend on the order, so every output of this file is repeatable bit for bit.
//
// fp64 points are 24-byte rows: a wave's three loads of x, y, z cover one contiguous 1536-byte range, every line of which is used by the
// three together.  The nearest-neighbour search, not these streams, is where the time goes (profiles/tnteval_bench.json).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_prims.h"
#include "rg_reduce.h"
#include "rg_workspace.h"

namespace rgte {

using rg::blocks_of;
using rg::kMaxItems;
constexpr int kMaxPolygon = 1024;        // vertices of the crop polygon staged in LDS (16 KB)
constexpr int kMaxEdges = 4096;          // histogram edges staged in LDS (32 KB) next to their counters (16 KB)
constexpr int kVoxelBits = 21;
constexpr unsigned long long kNoKey = ~0ull;

struct Affine {
  double m[12];   // rows 0-2 of the 4x4, by rows
};

// --------------------------------------------------------------- cloud of a mesh ---------------------------------------------------------------
// run.py:97: vertices[faces].mean(axis=1) -- numpy adds the three rows in order, then divides
__global__ void __launch_bounds__(256) centroid_kernel(long long V, long long F, const double* __restrict__ vertices, const long long* __restrict__ faces,
                                                       double* __restrict__ out) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const long long a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  const bool ok = a >= 0 && b >= 0 && c >= 0 && a < V && b < V && c < V;   // the Python layer refuses such input; a C caller gets no wild read
#pragma unroll
  for (int k = 0; k < 3; k++) out[3 * f + k] = ok ? ((vertices[3 * a + k] + vertices[3 * b + k]) + vertices[3 * c + k]) / 3.0 : NAN;
}

// ((m0 x + m1 y) + m2 z) + m3 per row: Eigen's 4x4 product with (x, y, z, 1), column by column
__global__ void __launch_bounds__(256) transform_kernel(long long N, const double* __restrict__ pts, Affine T, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
#pragma unroll
  for (int r = 0; r < 3; r++) out[3 * i + r] = ((T.m[4 * r] * x + T.m[4 * r + 1] * y) + T.m[4 * r + 2] * z) + T.m[4 * r + 3];
}

// ---------------------------------------------------------------------- crop ----------------------------------------------------------------------
// One thread per point walks the polygon (u, v pairs) in LDS; every lane reads the same vertex, a broadcast.  Even-odd rule on the crossings
// of the line v = p[v] that lie left of the point.
__global__ void __launch_bounds__(256) crop_kernel(long long N, const double* __restrict__ pts, int u, int v, int w, double axis_min, double axis_max,
                                                   int n, const double* __restrict__ polygon, uint8_t* __restrict__ keep) {
  __shared__ double poly[2 * kMaxPolygon];
  for (int k = threadIdx.x; k < 2 * n; k += 256) poly[k] = polygon[k];
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double pu = pts[3 * i + u], pv = pts[3 * i + v], pw = pts[3 * i + w];
  bool inside = false;
  if (!(pw < axis_min) && !(pw > axis_max)) {
    for (int a = 0; a < n; a++) {
      const int b = a + 1 == n ? 0 : a + 1;
      const double au = poly[2 * a], av = poly[2 * a + 1], bu = poly[2 * b], bv = poly[2 * b + 1];
      if ((av > pv) != (bv > pv)) {
        const double node = au + (pv - av) / (bv - av) * (bu - au);
        if (node < pu) inside = !inside;
      }
    }
  }
  keep[i] = inside;
}

// ------------------------------------------------------------------ voxel thinning ------------------------------------------------------------------
// key = ix << 42 | iy << 21 | iz, as two words; an index outside 21 bits (or not a number) sets the flag and takes the largest key
__global__ void __launch_bounds__(256) voxel_key_kernel(uint32_t N, const double* __restrict__ pts, double ox, double oy, double oz, double voxel,
                                                        uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const double c[3] = {floor((pts[3 * (size_t)i] - ox) / voxel), floor((pts[3 * (size_t)i + 1] - oy) / voxel), floor((pts[3 * (size_t)i + 2] - oz) / voxel)};
  const double top = (double)(1 << kVoxelBits);
  bool fits = true;
#pragma unroll
  for (int k = 0; k < 3; k++) fits = fits && c[k] >= 0.0 && c[k] < top;   // false for NaN
  const unsigned long long key =
      fits ? ((unsigned long long)c[0] << (2 * kVoxelBits)) | ((unsigned long long)c[1] << kVoxelBits) | (unsigned long long)c[2] : kNoKey >> 1;
  lo[i] = (uint32_t)key;
  hi[i] = (uint32_t)(key >> 32);
  if (!fits) *flag = 1u;
}

__global__ void __launch_bounds__(256) first_kernel(uint32_t N, const unsigned long long* __restrict__ sorted, uint32_t* __restrict__ first) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < N) first[i] = i == 0 || sorted[i] != sorted[i - 1];
}

__global__ void voxel_counts_kernel(uint32_t N, const uint32_t* __restrict__ incl, const uint32_t* __restrict__ flag, long long* __restrict__ counts2) {
  counts2[0] = (long long)incl[N - 1];
  counts2[1] = (long long)*flag;
}

// One thread per voxel: its points are a run of the sorted keys, in index order (the sort is stable); summed in that order, then divided.
__global__ void __launch_bounds__(256) voxel_emit_kernel(uint32_t N, uint32_t M, const double* __restrict__ pts, const unsigned long long* __restrict__ sorted,
                                                         const uint32_t* __restrict__ perm, const uint32_t* __restrict__ first,
                                                         const uint32_t* __restrict__ incl, double* __restrict__ means, int* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N || !first[i]) return;
  const uint32_t vox = incl[i] - 1u;
  if (vox >= M) return;
  const unsigned long long key = sorted[i];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  uint32_t k = i;
  for (; k < N && sorted[k] == key; k++) {
    const size_t p = perm[k];
    sx += pts[3 * p];
    sy += pts[3 * p + 1];
    sz += pts[3 * p + 2];
  }
  const double n = (double)(k - i);
  means[3 * (size_t)vox] = sx / n;
  means[3 * (size_t)vox + 1] = sy / n;
  means[3 * (size_t)vox + 2] = sz / n;
  counts[vox] = (int)(k - i);
}

struct VoxelView {
  unsigned long long* sorted;
  uint32_t *lo, *hi, *hi_sorted, *perm, *first, *incl, *spare, *flag;   // first, incl, spare: the sort's scratch before
  void* temp;
  size_t temp_bytes, bytes;
};
static VoxelView voxel_carve(long long N, void* base) {
  const size_t n = (size_t)N, ts = rg::sort_temp_bytes(n), tc = rg::scan_temp_bytes(n);
  rg::Carver c(base);
  VoxelView v;
  v.temp_bytes = ts > tc ? ts : tc;
  v.sorted = c.take<unsigned long long>(n);
  for (uint32_t** a : {&v.lo, &v.hi, &v.hi_sorted, &v.perm, &v.first, &v.incl, &v.spare}) *a = c.take<uint32_t>(n);
  v.flag = c.take<uint32_t>(1);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

// ------------------------------------------------------------ sums over the matched pairs ------------------------------------------------------------
// K sums in the fixed order of rg_reduce.h: per-block partials over a grid-stride loop, then one block over the partials.
// a pair: query q with index[q] in [0, NT); s = moved[q], t = target[index[q]]
struct Pair {
  double s[3], t[3];
};
__device__ __forceinline__ bool load_pair(long long q, const double* __restrict__ moved, const double* __restrict__ target, long long NT,
                                          const long long* __restrict__ index, Pair& p) {
  const long long j = index[q];
  if (j < 0 || j >= NT) return false;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    p.s[k] = moved[3 * q + k];
    p.t[k] = target[3 * j + k];
  }
  return true;
}

// {count, sum s [3], sum t [3], sum d^2}
__global__ void __launch_bounds__(256) pair_sums_partial_kernel(long long Q, const double* __restrict__ moved, const double* __restrict__ target, long long NT,
                                                                const long long* __restrict__ index, double* __restrict__ partial) {
  __shared__ double sh[8 * 256];
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < Q; q += (long long)gridDim.x * 256) {
    Pair p;
    if (!load_pair(q, moved, target, NT, index, p)) continue;
    const double dx = p.s[0] - p.t[0], dy = p.s[1] - p.t[1], dz = p.s[2] - p.t[2];
    a[0] += 1.0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      a[1 + k] += p.s[k];
      a[4 + k] += p.t[k];
    }
    a[7] += (dx * dx + dy * dy) + dz * dz;
  }
  rg::block_sum(a, sh);
  if (threadIdx.x < 8) partial[8 * blockIdx.x + threadIdx.x] = a[threadIdx.x];
}
// out[0..8) = the sums; means6 = sum s / count, sum t / count (zeros without a pair)
__global__ void __launch_bounds__(256) pair_sums_final_kernel(int nblocks, const double* __restrict__ partial, double* __restrict__ out, double* __restrict__ means6) {
  __shared__ double sh[8 * 256];
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  rg::add_partials(partial, nblocks, a);
  rg::block_sum(a, sh);
  if (threadIdx.x < 8) out[threadIdx.x] = a[threadIdx.x];
  if (threadIdx.x < 6) means6[threadIdx.x] = a[0] > 0.0 ? a[1 + threadIdx.x] / a[0] : 0.0;
}

// {sum (t - mt)(s - ms)^T [3][3] by rows, sum |s - ms|^2}
__global__ void __launch_bounds__(256) pair_moments_partial_kernel(long long Q, const double* __restrict__ moved, const double* __restrict__ target,
                                                                   long long NT, const long long* __restrict__ index, const double* __restrict__ means6,
                                                                   double* __restrict__ partial) {
  __shared__ double sh[10 * 256];
  double a[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double ms[3] = {means6[0], means6[1], means6[2]}, mt[3] = {means6[3], means6[4], means6[5]};
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < Q; q += (long long)gridDim.x * 256) {
    Pair p;
    if (!load_pair(q, moved, target, NT, index, p)) continue;
    const double ds[3] = {p.s[0] - ms[0], p.s[1] - ms[1], p.s[2] - ms[2]}, dt[3] = {p.t[0] - mt[0], p.t[1] - mt[1], p.t[2] - mt[2]};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) a[3 * r + c] += dt[r] * ds[c];
    a[9] += (ds[0] * ds[0] + ds[1] * ds[1]) + ds[2] * ds[2];
  }
  rg::block_sum(a, sh);
  if (threadIdx.x < 10) partial[10 * blockIdx.x + threadIdx.x] = a[threadIdx.x];
}
__global__ void __launch_bounds__(256) pair_moments_final_kernel(int nblocks, const double* __restrict__ partial, double* __restrict__ out) {
  __shared__ double sh[10 * 256];
  double a[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  rg::add_partials(partial, nblocks, a);
  rg::block_sum(a, sh);
  if (threadIdx.x < 10) out[threadIdx.x] = a[threadIdx.x];
}

struct SumsView {
  double *partial, *means6;
  size_t bytes;
};
static SumsView sums_carve(void* base) {
  rg::Carver c(base);
  SumsView v;
  v.partial = c.take<double>(10 * (size_t)rg::kSumBlocks);
  v.means6 = c.take<double>(6);
  v.bytes = c.off;
  return v;
}

// -------------------------------------------------------------------- histogram --------------------------------------------------------------------
// np.histogram over explicit edges: bin b holds edges[b] <= d < edges[b + 1], the last bin its right edge as well; anything else (NaN too) is
// in no bin.  Edges and one histogram per block in LDS; what a block counted goes to the 64-bit histogram with one atomic per non-empty bin.
__global__ void __launch_bounds__(256) histogram_kernel(long long N, const double* __restrict__ dist, int n_edges, const double* __restrict__ edges,
                                                        double threshold, unsigned long long* __restrict__ hist, unsigned long long* __restrict__ below) {
  __shared__ double e[kMaxEdges];
  __shared__ uint32_t h[kMaxEdges];
  __shared__ uint32_t under;
  const int bins = n_edges - 1;
  for (int k = threadIdx.x; k < n_edges; k += 256) {
    e[k] = edges[k];
    h[k] = 0u;
  }
  if (threadIdx.x == 0) under = 0u;
  __syncthreads();
  const double first = e[0], last = e[bins];
  uint32_t mine = 0u;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < N; q += (long long)gridDim.x * 256) {
    const double d = dist[q];
    mine += d < threshold ? 1u : 0u;
    if (!(d >= first) || !(d <= last)) continue;
    int lo = 0, hi = n_edges;   // the first edge above d
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (e[mid] <= d) lo = mid + 1; else hi = mid;
    }
    const int b = lo - 1 < bins ? lo - 1 : bins - 1;   // d == last: the last bin is closed
    atomicAdd(&h[b], 1u);
  }
  if (mine) atomicAdd(&under, mine);
  __syncthreads();
  for (int k = threadIdx.x; k < bins; k += 256)
    if (h[k]) atomicAdd(&hist[k], (unsigned long long)h[k]);
  if (threadIdx.x == 0 && under) atomicAdd(below, (unsigned long long)under);
}

}  // namespace rgte

extern "C" {

int radegs_tnteval_centroids(long long V, long long F, const double* vertices, const long long* faces, double* out, void* stream) {
  if (V < 0 || F < 0) return RADEGS_ERR_INVALID_ARG;
  if (F == 0) return 0;
  if (!vertices || !faces || !out) return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgte::centroid_kernel, dim3(rg::blocks_of((size_t)F)), dim3(256), 0, static_cast<hipStream_t>(stream), V, F, vertices, faces, out);
  return rg::launch_status();
}

int radegs_tnteval_transform(long long N, const double* points, const double* matrix12, double* out, void* stream) {
  if (N < 0 || !matrix12) return RADEGS_ERR_INVALID_ARG;
  rgte::Affine T;
  for (int k = 0; k < 12; k++) {
    if (!isfinite(matrix12[k])) return RADEGS_ERR_INVALID_ARG;
    T.m[k] = matrix12[k];
  }
  if (N == 0) return 0;
  if (!points || !out) return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgte::transform_kernel, dim3(rg::blocks_of((size_t)N)), dim3(256), 0, static_cast<hipStream_t>(stream), N, points, T, out);
  return rg::launch_status();
}

int radegs_tnteval_crop(long long N, const double* points, int orthogonal_axis, double axis_min, double axis_max, int n_polygon, const double* polygon_uv,
                        unsigned char* keep, void* stream) {
  if (N < 0 || orthogonal_axis < 0 || orthogonal_axis > 2 || n_polygon < 3 || axis_min != axis_min || axis_max != axis_max) return RADEGS_ERR_INVALID_ARG;
  if (n_polygon > rgte::kMaxPolygon) return RADEGS_ERR_TOO_LARGE;
  if (N == 0) return 0;
  if (!points || !polygon_uv || !keep) return RADEGS_ERR_INVALID_ARG;
  const int u = orthogonal_axis == 0 ? 1 : 0, v = orthogonal_axis == 2 ? 1 : 2, w = orthogonal_axis;   // X: (1, 2, 0), Y: (0, 2, 1), Z: (0, 1, 2)
  hipLaunchKernelGGL(rgte::crop_kernel, dim3(rg::blocks_of((size_t)N)), dim3(256), 0, static_cast<hipStream_t>(stream), N, points, u, v, w, axis_min, axis_max,
                     n_polygon, polygon_uv, keep);
  return rg::launch_status();
}

size_t radegs_tnteval_voxel_bytes(long long N) {
  if (N <= 0 || (unsigned long long)N >= rg::kMaxItems) return 0;
  return rgte::voxel_carve(N, nullptr).bytes;
}

int radegs_tnteval_voxel_plan(long long N, const double* points, const double* origin3, double voxel, void* workspace, size_t workspace_bytes,
                              long long* counts2, void* stream_v) {
  if (N < 0 || !counts2 || !origin3 || !(voxel > 0.0) || !isfinite(voxel) || !isfinite(origin3[0]) || !isfinite(origin3[1]) || !isfinite(origin3[2]))
    return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)N >= rg::kMaxItems) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (N == 0) return hipMemsetAsync(counts2, 0, 2 * sizeof(long long), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if (!points || !workspace || workspace_bytes < radegs_tnteval_voxel_bytes(N) || !rg::aligned16(workspace)) return RADEGS_ERR_INVALID_ARG;
  const rgte::VoxelView w = rgte::voxel_carve(N, workspace);
  const uint32_t n = (uint32_t)N;
  const unsigned nb = rg::blocks_of((size_t)N);
  if (hipMemsetAsync(w.flag, 0, sizeof(uint32_t), s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgte::voxel_key_kernel, dim3(nb), dim3(256), 0, s, n, points, origin3[0], origin3[1], origin3[2], voxel, w.lo, w.hi, w.flag);
  if (rg::radix_sort_order_2xu32(w.temp, w.temp_bytes, w.lo, w.hi, w.hi_sorted, w.perm, w.first, w.incl, w.spare, (size_t)N, 32, 32, s, nullptr,
                                 w.sorted) != hipSuccess)
    return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgte::first_kernel, dim3(nb), dim3(256), 0, s, n, w.sorted, w.first);
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, w.first, nullptr, w.incl, (size_t)N, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgte::voxel_counts_kernel, dim3(1), dim3(1), 0, s, n, w.incl, w.flag, counts2);
  return rg::launch_status();
}

int radegs_tnteval_voxel_emit(long long N, const double* points, const void* workspace, long long M, double* means, int* counts, void* stream) {
  if (N < 0 || M < 0 || M > N) return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)N >= rg::kMaxItems) return RADEGS_ERR_TOO_LARGE;
  if (N == 0 || M == 0) return 0;
  if (!points || !workspace || !means || !counts) return RADEGS_ERR_INVALID_ARG;
  const rgte::VoxelView w = rgte::voxel_carve(N, const_cast<void*>(workspace));
  hipLaunchKernelGGL(rgte::voxel_emit_kernel, dim3(rg::blocks_of((size_t)N)), dim3(256), 0, static_cast<hipStream_t>(stream), (uint32_t)N, (uint32_t)M, points,
                     w.sorted, w.perm, w.first, w.incl, means, counts);
  return rg::launch_status();
}

size_t radegs_tnteval_sums_bytes(void) { return rgte::sums_carve(nullptr).bytes; }

int radegs_tnteval_pair_sums(long long Q, const double* moved, long long NT, const double* target, const long long* index, void* workspace,
                             size_t workspace_bytes, double* out18, void* stream_v) {
  if (Q < 0 || NT < 0 || !out18) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (Q == 0 || NT == 0) return hipMemsetAsync(out18, 0, 18 * sizeof(double), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if (!moved || !target || !index || !workspace || workspace_bytes < radegs_tnteval_sums_bytes() || !rg::aligned16(workspace)) return RADEGS_ERR_INVALID_ARG;
  const rgte::SumsView w = rgte::sums_carve(workspace);
  const int nb = rg::sum_blocks(Q);
  hipLaunchKernelGGL(rgte::pair_sums_partial_kernel, dim3(nb), dim3(256), 0, s, Q, moved, target, NT, index, w.partial);
  hipLaunchKernelGGL(rgte::pair_sums_final_kernel, dim3(1), dim3(256), 0, s, nb, w.partial, out18, w.means6);
  hipLaunchKernelGGL(rgte::pair_moments_partial_kernel, dim3(nb), dim3(256), 0, s, Q, moved, target, NT, index, w.means6, w.partial);
  hipLaunchKernelGGL(rgte::pair_moments_final_kernel, dim3(1), dim3(256), 0, s, nb, w.partial, out18 + 8);
  return rg::launch_status();
}

int radegs_tnteval_histogram(long long N, const double* dist, int n_edges, const double* edges, double threshold, long long* hist, long long* below,
                             void* stream_v) {
  if (N < 0 || n_edges < 2 || !hist || !below || !edges || threshold != threshold) return RADEGS_ERR_INVALID_ARG;
  if (n_edges > rgte::kMaxEdges) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (hipMemsetAsync(hist, 0, (size_t)(n_edges - 1) * sizeof(long long), s) != hipSuccess || hipMemsetAsync(below, 0, sizeof(long long), s) != hipSuccess)
    return RADEGS_ERR_HIP;
  if (N == 0) return 0;
  if (!dist) return RADEGS_ERR_INVALID_ARG;
  const int nb = rg::sum_blocks(N);
  hipLaunchKernelGGL(rgte::histogram_kernel, dim3(nb), dim3(256), 0, s, N, dist, n_edges, edges, threshold, reinterpret_cast<unsigned long long*>(hist),
                     reinterpret_cast<unsigned long long*>(below));
  return rg::launch_status();
}

}  // extern "C"
