// radegs_mesheval.hip -- mesh evaluation: the consumer of recon.ply, evaluate_dtu_mesh.py + dtu_eval/eval.py.
//     dtu_eval/eval.py:50-71           sample the triangles at `density`         tri_count_kernel -> scan -> tri_emit_kernel
//     dtu_eval/eval.py:86-94           thin the shuffled cloud by a radius       cell_key / reorder (the grid), thin_round_kernel
//     dtu_eval/eval.py:102-110         bounding box + observation volume         obs_mask_kernel
//     dtu_eval/eval.py:119-134         nearest neighbour both ways, the means    nearest_kernel, below_partial / below_final
//     dtu_eval/eval.py:128-130         plane side                                plane_side_kernel
//     evaluate_dtu_mesh.py:82-138      cull the mesh against the training masks  dilate_kernel, cull_vertices_kernel (+ the tetmesh filter)
//
// All geometry of eval.py is fp64, as there: every step is a decision on an exact distance (kept / removed, inside / outside, which
// neighbour) and DTU coordinates of hundreds of mm against a 0.2 mm radius leave fp32 no room.  -ffp-contract=off: one rounding per
// operation, so the sums below are the reference's (numpy multiplies, then adds, in axis order).  The cull is fp32, as upstream's.
//
// The grid.  cell = floor((p - origin) / cell_size) per axis, wrapped into a 32-bit key (11 + 11 + 10 bits: DTU's box at 0.2 mm has
// about 3 000 cells per axis, a dense table is out of the question).  The cloud is sorted by key with rg::radix_sort_pairs_u32 (stable:
// inside a cell the points stay in index order) and gathered into cell order; a cell's range is a lower_bound in the sorted keys.  Two
// cells one key period apart share a key: harmless, every candidate is decided by its exact distance.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_prims.h"
#include "rg_reduce.h"
#include "rg_workspace.h"

namespace rgme {

using rg::kMaxItems;
constexpr double kMaxSubdiv = 30000.0;   // n1, n2 beyond this: the per-triangle count would leave 32 bits

// ---------------------------------------------------------------- triangle sampling ----------------------------------------------------------------
struct Tri {
  double v1[3], v2[3], p0[3], m1, m2;
  int n1, n2;   // rows i = 0..n1, columns j = 0..n2; n1 < 0: no samples
};

// eval.py:54-65 for one triangle.  `big` is set when a subdivision count leaves the supported range.
__device__ __forceinline__ void tri_setup(long long V, const double* __restrict__ vertices, const long long* __restrict__ faces, long long t,
                                          double density, Tri& T, bool& big) {
  T.n1 = T.n2 = -1;
  big = false;
  const long long a = faces[3 * t], b = faces[3 * t + 1], c = faces[3 * t + 2];
  if (a < 0 || b < 0 || c < 0 || a >= V || b >= V || c >= V) return;   // the Python layer refuses such input; a C caller gets no wild read
#pragma unroll
  for (int k = 0; k < 3; k++) {
    T.p0[k] = vertices[3 * a + k];
    T.v1[k] = vertices[3 * b + k] - T.p0[k];
    T.v2[k] = vertices[3 * c + k] - T.p0[k];
  }
  const double l1 = sqrt((T.v1[0] * T.v1[0] + T.v1[1] * T.v1[1]) + T.v1[2] * T.v1[2]);
  const double l2 = sqrt((T.v2[0] * T.v2[0] + T.v2[1] * T.v2[1]) + T.v2[2] * T.v2[2]);
  const double c0 = T.v1[1] * T.v2[2] - T.v1[2] * T.v2[1], c1 = T.v1[2] * T.v2[0] - T.v1[0] * T.v2[2], c2 = T.v1[0] * T.v2[1] - T.v1[1] * T.v2[0];
  const double area2 = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  if (!(area2 > 0.0)) return;
  const double thr = density * sqrt(l1 * l2 / area2);
  const double n1 = floor(l1 / thr), n2 = floor(l2 / thr);
  if (!(n1 >= 1.0) || !(n2 >= 1.0)) return;   // n = 0: max(n, 1e-7) sends the lattice outside the triangle; NaN: no samples either
  if (n1 > kMaxSubdiv || n2 > kMaxSubdiv) { big = true; return; }
  T.n1 = (int)n1;
  T.n2 = (int)n2;
  T.m1 = n1;   // max(n, 1e-7) for n >= 1
  T.m2 = n2;
}

// The lattice test of eval.py:14-17, as written there: two fp64 divisions and one addition.  No margin, no integer rewrite.
__device__ __forceinline__ bool inside(double k0, int j, double m2) { return k0 + ((double)j + 0.5) / m2 < 1.0; }

// number of j in [0, n2] with inside(k0, j): the test is monotone in j (a correctly rounded quotient is monotone in its numerator, the
// sum in its addend), so the count is the first failing j -- estimated, then walked to exactly
__device__ __forceinline__ int row_count(double k0, double m2, int n2) {
  const double je = (1.0 - k0) * m2 - 0.5;
  int c = je <= 0.0 ? 0 : (je >= (double)(n2 + 1) ? n2 + 1 : (int)ceil(je));
  while (c > 0 && !inside(k0, c - 1, m2)) c--;
  while (c <= n2 && inside(k0, c, m2)) c++;
  return c;
}

// counts[t]; totals[0] += the count as 64 bits (the u32 scan cannot tell a wrap), totals[1] != 0: a triangle out of range
__global__ void __launch_bounds__(256) tri_count_kernel(long long V, long long F, const double* __restrict__ vertices, const long long* __restrict__ faces,
                                                        double density, uint32_t* __restrict__ counts, unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long block_sum;
  if (threadIdx.x == 0) block_sum = 0ull;
  __syncthreads();
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < F) {
    Tri T;
    bool big;
    tri_setup(V, vertices, faces, t, density, T, big);
    if (big) atomicAdd(&totals[1], 1ull);
    uint32_t n = 0;
    for (int i = 0; i <= T.n1; i++) n += (uint32_t)row_count(((double)i + 0.5) / T.m1, T.m2, T.n2);
    counts[t] = n;
    if (n) atomicAdd(&block_sum, (unsigned long long)n);
  }
  __syncthreads();
  if (threadIdx.x == 0 && block_sum) atomicAdd(&totals[0], block_sum);
}

// One thread per sample g: its triangle by a search of the inclusive scan, its row by walking the row counts, then eval.py:18.
__global__ void __launch_bounds__(256) tri_emit_kernel(long long V, long long F, long long M, const double* __restrict__ vertices,
                                                       const long long* __restrict__ faces, double density, const uint32_t* __restrict__ incl,
                                                       double* __restrict__ out) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= M || g >= (long long)incl[F - 1]) return;
  long long lo = 0, hi = F - 1;   // first t with incl[t] > g
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if ((long long)incl[mid] > g) hi = mid; else lo = mid + 1;
  }
  const long long t = lo;
  Tri T;
  bool big;
  tri_setup(V, vertices, faces, t, density, T, big);
  long long r = g - (t ? (long long)incl[t - 1] : 0ll);
  for (int i = 0; i <= T.n1; i++) {
    const double k0 = ((double)i + 0.5) / T.m1;
    const int c = row_count(k0, T.m2, T.n2);
    if (r < c) {
      const double k1 = ((double)r + 0.5) / T.m2;
#pragma unroll
      for (int k = 0; k < 3; k++) out[3 * g + k] = (T.v1[k] * k0 + T.v2[k] * k1) + T.p0[k];
      return;
    }
    r -= c;
  }
}

struct SampleView {
  uint32_t* incl;
  void* temp;
  size_t temp_bytes, bytes;
};
static SampleView sample_carve(long long F, void* base) {
  rg::Carver c(base);
  SampleView v;
  v.temp_bytes = rg::scan_temp_bytes((size_t)F);
  v.incl = c.take<uint32_t>((size_t)F);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

// -------------------------------------------------------------------- the grid --------------------------------------------------------------------
struct Grid {
  double ox, oy, oz, cell;
};

__device__ __forceinline__ long long cell_of(double p, double o, double cell) {
  double c = floor((p - o) / cell);
  c = c > 1e15 ? 1e15 : (c < -1e15 ? -1e15 : c);   // keeps the conversion defined; NaN -> the comparisons fail -> converted below
  return c == c ? (long long)c : 0ll;
}
__device__ __forceinline__ uint32_t key_of(long long cx, long long cy, long long cz) {
  return (uint32_t)(cx & 2047) | ((uint32_t)(cy & 2047) << 11) | ((uint32_t)(cz & 1023) << 22);
}

__global__ void __launch_bounds__(256) cell_key_kernel(uint32_t N, const double* __restrict__ pts, Grid g, uint32_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  keys[i] = key_of(cell_of(pts[3 * (size_t)i], g.ox, g.cell), cell_of(pts[3 * (size_t)i + 1], g.oy, g.cell), cell_of(pts[3 * (size_t)i + 2], g.oz, g.cell));
}

__global__ void __launch_bounds__(256) reorder_kernel(uint32_t N, const double* __restrict__ pts, const uint32_t* __restrict__ perm, double* __restrict__ sorted) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= N) return;
  const size_t i = perm[s];
#pragma unroll
  for (int k = 0; k < 3; k++) sorted[3 * (size_t)s + k] = pts[3 * i + k];
}

struct GridView {
  uint32_t *keys, *perm, *keys_in;
  double* pts;
  void* temp;
  size_t temp_bytes, bytes;
};
static GridView grid_carve(long long N, void* base) {
  const size_t n = (size_t)N;
  rg::Carver c(base);
  GridView v;
  v.temp_bytes = rg::sort_temp_bytes(n);
  v.keys = c.take<uint32_t>(n);
  v.perm = c.take<uint32_t>(n);
  v.pts = c.take<double>(3 * n);
  v.keys_in = c.take<uint32_t>(n);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}
static bool grid_args_ok(long long N, const double* origin3, double cell) {
  return N > 0 && (unsigned long long)N < kMaxItems && origin3 && cell > 0.0 && isfinite(cell) && isfinite(origin3[0]) && isfinite(origin3[1]) &&
         isfinite(origin3[2]);
}

// ------------------------------------------------------------------ radius thinning ------------------------------------------------------------------
// state (by point index): 0 undecided, 1 kept, 2 removed.  One round: an undecided point is removed when a lower-index neighbour is kept,
// kept when all of them are removed.  A state only ever moves 0 -> 1 or 0 -> 2 and is final then, so reading a neighbour while another
// thread decides it is harmless: a stale 0 only postpones this point to the next round.  The fixed point is the lexicographically first
// maximal independent set of the radius graph -- what eval.py's sequential loop keeps.
__global__ void __launch_bounds__(256) thin_round_kernel(uint32_t N, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                         const double* __restrict__ pts, Grid g, double r2, uint8_t* state, uint32_t* undecided) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  bool decided = false;
  if (s < N) {
    const uint32_t i = perm[s];
    if (__atomic_load_n(&state[i], __ATOMIC_RELAXED) == 0) {
      const double px = pts[3 * (size_t)s], py = pts[3 * (size_t)s + 1], pz = pts[3 * (size_t)s + 2];
      const long long cx = cell_of(px, g.ox, g.cell), cy = cell_of(py, g.oy, g.cell), cz = cell_of(pz, g.oz, g.cell);
      bool kept_below = false, all_removed = true;
      for (int d = 0; d < 27 && !kept_below; d++) {
        const uint32_t key = key_of(cx + (d % 3) - 1, cy + ((d / 3) % 3) - 1, cz + (d / 9) - 1);
        for (uint32_t c = rg::lower_bound(keys, N, key); c < N && keys[c] == key; c++) {
          const uint32_t j = perm[c];
          if (j >= i) continue;
          const double dx = px - pts[3 * (size_t)c], dy = py - pts[3 * (size_t)c + 1], dz = pz - pts[3 * (size_t)c + 2];
          if (!((dx * dx + dy * dy) + dz * dz <= r2)) continue;
          const uint8_t st = __atomic_load_n(&state[j], __ATOMIC_RELAXED);
          if (st == 1) { kept_below = true; break; }
          if (st == 0) all_removed = false;
        }
      }
      if (kept_below || all_removed) {
        __atomic_store_n(&state[i], (uint8_t)(kept_below ? 2 : 1), __ATOMIC_RELAXED);
        decided = true;
      }
    }
  }
  const unsigned long long b = __ballot(decided);
  if ((threadIdx.x & 63u) == 0u && b) atomicSub(undecided, (uint32_t)__popcll(b));
}

// ------------------------------------------------------------------ nearest neighbour ------------------------------------------------------------------
__device__ __forceinline__ void scan_cell(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm, const double* __restrict__ pts, uint32_t N,
                                          uint32_t key, double qx, double qy, double qz, double& best, uint32_t& best_i) {
  for (uint32_t c = rg::lower_bound(keys, N, key); c < N && keys[c] == key; c++) {
    const double dx = qx - pts[3 * (size_t)c], dy = qy - pts[3 * (size_t)c + 1], dz = qz - pts[3 * (size_t)c + 2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const uint32_t j = perm[c];
    if (d2 < best || (d2 == best && j < best_i)) { best = d2; best_i = j; }
  }
}

// Shells of cells around the query's own, growing.  Every point of shell s is farther than (s - 1) cells away along one axis, so the
// search ends before shell s once the best distance is within that, or once that is beyond max_dist.  The 1e-9 keeps the comparison on
// the safe side of the rounding in cell_of.  Equal distances: the lower index (np.argmin's choice in the restatement).
__global__ void __launch_bounds__(256) nearest_kernel(uint32_t N, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                      const double* __restrict__ pts, Grid g, long long Q, const double* __restrict__ queries,
                                                      double max_dist, int max_shell, double* __restrict__ dist, long long* __restrict__ index) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  const double qx = queries[3 * q], qy = queries[3 * q + 1], qz = queries[3 * q + 2];
  const long long cx = cell_of(qx, g.ox, g.cell), cy = cell_of(qy, g.oy, g.cell), cz = cell_of(qz, g.oz, g.cell);
  double best = INFINITY;
  uint32_t best_i = 0xFFFFFFFFu;
  for (int s = 0; s <= max_shell; s++) {
    if (s > 1) {
      const double inner = (double)(s - 1) * g.cell * (1.0 - 1e-9);
      if (best <= inner * inner || inner >= max_dist) break;
    }
    for (int dz = -s; dz <= s; dz++)
      for (int dy = -s; dy <= s; dy++) {
        const bool face = dz == -s || dz == s || dy == -s || dy == s;
        const int step = (face || s == 0) ? 1 : 2 * s;   // inside the slab only the two end cells belong to the shell
        for (int dx = -s; dx <= s; dx += step) scan_cell(keys, perm, pts, N, key_of(cx + dx, cy + dy, cz + dz), qx, qy, qz, best, best_i);
      }
  }
  const double d = sqrt(best);
  const bool hit = best_i != 0xFFFFFFFFu && d < max_dist;
  dist[q] = hit ? d : INFINITY;
  index[q] = hit ? (long long)best_i : -1ll;
}

// sum and count of dist < max_dist in the fixed order of rg_reduce.h: per-block partials over a grid-stride loop, then one block over them
__global__ void __launch_bounds__(256) below_partial_kernel(long long Q, const double* __restrict__ dist, double max_dist, double* __restrict__ partial) {
  __shared__ double sh[512];
  double a[2] = {0.0, 0.0};
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < Q; q += (long long)gridDim.x * 256) {
    const double d = dist[q];
    if (d < max_dist) { a[0] += d; a[1] += 1.0; }
  }
  rg::block_sum(a, sh);
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = a[0]; partial[2 * blockIdx.x + 1] = a[1]; }
}
__global__ void __launch_bounds__(256) below_final_kernel(int nblocks, const double* __restrict__ partial, double* __restrict__ out2) {
  __shared__ double sh[512];
  double a[2] = {0.0, 0.0};
  rg::add_partials(partial, nblocks, a);
  rg::block_sum(a, sh);
  if (threadIdx.x == 0) { out2[0] = a[0]; out2[1] = a[1]; }
}

// ---------------------------------------------------------------------- masks ----------------------------------------------------------------------
struct ObsBox {
  double lo[3], hi[3], bb0[3], res;
  int dim[3];
};

// eval.py:103-109 per point, the three masks at full length: inbound, inbound & grid_inbound, ... & ObsMask[g]
__global__ void __launch_bounds__(256) obs_mask_kernel(long long N, const double* __restrict__ pts, ObsBox b, const uint8_t* __restrict__ volume,
                                                       uint8_t* __restrict__ inbound, uint8_t* __restrict__ grid_in, uint8_t* __restrict__ in_obs) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  bool in = true, gin = true;
  long long gi[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double p = pts[3 * i + k];
    in = in && p >= b.lo[k] && p < b.hi[k];
    double r = rint((p - b.bb0[k]) / b.res);   // np.around: half to even
    r = r > 2e9 ? 2e9 : (r < -2e9 ? -2e9 : r);
    gi[k] = r == r ? (long long)r : -1ll;
    gin = gin && gi[k] >= 0 && gi[k] < b.dim[k];
  }
  gin = gin && in;
  inbound[i] = in;
  grid_in[i] = gin;
  in_obs[i] = gin && volume[((size_t)gi[0] * b.dim[1] + gi[1]) * b.dim[2] + gi[2]] != 0;
}

__global__ void __launch_bounds__(256) plane_side_kernel(long long N, const double* __restrict__ pts, double p0, double p1, double p2, double p3,
                                                         uint8_t* __restrict__ above) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  above[i] = ((p0 * pts[3 * i] + p1 * pts[3 * i + 1]) + p2 * pts[3 * i + 2]) + p3 > 0.0;
}

// ----------------------------------------------------------------------- cull -----------------------------------------------------------------------
// binary dilation by the disk x^2 + y^2 <= radius^2, zero outside the image
__global__ void __launch_bounds__(256) dilate_kernel(int W, int H, const uint8_t* __restrict__ mask, int radius, uint8_t* __restrict__ out) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)W * H) return;
  const int x = (int)(p % W), y = (int)(p / W);
  uint8_t hit = 0;
  for (int dy = -radius; dy <= radius && !hit; dy++) {
    const int yy = y + dy;
    if (yy < 0 || yy >= H) continue;
    for (int dx = -radius; dx <= radius; dx++) {
      const int xx = x + dx;
      if (dx * dx + dy * dy > radius * radius || xx < 0 || xx >= W) continue;
      if (mask[(size_t)yy * W + xx]) { hit = 1; break; }
    }
  }
  out[p] = hit;
}

// evaluate_dtu_mesh.py:111-133 for one vertex over all views, fp32: kept iff every view either sees it outside (-1, 1) or samples a set
// pixel of its dilated mask (nearest, align_corners=True, zero padding, round half to even).  No [V, ncam] intermediate.
__global__ void __launch_bounds__(256) cull_vertices_kernel(long long NV, const float* __restrict__ vertices, int ncam,
                                                            const RadegsCullCamera* __restrict__ cams, const uint8_t* __restrict__ masks,
                                                            uint32_t* __restrict__ flags) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= NV) return;
  const float x = vertices[3 * v], y = vertices[3 * v + 1], z = vertices[3 * v + 2];
  uint32_t keep = 1;
  for (int c = 0; c < ncam && keep; c++) {
    const RadegsCullCamera cam = cams[c];
    const float X = ((cam.m[0] * x + cam.m[1] * y) + cam.m[2] * z) + cam.m[3];
    const float Y = ((cam.m[4] * x + cam.m[5] * y) + cam.m[6] * z) + cam.m[7];
    const float Z = ((cam.m[8] * x + cam.m[9] * y) + cam.m[10] * z) + cam.m[11];
    const float den = Z + 1e-6f;
    const float gx = ((X / den) / (float)(cam.W - 1) - 0.5f) * 2.0f, gy = ((Y / den) / (float)(cam.H - 1) - 0.5f) * 2.0f;
    const bool valid = gx > -1.0f && gx < 1.0f && gy > -1.0f && gy < 1.0f;
    if (!valid) continue;   // sampled + (1 - valid) >= 1
    const float ix = rintf(((gx + 1.0f) / 2.0f) * (float)(cam.W - 1)), iy = rintf(((gy + 1.0f) / 2.0f) * (float)(cam.H - 1));
    uint8_t m = 0;
    if (ix >= 0.0f && iy >= 0.0f && ix <= (float)(cam.W - 1) && iy <= (float)(cam.H - 1)) m = masks[cam.mask_offset + (long long)iy * cam.W + (long long)ix];
    keep = m != 0;
  }
  flags[v] = keep;
}

}  // namespace rgme

extern "C" {

size_t radegs_mesheval_sample_bytes(long long F) {
  if (F <= 0 || (unsigned long long)F >= rg::kMaxItems) return 0;
  return rgme::sample_carve(F, nullptr).bytes;
}

int radegs_mesheval_sample_count(long long V, long long F, const double* vertices, const long long* faces, double density, void* workspace,
                                 size_t workspace_bytes, int* counts, unsigned long long* totals2, void* stream_v) {
  if (V < 0 || F < 0 || !totals2 || !(density > 0.0) || !isfinite(density)) return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)F >= rg::kMaxItems) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (hipMemsetAsync(totals2, 0, 2 * sizeof(unsigned long long), s) != hipSuccess) return RADEGS_ERR_HIP;
  if (F == 0) return 0;
  if (!vertices || !faces || !counts || !workspace || workspace_bytes < radegs_mesheval_sample_bytes(F) || !rg::aligned16(workspace))
    return RADEGS_ERR_INVALID_ARG;
  const rgme::SampleView w = rgme::sample_carve(F, workspace);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(counts);
  hipLaunchKernelGGL(rgme::tri_count_kernel, dim3(rg::blocks_of((size_t)F)), dim3(256), 0, s, V, F, vertices, faces, density, cnt, totals2);
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, cnt, nullptr, w.incl, (size_t)F, s) != hipSuccess) return RADEGS_ERR_HIP;
  return rg::launch_status();
}

int radegs_mesheval_sample_emit(long long V, long long F, const double* vertices, const long long* faces, double density, const void* workspace,
                                long long M, double* out, void* stream) {
  if (V < 0 || F < 0 || M < 0 || !(density > 0.0)) return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)F >= rg::kMaxItems || (unsigned long long)M >= 0xFFFFFFFFull) return RADEGS_ERR_TOO_LARGE;
  if (F == 0 || M == 0) return 0;
  if (!vertices || !faces || !workspace || !out) return RADEGS_ERR_INVALID_ARG;
  const rgme::SampleView w = rgme::sample_carve(F, const_cast<void*>(workspace));
  hipLaunchKernelGGL(rgme::tri_emit_kernel, dim3(rg::blocks_of((size_t)M)), dim3(256), 0, static_cast<hipStream_t>(stream), V, F, M, vertices, faces,
                     density, w.incl, out);
  return rg::launch_status();
}

size_t radegs_mesheval_grid_bytes(long long N) {
  if (N <= 0 || (unsigned long long)N >= rg::kMaxItems) return 0;
  return rgme::grid_carve(N, nullptr).bytes;
}

int radegs_mesheval_grid_build(long long N, const double* points, const double* origin3, double cell, void* workspace, size_t workspace_bytes,
                               void* stream_v) {
  if (N < 0) return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)N >= rg::kMaxItems) return RADEGS_ERR_TOO_LARGE;
  if (N == 0) return 0;
  if (!rgme::grid_args_ok(N, origin3, cell) || !points || !workspace || workspace_bytes < radegs_mesheval_grid_bytes(N) ||
      !rg::aligned16(workspace))
    return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const rgme::GridView w = rgme::grid_carve(N, workspace);
  const rgme::Grid g{origin3[0], origin3[1], origin3[2], cell};
  const unsigned nb = rg::blocks_of((size_t)N);
  hipLaunchKernelGGL(rgme::cell_key_kernel, dim3(nb), dim3(256), 0, s, (uint32_t)N, points, g, w.keys_in);
  if (rg::radix_sort_pairs_u32(w.temp, w.temp_bytes, w.keys_in, w.keys, nullptr, w.perm, (size_t)N, 32, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgme::reorder_kernel, dim3(nb), dim3(256), 0, s, (uint32_t)N, points, w.perm, w.pts);
  return rg::launch_status();
}

int radegs_mesheval_thin_rounds(long long N, const void* grid_workspace, const double* origin3, double cell, double radius, int rounds,
                                unsigned char* state, unsigned* undecided, void* stream_v) {
  if (N < 0 || rounds < 0) return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)N >= rg::kMaxItems) return RADEGS_ERR_TOO_LARGE;
  if (N == 0 || rounds == 0) return 0;
  if (!rgme::grid_args_ok(N, origin3, cell) || !grid_workspace || !state || !undecided || !(radius >= 0.0) || !(radius <= cell))
    return RADEGS_ERR_INVALID_ARG;   // 27 cells cover the radius only while it is no larger than a cell
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const rgme::GridView w = rgme::grid_carve(N, const_cast<void*>(grid_workspace));
  const rgme::Grid g{origin3[0], origin3[1], origin3[2], cell};
  for (int r = 0; r < rounds; r++)
    hipLaunchKernelGGL(rgme::thin_round_kernel, dim3(rg::blocks_of((size_t)N)), dim3(256), 0, s, (uint32_t)N, w.keys, w.perm, w.pts, g, radius * radius,
                       state, undecided);
  return rg::launch_status();
}

int radegs_mesheval_nearest(long long N, const void* grid_workspace, const double* origin3, double cell, long long Q, const double* queries,
                            double max_dist, double* dist, long long* index, void* stream) {
  if (N < 0 || Q < 0 || !(max_dist > 0.0) || !isfinite(max_dist)) return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)N >= rg::kMaxItems) return RADEGS_ERR_TOO_LARGE;
  if (Q == 0) return 0;
  if (N == 0 || !rgme::grid_args_ok(N, origin3, cell) || !grid_workspace || !queries || !dist || !index) return RADEGS_ERR_INVALID_ARG;
  const double shells = ceil(max_dist / cell) + 1.0;
  if (!(shells <= 512.0)) return RADEGS_ERR_INVALID_ARG;   // half the shortest key period: a larger shell would visit a cell twice
  const rgme::GridView w = rgme::grid_carve(N, const_cast<void*>(grid_workspace));
  const rgme::Grid g{origin3[0], origin3[1], origin3[2], cell};
  hipLaunchKernelGGL(rgme::nearest_kernel, dim3(rg::blocks_of((size_t)Q)), dim3(256), 0, static_cast<hipStream_t>(stream), (uint32_t)N, w.keys, w.perm,
                     w.pts, g, Q, queries, max_dist, (int)shells, dist, index);
  return rg::launch_status();
}

size_t radegs_mesheval_sum_bytes(void) { return rg::align256(2 * rg::kSumBlocks * sizeof(double)); }

int radegs_mesheval_sum_below(long long Q, const double* dist, double max_dist, void* workspace, size_t workspace_bytes, double* out2, void* stream_v) {
  if (Q < 0 || !out2) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (Q == 0) return hipMemsetAsync(out2, 0, 2 * sizeof(double), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if (!dist || !workspace || workspace_bytes < radegs_mesheval_sum_bytes() || (reinterpret_cast<uintptr_t>(workspace) & 7)) return RADEGS_ERR_INVALID_ARG;
  const int nb = rg::sum_blocks(Q);
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(rgme::below_partial_kernel, dim3(nb), dim3(256), 0, s, Q, dist, max_dist, partial);
  hipLaunchKernelGGL(rgme::below_final_kernel, dim3(1), dim3(256), 0, s, nb, partial, out2);
  return rg::launch_status();
}

int radegs_mesheval_obs_mask(long long N, const double* points, const double* box10, const int* dims3, const unsigned char* volume,
                             unsigned char* inbound, unsigned char* grid_inbound, unsigned char* in_obs, void* stream) {
  if (N < 0 || !box10 || !dims3) return RADEGS_ERR_INVALID_ARG;
  if (dims3[0] < 1 || dims3[1] < 1 || dims3[2] < 1 || !(box10[9] > 0.0) || !isfinite(box10[9])) return RADEGS_ERR_INVALID_ARG;
  if (N == 0) return 0;
  if (!points || !volume || !inbound || !grid_inbound || !in_obs) return RADEGS_ERR_INVALID_ARG;
  rgme::ObsBox b;
  for (int k = 0; k < 3; k++) {
    b.lo[k] = box10[k];
    b.hi[k] = box10[3 + k];
    b.bb0[k] = box10[6 + k];
    b.dim[k] = dims3[k];
  }
  b.res = box10[9];
  hipLaunchKernelGGL(rgme::obs_mask_kernel, dim3(rg::blocks_of((size_t)N)), dim3(256), 0, static_cast<hipStream_t>(stream), N, points, b, volume, inbound,
                     grid_inbound, in_obs);
  return rg::launch_status();
}

int radegs_mesheval_above_plane(long long N, const double* points, const double* plane4, unsigned char* above, void* stream) {
  if (N < 0 || !plane4) return RADEGS_ERR_INVALID_ARG;
  if (N == 0) return 0;
  if (!points || !above) return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgme::plane_side_kernel, dim3(rg::blocks_of((size_t)N)), dim3(256), 0, static_cast<hipStream_t>(stream), N, points, plane4[0],
                     plane4[1], plane4[2], plane4[3], above);
  return rg::launch_status();
}

int radegs_mesheval_dilate(int W, int H, const unsigned char* mask, int radius, unsigned char* out, void* stream) {
  if (W < 1 || H < 1 || radius < 0 || radius > 64 || !mask || !out) return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgme::dilate_kernel, dim3(rg::blocks_of((size_t)W * H)), dim3(256), 0, static_cast<hipStream_t>(stream), W, H, mask, radius, out);
  return rg::launch_status();
}

int radegs_mesheval_cull_vertices(long long NV, const float* vertices, int ncam, const RadegsCullCamera* cameras, const unsigned char* masks,
                                  unsigned* flags, void* stream) {
  if (NV < 0 || ncam < 0) return RADEGS_ERR_INVALID_ARG;
  if (NV == 0) return 0;
  if (!vertices || !flags || (ncam && (!cameras || !masks)) || (reinterpret_cast<uintptr_t>(cameras) & 7)) return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgme::cull_vertices_kernel, dim3(rg::blocks_of((size_t)NV)), dim3(256), 0, static_cast<hipStream_t>(stream), NV, vertices, ncam,
                     cameras, masks, flags);
  return rg::launch_status();
}

}  // extern "C"
