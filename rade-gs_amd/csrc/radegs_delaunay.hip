// radegs_delaunay.hip -- Delaunay tetrahedralisation of N points: the `cpp.triangulate(points)` of
// mesh_extract_tetrahedra.py:63, which upstream hands to tetranerf's CGAL Delaunay_triangulation_3.  The specification is
// include/radegs.h, "Delaunay", and DESIGN.md 11 N13; tests/delaunay_restatement.py restates it in NumPy.
//
// "Meshless Voronoi" (Ray, Sokolov, Lefebvre, Levy 2018): every point computes its own Voronoi cell by clipping against its neighbours, and
// the cell's vertices are the tetrahedra incident to the point.  rg_delaunay_cell.h holds the cell, the clip and the predicates.  There is
// no concurrent data structure, no lock, no spin-wait and no dependency between workgroups; every loop has a bound known at launch
// (shells <= kShellMax, candidates <= N, triangles and faces <= the cell's capacity), so a mistake gives a wrong answer, never a hang.
//
//   plan   perturb_kernel        x + scale (u - 0.5), u from the counter hash of (seed, 3 i + axis)
//          cell_key_kernel       uniform grid of about two points per cell over the caller's bounds; rg::radix_sort_pairs_u32 puts the
//          gather / cell_start   points in cell order, cell c's points are positions [start[c], start[c + 1])
//          fast_kernel           one LANE per point, its cell in LDS; Chebyshev shells of grid cells until the cell is bounded and twice its
//                                largest circumradius is within what every unvisited point must exceed.  Out of shells or of room: deferred.
//          slow_kernel           one WAVE per deferred point (every hull point is one: its cell keeps ghost triangles and must see all N);
//                                64 candidates at a time against the triangles, a ballot picks those that cut, lane 0 applies them in turn.
//                                A block of 64 whose bounding box lies outside every triangle's sphere or half-space is skipped whole.
//          Both kernels answer the cell's second_look: an in-sphere value within its error bound is evaluated once more about the sphere
//          point nearest the candidate, from the absolute coordinates (rg_delaunay_cell.h, in_sphere_recentred), before it counts.
//          A finished cell appends its all-real triangles as ascending quadruples (i, a, b, c) to the record arrays at an atomic cursor: the
//          order of the records is arbitrary, what the sort makes of them is not.
//   emit   two rg::radix_sort_order_2xu32 (LSD over the four words), heads of runs, rg::inclusive_scan_gather_u32, one oriented row per run.
//          A tetrahedron found by all four of its corners is a run of four; any other length counts as inconsistent.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_delaunay_cell.h"
#include "rg_prims.h"
#include "rg_workspace.h"

namespace rgdl {

using rg::blocks_of;
typedef unsigned long long u64;

constexpr long long kMaxPoints = (1ll << 31) - 8;   // ids and the four ghosts past them stay below 2^31: int32 rows, u32 sort words
constexpr int kGridMax = 512;                       // cells per axis
// Fast cell: 48 faces x 4 B + 92 triangles x 3 B = 468 B a lane, 29 952 B a 64-lane workgroup: five workgroups share a CU's 160 KB.
constexpr int kFastFaces = 48, kFastTris = 92;
constexpr int kShellMax = 6;      // shells 0 .. 6: at most 13^3 cells
constexpr int kGhostShells = 3;   // a cell that still holds a ghost after this shell is taken for a hull point's
// Slow cell: the byte face numbers' limit, 256 faces and 2 x 256 - 4 triangles; with the cached coordinates and spheres 24 968 B a wave.
constexpr int kSlowFaces = 256, kSlowTris = 508;
// The slow kernel's sphere test inflates the squared radius by 2^-10.  circumsphere() answers only where det[a,b,c] has twenty good bits;
// the numerator's error relative to its own length is of the same order (its permanent over its length is at most the inverse normalised
// volume, which that condition bounds), so centre and radius are good to about 2^-19 and |q - c|^2 - r^2 to 2^-18 r^2 near the sphere.
constexpr double kFilterInflate = 1.0 + 1.0 / 1024.0;
constexpr double kHalfSpace = -1.0, kMargin = 1e-12;
enum { kRecords = 0, kDeferred = 1, kUncertain = 2, kOverflow = 3, kUnique = 4, kInconsistent = 5, kCounters = 8 };

inline int bits_for(u64 max_value) {
  int b = 1;
  while (b < 32 && (max_value >> b)) b++;
  return b;
}

struct Grid {
  double lo[3], h;
  int dim[3];
};
inline int grid_side(long long N) {
  int g = (int)ceil(cbrt((double)N / 2.0));
  return g < 1 ? 1 : (g > kGridMax ? kGridMax : g);
}
inline Grid make_grid(long long N, const double* bounds) {
  Grid g;
  const int side = grid_side(N);
  double ext[3], m = 0.0;
  for (int k = 0; k < 3; k++) g.lo[k] = bounds[k], ext[k] = bounds[3 + k] - bounds[k], m = ext[k] > m ? ext[k] : m;
  g.h = m > 0.0 ? m / side : 0.0;      // a box of no extent is one cell of no size: it says nothing about distances, so the fast kernel's
  for (int k = 0; k < 3; k++) {        // stop test (reach = r h = 0) never holds and every point is the slow kernel's, whatever the units
    const double c = g.h > 0.0 ? floor(ext[k] / g.h) + 1.0 : 1.0;
    g.dim[k] = c >= (double)side ? side : (c >= 1.0 ? (int)c : 1);
  }
  return g;
}

struct View {
  double *P, *Ps, *blockbox;
  uint32_t *key, *key_sorted, *perm, *cell_start, *deferred;
  u64* counters;
  uint32_t* k[4];
  uint32_t *g0, *g1, *major_sorted, *perm1, *perm2, *s0, *s1, *s2;
  u64 *joined1, *joined2;
  void* temp;
  size_t temp_bytes, bytes;
};
inline View carve(long long N, long long R, void* base) {
  rg::Carver c(base);
  View v;
  const size_t n = (size_t)N, r = (size_t)R, side = (size_t)grid_side(N);
  const size_t a = rg::sort_temp_bytes(n > r ? n : r), b = rg::scan_temp_bytes(r);
  v.temp_bytes = a > b ? a : b;
  v.P = c.take<double>(3 * n), v.Ps = c.take<double>(3 * n), v.blockbox = c.take<double>(6 * ((n + 63) / 64));
  v.key = c.take<uint32_t>(n), v.key_sorted = c.take<uint32_t>(n), v.perm = c.take<uint32_t>(n);
  v.cell_start = c.take<uint32_t>(side * side * side + 1), v.deferred = c.take<uint32_t>(n);
  v.counters = c.take<u64>(kCounters);
  for (int k = 0; k < 4; k++) v.k[k] = c.take<uint32_t>(r);
  v.g0 = c.take<uint32_t>(r), v.g1 = c.take<uint32_t>(r), v.major_sorted = c.take<uint32_t>(r), v.perm1 = c.take<uint32_t>(r), v.perm2 = c.take<uint32_t>(r);
  v.s0 = c.take<uint32_t>(r), v.s1 = c.take<uint32_t>(r), v.s2 = c.take<uint32_t>(r);
  v.joined1 = c.take<u64>(r), v.joined2 = c.take<u64>(r);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

// ------------------------------------------------------------------------- perturb and grid -------------------------------------------------------------------------
__global__ void __launch_bounds__(256) perturb_kernel(uint32_t N, const double* __restrict__ in, double scale, u64 seed, double* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    const double x = in[3 * (size_t)i + k];
    out[3 * (size_t)i + k] = scale == 0.0 ? x : x + scale * (hash_unit(seed, 3ull * i + k) - 0.5);
  }
}

__device__ __forceinline__ int cell_coord(double x, double lo, double h, int dim) {
  const double t = h > 0.0 ? floor((x - lo) / h) : 0.0;
  return t >= (double)(dim - 1) ? dim - 1 : (t >= 1.0 ? (int)t : 0);     // a point outside the bounds lands in the border cell
}

__global__ void __launch_bounds__(256) cell_key_kernel(uint32_t N, Grid g, const double* __restrict__ P, uint32_t* __restrict__ key) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= N) return;
  const int cx = cell_coord(P[3 * (size_t)i], g.lo[0], g.h, g.dim[0]), cy = cell_coord(P[3 * (size_t)i + 1], g.lo[1], g.h, g.dim[1]),
            cz = cell_coord(P[3 * (size_t)i + 2], g.lo[2], g.h, g.dim[2]);
  key[i] = (uint32_t)((cz * g.dim[1] + cy) * g.dim[0] + cx);
}

__global__ void __launch_bounds__(256) gather_points_kernel(uint32_t N, const double* __restrict__ P, const uint32_t* __restrict__ perm, double* __restrict__ Ps) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= N) return;
  const size_t i = perm[j];
  Ps[3 * (size_t)j] = P[3 * i], Ps[3 * (size_t)j + 1] = P[3 * i + 1], Ps[3 * (size_t)j + 2] = P[3 * i + 2];
}

// start[c], c in [0, ncells]: the first sorted position whose cell is not below c (N past the last); one binary search a cell
__global__ void __launch_bounds__(256) cell_start_kernel(uint32_t N, uint32_t ncells, const uint32_t* __restrict__ key_sorted, uint32_t* __restrict__ start) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c > ncells) return;
  start[c] = c == ncells ? N : rg::lower_bound(key_sorted, N, c);
}

// the bounding box {min x, y, z, max x, y, z} of every 64 consecutive points of the sorted order: what the slow kernel culls by
__global__ void __launch_bounds__(256) block_box_kernel(uint32_t N, const double* __restrict__ Ps, double* __restrict__ box) {
  const uint32_t b = blockIdx.x * 256u + threadIdx.x;
  if (b >= (N + 63u) / 64u) return;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t k = b * 64u; k < min(b * 64u + 64u, N); k++)
#pragma unroll
    for (int a = 0; a < 3; a++) lo[a] = fmin(lo[a], Ps[3 * (size_t)k + a]), hi[a] = fmax(hi[a], Ps[3 * (size_t)k + a]);
#pragma unroll
  for (int a = 0; a < 3; a++) box[6 * (size_t)b + a] = lo[a], box[6 * (size_t)b + 3 + a] = hi[a];
}

// ---------------------------------------------------------------------------- records ----------------------------------------------------------------------------
struct Records {
  uint32_t* k[4];
  u64 capacity;
};

__device__ __forceinline__ void order2(uint32_t& a, uint32_t& b) {
  const uint32_t lo = min(a, b), hi = max(a, b);
  a = lo, b = hi;
}

// the all-real triangles of a finished cell of sorted position j, as ascending quadruples of ORIGINAL ids; one atomic reserves the room
template <class C>
__device__ __forceinline__ void write_records(const C& cell, uint32_t j, uint32_t N, const uint32_t* __restrict__ perm, Records rec, u64* counters) {
  int n = 0;
  for (int t = 0; t < cell.nt; t++) n += (cell.id(cell.corner(t, 0)) < N && cell.id(cell.corner(t, 1)) < N && cell.id(cell.corner(t, 2)) < N) ? 1 : 0;
  if (n == 0) return;
  u64 pos = atomicAdd(counters + kRecords, (u64)n);
  const uint32_t self = perm[j];
  for (int t = 0; t < cell.nt; t++) {
    const uint32_t ia = cell.id(cell.corner(t, 0)), ib = cell.id(cell.corner(t, 1)), ic = cell.id(cell.corner(t, 2));
    if (ia >= N || ib >= N || ic >= N) continue;
    if (pos < rec.capacity) {
      uint32_t a = self, b = perm[ia], c = perm[ib], d = perm[ic];
      order2(a, b), order2(c, d), order2(a, c), order2(b, d), order2(b, c);
      rec.k[0][pos] = a, rec.k[1][pos] = b, rec.k[2][pos] = c, rec.k[3][pos] = d;
    }
    pos++;
  }
}

// ---------------------------------------------------------------------------- fast cells ----------------------------------------------------------------------------
__device__ __forceinline__ V3 point_at(const double* __restrict__ Ps, uint32_t k) { return V3{Ps[3 * (size_t)k], Ps[3 * (size_t)k + 1], Ps[3 * (size_t)k + 2]}; }

struct FastData : NoTriangleData {
  const double* Ps;
  V3 xi;
  __device__ __forceinline__ V3 rel(int, uint32_t g) const { return V3{Ps[3 * (size_t)g] - xi.x, Ps[3 * (size_t)g + 1] - xi.y, Ps[3 * (size_t)g + 2] - xi.z}; }
  // rare, and kept out of line so that the clip's hot loop keeps its registers
  __device__ __noinline__ int second_look(uint32_t ia, uint32_t ib, uint32_t ic, uint32_t iq, V3 a, V3 b, V3 c, V3 q) const {
    return in_sphere_recentred(xi, point_at(Ps, ia), point_at(Ps, ib), point_at(Ps, ic), point_at(Ps, iq), a, b, c, q);
  }
};
typedef Cell<kFastFaces, kFastTris, 64> FastCell;

// candidates [kbeg, kend) of the sorted order against the cell; false on overflow
__device__ __forceinline__ bool visit(FastCell& cell, FastData& data, uint32_t j, uint32_t kbeg, uint32_t kend, double r2lim, unsigned& uncertain) {
  for (uint32_t k = kbeg; k < kend; k++) {
    if (k == j) continue;
    const V3 q = data.rel(0, k);
    if (dot(q, q) > r2lim) continue;       // a bounded cell only shrinks: nothing beyond twice its largest circumradius can cut it
    cell.clip(k, q, data, uncertain);
    if (cell.overflow) return false;
  }
  return true;
}

__global__ void __launch_bounds__(64) fast_kernel(uint32_t N, Grid g, const double* __restrict__ Ps, const uint32_t* __restrict__ key_sorted,
                                                  const uint32_t* __restrict__ start, const uint32_t* __restrict__ perm, Records rec,
                                                  uint32_t* __restrict__ deferred, u64* counters) {
  __shared__ uint32_t s_face[kFastFaces * 64];
  __shared__ uint8_t s_tri[3 * kFastTris * 64];
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= N) return;                      // no barrier below: a lane owns its slice of the two arrays
  FastCell cell;
  cell.init(s_face + threadIdx.x, s_tri + threadIdx.x, N);
  FastData data;
  data.Ps = Ps, data.xi = V3{Ps[3 * (size_t)j], Ps[3 * (size_t)j + 1], Ps[3 * (size_t)j + 2]};
  const int dx = g.dim[0], dy = g.dim[1], dz = g.dim[2];
  const uint32_t key = min(key_sorted[j], (uint32_t)(dx * dy * dz) - 1u);
  const int cx = (int)(key % (uint32_t)dx), cy = (int)((key / (uint32_t)dx) % (uint32_t)dy), cz = (int)(key / (uint32_t)(dx * dy));
  unsigned uncertain = 0;
  double r2lim = INFINITY;
  bool done = false;
  for (int r = 0; r <= kShellMax && !done; r++) {
    bool ok = true;
    for (int z = max(cz - r, 0); z <= min(cz + r, dz - 1) && ok; z++)
      for (int y = max(cy - r, 0); y <= min(cy + r, dy - 1) && ok; y++) {
        const uint32_t row = (uint32_t)((z * dy + y) * dx);
        if (abs(z - cz) == r || abs(y - cy) == r) {          // a whole row of the shell: its cells are consecutive in the sorted order
          ok = visit(cell, data, j, start[row + (uint32_t)max(cx - r, 0)], start[row + (uint32_t)min(cx + r, dx - 1) + 1u], r2lim, uncertain);
        } else {                                             // the two end cells of the row
          if (cx - r >= 0) ok = visit(cell, data, j, start[row + (uint32_t)(cx - r)], start[row + (uint32_t)(cx - r) + 1u], r2lim, uncertain);
          if (ok && r > 0 && cx + r < dx) ok = visit(cell, data, j, start[row + (uint32_t)(cx + r)], start[row + (uint32_t)(cx + r) + 1u], r2lim, uncertain);
        }
      }
    if (!ok) break;
    double r2max;
    if (cell.bounded(data, r2max)) {
      r2lim = 4.0 * r2max * kInflate;
      const double reach = (double)r * g.h * (1.0 - 1.0 / 1048576.0);     // every unvisited point is farther than r cells away, less the rounding of the keys
      done = r2lim <= reach * reach;
    } else if (r >= kGhostShells) {
      break;
    }
    if (r >= dx && r >= dy && r >= dz) break;                // the whole grid has been seen: the rest is the slow kernel's
  }
  if (uncertain) atomicAdd(counters + kUncertain, (u64)uncertain);
  if (done) {
    write_records(cell, j, N, perm, rec, counters);
  } else {
    const u64 d = atomicAdd(counters + kDeferred, 1ull);
    if (d < N) deferred[d] = j;
  }
}

// ---------------------------------------------------------------------------- slow cells ----------------------------------------------------------------------------
struct SlowData {
  V3* relc;        // [kSlowFaces] relative coordinates of the real faces
  // [kSlowTris][4], what a candidate must satisfy to be inside triangle t, in the fourth word:
  //   r2 >= 0     all real: within the sphere (c, r2), the circumsphere with its squared radius inflated by kFilterInflate
  //   kHalfSpace  a ghost: m.q > 0 for the inward normal m in the first three words
  //   INFINITY    nothing is known (the determinant behind either is too close to its error bound): every candidate takes the predicate
  double* sph;
  const double* Ps;   // the absolute coordinates, for the second look only
  V3 xi;
  __device__ __forceinline__ V3 rel(int f, uint32_t) const { return relc[f]; }
  __device__ __noinline__ int second_look(uint32_t ia, uint32_t ib, uint32_t ic, uint32_t iq, V3 a, V3 b, V3 c, V3 q) const {
    return in_sphere_recentred(xi, point_at(Ps, ia), point_at(Ps, ib), point_at(Ps, ic), point_at(Ps, iq), a, b, c, q);
  }
  __device__ __forceinline__ void put_face(int f, V3 q) { relc[f] = q; }
  __device__ __forceinline__ void move_tri(int from, int to) {
#pragma unroll
    for (int k = 0; k < 4; k++) sph[4 * to + k] = sph[4 * from + k];
  }
  __device__ __forceinline__ void new_tri(int t, V3 p0, bool g0, V3 p1, bool g1, V3 p2, bool g2) {
    V3 c = V3{0.0, 0.0, 0.0};
    double r2;
    if (g0 || g1 || g2) r2 = halfspace_normal(p0, g0, p1, g1, p2, g2, c) ? kHalfSpace : INFINITY;
    else r2 = circumsphere(p0, p1, p2, c) * kFilterInflate;
    sph[4 * t] = c.x, sph[4 * t + 1] = c.y, sph[4 * t + 2] = c.z, sph[4 * t + 3] = r2;
  }
};
typedef Cell<kSlowFaces, kSlowTris, 1> SlowCell;

// may a candidate at q be inside triangle t?  The half-space margin, 1e-12 of the permanent, is ten thousand times the predicate's own bound.
__device__ __forceinline__ bool may_hold_point(const double* __restrict__ sph, int t, V3 q) {
  const double r2 = sph[4 * t + 3];
  const V3 c = V3{sph[4 * t], sph[4 * t + 1], sph[4 * t + 2]};
  if (r2 == INFINITY) return true;
  if (r2 == kHalfSpace) return dot(c, q) >= -kMargin * dot_abs(c, q);
  const V3 e = q - c;
  return dot(e, e) <= r2;
}
// may any point of the box [lo, hi] (relative coordinates) be inside triangle t?
__device__ __forceinline__ bool may_hold_box(const double* __restrict__ sph, int t, V3 lo, V3 hi) {
  const double r2 = sph[4 * t + 3];
  const V3 c = V3{sph[4 * t], sph[4 * t + 1], sph[4 * t + 2]};
  if (r2 == INFINITY) return true;
  if (r2 == kHalfSpace) {
    const double best = (fmax(c.x * lo.x, c.x * hi.x) + fmax(c.y * lo.y, c.y * hi.y)) + fmax(c.z * lo.z, c.z * hi.z);
    const double size = (fabs(c.x) * fmax(fabs(lo.x), fabs(hi.x)) + fabs(c.y) * fmax(fabs(lo.y), fabs(hi.y))) + fabs(c.z) * fmax(fabs(lo.z), fabs(hi.z));
    return best >= -kMargin * size;
  }
  const V3 e = V3{fmax(fmax(lo.x - c.x, c.x - hi.x), 0.0), fmax(fmax(lo.y - c.y, c.y - hi.y), 0.0), fmax(fmax(lo.z - c.z, c.z - hi.z), 0.0)};
  return dot(e, e) <= r2;
}

// Does the candidate at q cut the cell?  The uncertain values it meets are added to `uncertain` only where the answer is no: a candidate
// that cuts is clipped again by lane 0, which counts them there.
__device__ __forceinline__ bool cuts_any(const SlowCell& cell, const SlowData& data, uint32_t k, V3 q, unsigned& uncertain) {
  unsigned met = 0;
  for (int t = 0; t < cell.nt; t++) {
    if (!may_hold_point(data.sph, t, q)) continue;
    if (cell.tri_inside(t, k, q, data, met)) return true;
  }
  uncertain += met;
  return false;
}

__global__ void __launch_bounds__(64) slow_kernel(uint32_t N, const double* __restrict__ Ps, const uint32_t* __restrict__ perm,
                                                  const double* __restrict__ blockbox, const uint32_t* __restrict__ deferred, Records rec,
                                                  u64* counters) {
  __shared__ uint32_t s_face[kSlowFaces];
  __shared__ uint8_t s_tri[3 * kSlowTris];
  __shared__ V3 s_rel[kSlowFaces];
  __shared__ double s_sph[4 * kSlowTris];
  __shared__ int s_nt, s_overflow;
  __shared__ double s_r2lim;
  const u64 nd64 = counters[kDeferred];
  const uint32_t ndef = nd64 < (u64)N ? (uint32_t)nd64 : N;
  const uint32_t nblk = (N + 63u) / 64u, lane = threadIdx.x;
  for (uint32_t d = blockIdx.x; d < ndef; d += gridDim.x) {          // uniform over the workgroup, which is one wave
    const uint32_t j = min(deferred[d], N - 1u);
    SlowData data;
    const V3 xi = V3{Ps[3 * (size_t)j], Ps[3 * (size_t)j + 1], Ps[3 * (size_t)j + 2]};
    data.relc = s_rel, data.sph = s_sph, data.Ps = Ps, data.xi = xi;
    SlowCell cell;
    __syncthreads();                                                  // the last point's readers are through
    if (lane == 0) {
      cell.init(s_face, s_tri, N);
      for (int t = 0; t < 16; t++) s_sph[t] = (t & 3) == 3 ? INFINITY : 0.0;      // the four all-ghost triangles: nothing known
      s_nt = 4, s_overflow = 0, s_r2lim = INFINITY;
    }
    __syncthreads();
    cell.face = s_face, cell.tri = s_tri, cell.N = N, cell.nt = 4, cell.ne = 0, cell.overflow = false;
    double r2lim = INFINITY;
    unsigned uncertain = 0;
    const uint32_t jb = j / 64u;
    bool overflow = false;
    for (uint32_t it = 0; it < 2u * nblk && !overflow; it++) {        // blocks of 64 candidates outwards from the point's own: jb, jb + 1, jb - 1, ..
      const uint32_t off = (it + 1u) / 2u;
      if ((it & 1u) ? off >= nblk - jb : off > jb) continue;
      const uint32_t blk = (it & 1u) ? jb + off : jb - off;
      // the block's box against the cell: beyond twice the largest circumradius of a bounded cell, or outside every triangle's sphere or
      // half-space, none of its 64 points can cut.  The lanes share out the triangles.
      const double* bb = blockbox + 6 * (size_t)blk;
      const V3 blo = V3{bb[0], bb[1], bb[2]} - xi, bhi = V3{bb[3], bb[4], bb[5]} - xi;
      const V3 near = V3{fmax(fmax(blo.x, -bhi.x), 0.0), fmax(fmax(blo.y, -bhi.y), 0.0), fmax(fmax(blo.z, -bhi.z), 0.0)};
      bool touch = false;
      if (dot(near, near) * (1.0 - 1.0 / 1048576.0) <= r2lim)
        for (int t = (int)lane; t < cell.nt && !touch; t += 64) touch = may_hold_box(s_sph, t, blo, bhi);
      if (__ballot(touch) == 0ull) continue;                          // uniform
      const uint32_t k = blk * 64u + lane;
      bool c = false;
      if (k < N && k != j) {
        const V3 q = V3{Ps[3 * (size_t)k], Ps[3 * (size_t)k + 1], Ps[3 * (size_t)k + 2]} - xi;
        if (dot(q, q) <= r2lim) c = cuts_any(cell, data, k, q, uncertain);
      }
      u64 mask = __ballot(c);
      if (mask == 0ull) continue;                                     // uniform
      if (lane == 0) {
        while (mask != 0ull && !cell.overflow) {
          const uint32_t kk = blk * 64u + (uint32_t)__builtin_ctzll(mask);
          mask &= mask - 1ull;
          const V3 q = V3{Ps[3 * (size_t)kk], Ps[3 * (size_t)kk + 1], Ps[3 * (size_t)kk + 2]} - xi;
          cell.clip(kk, q, data, uncertain);                          // tests again: an earlier candidate of this block may have cut it out
        }
        double r2max;
        if (!cell.overflow && cell.bounded(data, r2max)) s_r2lim = 4.0 * r2max * kInflate;
        s_nt = cell.nt, s_overflow = cell.overflow ? 1 : 0;
      }
      __syncthreads();
      cell.nt = s_nt, r2lim = s_r2lim, overflow = s_overflow != 0;
      __syncthreads();
    }
    if (uncertain) atomicAdd(counters + kUncertain, (u64)uncertain);      // every lane's: its candidates that did not cut, and lane 0's clips
    if (lane == 0) {
      if (overflow) atomicAdd(counters + kOverflow, 1ull);
      else write_records(cell, j, N, perm, rec, counters);
    }
  }
}

__global__ void counts_out_kernel(const u64* __restrict__ counters, long long* __restrict__ out) {
  if (threadIdx.x < 4) out[threadIdx.x] = (long long)counters[threadIdx.x];
}

// ------------------------------------------------------------------------------ emit ------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gather2_kernel(uint32_t R, const uint32_t* __restrict__ perm1, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                      uint32_t* __restrict__ ga, uint32_t* __restrict__ gb) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= R) return;
  const uint32_t p = min(perm1[i], R - 1u);
  ga[i] = a[p], gb[i] = b[p];
}

// position i of the final order: words 0, 1 are joined2[i], words 2, 3 are joined1[perm2[i]]
__global__ void __launch_bounds__(256) heads_kernel(uint32_t R, const u64* __restrict__ joined1, const u64* __restrict__ joined2, const uint32_t* __restrict__ perm2,
                                                    uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= R) return;
  head[i] = (i == 0u || joined2[i] != joined2[i - 1] || joined1[min(perm2[i], R - 1u)] != joined1[min(perm2[i - 1], R - 1u)]) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) rows_kernel(uint32_t N, uint32_t R, const double* __restrict__ P, const u64* __restrict__ joined1,
                                                   const u64* __restrict__ joined2, const uint32_t* __restrict__ perm2, const uint32_t* __restrict__ head,
                                                   const uint32_t* __restrict__ incl, long long out_capacity, int* __restrict__ cells, u64* counters) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= R) return;
  if (i == R - 1u) counters[kUnique] = incl[i];
  if (!head[i]) return;
  uint32_t len = 1;
  while (len < 5u && i + len < R && !head[i + len]) len++;
  const u64 hi = joined2[i], lo = joined1[min(perm2[i], R - 1u)];
  const uint32_t a = (uint32_t)(hi >> 32), b = (uint32_t)hi, c = (uint32_t)(lo >> 32), d = (uint32_t)lo;
  bool good = len == 4u && a < N && b < N && c < N && d < N;
  bool swap = false;
  if (good) {
    const V3 pa = V3{P[3 * (size_t)a], P[3 * (size_t)a + 1], P[3 * (size_t)a + 2]};
    const V3 u = V3{P[3 * (size_t)b], P[3 * (size_t)b + 1], P[3 * (size_t)b + 2]} - pa, v = V3{P[3 * (size_t)c], P[3 * (size_t)c + 1], P[3 * (size_t)c + 2]} - pa,
             w = V3{P[3 * (size_t)d], P[3 * (size_t)d + 1], P[3 * (size_t)d + 2]} - pa;
    const double det = dot(cross(u, v), w);
    swap = det < 0.0;
    good = det != 0.0;                     // a flat tetrahedron has no positive orientation
  }
  if (!good) atomicAdd(counters + kInconsistent, 1ull);
  const long long row = (long long)incl[i] - 1;
  if (row < 0 || row >= out_capacity) return;
  cells[4 * row] = (int)a, cells[4 * row + 1] = (int)b, cells[4 * row + 2] = (int)(swap ? d : c), cells[4 * row + 3] = (int)(swap ? c : d);
}

__global__ void counts2_out_kernel(const u64* __restrict__ counters, long long* __restrict__ out) {
  if (threadIdx.x < 2) out[threadIdx.x] = (long long)counters[kUnique + threadIdx.x];
}

inline bool sizes_ok(long long N, long long R) { return N <= kMaxPoints && R >= 0 && (u64)R <= rg::kMaxItems; }

}  // namespace rgdl

extern "C" {

size_t radegs_delaunay_bytes(long long N, long long record_capacity) {
  if (N < 4 || record_capacity < 1 || !rgdl::sizes_ok(N, record_capacity)) return 0;
  return rgdl::carve(N, record_capacity, nullptr).bytes;
}

int radegs_delaunay_perturb(long long N, const double* points, double scale, unsigned long long seed, double* out, void* stream) {
  if (N < 0 || !(scale >= 0.0) || !isfinite(scale)) return RADEGS_ERR_INVALID_ARG;
  if (N > rgdl::kMaxPoints) return RADEGS_ERR_TOO_LARGE;
  if (N == 0) return 0;
  if (!points || !out) return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgdl::perturb_kernel, dim3(rg::blocks_of((size_t)N)), dim3(256), 0, static_cast<hipStream_t>(stream), (uint32_t)N, points, scale, seed, out);
  return rg::launch_status();
}

int radegs_delaunay_plan(long long N, const double* points, const double* bounds, double scale, unsigned long long seed, long long record_capacity,
                         void* workspace, size_t workspace_bytes, long long* counts4, void* stream_v) {
  if (N < 4 || !points || !bounds || !counts4 || record_capacity < 1 || !(scale >= 0.0) || !isfinite(scale)) return RADEGS_ERR_INVALID_ARG;
  for (int k = 0; k < 6; k++)
    if (!isfinite(bounds[k])) return RADEGS_ERR_INVALID_ARG;
  if (!rgdl::sizes_ok(N, record_capacity)) return RADEGS_ERR_TOO_LARGE;
  if (!workspace || workspace_bytes < radegs_delaunay_bytes(N, record_capacity) || !rg::aligned16(workspace)) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const rgdl::View w = rgdl::carve(N, record_capacity, workspace);
  const rgdl::Grid g = rgdl::make_grid(N, bounds);
  const uint32_t n = (uint32_t)N, ncells = (uint32_t)(g.dim[0] * g.dim[1] * g.dim[2]);
  if (hipMemsetAsync(w.counters, 0, rgdl::kCounters * sizeof(rgdl::u64), s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgdl::perturb_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, n, points, scale, seed, w.P);
  hipLaunchKernelGGL(rgdl::cell_key_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, n, g, w.P, w.key);
  if (rg::radix_sort_pairs_u32(w.temp, w.temp_bytes, w.key, w.key_sorted, nullptr, w.perm, n, rgdl::bits_for(ncells - 1u), s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgdl::gather_points_kernel, dim3(rg::blocks_of(n)), dim3(256), 0, s, n, w.P, w.perm, w.Ps);
  hipLaunchKernelGGL(rgdl::cell_start_kernel, dim3(rg::blocks_of((size_t)ncells + 1)), dim3(256), 0, s, n, ncells, w.key_sorted, w.cell_start);
  rgdl::Records rec;
  for (int k = 0; k < 4; k++) rec.k[k] = w.k[k];
  rec.capacity = (rgdl::u64)record_capacity;
  hipLaunchKernelGGL(rgdl::fast_kernel, dim3((n + 63u) / 64u), dim3(64), 0, s, n, g, w.Ps, w.key_sorted, w.cell_start, w.perm, rec, w.deferred, w.counters);
  const uint32_t waves = n < 8192u ? n : 8192u;      // the deferred points are shared out over at most this many waves
  hipLaunchKernelGGL(rgdl::block_box_kernel, dim3(rg::blocks_of((n + 63u) / 64u)), dim3(256), 0, s, n, w.Ps, w.blockbox);
  hipLaunchKernelGGL(rgdl::slow_kernel, dim3(waves), dim3(64), 0, s, n, w.Ps, w.perm, w.blockbox, w.deferred, rec, w.counters);
  hipLaunchKernelGGL(rgdl::counts_out_kernel, dim3(1), dim3(64), 0, s, w.counters, counts4);
  return rg::launch_status();
}

int radegs_delaunay_emit(long long N, long long records, long long record_capacity, void* workspace, size_t workspace_bytes, long long out_capacity,
                         int* cells, long long* counts2, void* stream_v) {
  if (N < 4 || records < 1 || records > record_capacity || out_capacity < 0 || !counts2 || (out_capacity && !cells)) return RADEGS_ERR_INVALID_ARG;
  if (!rgdl::sizes_ok(N, record_capacity)) return RADEGS_ERR_TOO_LARGE;
  if (!workspace || workspace_bytes < radegs_delaunay_bytes(N, record_capacity) || !rg::aligned16(workspace)) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const rgdl::View w = rgdl::carve(N, record_capacity, workspace);
  const uint32_t R = (uint32_t)records;
  const int bits = rgdl::bits_for((rgdl::u64)(N - 1));
  if (hipMemsetAsync(w.counters + rgdl::kUnique, 0, 2 * sizeof(rgdl::u64), s) != hipSuccess) return RADEGS_ERR_HIP;
  // LSD over the four words: (k2, k3) first, then, stable, (k0, k1) of the records in that order
  if (rg::radix_sort_order_2xu32(w.temp, w.temp_bytes, w.k[3], w.k[2], w.major_sorted, w.perm1, w.s0, w.s1, w.s2, R, bits, bits, s, nullptr, w.joined1) != hipSuccess)
    return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgdl::gather2_kernel, dim3(rg::blocks_of(R)), dim3(256), 0, s, R, w.perm1, w.k[0], w.k[1], w.g0, w.g1);
  if (rg::radix_sort_order_2xu32(w.temp, w.temp_bytes, w.g1, w.g0, w.major_sorted, w.perm2, w.s0, w.s1, w.s2, R, bits, bits, s, nullptr, w.joined2) != hipSuccess)
    return RADEGS_ERR_HIP;
  uint32_t *head = w.s0, *incl = w.s1;               // the sort's scratch is free again
  hipLaunchKernelGGL(rgdl::heads_kernel, dim3(rg::blocks_of(R)), dim3(256), 0, s, R, w.joined1, w.joined2, w.perm2, head);
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, head, nullptr, incl, R, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgdl::rows_kernel, dim3(rg::blocks_of(R)), dim3(256), 0, s, (uint32_t)N, R, w.P, w.joined1, w.joined2, w.perm2, head, incl, out_capacity, cells,
                     w.counters);
  hipLaunchKernelGGL(rgdl::counts2_out_kernel, dim3(1), dim3(64), 0, s, w.counters, counts2);
  return rg::launch_status();
}

}  // extern "C"
