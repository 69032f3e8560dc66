// rg_delaunay_cell.h -- the arithmetic of radegs_delaunay.hip that does not care where it runs: the jitter hash, the four
// ghost directions, the fp64 predicates with their static filters, and one point's Voronoi cell in dual form with the clip that cuts it by
// one more point.  Plain C++ behind RG_HD, so the same text compiles for the host; nothing here touches the GPU.
//
// The cell of point i is a closed triangulated surface: a list of triangles, each an unordered triple of generator ids other than i.  A
// triangle {a, b, c} is the Voronoi vertex where the cells of i, a, b, c meet, that is the tetrahedron (i, a, b, c).  Ids N .. N + 3 are four
// ghost generators at infinity in the directions ghost_dir(k): with them the unbounded cell of a hull point is closed too, and a tetrahedron
// holding a ghost stands for a hull facet, edge or vertex and is not written out.  A triangle is three BYTES: local face numbers into a small
// table face[] of generator ids.
//
// Predicates (DESIGN 11 N13 derives the ghost rules).  All coordinates are relative to x_i: q = p - x_i is the candidate, a, b, c the real
// members, d1 .. d3 the ghost members' directions, in the order the triangle holds them.
//     no ghost     o = det[a,b,c],  s = -|a|^2 det[b,c,q] + |b|^2 det[a,c,q] - |c|^2 det[a,b,q] + |q|^2 det[a,b,c];    inside iff s o < 0
//     one ghost    n = a x b                                                                             inside iff (n.q)(n.d1) > 0
//     two ghosts   n = a x (d1 - d2)                                                                     inside iff (n.q)(n.d1) > 0
//     three        n = (d1 - d2) x (d1 - d3)                                                             inside iff (n.q)(n.d1) > 0
//
// Static filter.  e = 2^-53.  Every predicate is a sum of monomials in coordinate DIFFERENCES, and the bound on its forward error is a
// multiple of e times its permanent, the same expression with every term replaced by its magnitude (Shewchuk 1997, section 4):
//   det[u,v,w] is evaluated as (u x v).w.  A monomial u_y v_z w_x passes 3 roundings in the differences (x_k - x_i is rounded once), one in
//   u_y v_z, one in the subtraction that forms (u x v)_x, one in the product with w_x and two in the two additions of the dot product: 8
//   factors (1 + d), |d| <= e, so its relative error is below (1 + e)^8 - 1 < 8.01 e.  The permanent is itself computed in floating point
//   from the same rounded differences and may come out low by its own (1 + e)^8: kDet3 = 10 e covers both with room for the e^2 terms.
//   s: |a|^2 = a_x a_x + .. is 2 differences, a product and two additions, 5 roundings; times an 8-rounding determinant, 1 more; the sum of
//   the four terms, 3 more: 17 in all, and as many again at second order for the permanent: kSphere = 20 e.
// A value whose magnitude is within its bound is UNCERTAIN: it is counted, and the decision taken is "not inside".  On an input with no
// uncertain value every decision is the exact one, whatever the order of clipping.  An in-sphere value gets a second look about the
// nearest origin first (in_sphere_recentred), where the kernel can supply absolute coordinates: a decision taken there is exact as well.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RG_HD __host__ __device__ __forceinline__
#else
#define RG_HD inline
#endif

namespace rgdl {

constexpr double kEps = 1.1102230246251565e-16;   // 2^-53
constexpr double kDet3 = 10.0 * kEps;
constexpr double kSphere = 20.0 * kEps;
constexpr double kInflate = 1.0 + 1.0 / 524288.0;   // a radius one part in 2^20 larger: its square 2^-19

struct V3 {
  double x, y, z;
};
RG_HD V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RG_HD double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RG_HD double dot_abs(V3 a, V3 b) { return (fabs(a.x * b.x) + fabs(a.y * b.y)) + fabs(a.z * b.z); }
RG_HD V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
RG_HD V3 cross_abs(V3 a, V3 b) {   // the permanent of the cross product, component by component
  return V3{fabs(a.y * b.z) + fabs(a.z * b.y), fabs(a.z * b.x) + fabs(a.x * b.z), fabs(a.x * b.y) + fabs(a.y * b.x)};
}
RG_HD double det3(V3 u, V3 v, V3 w, double& perm) {
  perm = dot_abs(cross_abs(u, v), w);
  return dot(cross(u, v), w);
}

// The four unit vertex directions of a regular tetrahedron, (+-1, +-1, +-1) / sqrt(3) under Rz(0.37) Rx(0.53): none is parallel to a
// coordinate plane, so an axis-aligned input does not sit on a ghost half-space.  tests/delaunay_restatement.py carries the same literals.
RG_HD V3 ghost_dir(uint32_t k) {
  switch (k) {
    case 0: return V3{0.4636882752759316, 0.40109187134201146, 0.7900117050493591};
    case 1: return V3{0.6128706126410551, 0.01646566263417587, -0.7900117050493591};
    case 2: return V3{-0.8239598679372936, 0.5277707489782728, -0.20627208379146042};
    default: return V3{-0.25259901997969325, -0.9453282829544601, 0.20627208379146042};
  }
}

// u in [0, 1) of (seed, counter): a splitmix64 finaliser over the counter and the seed spread by two odd constants; the top 53 bits
RG_HD double hash_unit(uint64_t seed, uint64_t counter) {
  uint64_t z = (counter + 1ull) * 0x9E3779B97F4A7C15ull + seed * 0xD1B54A32D192ED03ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * 1.1102230246251565e-16;
}

RG_HD bool opposite_signs(double s, double o) { return (s < 0.0 && o > 0.0) || (s > 0.0 && o < 0.0); }
RG_HD bool same_signs(double s, double o) { return (s < 0.0 && o < 0.0) || (s > 0.0 && o > 0.0); }

// no ghost: 1 inside, 0 not inside, -1 where s or o is within its bound
RG_HD int in_sphere_sign(V3 a, V3 b, V3 c, V3 q) {
  double pbcq, pacq, pabq, pabc;
  const double dbcq = det3(b, c, q, pbcq), dacq = det3(a, c, q, pacq), dabq = det3(a, b, q, pabq), o = det3(a, b, c, pabc);
  const double la = dot(a, a), lb = dot(b, b), lc = dot(c, c), lq = dot(q, q);
  const double s = ((lb * dacq - la * dbcq) - lc * dabq) + lq * o;
  const double ps = ((lb * pacq + la * pbcq) + lc * pabq) + lq * pabc;
  if (fabs(s) <= kSphere * ps || fabs(o) <= kDet3 * pabc) return -1;
  return opposite_signs(s, o) ? 1 : 0;
}
RG_HD bool in_sphere(V3 a, V3 b, V3 c, V3 q, unsigned& uncertain) {
  const int r = in_sphere_sign(a, b, c, q);
  if (r < 0) uncertain++;
  return r > 0;
}

// The second look at an uncertain in-sphere value: the same predicate about another origin.  "q inside the sphere through four points" does
// not care which of the four the coordinates are relative to (exchanging two of them changes the sign of s and of o), but the bound does:
// every monomial of s holds one coordinate of q - origin, so with the origin at the sphere point NEAREST q the permanent, and the bound
// with it, shrinks by |q - nearest| / |q - x_i|.  That is the case of a candidate next to a member of the triangle -- a point listed twice
// and parted only by the jitter, two corners of neighbouring boxes a hair apart: q is then nearly ON the sphere, s is of the order of
// o |q - c| R, and about x_i it drowns in 20 e times a permanent of order |q|^2 |a| |b| |c|.  The differences must be taken from the
// ABSOLUTE coordinates, one rounding each as the bound assumes: a - c formed from the relative a and c would carry x_i's roundings, which
// are of the size of the value sought.  xi, xa, xb, xc, xq absolute; a, b, c, q relative to xi (only to find the nearest).  -1: the origin
// was the nearest already, or the value is within its bound there too.
RG_HD int in_sphere_recentred(V3 xi, V3 xa, V3 xb, V3 xc, V3 xq, V3 a, V3 b, V3 c, V3 q) {
  const V3 qa = q - a, qb = q - b, qc = q - c;
  const double d0 = dot(q, q), da = dot(qa, qa), db = dot(qb, qb), dc = dot(qc, qc);
  if (d0 <= da && d0 <= db && d0 <= dc) return -1;
  if (da <= db && da <= dc) return in_sphere_sign(xi - xa, xb - xa, xc - xa, xq - xa);
  if (db <= dc) return in_sphere_sign(xa - xb, xi - xb, xc - xb, xq - xb);
  return in_sphere_sign(xa - xc, xb - xc, xi - xc, xq - xc);
}

// one to three ghosts: the half-space through x_i with normal n = u x v on the side of d
RG_HD bool in_halfspace(V3 u, V3 v, V3 d, V3 q, unsigned& uncertain) {
  const V3 n = cross(u, v), pn = cross_abs(u, v);
  const double nq = dot(n, q), nd = dot(n, d);
  if (fabs(nq) <= kDet3 * dot_abs(pn, q) || fabs(nd) <= kDet3 * dot_abs(pn, d)) {
    uncertain++;
    return false;
  }
  return same_signs(nq, nd);
}

// The members p0, p1, p2 of a triangle with ng >= 1 ghosts (relative coordinates, or directions where ghost) as the half-space's (u, v, d):
// the real members first, each kind in the order the triangle holds it (three compare-exchanges), then the rule of that ghost count.
RG_HD void halfspace_of(V3 p0, bool g0, V3 p1, bool g1, V3 p2, bool g2, V3& u, V3& v, V3& d) {
  const int ng = (int)g0 + (int)g1 + (int)g2;
  V3 t;
  bool tb;
  if (g0 && !g1) { t = p0, p0 = p1, p1 = t, tb = g0, g0 = g1, g1 = tb; }
  if (g1 && !g2) { t = p1, p1 = p2, p2 = t, tb = g1, g1 = g2, g2 = tb; }
  if (g0 && !g1) { t = p0, p0 = p1, p1 = t, tb = g0, g0 = g1, g1 = tb; }
  if (ng == 1) { u = p0, v = p1, d = p2; }
  else if (ng == 2) { u = p0, v = p1 - p2, d = p1; }
  else { u = p0 - p1, v = p0 - p2, d = p0; }
}

// the members of one triangle against q
RG_HD bool inside(V3 p0, bool g0, V3 p1, bool g1, V3 p2, bool g2, V3 q, unsigned& uncertain) {
  if (!(g0 || g1 || g2)) return in_sphere(p0, p1, p2, q, uncertain);
  V3 u, v, d;
  halfspace_of(p0, g0, p1, g1, p2, g2, u, v, d);
  return in_halfspace(u, v, d, q, uncertain);
}

// The inward normal m of a ghost triangle's half-space, "inside only if m.q > 0": n or -n by the sign of n.d.  False where n.d is within
// its error bound (in_halfspace then calls nothing inside, and nothing may be concluded from m).
RG_HD bool halfspace_normal(V3 p0, bool g0, V3 p1, bool g1, V3 p2, bool g2, V3& m) {
  V3 u, v, d;
  halfspace_of(p0, g0, p1, g1, p2, g2, u, v, d);
  const V3 n = cross(u, v);
  const double nd = dot(n, d);
  m = nd > 0.0 ? n : V3{-n.x, -n.y, -n.z};
  return fabs(nd) > kDet3 * dot_abs(cross_abs(u, v), d);
}

// The circumsphere of (x_i, a, b, c) relative to x_i: centre (|a|^2 b x c + |b|^2 c x a + |c|^2 a x b) / (2 det[a,b,c]) and squared radius,
// which is the centre's own squared length.  INFINITY where the determinant is within 2^20 of its error bound: the quotient then has no
// twenty good bits, and a radius inflated by one part in 2^20 (kInflate on its square) would not cover the error.
RG_HD double circumsphere(V3 a, V3 b, V3 c, V3& centre) {
  double perm;
  const double o = det3(a, b, c, perm);
  centre = V3{0.0, 0.0, 0.0};
  if (!(fabs(o) > 1048576.0 * kDet3 * perm)) return INFINITY;
  const double la = dot(a, a), lb = dot(b, b), lc = dot(c, c), h = 0.5 / o;
  const V3 bc = cross(b, c), ca = cross(c, a), ab = cross(a, b);
  centre = V3{((la * bc.x + lb * ca.x) + lc * ab.x) * h, ((la * bc.y + lb * ca.y) + lc * ab.y) * h, ((la * bc.z + lb * ca.z) + lc * ab.z) * h};
  return dot(centre, centre);
}

// What a kernel adds to the cell: where a face's relative coordinates come from, and what it keeps per triangle.
//   V3   rel(int f, uint32_t id)                      relative coordinates of real face f (generator id)
//   void put_face(int f, V3 q)                        face f was taken by the candidate at q
//   void move_tri(int from, int to), void new_tri(int t, ..)   per-triangle data follows the triangle list
//   int  second_look(ia, ib, ic, iq, a, b, c, q)      an uncertain in-sphere value of generators ia, ib, ic against iq once more, from
//                                                     absolute coordinates (in_sphere_recentred); -1 where the kernel has none
struct NoTriangleData {
  RG_HD int second_look(uint32_t, uint32_t, uint32_t, uint32_t, V3, V3, V3, V3) const { return -1; }
  RG_HD void put_face(int, V3) {}
  RG_HD void move_tri(int, int) {}
  RG_HD void new_tri(int, V3, bool, V3, bool, V3, bool) {}
};

// FCAP <= 256 faces, TCAP triangles; element k of an array sits at [k * STRIDE], so 64 lanes' cells interleave with STRIDE 64.  While a
// clip runs the boundary edges of the hole live in the unused top of the triangle array, two bytes each, downwards from slot TCAP - 1:
// triangles [0, nt) and edges (TCAP - 1 - ne, TCAP - 1] never meet because a push is refused (overflow) unless nt + ne < TCAP.
template <int FCAP, int TCAP, int STRIDE>
struct Cell {
  static_assert(FCAP <= 256 && FCAP >= 4 && TCAP >= 4, "face numbers are bytes");
  static constexpr int kWords = (FCAP + 63) / 64;
  uint32_t* face;
  uint8_t* tri;
  uint32_t N;      // ids >= N are ghosts
  int nt, ne;
  bool overflow;

  RG_HD uint32_t id(int f) const { return face[f * STRIDE]; }
  RG_HD int corner(int t, int k) const { return tri[(3 * t + k) * STRIDE]; }
  RG_HD void set_tri(int t, int a, int b, int c) {
    tri[(3 * t) * STRIDE] = (uint8_t)a, tri[(3 * t + 1) * STRIDE] = (uint8_t)b, tri[(3 * t + 2) * STRIDE] = (uint8_t)c;
  }

  // the four triangles over the four ghosts
  RG_HD void init(uint32_t* face_, uint8_t* tri_, uint32_t n) {
    face = face_, tri = tri_, N = n, nt = 4, ne = 0, overflow = false;
    for (int k = 0; k < 4; k++) face[k * STRIDE] = n + (uint32_t)k;
    set_tri(0, 0, 1, 2), set_tri(1, 0, 1, 3), set_tri(2, 0, 2, 3), set_tri(3, 1, 2, 3);
  }

  template <class Data>
  RG_HD V3 member(int f, const Data& data, bool& ghost) const {
    const uint32_t g = id(f);
    ghost = g >= N;
    return ghost ? ghost_dir(g - N) : data.rel(f, g);
  }

  // is the candidate `pid` at q inside triangle t?  An in-sphere value within its bound gets the kernel's second look before it counts.
  template <class Data>
  RG_HD bool tri_inside(int t, uint32_t pid, V3 q, const Data& data, unsigned& uncertain) const {
    bool g0, g1, g2;
    const V3 p0 = member(corner(t, 0), data, g0), p1 = member(corner(t, 1), data, g1), p2 = member(corner(t, 2), data, g2);
    if (g0 || g1 || g2) return inside(p0, g0, p1, g1, p2, g2, q, uncertain);
    int r = in_sphere_sign(p0, p1, p2, q);
    if (r < 0) r = data.second_look(id(corner(t, 0)), id(corner(t, 1)), id(corner(t, 2)), pid, p0, p1, p2, q);
    if (r < 0) uncertain++;
    return r > 0;
  }

  // an edge met twice is interior to the hole: the two meetings cancel
  RG_HD void push_edge(int u, int v) {
    for (int e = 0; e < ne; e++) {
      const int a = tri[(3 * (TCAP - 1 - e)) * STRIDE], b = tri[(3 * (TCAP - 1 - e) + 1) * STRIDE];
      if ((a == u && b == v) || (a == v && b == u)) {
        const int last = TCAP - ne;   // slot of edge ne - 1
        tri[(3 * (TCAP - 1 - e)) * STRIDE] = tri[(3 * last) * STRIDE], tri[(3 * (TCAP - 1 - e) + 1) * STRIDE] = tri[(3 * last + 1) * STRIDE];
        ne--;
        return;
      }
    }
    if (nt + ne >= TCAP) {
      overflow = true;
      return;
    }
    tri[(3 * (TCAP - 1 - ne)) * STRIDE] = (uint8_t)u, tri[(3 * (TCAP - 1 - ne) + 1) * STRIDE] = (uint8_t)v;
    ne++;
  }

  static RG_HD void set_bit(uint64_t (&m)[kWords], int f) {
#pragma unroll
    for (int w = 0; w < kWords; w++)
      if ((f >> 6) == w) m[w] |= 1ull << (f & 63);
  }

  // Cuts the cell by the candidate `pid` at q: the triangles it is inside go, and every edge of the hole's rim gets a triangle with pid.
  // Returns whether it cut.  On overflow the cell is no longer valid.  Every loop is bounded by TCAP or FCAP.
  template <class Data>
  RG_HD bool clip(uint32_t pid, V3 q, Data& data, unsigned& uncertain) {
    ne = 0;
    int t = 0;
    while (t < nt) {
      if (!tri_inside(t, pid, q, data, uncertain)) {
        t++;
        continue;
      }
      const int a = corner(t, 0), b = corner(t, 1), c = corner(t, 2);
      nt--;
      if (t != nt) {
        set_tri(t, corner(nt, 0), corner(nt, 1), corner(nt, 2));
        data.move_tri(nt, t);
      }
      push_edge(a, b), push_edge(a, c), push_edge(b, c);
      if (overflow) return true;
    }
    if (ne == 0) return false;
    uint64_t used[kWords];
#pragma unroll
    for (int w = 0; w < kWords; w++) used[w] = 0ull;
    for (int k = 0; k < nt; k++) set_bit(used, corner(k, 0)), set_bit(used, corner(k, 1)), set_bit(used, corner(k, 2));
    for (int e = 0; e < ne; e++) set_bit(used, tri[(3 * (TCAP - 1 - e)) * STRIDE]), set_bit(used, tri[(3 * (TCAP - 1 - e) + 1) * STRIDE]);
    int fp = -1;
#pragma unroll
    for (int w = kWords - 1; w >= 0; w--)
      if (~used[w] != 0ull) fp = w * 64 + __builtin_ctzll(~used[w]);
    if (fp < 0 || fp >= FCAP) {
      overflow = true;
      return true;
    }
    face[fp * STRIDE] = pid;
    data.put_face(fp, q);
    // edges from the lowest slot up, triangles from nt up: a triangle is written at or below the slot of the edge just read
    const int count = ne;
    for (int k = 0; k < count; k++) {
      const int slot = TCAP - count + k;
      const int u = tri[(3 * slot) * STRIDE], v = tri[(3 * slot + 1) * STRIDE];
      set_tri(nt, u, v, fp);
      bool gu, gv;
      const V3 pu = member(u, data, gu), pv = member(v, data, gv);
      data.new_tri(nt, pu, gu, pv, gv, q, false);
      nt++;
    }
    ne = 0;
    return true;
  }

  // no triangle holds a ghost: the cell is bounded.  r2max: the largest squared circumradius (INFINITY where one is not trustworthy)
  template <class Data>
  RG_HD bool bounded(const Data& data, double& r2max) const {
    r2max = 0.0;
    for (int t = 0; t < nt; t++) {
      bool g0, g1, g2;
      const V3 p0 = member(corner(t, 0), data, g0), p1 = member(corner(t, 1), data, g1), p2 = member(corner(t, 2), data, g2);
      if (g0 || g1 || g2) return false;
      V3 centre;
      r2max = fmax(r2max, circumsphere(p0, p1, p2, centre));
    }
    return true;
  }
};

}  // namespace rgdl
