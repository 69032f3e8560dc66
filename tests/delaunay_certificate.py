"""A reference-free certificate that rows of point indices are THE Delaunay triangulation of float64 coordinates, in
NumPy with exact rational arithmetic where float64 cannot decide a sign.  No GPU, no scipy in the verdict.

    res = certify(X, cells);  defects(res) == {}  <=>  accepted

What is checked, and why it suffices.  (1) The rows have the format delaunay.triangulate promises.  (2) Every point is a corner.  (3) Every
row is positively oriented.  (4) No face lies in more than two rows, and the two rows of a shared face lie strictly on opposite sides of it.
(5) The faces of exactly one row form a closed surface with no point of X strictly outside any of them: with (4) that surface is the
boundary of the convex hull, and the rows, which cannot overlap across a face, tile what it encloses; the volume sum (6) is a float64
sanity figure on that tiling.  (7) Every shared face is locally Delaunay: the corner of one row opposite the face is not strictly inside the
other's circumsphere.  By the Delaunay lemma a triangulation of the hull of X whose interior faces are all locally Delaunay is a Delaunay
triangulation, and with no zero in-sphere sign (`cospherical`) it is the only one.  No neighbour search, no undecided case.

Signs.  e = 2^-53.  Both determinants are sums of monomials in coordinate differences, each difference rounded once.
  orient  det[b-a, c-a, d-a] = ((u x v) . w): a monomial u_y v_z w_x passes 3 roundings in the differences, 1 in u_y v_z, 1 in the
          subtraction forming (u x v)_x, 1 in the product with w_x and 2 in the two additions: 8 factors (1 + d), |d| <= e, a relative
          error below 8.01 e of the monomial's magnitude.  Summed, the error is below 8.01 e times the PERMANENT, the same expression with
          magnitudes for terms (Shewchuk 1997, section 4).  The permanent is computed in floating point too and may come out low by its
          own (1 + e)^8.  The float64 sign is taken where |det| > 16 e perm: twice the derived 8.01 e, which covers both and every e^2 term.
  sphere  with a, b, c, q relative to the row's first corner:  s = -|a|^2 det[b,c,q] + |b|^2 det[a,c,q] - |c|^2 det[a,b,q] + |q|^2 det[a,b,c];
          q is strictly inside iff s and det[a,b,c] have opposite signs.  |a|^2 is 2 differences, a product and two additions (5 roundings),
          times an 8-rounding determinant (1 more), and the sum of four terms (3 more): 17 roundings, below 17.01 e of the permanent, and the
          same again for the computed permanent's own shortfall.  The float64 sign is taken where |s| > 40 e perm.
A cruder filter, 1e-10 x the product of the row norms against an LU determinant's error near 1e-14 x that product, is safe as well; the
permanent is at most 3^(3/2) times that product (each row's 1-norm against its 2-norm) and the constants above are 1.8e-15 and 4.4e-15, so
this one is derived, not measured, and four orders tighter: fewer exact evaluations, none skipped.  Where a product could underflow
(permanent below 1e-280) the filter does not apply and the exact path decides.  Below the bound the sign is that of a fractions.Fraction determinant built from the ORIGINAL float64
coordinates, subtracted in rationals: exact, whatever the magnitude or offset of the cloud.

The hull's "no point outside" is F faces x N points, too many for determinants: one matrix product n . p against n . f0 is the coarse
filter, with its own bound (see _outside), and only the pairs it cannot decide go through the orient filter above."""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -53
ORIENT_BOUND = 16.0 * EPS
SPHERE_BOUND = 40.0 * EPS
TINY = 1e-280
COVER_RTOL = 1e-9
COUNTERS = ("format", "range", "order", "duplicate", "uncovered", "orientation", "face_multiplicity", "face_sides", "hull_open", "outside",
            "cover", "not_delaunay", "cospherical")


# ------------------------------------------------------------------------- exact arithmetic -------------------------------------------------------------------------
def _frac_rows(X, base, others):
    b = [Fraction(float(v)) for v in X[base]]
    return [[Fraction(float(v)) - b[k] for k, v in enumerate(X[o])] for o in others]


def _fdet3(u, v, w):
    return (u[1] * v[2] - u[2] * v[1]) * w[0] + (u[2] * v[0] - u[0] * v[2]) * w[1] + (u[0] * v[1] - u[1] * v[0]) * w[2]


def _sgn(x):
    return (x > 0) - (x < 0)


def exact_orient(X, a, b, c, d):
    """sign of det[b-a, c-a, d-a] on the float64 coordinates X, exactly"""
    u, v, w = _frac_rows(X, a, (b, c, d))
    return _sgn(_fdet3(u, v, w))


def exact_insphere(X, p, a, b, c, q):
    """+1: q strictly inside the sphere through p, a, b, c; 0: on it; -1: outside.  Exactly.  (0 also where p, a, b, c are coplanar.)"""
    ra, rb, rc, rq = _frac_rows(X, p, (a, b, c, q))
    n = [sum(x * x for x in r) for r in (ra, rb, rc, rq)]
    s = -n[0] * _fdet3(rb, rc, rq) + n[1] * _fdet3(ra, rc, rq) - n[2] * _fdet3(ra, rb, rq) + n[3] * _fdet3(ra, rb, rc)
    return -_sgn(s) * _sgn(_fdet3(ra, rb, rc))


# ------------------------------------------------------------------------- filtered signs -------------------------------------------------------------------------
def _det3(u, v, w):
    """(det[u,v,w] as (u x v).w, its permanent) of [K,3] arrays"""
    ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
    det = ((uy * vz - uz * vy) * wx + (uz * vx - ux * vz) * wy) + (ux * vy - uy * vx) * wz
    perm = (((np.abs(uy * vz) + np.abs(uz * vy)) * np.abs(wx) + (np.abs(uz * vx) + np.abs(ux * vz)) * np.abs(wy))
            + (np.abs(ux * vy) + np.abs(uy * vx)) * np.abs(wz))
    return det, perm


class Signs:
    """the two predicates over index arrays; `exact` counts the rational evaluations"""

    def __init__(self, X):
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.exact = 0

    def orient(self, a, b, c, d):
        """int8 signs of det[X[b]-X[a], X[c]-X[a], X[d]-X[a]]"""
        X = self.X
        a, b, c, d = (np.asarray(i, dtype=np.int64) for i in (a, b, c, d))
        det, perm = _det3(X[b] - X[a], X[c] - X[a], X[d] - X[a])
        sign = np.sign(det).astype(np.int8)
        for k in np.nonzero(~((np.abs(det) > ORIENT_BOUND * perm) & (perm > TINY)))[0]:
            sign[k] = exact_orient(X, int(a[k]), int(b[k]), int(c[k]), int(d[k]))
            self.exact += 1
        return sign

    def insphere(self, p, a, b, c, q):
        """int8: +1 where X[q] is strictly inside the sphere through X[p], X[a], X[b], X[c], 0 on it, -1 outside"""
        X = self.X
        p, a, b, c, q = (np.asarray(i, dtype=np.int64) for i in (p, a, b, c, q))
        ra, rb, rc, rq = X[a] - X[p], X[b] - X[p], X[c] - X[p], X[q] - X[p]
        dbcq, pbcq = _det3(rb, rc, rq)
        dacq, pacq = _det3(ra, rc, rq)
        dabq, pabq = _det3(ra, rb, rq)
        o, pabc = _det3(ra, rb, rc)
        la, lb, lc, lq = ((r * r).sum(axis=1) for r in (ra, rb, rc, rq))
        s = ((lb * dacq - la * dbcq) - lc * dabq) + lq * o
        ps = ((lb * pacq + la * pbcq) + lc * pabq) + lq * pabc
        sign = (-np.sign(s) * np.sign(o)).astype(np.int8)
        sure = (np.abs(s) > SPHERE_BOUND * ps) & (np.abs(o) > ORIENT_BOUND * pabc) & (ps > TINY) & (pabc > TINY)
        for k in np.nonzero(~sure)[0]:
            sign[k] = exact_insphere(X, int(p[k]), int(a[k]), int(b[k]), int(c[k]), int(q[k]))
            self.exact += 1
        return sign


# ------------------------------------------------------------------------- the parts -------------------------------------------------------------------------
def _faces(asc):
    """the 4 T faces of ascending rows [T,4]: (face [4T,3] ascending, opposite corner [4T], row [4T])"""
    T = asc.shape[0]
    keep = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])
    face = asc[:, keep].reshape(4 * T, 3)
    opp = asc.reshape(4 * T)
    row = np.repeat(np.arange(T, dtype=np.int64), 4)
    return face, opp, row


def _group(keys_cols, n):
    """(order, start of every run, length of every run) of rows of small non-negative integers below n, by one packed int64 key or lexsort"""
    if float(n) ** len(keys_cols) < 2.0 ** 62:
        key = np.zeros(keys_cols[0].shape[0], dtype=np.int64)
        for col in keys_cols:
            key = key * n + col
        order = np.argsort(key, kind="stable")
        s = key[order]
        head = np.concatenate([[True], s[1:] != s[:-1]]) if s.size else np.zeros(0, dtype=bool)
    else:
        order = np.lexsort(keys_cols[::-1])
        cols = [col[order] for col in keys_cols]
        head = np.ones(order.shape[0], dtype=bool)
        if order.size:
            head[1:] = np.any([col[1:] != col[:-1] for col in cols], axis=0)
    start = np.nonzero(head)[0]
    length = np.diff(np.concatenate([start, [order.shape[0]]]))
    return order, start, length


def _outside(sg, hull, inner, chunk=256):
    """How many (once-face, point) pairs have the point strictly on the other side of the face than the face's own row.
    hull [F,3], inner [F]: the opposite corner.  Coarse filter: with n = (f1 - f0) x (f2 - f0) and En its permanent, component by
    component, v = n . p - n . f0 evaluated as a matrix product.  n_k carries 2 difference roundings, a product and a subtraction: an error
    below 4.01 e En_k; n_k p_k one more rounding and the three-term sums two more, on magnitudes at most |n_k| M <= En_k M with M the
    largest |coordinate|; the same for n . f0 and one rounding for the final subtraction.  In all below 2 x (4.01 + 3.01) e sum(En) M plus the
    subtraction's e |v|: the sign of v is taken where |v| > 32 e sum(En) M, and every other pair, a face's own corners apart (exactly on
    it), goes through the orient filter."""
    X = sg.X
    F, N = hull.shape[0], X.shape[0]
    if F == 0:
        return 0
    side_in = sg.orient(hull[:, 0], hull[:, 1], hull[:, 2], inner)       # non-zero: rows are not flat (checked by the caller)
    M = float(np.abs(X).max())
    bad = 0
    for lo in range(0, F, chunk):
        h = hull[lo:lo + chunk]
        f0, e1, e2 = X[h[:, 0]], X[h[:, 1]] - X[h[:, 0]], X[h[:, 2]] - X[h[:, 0]]
        n = np.cross(e1, e2)
        En = (np.abs(e1[:, [1, 2, 0]] * e2[:, [2, 0, 1]]) + np.abs(e1[:, [2, 0, 1]] * e2[:, [1, 2, 0]])).sum(axis=1)
        v = n @ X.T - (n * f0).sum(axis=1)[:, None]                        # [f, N]
        bound = (32.0 * EPS * M) * En
        s_in = side_in[lo:lo + chunk].astype(np.float64)[:, None]
        sure = (np.abs(v) > bound[:, None]) & (bound[:, None] > TINY)
        bad += int((sure & (np.sign(v) == -s_in)).sum())
        fi, pi = np.nonzero(~sure)
        own = (pi[:, None] == h[fi]).any(axis=1)
        fi, pi = fi[~own], pi[~own]
        if fi.size:
            s = sg.orient(h[fi, 0], h[fi, 1], h[fi, 2], pi)
            bad += int((s == -side_in[lo + fi]).sum())
    return bad


def _scipy_hull_agrees(X, hull):
    """None where scipy is absent or refuses; else whether its facets are the same set of triangles.  Information only."""
    try:
        from scipy.spatial import ConvexHull
        theirs = np.unique(np.sort(ConvexHull(X).simplices, axis=1), axis=0)
    except Exception:
        return None
    mine = np.unique(hull, axis=0)
    return bool(mine.shape == theirs.shape and np.array_equal(mine, theirs))


def certify(X, cells, cross_check=False):
    """X float64 [N,3], cells int [T,4]: a dict of the COUNTERS, every one the number of defects of that kind (all 0: accepted;
    `cospherical` is a defect only for points claimed to be in general position), plus information: `exact`, the rational evaluations;
    `hull_faces`; `interior_faces`; `volume`; `scipy_hull_agrees` (with cross_check).  A row with an index out of range ends the check
    after the format counters: nothing geometric can be said of it."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    cells = np.asarray(cells)
    assert X.ndim == 2 and X.shape[1] == 3 and cells.ndim == 2 and cells.shape[1] == 4 and cells.dtype.kind in "iu" and np.isfinite(X).all()
    N, T = X.shape[0], cells.shape[0]
    cells = cells.astype(np.int64)
    res = dict.fromkeys(COUNTERS, 0)
    res.update(exact=0, hull_faces=0, interior_faces=0, volume=0.0, scipy_hull_agrees=None)
    # (1) format
    asc = np.sort(cells, axis=1)
    res["range"] = int(((cells < 0) | (cells >= N)).any(axis=1).sum())
    shape_ok = (cells[:, :2] == asc[:, :2]).all(axis=1) & (np.sort(cells[:, 2:], axis=1) == asc[:, 2:]).all(axis=1) & (asc[:, :-1] < asc[:, 1:]).all(axis=1)
    res["format"] = int((~shape_ok).sum())
    if T > 1:
        diff = asc[1:] - asc[:-1]
        first = np.argmax(diff != 0, axis=1)                               # the first column that differs (0 where none does)
        lead = diff[np.arange(T - 1), first]
        res["order"], res["duplicate"] = int((lead < 0).sum()), int((lead == 0).sum())
    if res["range"] or T == 0:
        res["uncovered"] = N if T == 0 else 0
        return res
    # (2) every point is a corner
    res["uncovered"] = int(N - np.unique(cells).shape[0])
    sg = Signs(X)
    # (3) orientation of the rows as presented
    row_sign = sg.orient(cells[:, 0], cells[:, 1], cells[:, 2], cells[:, 3])
    res["orientation"] = int((row_sign <= 0).sum())
    # the geometry of the SET of tetrahedra: distinct ascending quadruples without a repeated index
    quads = np.unique(asc[(asc[:, :-1] < asc[:, 1:]).all(axis=1)], axis=0)
    quad_sign = sg.orient(quads[:, 0], quads[:, 1], quads[:, 2], quads[:, 3])
    flat = quad_sign == 0
    # (4) faces
    face, opp, row = _faces(quads)
    order, start, length = _group([face[:, 0], face[:, 1], face[:, 2]], N)
    res["face_multiplicity"] = int((length > 2).sum())
    two, one = start[length == 2], start[length == 1]
    fa, fb = order[two], order[two + 1]
    res["interior_faces"] = int(two.shape[0])
    sa = sg.orient(face[fa, 0], face[fa, 1], face[fa, 2], opp[fa])
    sb = sg.orient(face[fb, 0], face[fb, 1], face[fb, 2], opp[fb])
    res["face_sides"] = int((sa * sb >= 0).sum())
    # (5) hull
    h = order[one]
    hull, inner = face[h], opp[h]
    res["hull_faces"] = int(hull.shape[0])
    edges = np.concatenate([hull[:, [0, 1]], hull[:, [0, 2]], hull[:, [1, 2]]])
    _, _, elen = _group([edges[:, 0], edges[:, 1]], N)
    res["hull_open"] = int((elen != 2).sum()) + (1 if hull.shape[0] == 0 else 0)
    proper = ~flat[row[h]]
    res["outside"] = _outside(sg, hull[proper], inner[proper])
    # (6) cover: float64 sums about the centroid, a sanity figure
    C = X - X.mean(axis=0)
    a, b, c, d = (C[quads[:, k]] for k in range(4))
    vol_rows = float(np.abs(np.einsum("ij,ij->i", np.cross(b - a, c - a), d - a)).sum() / 6.0)
    f0, f1, f2, pin = C[hull[:, 0]], C[hull[:, 1]], C[hull[:, 2]], C[inner]
    nrm = np.cross(f1 - f0, f2 - f0)
    outward = np.where(np.einsum("ij,ij->i", nrm, pin - f0) > 0, -1.0, 1.0)
    vol_hull = float((outward * np.einsum("ij,ij->i", nrm, f0)).sum() / 6.0)
    res["volume"] = vol_rows
    res["cover"] = 0 if abs(vol_rows - vol_hull) <= COVER_RTOL * max(abs(vol_hull), abs(vol_rows)) and vol_rows > 0 else 1
    # (7) local Delaunay across every shared face whose first row is not flat
    ok = ~flat[row[fa]]
    qa = quads[row[fa[ok]]]
    s = sg.insphere(qa[:, 0], qa[:, 1], qa[:, 2], qa[:, 3], opp[fb[ok]])
    res["not_delaunay"], res["cospherical"] = int((s > 0).sum()), int((s == 0).sum())
    res["exact"] = sg.exact
    if cross_check:
        res["scipy_hull_agrees"] = _scipy_hull_agrees(X, hull)
    return res


def defects(res, general_position=True):
    """the non-zero counters of a certify() result; {} is acceptance"""
    return {k: res[k] for k in COUNTERS if res[k] and (general_position or k != "cospherical")}
