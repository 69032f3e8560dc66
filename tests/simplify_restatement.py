"""NumPy restatement of the mesh simplification (include/radegs.h, "Mesh simplification"; rade-gs_amd/csrc/radegs_meshsimplify.hip): float64,
operation for operation in the order the header writes, one function per stage.  Per-cell sums use np.add.at, which adds unbuffered in index
order: every cell's sum starts at 0.0 and takes its records one by one, ascending -- the order of the kernels.  The Jacobi sweeps run over all
cells at once; a pair the kernel leaves alone (a_pq == 0) keeps its values through np.where, which is also all the early exit does."""
import numpy as np

CELL_BITS = 21
SWEEPS = 8
CUT = 1e-3


# ----------------------------------------------------------------------------- cells -----------------------------------------------------------------------------
def default_origin(v, h):
    """Open3D's rule (from memory): the per-axis minimum less half a voxel"""
    return np.asarray(v, np.float64).min(0) - np.float64(h) / 2.0


def cell_coordinates(v, h, origin):
    c = np.floor((np.asarray(v, np.float64) - np.asarray(origin, np.float64)) / np.float64(h))
    if c.size and not (c.min() >= 0 and c.max() < 2 ** CELL_BITS):
        raise RuntimeError("a cell coordinate outside [0, 2^21)")
    return c.astype(np.int64)


def cells(v, h, origin):
    """(vertex_cell int64 [V], cell_key int64 [K]): the occupied cells numbered by ascending key"""
    c = cell_coordinates(v, h, origin)
    key = c[:, 0] << (2 * CELL_BITS) | c[:, 1] << CELL_BITS | c[:, 2]
    cell_key, vertex_cell = np.unique(key, return_inverse=True)
    return vertex_cell.astype(np.int64).reshape(-1), cell_key


def cell_sums(values, cell, K):
    """[K,C]: per cell the rows of `values` [N,C] with that cell, added to 0.0 in ascending row order"""
    values = np.asarray(values, np.float64)
    out = np.zeros((values.shape[1], K))
    for e in range(values.shape[1]):
        np.add.at(out[e], cell, np.ascontiguousarray(values[:, e]))
    return np.ascontiguousarray(out.T)


def cell_averages(values, vertex_cell, K):
    return cell_sums(values, vertex_cell, K) / np.bincount(vertex_cell, minlength=K).astype(np.float64)[:, None]


# ---------------------------------------------------------------------------- quadrics ----------------------------------------------------------------------------
def face_quadrics(v, f):
    """[F,10]: xx xy xz xd yy yz yd zz zd dd of w [n; d][n; d]^T, rows of 0.0 where the length is not positive and finite"""
    v = np.asarray(v, np.float64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w_ = b - a, c - a
    nx = u[:, 1] * w_[:, 2] - u[:, 2] * w_[:, 1]
    ny = u[:, 2] * w_[:, 0] - u[:, 0] * w_[:, 2]
    nz = u[:, 0] * w_[:, 1] - u[:, 1] * w_[:, 0]
    with np.errstate(all="ignore"):
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = (length > 0.0) & np.isfinite(length)
        w = 0.5 * length
        hx, hy, hz = nx / length, ny / length, nz / length
        d = -((hx * a[:, 0] + hy * a[:, 1]) + hz * a[:, 2])
        wx, wy, wz, wd = w * hx, w * hy, w * hz, w * d
        q = np.stack([wx * hx, wx * hy, wx * hz, wx * d, wy * hy, wy * hz, wy * d, wz * hz, wz * d, wd * d], 1)
    return np.where(ok[:, None], q, 0.0)


def cell_quadrics(v, f, vertex_cell, K):
    """[K,10]: one record per corner, added to the corner's cell in ascending (triangle, corner)"""
    return cell_sums(np.repeat(face_quadrics(v, f), 3, axis=0), vertex_cell[f.reshape(-1)], K)


def _rotate(app, aqq, apq, arp, arq, R, p, q):
    with np.errstate(all="ignore"):
        go = apq != 0.0
        theta = (aqq - app) / (2.0 * apq)
        t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        tp = t * apq
        new = (app - tp, aqq + tp, np.zeros_like(apq), c * arp - s * arq, s * arp + c * arq)
        app, aqq, apq, arp, arq = (np.where(go, n, o) for n, o in zip(new, (app, aqq, apq, arp, arq)))
        for k in range(3):
            kp, kq = c * R[k][p] - s * R[k][q], s * R[k][p] + c * R[k][q]
            R[k][p], R[k][q] = np.where(go, kp, R[k][p]), np.where(go, kq, R[k][q])
    return app, aqq, apq, arp, arq


def jacobi(Q):
    """(lambda [K,3], R: R[k][i] [K] = component k of eigenvector i) of the 3x3 blocks of Q [K,10]"""
    a00, a01, a02, a11, a12, a22 = (Q[:, i].copy() for i in (0, 1, 2, 4, 5, 7))
    one, zero = np.ones(Q.shape[0]), np.zeros(Q.shape[0])
    R = [[one.copy(), zero.copy(), zero.copy()], [zero.copy(), one.copy(), zero.copy()], [zero.copy(), zero.copy(), one.copy()]]
    for _ in range(SWEEPS):
        a00, a11, a01, a02, a12 = _rotate(a00, a11, a01, a02, a12, R, 0, 1)
        a00, a22, a02, a01, a12 = _rotate(a00, a22, a02, a01, a12, R, 0, 2)
        a11, a22, a12, a01, a02 = _rotate(a11, a22, a12, a01, a02, R, 1, 2)
    return np.stack([a00, a11, a22], 1), R


def cell_box(cell_key, h, origin):
    mask = (1 << CELL_BITS) - 1
    c = np.stack([(cell_key >> (2 * CELL_BITS)) & mask, (cell_key >> CELL_BITS) & mask, cell_key & mask], 1).astype(np.float64)
    o, h = np.asarray(origin, np.float64), np.float64(h)
    return o + c * h, o + (c + 1.0) * h


def solve(Q, m, cell_key, h, origin, details=False):
    """positions [K,3]; with details also (the unrestricted x, solved: lambda_max positive and finite, kept: x finite and inside the box)"""
    g = [((Q[:, r[0]] * m[:, 0] + Q[:, r[1]] * m[:, 1]) + Q[:, r[2]] * m[:, 2]) + Q[:, r[3]] for r in ((0, 1, 2, 3), (1, 4, 5, 6), (2, 5, 7, 8))]
    lam, R = jacobi(Q)
    lmax = lam[:, 0].copy()
    for i in (1, 2):
        lmax = np.where(lam[:, i] > lmax, lam[:, i], lmax)
    with np.errstate(all="ignore"):
        cut = CUT * lmax
        x = [m[:, 0].copy(), m[:, 1].copy(), m[:, 2].copy()]
        for i in range(3):
            coef = ((R[0][i] * g[0] + R[1][i] * g[1]) + R[2][i] * g[2]) / lam[:, i]
            use = lam[:, i] > cut
            for a in range(3):
                x[a] = np.where(use, x[a] - coef * R[a][i], x[a])
    x = np.stack(x, 1)
    lo, hi = cell_box(cell_key, h, origin)
    solved = (lmax > 0.0) & np.isfinite(lmax)
    kept = solved & np.isfinite(x).all(1) & ((x >= lo) & (x <= hi)).all(1)
    out = np.where(kept[:, None], x, m)
    return (out, x, solved, kept) if details else out


def quadric_error(Q, x):
    """E(x) = x^T A x + 2 b^T x + c per cell (plain NumPy, not part of the specification)"""
    A = np.stack([Q[:, [0, 1, 2]], Q[:, [1, 4, 5]], Q[:, [2, 5, 7]]], 1)
    return np.einsum("ki,kij,kj->k", x, A, x) + 2.0 * (Q[:, [3, 6, 8]] * x).sum(1) + Q[:, 9]


# ----------------------------------------------------------------------------- faces -----------------------------------------------------------------------------
def cell_faces(f, vertex_cell, K, remove_duplicates=True):
    """(cell_faces int64 [F,3]: rotated smallest first, rows of 0 where removed for a shared cell; remove bool [F])"""
    t = vertex_cell[f]
    dead = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 2] == t[:, 0])
    shift = np.argmin(t, axis=1)
    rot = np.take_along_axis(t, (shift[:, None] + np.arange(3)[None]) % 3, axis=1)
    rot[dead] = 0
    remove = dead.copy()
    if remove_duplicates and f.shape[0]:
        key = np.where(dead[:, None], K, rot)
        order = np.lexsort((np.arange(f.shape[0]), key[:, 2], key[:, 1], key[:, 0]))
        ks = key[order]
        same = (ks[1:] == ks[:-1]).all(1) & (ks[1:, 0] != K)
        remove[order[1:][same]] = True
    return rot.astype(np.int64), remove


def compact(K, faces, remove, drop_unreferenced=True):
    """(kept_cells int64 [K'], faces int64 [F',3] renumbered, face_source int64 [F']): radegs_meshclean_compact_plan / _apply"""
    source = np.flatnonzero(~remove)
    live = faces[source]
    keep = np.zeros(K, bool)
    if drop_unreferenced:
        keep[live.reshape(-1)] = True
    else:
        keep[:] = True
    kept = np.flatnonzero(keep)
    new = np.cumsum(keep) - 1
    return kept.astype(np.int64), new[live].astype(np.int64).reshape(-1, 3), source.astype(np.int64)


# --------------------------------------------------------------------------- the whole ---------------------------------------------------------------------------
def stages(vertices, faces, voxel_size, contraction="quadric", origin=None, attributes=None):
    """dict of every stage's result before compaction and rounding"""
    v = np.asarray(vertices, np.float64)
    origin = default_origin(v, voxel_size) if origin is None else np.asarray(origin, np.float64)
    vertex_cell, cell_key = cells(v, voxel_size, origin)
    K = cell_key.shape[0]
    out = dict(origin=origin, vertex_cell=vertex_cell, cell_key=cell_key, K=K, averages=cell_averages(v, vertex_cell, K), quadrics=None,
               attributes=None if attributes is None else cell_averages(np.asarray(attributes, np.float64), vertex_cell, K))
    out["positions"] = out["averages"]
    if contraction == "quadric":
        out["quadrics"] = cell_quadrics(v, faces, vertex_cell, K)
        out["positions"] = solve(out["quadrics"], out["averages"], cell_key, voxel_size, origin)
    return out


def simplify_vertex_clustering(vertices, faces, voxel_size, contraction="quadric", origin=None, attributes=None, remove_duplicates=True,
                               drop_unreferenced=True):
    """(vertices in the input dtype, faces int64, vertex_map int64 [V], face_source int64, attributes or None)"""
    vertices, faces = np.asarray(vertices), np.asarray(faces).astype(np.int64)
    s = stages(vertices, faces, voxel_size, contraction, origin, attributes)
    cf, remove = cell_faces(faces, s["vertex_cell"], s["K"], remove_duplicates)
    kept, out_f, source = compact(s["K"], cf, remove, drop_unreferenced)
    new = np.full(s["K"], -1, np.int64)
    new[kept] = np.arange(kept.shape[0])
    attr = None if attributes is None else s["attributes"][kept].astype(np.asarray(attributes).dtype)
    return s["positions"][kept].astype(vertices.dtype), out_f, new[s["vertex_cell"]], source, attr
