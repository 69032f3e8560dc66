"""NumPy restatement of rade-gs_amd/delaunay.py (include/radegs.h, "Delaunay"): the perturbation, bit for bit, and the
per-point cell clipping with the four ghost generators at infinity, by brute force over all points.

A cell is a list of triangles, each an ascending triple of generator ids; ids N..N+3 are the ghosts.  With q = p - x_i and a, b, c the real
members of a triangle relative to x_i, every rule of the specification is linear in (q, |q|^2):
    no ghost     s = A.q + |q|^2 o,  A = -|a|^2 b x c + |b|^2 a x c - |c|^2 a x b,  o = det[a,b,c];   inside iff s o < 0
    ghosts       n = a x b | a x (d1 - d2) | (d1 - d2) x (d1 - d3);                                   inside iff (n.q)(n.d1) > 0
so a triangle is one row m of four numbers with "inside iff m.(q, |q|^2) < 0", and a whole cell against many candidates is one matrix
product.  The regrouping changes roundings, not rules: the fixtures are the cases on which no predicate is near its error bound."""
import math

import numpy as np

# the four unit vertex directions of a regular tetrahedron, (+-1,+-1,+-1)/sqrt(3) under Rz(0.37) Rx(0.53): none parallel to a coordinate
# plane.  The same twelve literals as csrc/rg_delaunay_cell.h.
GHOST_DIRECTIONS = np.array([
    [0.4636882752759316, 0.40109187134201146, 0.7900117050493591],
    [0.6128706126410551, 0.01646566263417587, -0.7900117050493591],
    [-0.8239598679372936, 0.5277707489782728, -0.20627208379146042],
    [-0.25259901997969325, -0.9453282829544601, 0.20627208379146042]])

_M64 = (1 << 64) - 1


def hash_u53(seed, counter):
    """the 53-bit integer of (seed, counter): a splitmix64 finaliser over counter and seed spread by two odd constants, top 53 bits"""
    z = ((counter + 1) * 0x9E3779B97F4A7C15 + seed * 0xD1B54A32D192ED03) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return (z ^ (z >> 31)) >> 11


def diagonal(points64):
    d = points64.max(axis=0) - points64.min(axis=0)
    return math.sqrt((float(d[0]) * float(d[0]) + float(d[1]) * float(d[1])) + float(d[2]) * float(d[2]))


def perturbed(points, jitter, seed):
    """x + (jitter diag) (u - 0.5), u = hash_u53(seed, 3 i + axis) 2^-53; float64 [N,3]; jitter = 0 is the input widened"""
    x = np.asarray(points).astype(np.float64)
    if jitter == 0:
        return x
    scale = float(jitter) * diagonal(x)
    u = np.array([[hash_u53(seed, 3 * i + k) for k in range(3)] for i in range(x.shape[0])], dtype=np.float64) * 2.0 ** -53
    return x + scale * (u - 0.5)


def _rows(X, xi, tris):
    """the [T,4] rows m of ascending triangles `tris` [T,3]: inside iff m.(q, |q|^2) < 0"""
    N = X.shape[0]
    out = np.zeros((tris.shape[0], 4))
    for t, tri in enumerate(tris):
        real = [X[g] - xi for g in tri if g < N]
        gh = [GHOST_DIRECTIONS[g - N] for g in tri if g >= N]
        if not gh:
            a, b, c = real
            o = float(np.dot(np.cross(a, b), c))
            A = -np.dot(a, a) * np.cross(b, c) + np.dot(b, b) * np.cross(a, c) - np.dot(c, c) * np.cross(a, b)
            out[t, :3], out[t, 3] = A, o
            out[t] *= 1.0 if o > 0 else -1.0
        else:
            if len(gh) == 1:
                n = np.cross(real[0], real[1])
            elif len(gh) == 2:
                n = np.cross(real[0], gh[0] - gh[1])
            else:
                n = np.cross(gh[0] - gh[1], gh[0] - gh[2])
            out[t, :3] = -n if float(np.dot(n, gh[0])) > 0 else n
    return out


def cell(X, i):
    """the triangles [T,3] (ascending ids, ghosts >= N) of point i's cell among all the points X [N,3] float64"""
    N = X.shape[0]
    xi = X[i]
    tris = np.array([[N, N + 1, N + 2], [N, N + 1, N + 3], [N, N + 2, N + 3], [N + 1, N + 2, N + 3]], dtype=np.int64)
    M = _rows(X, xi, tris)
    cand = np.array([p for p in range(N) if p != i], dtype=np.int64)
    Q = X[cand] - xi
    cand = cand[np.argsort((Q * Q).sum(axis=1), kind="stable")]             # nearest first: the order changes the work, not the cell
    while cand.size:
        Q = X[cand] - xi
        Q4 = np.concatenate([Q, (Q * Q).sum(axis=1, keepdims=True)], axis=1)
        vals = M @ Q4.T                                                     # [T, K]
        cuts = (vals < 0).any(axis=0)
        cand, vals = cand[cuts], vals[:, cuts]                              # a cell only shrinks: who does not cut now never will
        if not cand.size:
            break
        p, marked = int(cand[0]), vals[:, 0] < 0
        cand = cand[1:]
        gone = tris[marked]
        edges = np.concatenate([gone[:, [0, 1]], gone[:, [0, 2]], gone[:, [1, 2]]])
        uniq, cnt = np.unique(edges, axis=0, return_counts=True)
        new = np.sort(np.concatenate([uniq[cnt == 1], np.full((int((cnt == 1).sum()), 1), p, dtype=np.int64)], axis=1), axis=1)
        tris = np.concatenate([tris[~marked], new])
        M = np.concatenate([M[~marked], _rows(X, xi, new)])
    return tris


def records(X):
    """every all-real triangle of every cell as the ascending quadruple (i, a, b, c): [R,4] int64, R = 4 T on a consistent input"""
    N = X.shape[0]
    out = []
    for i in range(N):
        t = cell(X, i)
        t = t[(t < N).all(axis=1)]
        out.append(np.sort(np.concatenate([np.full((t.shape[0], 1), i, dtype=np.int64), t], axis=1), axis=1))
    return np.concatenate(out)


def orient(X, cells):
    """rows with the last two swapped where det[b-a, c-a, d-a] < 0"""
    a, b, c, d = (X[cells[:, k]] for k in range(4))
    det = np.einsum("ij,ij->i", np.cross(b - a, c - a), d - a)
    out = cells.copy()
    out[det < 0] = out[det < 0][:, [0, 1, 3, 2]]
    return out


def volume(X, cells):
    a, b, c, d = (X[cells[:, k]] for k in range(4))
    return float(np.abs(np.einsum("ij,ij->i", np.cross(b - a, c - a), d - a)).sum() / 6.0)


def triangulate(X):
    """(cells int32 [T,4]: unique ascending rows in lexicographic order, oriented; found: how often each was found)"""
    rec = records(X)
    uniq, found = np.unique(rec, axis=0, return_counts=True)
    return orient(X, uniq).astype(np.int32), found
