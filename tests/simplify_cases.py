"""The seeded meshes of the mesh simplification tests, each the smallest input at which one stage can go wrong.  CASES maps a name to a Case
(vertices float64 [V,3], faces int64 [F,3], voxel size, origin or None for the default, attributes float64 [V,A] or None); the restatement's
stages are computed once per (case, contraction) and shared (reference())."""
import collections
import functools

import numpy as np

import simplify_restatement as sr

Case = collections.namedtuple("Case", "vertices faces h origin attributes")
COUNTS = (1, 63, 64, 65, 255, 256, 257)      # the wave and block edges of the per-cell sums


def I(rows):
    return np.array(rows, np.int64).reshape(-1, 3)


def inside(rng, cell, n, h=1.0, margin=0.1):
    """n points strictly inside the cell (integer coordinates) of a grid of step h at the origin"""
    return (np.asarray(cell, np.float64) + rng.uniform(margin, 1.0 - margin, (n, 3))) * h


def join(*parts):
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + base)
        base += v.shape[0]
    return np.concatenate(vs), np.concatenate(fs)


def fans(rng, counts=COUNTS):
    """per count n: a cell of n vertices, each the first corner of one triangle whose other corners are two single vertices in two other cells --
    the cell holds n vertices and n corner records, the two apex cells 1 vertex and n records each"""
    parts = []
    for k, n in enumerate(counts):
        v = np.concatenate([inside(rng, (4 * k, 0, 0), n), inside(rng, (4 * k, 2, 0), 1), inside(rng, (4 * k, 0, 2), 1)])
        i = np.arange(n)
        parts.append((v, np.stack([i, np.full(n, n), np.full(n, n + 1)], 1).astype(np.int64)))
    return join(*parts)


def surface(nx, ny, height, rng=None, jitter=0.0, step=1.0):
    """an nx x ny grid of quads over z = height(x, y), two triangles each, counter-clockwise seen from +z"""
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    x, y = gx.reshape(-1) * step, gy.reshape(-1) * step
    if rng is not None:
        x, y = x + rng.uniform(-jitter, jitter, x.shape) * step, y + rng.uniform(-jitter, jitter, y.shape) * step
    v = np.stack([x, y, height(x, y)], 1).astype(np.float64)
    q = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([q, q + 1, q + nx + 2], 1), np.stack([q, q + nx + 2, q + nx + 1], 1)])
    return v, f.astype(np.int64)


def sphere(levels):
    """a closed, outward-oriented surface: an octahedron subdivided `levels` times and pushed onto the unit sphere"""
    v = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, g = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = (np.asarray(v[a]) + np.asarray(v[b])) / 2.0
                v.append(tuple(p / np.linalg.norm(p)))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = g
    return np.array(v, np.float64), np.array(f, np.int64)


ROOF_RIDGE = 10.0          # the roof's two planes z = +-0.5 (x - ROOF_RIDGE) + const meet on the line x = ROOF_RIDGE


def roof_height(x, y):
    return 3.2 - 0.5 * np.abs(x - ROOF_RIDGE)


def _build():
    rng = np.random.default_rng(21)
    c = {}
    v, f = fans(rng)
    c["fans"] = Case(v, f, 1.0, (0.0, 0.0, 0.0), rng.uniform(0.0, 1.0, (v.shape[0], 3)))
    c["fans_shuffled"] = Case(v, f[np.random.default_rng(3).permutation(f.shape[0])], 1.0, (0.0, 0.0, 0.0), c["fans"].attributes)
    # a vertex no face references, in a cell of its own: dropped with drop_unreferenced, kept without
    v, f = surface(6, 6, lambda x, y: 0.3 * np.sin(x) + 0.2 * y, rng, 0.2)
    c["unreferenced_cell"] = Case(np.concatenate([v, [[40.0, 40.0, 40.0]]]), f, 2.0, None, None)
    c["one_cell"] = Case(v, f, 64.0, None, None)                                                    # K = 1, F' = 0
    # vertices exactly on cell faces: a power-of-two step and coordinates k h / 2, so the division is exact and floor decides
    v, f = surface(16, 16, lambda x, y: 0.125 * ((x * 8).astype(np.int64) % 3), None, 0.0, 0.125)
    c["on_cell_faces"] = Case(v, f, 0.25, (0.0, 0.0, 0.0), None)
    # the last cell of an axis: cx = 2^21 - 1
    # (margin 0.25: a float32 at 2^21 has steps of 0.25, and the rounded copy of the case must stay in its cells)
    v = np.concatenate([inside(rng, (2 ** 21 - 1, 0, 0), 3, 1.0, 0.25), inside(rng, (2 ** 21 - 3, 1, 0), 2, 1.0, 0.25), inside(rng, (2 ** 21 - 2, 0, 1), 2, 1.0, 0.25)])
    c["last_cell"] = Case(v, I([[0, 3, 5], [1, 4, 6], [2, 3, 6]]), 1.0, (0.0, 0.0, 0.0), None)
    # zero-area (collinear, and two equal positions) and index-degenerate triangles among good ones
    v, f = surface(8, 8, lambda x, y: 0.1 * x * y, rng, 0.2)
    line = np.array([[20.0, 0.5, 0.5], [23.0, 0.5, 0.5], [26.0, 0.5, 0.5], [29.5, 3.5, 0.5], [29.5, 3.5, 0.5]])
    c["degenerate_triangles"] = Case(np.concatenate([v, line]), np.concatenate([f, I([[81, 82, 83], [81, 84, 85], [0, 0, 20], [5, 40, 5], [81, 83, 84]])]), 2.5,
                                     None, None)
    # duplicates after clustering, of equal and of opposite orientation, and a face that only collapses
    v = np.concatenate([inside(rng, (0, 0, 0), 4), inside(rng, (3, 0, 0), 4), inside(rng, (0, 3, 0), 4), inside(rng, (3, 3, 3), 2)])
    c["duplicates"] = Case(v, I([[0, 4, 8], [5, 9, 1], [10, 2, 6], [3, 7, 11], [8, 4, 0], [0, 1, 4], [1, 5, 12], [13, 2, 6], [6, 2, 13]]), 1.0, (0.0, 0.0, 0.0),
                           rng.uniform(0.0, 1.0, (14, 2)))
    # rank 1: a plane (tilted, so that no axis is special)
    c["plane"] = Case(*surface(24, 24, lambda x, y: 0.25 * x - 0.4 * y + 7.0, rng, 0.2), 4.0, None, None)
    # rank 2: a crease
    c["roof"] = Case(*surface(24, 12, roof_height, rng, 0.0), 3.0, (-0.5, -0.5, -4.0), None)
    # rank 3: a corner of three planes, z = max of two slopes over a floor
    c["corner"] = Case(*surface(20, 20, lambda x, y: np.maximum(np.maximum(0.7 * (x - 10.0), 0.6 * (y - 10.0)), 0.0), rng, 0.0), 5.0, (-0.5, -0.5, -1.0), None)
    # two sheets through the same cells whose planes meet outside them: the solve leaves the box and the mean is taken
    lower, upper = surface(3, 3, lambda x, y: 0.3 + 0.1 * x, None, 0.0, 0.3), surface(3, 3, lambda x, y: 0.6 - 0.1 * x, None, 0.0, 0.3)
    v, f = join(lower, upper)
    c["leaves_the_box"] = Case(v + np.array([0.05, 0.05, 0.0]), f, 1.0, (0.0, 0.0, 0.0), None)
    v, f = surface(40, 40, lambda x, y: 1.5 * np.sin(0.3 * x) * np.cos(0.25 * y) + 0.05 * x, rng, 0.25)
    order = np.random.default_rng(8).permutation(f.shape[0])
    c["bumpy_coloured"] = Case(v, f[order], 3.7, None, rng.uniform(0.0, 1.0, (v.shape[0], 3)))
    c["sphere"] = Case(*sphere(4), 0.23, None, None)                                                # 2048 triangles, closed
    return c


CASES = _build()
NAMES = tuple(CASES)
CONTRACTIONS = ("quadric", "average")


@functools.lru_cache(maxsize=None)
def reference(name, contraction="quadric", dtype="float64"):
    """the restatement's stages of a case (vertices first rounded to `dtype`): computed once, shared, not to be written to"""
    c = CASES[name]
    attributes = None if c.attributes is None else c.attributes.astype(dtype)
    out = sr.stages(c.vertices.astype(dtype), c.faces, c.h, contraction, c.origin, attributes)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
