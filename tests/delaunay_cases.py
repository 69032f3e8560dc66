"""The Delaunay fixtures (tests/golden/make_golden_delaunay.py wrote them from scipy.spatial.Delaunay), shared by the CPU and GPU tiers."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name: (points, tetrahedra); the jittered cases are the exactly degenerate ones
CASES = {"random4": (4, 1), "random5": (5, 3), "random8": (8, 10), "random64": (64, 296), "random65": (65, 296), "random200": (200, 1133),
         "random1000": (1000, 6380), "sphere120": (120, 343), "shell151": (151, 296), "clusters120": (120, 643), "grid64": (64, 308),
         "boxes270": (270, 1591)}
JITTERED = ("grid64", "boxes270")
_cache = {}


def load(name):
    """the fixture as a dict of arrays; loaded once, never modified"""
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, f"delaunay_{name}.npz")) as z:
            fx = {k: z[k] for k in z.files}
        for v in fx.values():
            v.setflags(write=False)
        assert fx["points"].shape == (CASES[name][0], 3) and fx["cells"].shape == (CASES[name][1], 4), name
        assert (float(fx["jitter"]) > 0) == (name in JITTERED)
        _cache[name] = fx
    return _cache[name]


# ------------------------------------------------------------------------- generated clouds -------------------------------------------------------------------------
# The clouds of the scale tier (tests/test_gpu_delaunay_scale.py, tests/test_delaunay_certificate.py): float32, seeded, generated and never
# committed.  tests/delaunay_certificate.py, not a fixture, is what their triangulations are held to.
f32 = np.float32
SHELL_LADDER = (150, 200, 240, 250, 253, 254, 255, 256, 257, 300)      # round the slow kernel's 256 faces / 508 triangles
FAST_LADDER = (40, 47, 48, 49, 60)                                     # round the fast kernel's 48 faces / 92 triangles


def _surface_z(x, y):
    return 0.1 * np.sin(6.0 * x) * np.cos(5.0 * y)


def uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(f32)


def slab(n, seed):
    """a 1000 : 1 : 1 box: the search grid is (side, 1, 1)"""
    return (np.random.default_rng(seed).random((n, 3)) * np.array([1000.0, 1.0, 1.0])).astype(f32)


def clustered(n, seed):
    """nine points in ten inside a cube of side 1e-3 of the unit cube: one grid cell holds them all"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3))
    moved = rng.permutation(n)[:(9 * n) // 10]
    p[moved] = 0.4 + 1e-3 * rng.random((moved.shape[0], 3))
    return p.astype(f32)


def surface(n, seed):
    """(4 u, 2 v, 0.1 sin 6x cos 5y + 1e-3 n): a thin wavy sheet, as a reconstruction's points are"""
    rng = np.random.default_rng(seed)
    x, y = 4.0 * rng.random(n), 2.0 * rng.random(n)
    return np.stack([x, y, _surface_z(x, y) + 1e-3 * rng.normal(size=n)], axis=1).astype(f32)


def box_gaussians(n, seed):
    """(xyz, scales, raw rotation) float32 of n Gaussians near the sheet: scales 0.01 .. 0.04 with one axis x 0.05, random rotations.
    tetmesh.tetra_points (GPU) or tetmesh_restatement.tetra_points (NumPy) makes the 9 n exactly degenerate box points of them."""
    rng = np.random.default_rng(seed)
    x, y = 4.0 * rng.random(n), 2.0 * rng.random(n)
    xyz = np.stack([x, y, _surface_z(x, y) + 1e-2 * rng.normal(size=n)], axis=1)
    scales = 0.01 + 0.03 * rng.random((n, 3))
    scales[np.arange(n), rng.integers(0, 3, size=n)] *= 0.05
    return xyz.astype(f32), scales.astype(f32), rng.normal(size=(n, 4)).astype(f32)


def two_lines(noise, seed):
    """100 sorted points on (t, 0, 0) and 100 on (0.5, s - 0.5, 1), skew lines, plus Gaussian noise: nearly every point of one line is
    joined to every one of the other, about n^2 / 4 tetrahedra: far more than the 32 N + 1024 records a first plan has room for"""
    rng = np.random.default_rng(seed)
    t, s = np.sort(rng.random(100)), np.sort(rng.random(100))
    a = np.stack([t, np.zeros(100), np.zeros(100)], axis=1)
    b = np.stack([np.full(100, 0.5), s - 0.5, np.ones(100)], axis=1)
    return (np.concatenate([a, b]) + noise * rng.normal(size=(200, 3))).astype(f32)


def shell(k, seed=None):
    """k unit vectors and, last, the origin: the centre's cell has k faces and 2 k - 4 vertices"""
    v = np.random.default_rng(1000 + k if seed is None else seed).normal(size=(k, 3))
    return np.concatenate([v / np.linalg.norm(v, axis=1, keepdims=True), np.zeros((1, 3))]).astype(f32)


def duplicated(n, seed):
    """n uniform points, each listed twice: only the jitter separates a pair"""
    return np.repeat(uniform(n, seed), 2, axis=0)


GENERATED = {"uniform50k": lambda: uniform(50000, 50), "slab20k": lambda: slab(20000, 51), "clustered20k": lambda: clustered(20000, 52),
             "surface20k": lambda: surface(20000, 53), "lines200a": lambda: two_lines(1e-4, 54), "lines200b": lambda: two_lines(1e-6, 55),
             "dup200": lambda: duplicated(100, 56)}
BOXES2000 = (2000, 57)


def cloud(name):
    """a generated cloud by name (`boxes2000`: the NumPy restatement of the box points); made once, never modified"""
    if name not in _cache:
        if name == "boxes2000":
            import tetmesh_restatement as tr
            p = tr.tetra_points(*box_gaussians(*BOXES2000))[0]
        else:
            p = GENERATED[name]()
        p.setflags(write=False)
        _cache[name] = p
    return _cache[name]


# the search grid of csrc/radegs_delaunay.hip (grid_side, make_grid, cell_coord), restated
GRID_MAX = 512


def make_grid(N, bounds):
    """(lo [3], h, dim [3]) of the grid plan lays over `bounds` = [min x, y, z, max x, y, z]"""
    side = min(max(int(np.ceil(np.cbrt(N / 2.0))), 1), GRID_MAX)
    lo, ext = np.asarray(bounds[:3], dtype=np.float64), np.asarray(bounds[3:], dtype=np.float64) - np.asarray(bounds[:3], dtype=np.float64)
    m = max(float(ext.max()), 0.0)
    if not m > 0.0:
        return lo, 0.0, [1, 1, 1]                                              # a box of no extent: one cell of no size
    h = m / side
    dim = [side if c >= side else (int(c) if c >= 1.0 else 1) for c in (np.floor(ext / h) + 1.0)]
    return lo, h, dim


def cell_keys(X, grid):
    """the cell of every point: a point outside the bounds lands in the border cell"""
    lo, h, dim = grid
    t = np.floor((X - lo) / h) if h > 0.0 else np.zeros_like(X)
    c = [np.where(t[:, k] >= dim[k] - 1, dim[k] - 1, np.where(t[:, k] >= 1.0, t[:, k], 0)).astype(np.int64) for k in range(3)]
    return (c[2] * dim[1] + c[1]) * dim[0] + c[0]


def vertex_degrees(N, cells):
    """the number of distinct neighbours of every point"""
    pairs = np.concatenate([cells[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    pairs = np.unique(np.sort(pairs, axis=1), axis=0)
    return np.bincount(pairs.reshape(-1), minlength=N)
