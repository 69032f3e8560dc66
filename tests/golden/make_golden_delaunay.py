"""Writes tests/golden/delaunay_*.npz: the Delaunay fixtures.  scipy.spatial.Delaunay (Qhull) is the reference; no other
code is involved.  Every file holds `points`, `jitter`, `seed`, `perturbed` (float64: the coordinates triangulated; the points widened
where jitter is 0), `cells` (scipy's simplices as ascending int32 rows in lexicographic order) and `hull_volume`.

    python tests/golden/make_golden_delaunay.py

Before a file is written the maker asserts that scipy reports no coplanar point and that tests/delaunay_restatement.py gives the same set
of cells, each found exactly four times.  A case that fails is to be replaced, not tolerated."""
import os
import sys

import numpy as np
from scipy.spatial import ConvexHull, Delaunay

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import delaunay_restatement as dr  # noqa: E402
import tetmesh_restatement as tr   # noqa: E402

f32 = np.float32


def random_points(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(f32)


def sphere(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def shell_and_centre(n, seed):
    """n points on the unit sphere round one at its centre: the centre's cell has about n faces"""
    return np.concatenate([sphere(n, seed), np.array([[0.013, -0.007, 0.009]], dtype=f32)])


def two_clusters(n, seed):
    p = random_points(n, seed)
    p[n // 2:, 0] += f32(60.0)
    return p


def grid(k):
    g = np.arange(k, dtype=f32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def box_cloud(n_boxes, seed):
    """the 9 P points get_tetra_points makes of P Gaussians (tests/tetmesh_restatement.py): float32 box corners, exactly degenerate"""
    rng = np.random.default_rng(seed)
    xyz = rng.random((n_boxes, 3)).astype(f32)
    scales = (0.02 + 0.05 * rng.random((n_boxes, 3))).astype(f32)
    rot = rng.normal(size=(n_boxes, 4)).astype(f32)
    return tr.tetra_points(xyz, scales, rot)[0]


CASES = {                                                  # name: (points, jitter)
    "random4": (random_points(4, 4), 0.0), "random5": (random_points(5, 5), 0.0), "random8": (random_points(8, 8), 0.0),
    "random64": (random_points(64, 64), 0.0), "random65": (random_points(65, 65), 0.0), "random200": (random_points(200, 200), 0.0),
    "random1000": (random_points(1000, 1000), 0.0),
    "sphere120": (sphere(120, 1), 0.0), "shell151": (shell_and_centre(150, 2), 0.0), "clusters120": (two_clusters(120, 3), 0.0),
    "grid64": (grid(4), 1e-9), "boxes270": (box_cloud(30, 5), 1e-9),
}
SEED = 0


def make(name, points, jitter):
    X = dr.perturbed(points, jitter, SEED)
    tri = Delaunay(X)
    assert tri.coplanar.size == 0, (name, "scipy reports coplanar points")
    cells = np.unique(np.sort(tri.simplices, axis=1), axis=0).astype(np.int32)
    got, found = dr.triangulate(X)
    assert (found == 4).all(), (name, "a tetrahedron was not found four times")
    assert np.array_equal(np.sort(got, axis=1), cells), (name, "the restatement differs from scipy")
    hull = float(ConvexHull(X).volume)
    assert abs(dr.volume(X, cells) - hull) <= 1e-9 * hull, name
    np.savez_compressed(os.path.join(HERE, f"delaunay_{name}.npz"), points=points, jitter=np.float64(jitter), seed=np.int64(SEED), perturbed=X,
                        cells=cells, hull_volume=np.float64(hull))
    print(name, points.shape[0], "points", cells.shape[0], "tetrahedra")


if __name__ == "__main__":
    for name, (points, jitter) in CASES.items():
        make(name, points, jitter)
