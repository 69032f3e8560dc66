"""CPU tier of mesh extraction: tests/tetmesh_restatement.py -- the specification of include/radegs.h's "Mesh extraction"
block in numpy -- against the fixtures the reference's own code wrote (tests/golden/make_golden_tetmesh.py).  Everything is exact but
get_tetra_points' computed coordinates: the reference forms them with a batched matrix product whose accumulation (fused or not, and
in which order) is the BLAS library's, so they are held to the project's bar for computed floats, 1e-5 abs / 1e-4 rel."""
import os

import numpy as np
import pytest

import tetmesh_restatement as tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARCH_KEYS = ("end_points", "end_sdf", "end_scales", "faces", "interp_v")


def load(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def check_marching(out, fx, prefix=""):
    """out: (end_points, end_sdf, end_scales, faces, interp_v) as numpy arrays; exact, shapes and dtypes of the integer outputs included"""
    for got, key in zip(out, MARCH_KEYS):
        want = fx[prefix + key]
        assert got.shape == want.shape, (key, got.shape, want.shape)
        assert np.array_equal(got, want), key
    assert out[3].dtype == np.int64 and out[4].dtype == np.int64


def within_bar(a, b):
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= 1e-5 + 1e-4 * np.abs(b.astype(np.float64))).all())


def test_marching_delaunay_fixture():
    fx = load("tetmesh_delaunay.npz")
    assert fx["points"].shape == (2700, 3) and fx["cells"].dtype == np.int32 and int(fx["crossing_instances"]) > 2048
    assert int((fx["sdf"] == 0).sum()) == 5
    check_marching(tr.marching(fx["points"], fx["cells"], fx["sdf"], fx["points_scale"]), fx)


def test_marching_small_fixture_with_repeated_corners():
    fx = load("tetmesh_small.npz")
    assert (np.sort(fx["tets"], axis=1)[:, 1:] == np.sort(fx["tets"], axis=1)[:, :-1]).any()
    check_marching(tr.marching(fx["vertices"], fx["tets"], fx["sdf"], fx["scales"]), fx)


def test_marching_all_outside_is_empty():
    fx = load("tetmesh_small.npz")
    assert (fx["sdf_outside"] < 0).all()
    check_marching(tr.marching(fx["vertices"], fx["tets"], fx["sdf_outside"], fx["scales"]), fx, "empty_")


def test_tetra_points_fixture():
    fx = load("tetmesh_delaunay.npz")
    pts, sc = tr.tetra_points(fx["xyz"], fx["scales3"], fx["rotation"])
    assert pts.shape == fx["points"].shape and sc.shape == fx["points_scale"].shape
    assert np.array_equal(sc, fx["points_scale"])
    assert np.array_equal(pts[2400:], fx["points"][2400:])          # the centres are copies
    assert within_bar(pts, fx["points"]), float(np.abs(pts - fx["points"]).max())


@pytest.mark.parametrize("tag", ["", "x_"], ids=["view_masks", "extra_masks"])
def test_cull_alpha_fixture(tag):
    fx = load("tetmesh_cull.npz")
    PN = fx["alpha0"].shape[0]
    final, weight = np.ones(PN, np.float32), np.zeros(PN, np.int32)
    for v in range(2):
        W, H = fx[f"size{v}"]
        assert fx[f"mask{v}"].shape == (H, W)
        c = fx[f"coord{v}"]
        assert 0.1 < ((c[:, 0] < -0.5) | (c[:, 0] > W - 0.5) | (c[:, 1] < -0.5) | (c[:, 1] > H - 0.5)).mean() < 0.3
        final, weight = tr.cull_alpha_accumulate(final, weight, fx[f"alpha{v}"], c, fx[f"mask{v}"], fx.get(f"gt{v}"), fx[f"extra{v}"] if tag else None)
        assert np.array_equal(final, fx[f"{tag}final_sdf{v}"]) and np.array_equal(weight, fx[f"{tag}weight{v}"]), v
    assert "gt0" in fx and "gt1" not in fx
    sdf = tr.cull_alpha_finish(final, weight)
    assert np.array_equal(sdf, fx[f"{tag}sdf"])
    assert (sdf == -100).any() and (weight == 2).any()


def test_bisection_and_filter_fixture():
    a, fx = load("tetmesh_delaunay.npz"), load("tetmesh_bisect.npz")
    l, r = a["end_points"][:, 0].copy(), a["end_points"][:, 1].copy()
    ls, rs = a["end_sdf"][:, 0, 0].copy(), a["end_sdf"][:, 1, 0].copy()
    zeros = 0
    for k in range(8):
        zeros += int((fx[f"mid_sdf{k}"] == 0).sum())
        l, r, ls, rs, mid = tr.bisect(l, r, ls, rs, fx[f"mid_sdf{k}"])
        assert np.array_equal(l, fx[f"end_points{k}"][:, 0]) and np.array_equal(r, fx[f"end_points{k}"][:, 1]), k
        assert np.array_equal(ls, fx[f"end_sdf{k}"][:, 0, 0]) and np.array_equal(rs, fx[f"end_sdf{k}"][:, 1, 0]), k
    assert zeros >= 8
    assert np.array_equal(mid, fx["final_points"])
    assert np.array_equal(tr.keep_vertices(a["end_points"], fx["end_scales"]), fx["vertex_mask"])
    v, f = tr.filter_mesh(a["end_points"], fx["end_scales"], mid, a["faces"])
    assert np.array_equal(v, fx["out_vertices"]) and np.array_equal(f, fx["out_faces"]) and f.dtype == np.int64
    assert 0 < v.shape[0] < mid.shape[0] and 0 < f.shape[0] < a["faces"].shape[0]


def test_driver_on_an_analytic_sphere():
    """the restated driver: the bracket halves eight times and the vertex is its midpoint, so it lies within len * 2^-9 of the zero of
    R - |p| along its edge, and |v| is 1-Lipschitz along the edge: | |v| - R | <= len * 2^-8 with room, + 1e-6 for the float32 arithmetic"""
    a = load("tetmesh_delaunay.npz")
    R = np.float32(1.0)
    sphere = lambda p: (R - np.sqrt((p.astype(np.float32) ** 2).sum(1))).astype(np.float32)   # noqa: E731
    v, f = tr.driver(a["points"], a["points_scale"], a["cells"], sphere)
    ep, _, esc, faces, _ = tr.marching(a["points"], a["cells"], sphere(a["points"]), a["points_scale"])
    keep = tr.keep_vertices(ep, esc)
    length = np.linalg.norm(ep[keep, 0].astype(np.float64) - ep[keep, 1], axis=1)
    assert v.shape[0] == keep.sum() > 100 and f.shape[0] > 100 and f.max() < v.shape[0] and f.min() >= 0
    assert (np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0) <= length * 2.0 ** -8 + 1e-6).all()
