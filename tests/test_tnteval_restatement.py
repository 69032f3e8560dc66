"""CPU tier of the Tanks-and-Temples evaluation: tests/tnteval_restatement.py equals what the reference's own NumPy code
wrote (tests/golden/tnteval_fscore.npz: evaluation.get_f1_score_histo2 and run.py's vertex-plus-centroid cloud, exactly), reproduces the
pipeline run recorded in tests/golden/tnteval_pipeline.npz, and has the properties that do not depend on it: the crop rule against a
winding-number test, the voxel means against a dictionary, umeyama against a known similarity."""
import os

import numpy as np
import pytest

import tnteval_restatement as tr

HERE = os.path.dirname(os.path.abspath(__file__))
REG_TAGS = ("r2", "r3", "r")


def load(name):
    with np.load(os.path.join(HERE, "golden", name)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def fscore_fx():
    return load("tnteval_fscore.npz")


@pytest.fixture(scope="module")
def pipeline_fx():
    return load("tnteval_pipeline.npz")


def pipeline_inputs(fx):
    """the fixture's inputs as the evaluation saw them: float64 arrays of float32 values"""
    return dict(vertices=fx["vertices"].astype(np.float64), faces=fx["faces"].astype(np.int64), gt=fx["gt"].astype(np.float64), init=fx["init"],
                volume=tr.volume_of(fx), tau=float(fx["tau"]))


_RUN = {}


def pipeline_run(fx):
    """the restatement's full run on the fixture, computed once per process and shared (the GPU tier starts every stage from it)"""
    if "out" not in _RUN:
        a = pipeline_inputs(fx)
        _RUN["out"] = tr.evaluate(a["vertices"], a["faces"], a["gt"], a["init"], a["volume"], a["tau"])
    return _RUN["out"]


def unpack(bits, n):
    return np.unpackbits(bits)[:n].astype(bool)


def check_scores(got, fx):
    """the seven values of precision_recall against the fixture the reference wrote: exact counts, scores at 1e-15"""
    for k, name in enumerate(("precision", "recall", "fscore")):
        assert abs(float(got[k]) - float(fx[name])) <= 1e-15 * abs(float(fx[name])), name
    for k, name in ((3, "edges_source"), (4, "cum_source"), (5, "edges_target"), (6, "cum_target")):
        assert np.array_equal(np.asarray(got[k]), fx[name]), name


# -------------------------------------------------------------------- against the reference's code --------------------------------------------------------------------
def test_restated_scores_equal_the_reference_run(fscore_fx):
    fx = fscore_fx
    got = tr.precision_recall(fx["dist1"], fx["dist2"], float(fx["tau"]), int(fx["plot_stretch"]))
    check_scores(got, fx)
    assert got[0] == float(fx["precision"]) and got[1] == float(fx["recall"]) and got[2] == float(fx["fscore"])       # the same operations
    n1, n2 = len(fx["dist1"]), len(fx["dist2"])
    assert np.array_equal(np.rint(got[4] * n1), np.cumsum(tr.histogram(fx["dist1"], got[3]))) and got[4][-1] < 1     # some lie beyond the last edge
    assert np.isinf(fx["dist2"]).sum() > 10 and got[6][-1] <= 1 - np.isinf(fx["dist2"]).sum() / n2
    empty = tr.precision_recall(fx["dist1"], np.zeros(0), float(fx["tau"]))
    assert [float(np.asarray(e).reshape(-1)[0]) for e in empty] == list(fx["empty"]) and [np.asarray(e).size for e in empty] == list(fx["empty_sizes"])


def test_restated_histogram_is_numpys(fscore_fx):
    edges = fscore_fx["edges_source"]
    d = np.concatenate([fscore_fx["dist1"], edges, [edges[-1], np.nextafter(edges[-1], 1), np.inf, -1e-9, 0.0]])
    assert np.array_equal(tr.histogram(d, edges), np.histogram(d[np.isfinite(d)], edges)[0])


def test_restated_mesh_cloud_equals_the_reference_expression(fscore_fx):
    fx = fscore_fx
    got = tr.mesh_points(fx["mesh_vertices"], fx["mesh_faces"])
    assert got.shape == (fx["mesh_vertices"].shape[0] + fx["mesh_faces"].shape[0], 3) and np.array_equal(got, fx["mesh_cloud"])


# ------------------------------------------------------------------------------ the recorded run ------------------------------------------------------------------------------
def test_fixture_has_the_cases_the_issue_names(pipeline_fx):
    fx = pipeline_fx
    assert 2800 < fx["vertices"].shape[0] < 3200 and fx["gt"].shape[0] == 8000 and fx["bounding_polygon"].shape == (5, 3)
    assert fx["vertices"].nbytes + fx["gt"].nbytes < 200_000
    n = fx["vertices"].shape[0] + fx["faces"].shape[0]
    for tag in REG_TAGS:
        s_keep, t_keep = unpack(fx[tag + "_s_keep"], n), unpack(fx[tag + "_t_keep"], 8000)
        assert 0 < s_keep.sum() < n and 0 < t_keep.sum() < 8000                          # the polygon cuts both clouds
        assert fx[tag + "_count"].shape[0] == int(fx[tag + "_iterations"]) + 1
    A, K = fx["init"][:3, :3], fx["known"][:3, :3]
    scale = np.cbrt(np.linalg.det(A) / np.linalg.det(K))
    angle = np.degrees(np.arccos(np.clip((np.trace(A @ np.linalg.inv(K)) / scale - 1) / 2, -1, 1)))
    assert 1.5 < angle < 2.5 and 1.005 < scale < 1.015
    cut = fx["edges"][-1]
    assert (fx["dist2"] > cut).sum() > 10 and (fx["s_counts"] > 1).any()
    assert float(fx["recovery_error"]) < np.abs(fx["init"] - fx["known"]).max() / 3
    u, v = fx["bounding_polygon"][:, 0], fx["bounding_polygon"][:, 2]                    # concave: the turns of its corners differ in sign
    turn = [(u[(i + 1) % 5] - u[i]) * (v[(i + 2) % 5] - v[(i + 1) % 5]) - (v[(i + 1) % 5] - v[i]) * (u[(i + 2) % 5] - u[(i + 1) % 5]) for i in range(5)]
    assert min(turn) < 0 < max(turn)


def test_restatement_reproduces_the_recorded_run(pipeline_fx):
    fx, out = pipeline_fx, pipeline_run(pipeline_fx)
    for tag in REG_TAGS:
        r = out[tag]
        assert r["iterations"] == int(fx[tag + "_iterations"]) and np.array_equal([h["count"] for h in r["history"]], fx[tag + "_count"]), tag
        assert np.array_equal(np.packbits(r["s_keep"]), fx[tag + "_s_keep"]) and np.array_equal(np.packbits(r["t_keep"]), fx[tag + "_t_keep"]), tag
        assert np.allclose(r["transformation"], fx[tag + "_transformation"], rtol=1e-9, atol=1e-12), tag
        assert np.allclose([h["inlier_rmse"] for h in r["history"]], fx[tag + "_rmse"], rtol=1e-9, atol=0), tag
    assert np.array_equal(out["idx1"], fx["idx1"]) and np.array_equal(out["idx2"], fx["idx2"])
    assert np.allclose(out["dist1"], fx["dist1"], rtol=1e-12, atol=0) and np.allclose(out["dist2"], fx["dist2"], rtol=1e-12, atol=0)
    assert np.array_equal(out["s_counts"], fx["s_counts"]) and np.array_equal(out["t_counts"], fx["t_counts"])
    for key in ("precision", "recall", "fscore"):
        assert abs(out[key] - float(fx[key])) <= 1e-12 * float(fx[key]), key
    assert np.array_equal(out["cum_source"], fx["cum_source"]) and np.array_equal(out["cum_target"], fx["cum_target"])
    assert abs(np.abs(out["transformation"] - fx["known"]).max() - float(fx["recovery_error"])) < 1e-9


# ------------------------------------------------------------------------ properties of the restatement ------------------------------------------------------------------------
def _winding_inside(pu, pv, poly):
    """non-zero winding number by summed signed angles: for a simple polygon the same set as even-odd"""
    total = np.zeros(pu.shape[0])
    n = poly.shape[0]
    for i in range(n):
        a, b = poly[i], poly[(i + 1) % n]
        ax, ay, bx, by = a[0] - pu, a[1] - pv, b[0] - pu, b[1] - pv
        total += np.arctan2(ax * by - ay * bx, ax * bx + ay * by)
    return np.abs(total) > np.pi


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_crop_rule_is_point_in_polygon(axis):
    rng = np.random.default_rng(5)
    u, v, w = tr.axes_of(axis)
    flat = np.array([[0.1, 0.2], [2.0, 0.0], [2.2, 1.9], [1.0, 0.8], [0.0, 2.1]])        # concave
    poly = np.zeros((5, 3))
    poly[:, u], poly[:, v] = flat[:, 0], flat[:, 1]
    vol = dict(orthogonal_axis=axis, axis_min=-0.5, axis_max=0.75, bounding_polygon=poly)
    p = rng.uniform(-0.5, 2.7, (4000, 3))
    p[:, w] = rng.uniform(-1.0, 1.2, 4000)
    p[0, w], p[1, w] = -0.5, 0.75                                                          # on the two bounds: kept when inside the polygon
    p[:2, u], p[:2, v] = 1.0, 0.5
    keep = tr.crop_mask(p, vol)
    want = _winding_inside(p[:, u], p[:, v], flat) & (p[:, w] >= -0.5) & (p[:, w] <= 0.75)
    assert np.array_equal(keep, want) and keep[0] and keep[1] and 0.1 < keep.mean() < 0.6


def test_crop_margin_is_raised():
    poly = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    vol = dict(orthogonal_axis="Z", axis_min=0.0, axis_max=1.0, bounding_polygon=poly)
    with pytest.raises(tr.Margin):
        tr.crop_mask(np.array([[0.5, 0.5 + 1e-12, 0.5]]), vol)                             # on the hypotenuse
    with pytest.raises(tr.Margin):
        tr.crop_mask(np.array([[0.2, 0.2, 1.0 + 1e-12]]), vol)
    assert tr.crop_mask(np.array([[0.2, 0.2, 1.0]]), vol)[0]


def test_voxel_means_against_a_dictionary():
    rng = np.random.default_rng(6)
    voxel = 0.25
    p = tr.redraw(rng.uniform(-3, 3, (3000, 3)), lambda q: tr.voxel_bad(q, voxel), lambda n: rng.uniform(-3, 3, (n, 3)))
    means, counts, index = tr.voxel_down_sample(p, voxel)
    cells = {}
    for q in p:
        cells.setdefault(tuple(np.floor((q - (p.min(0) - 0.5 * voxel)) / voxel).astype(int)), []).append(q)
    keys = sorted(cells)
    assert [tuple(i) for i in index] == keys and counts.sum() == 3000 and counts.dtype == np.int32
    for k, key in enumerate(keys):
        s = np.zeros(3)
        for q in cells[key]:
            s = s + q
        assert np.array_equal(means[k], s / len(cells[key]))
    with pytest.raises(tr.Margin):
        tr.voxel_down_sample(np.array([[0.0, 0.0, 0.0], [0.125 + 1e-9, 0.3, 0.3]]), voxel)


def test_umeyama_recovers_a_similarity_and_refuses_degenerate_input():
    rng = np.random.default_rng(7)
    s = rng.standard_normal((50, 3))
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = 1.3 * q, [0.5, -2.0, 4.0]
    assert np.allclose(tr.umeyama(s, tr.transform(s, T)), T, rtol=0, atol=1e-12)
    assert np.array_equal(tr.umeyama(s[:2], s[:2] + 1.0), np.eye(4)) and np.array_equal(tr.umeyama(np.ones((5, 3)), s[:5]), np.eye(4))
    flat = s.copy()
    flat[:, 2] = 0.0                                                                       # coplanar: the reflection case of S must not appear
    got = tr.umeyama(flat, tr.transform(flat, T))
    assert np.linalg.det(got[:3, :3]) > 0 and np.allclose(tr.transform(flat, got), tr.transform(flat, T), atol=1e-12)


def test_icp_stopping_rule():
    rng = np.random.default_rng(8)
    t = rng.uniform(0, 1, (400, 3))
    same = tr.icp(t, t, 0.05)
    assert same["iterations"] == 1 and same["fitness"] == 1.0 and same["inlier_rmse"] < 1e-12 and len(same["history"]) == 2
    none = tr.icp(t + 10.0, t, 0.05)
    assert none["iterations"] == 1 and none["fitness"] == 0.0 and np.array_equal(none["transformation"], np.eye(4)) and (none["correspondence"] == -1).all()
    assert tr.icp(t, t, 0.05, max_iter=0)["iterations"] == 0
