"""CPU tier of mesh evaluation: tests/mesheval_restatement.py equals the fixtures the reference's own code wrote
(tests/golden/make_golden_mesheval.py: dtu_eval/eval.py run under runpy, evaluate_dtu_mesh.cull_mesh called).  Exact: counts, point order,
masks, indices.  Sampled coordinates and distances: 1e-12 relative (the same few fp64 operations on both sides; the slack is for a square
root or a BLAS product rounded differently).  The three means: 1e-9 relative."""
import math
import os

import numpy as np
import pytest

import mesheval_restatement as mr

HERE = os.path.dirname(os.path.abspath(__file__))


def load(name):
    with np.load(os.path.join(HERE, "golden", name)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def chamfer_fx():
    return load("mesheval_chamfer.npz")


@pytest.fixture(scope="module")
def cull_fx():
    return load("mesheval_cull.npz")


def chamfer_inputs(fx):
    """the fixture's inputs as eval.py saw them: float64 arrays of float32 values, the permutation, the three thresholds"""
    return dict(vertices=fx["vertices"].astype(np.float64), faces=fx["faces"].astype(np.int64), stl=fx["stl"].astype(np.float64),
                obs_mask=fx["obs_mask"], BB=fx["BB"], Res=float(fx["Res"]), plane=fx["plane"], perm=fx["perm"].astype(np.int64),
                density=float(fx["density"]), patch=float(fx["patch"]), max_dist=float(fx["max_dist"]))


def close(a, b, rtol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    both_inf = np.isinf(a) & np.isinf(b)
    with np.errstate(invalid="ignore"):
        return bool((both_inf | (np.abs(a - b) <= rtol * np.abs(b))).all())


def check_chamfer(got, fx):
    """every stage of a chamfer run (numpy values under the restatement's keys) against the fixture"""
    assert np.array_equal(got["counts"], fx["counts"])
    assert got["data_pcd"].shape == fx["data_pcd"].shape and close(got["data_pcd"], fx["data_pcd"], 1e-12)
    for key in ("keep", "inbound", "grid_inbound", "in_obs", "above"):
        assert got[key].dtype == bool and np.array_equal(got[key], fx[key]), key
    for tag in ("d2s", "s2d"):
        assert np.array_equal(got["idx_" + tag], fx["idx_" + tag].astype(np.int64)), tag
        assert close(got["dist_" + tag], fx["dist_" + tag], 1e-12), tag
    for key in ("mean_d2s", "mean_s2d", "overall"):
        assert math.isclose(float(got[key]), float(fx[key]), rel_tol=1e-9), key


def cull_cameras(fx, dilated=False):
    """[(w2c float32 [4,4], fx, fy, W, H, mask uint8 [H,W])] -- the focal lengths by the reference's fov2focal"""
    cams = []
    for i in range(int(fx["ncam"])):
        W, H = (int(v) for v in fx[f"size{i}"])
        fovx, fovy = (float(v) for v in fx[f"fov{i}"])
        cams.append((fx[f"w2c{i}"], W / (2 * math.tan(fovx / 2)), H / (2 * math.tan(fovy / 2)), W, H, fx[f"dilated{i}" if dilated else f"mask{i}"]))
    return cams


def projection_rows(cam):
    """rows 0-2 of K w2c in float32, K as evaluate_dtu_mesh.py:100-104 fills it"""
    w2c, fx, fy, W, H, _ = cam
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, W / 2.0, H / 2.0
    return (K @ np.asarray(w2c, np.float32))[:3]


def test_fixture_has_the_cases_the_issue_names(chamfer_fx):
    fx = chamfer_fx
    assert 550 < fx["faces"].shape[0] < 650 and 9000 < fx["data_pcd"].shape[0] < 11000 and 7000 < fx["stl"].shape[0] < 9000
    assert int(fx["rounds"]) >= 4
    assert (fx["counts"] == 0).sum() >= 5                                   # the zero-area triangle and those smaller than thr
    assert np.isinf(fx["dist_s2d"]).sum() > 100 and (fx["idx_s2d"] == -1).sum() == np.isinf(fx["dist_s2d"]).sum()
    assert 0 < fx["in_obs"].sum() < fx["grid_inbound"].sum() < fx["inbound"].sum() < fx["inbound"].shape[0]
    assert 0 < fx["above"].sum() < fx["above"].shape[0]


def test_restated_chamfer_equals_the_reference_run(chamfer_fx):
    a = chamfer_inputs(chamfer_fx)
    got = mr.chamfer(a["vertices"], a["faces"], a["stl"], a["obs_mask"], a["BB"], a["Res"], a["plane"], a["perm"], a["density"], a["patch"], a["max_dist"])
    check_chamfer(got, chamfer_fx)


def test_round_based_thinning_is_the_sequential_loop(chamfer_fx):
    a = chamfer_inputs(chamfer_fx)
    shuffled = chamfer_fx["data_pcd"][a["perm"]]
    keep, rounds = mr.thin_rounds(shuffled, a["density"])
    assert np.array_equal(keep, chamfer_fx["keep"]) and rounds == int(chamfer_fx["rounds"])
    line = np.stack([np.arange(40) * 0.6, np.zeros(40), np.zeros(40)], 1)   # a chain: point i waits for point i - 1
    keep, rounds = mr.thin_rounds(line, 1.0)
    assert rounds == 40 and np.array_equal(keep, mr.thin(line, 1.0)) and np.array_equal(keep, np.arange(40) % 2 == 0)


def test_restated_dilation_and_cull_equal_the_reference_run(cull_fx):
    fx = cull_fx
    cams = cull_cameras(fx)
    for i, cam in enumerate(cams):
        assert np.array_equal(mr.dilate(cam[5], 6), fx[f"dilated{i}"]), i
    keep = mr.cull_vertex_mask(fx["vertices"], [(projection_rows(c), c[3], c[4], c[5]) for c in cams], 6)
    assert np.array_equal(keep, fx["vertex_mask"])
    v, f, fmask = mr.apply_vertex_mask(fx["vertices"], fx["faces"].astype(np.int64), keep)
    assert np.array_equal(fmask, fx["face_mask"]) and np.array_equal(v, fx["out_vertices"]) and np.array_equal(f, fx["out_faces"])
    assert 0 < keep.sum() < keep.shape[0]
