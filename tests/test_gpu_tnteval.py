"""GPU tier of the Tanks-and-Temples evaluation: tnt_eval.py and the kernels of csrc/radegs_tnteval.hip against the fixtures
(tests/golden/make_golden_tnteval.py) and against tests/tnteval_restatement.py at the sizes and edge cases the fixtures do not reach.
Exact: masks, voxel counts and order, neighbour indices, per-iteration correspondence counts, histogram counts.  Bit-equal: transformed
points, centroids, voxel means (the same fp64 operations in the same order).  Distances and clouds: 1e-12 relative.  What passes through a
sum over the pairs and an SVD (fitness aside: it is a count) -- rmse, transformations: 1e-9 relative.  Scores: 1e-12 (1e-15 against the
reference-written fixture, where the counts are the same integers)."""
import math

import numpy as np
import pytest
import torch

import tnteval_restatement as tr
from test_tnteval_restatement import REG_TAGS, check_scores, load, pipeline_inputs, pipeline_run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONCAVE = np.array([[0.1, 0.2], [2.0, 0.0], [2.2, 1.9], [1.0, 0.8], [0.0, 2.1]])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def close(a, b, rtol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    both_inf = np.isinf(a) & np.isinf(b)
    with np.errstate(invalid="ignore"):
        return bool((both_inf | (np.abs(a - b) <= rtol * np.abs(b))).all())


def volume(v):
    import tnt_eval as te
    return te.CropVolume(v["orthogonal_axis"], v["axis_min"], v["axis_max"], v["bounding_polygon"])


@pytest.fixture(scope="module")
def fscore_fx():
    return load("tnteval_fscore.npz")


@pytest.fixture(scope="module")
def pipeline_fx():
    return load("tnteval_pipeline.npz")


@pytest.fixture(scope="module")
def run(pipeline_fx):
    """the restatement's run on the pipeline fixture (checked against the fixture's records in the CPU tier): every stage's intermediates"""
    return pipeline_run(pipeline_fx)


# ------------------------------------------------------------------------- cloud of a mesh -------------------------------------------------------------------------
def test_mesh_points_equal_the_reference_expression(fscore_fx):
    import tnt_eval as te
    fx = fscore_fx
    got = te.mesh_points(dev(fx["mesh_vertices"]), dev(fx["mesh_faces"]))
    assert got.dtype == torch.float64 and np.array_equal(host(got), fx["mesh_cloud"])
    v = dev(fx["mesh_vertices"])
    assert np.array_equal(host(te.mesh_points(v, torch.zeros((0, 3), dtype=torch.int64, device=DEV))), fx["mesh_vertices"])
    with pytest.raises(RuntimeError, match="outside the"):
        te.mesh_points(v, dev(np.array([[0, 1, 30]])))


# ------------------------------------------------------------------------------- crop -------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_crop_mask_is_the_restatements(axis):
    import tnt_eval as te
    rng = np.random.default_rng(20 + ord(axis))
    u, v, w = tr.axes_of(axis)
    poly = np.zeros((5, 3))
    poly[:, u], poly[:, v], poly[:, w] = CONCAVE[:, 0], CONCAVE[:, 1], 7.0                 # the polygon's own w is not used
    vol = dict(orthogonal_axis=axis, axis_min=-0.5, axis_max=0.75, bounding_polygon=poly)
    T = np.eye(4)
    T[:3, :3] = 1.1 * np.array([[0.96, -0.28, 0.0], [0.28, 0.96, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = [0.15, -0.2, 0.05]

    def draw(n):
        p = rng.uniform(-0.5, 2.7, (n, 3))
        p[:, w] = rng.uniform(-1.0, 1.2, n)
        return p
    for N in (0, 1, 63, 64, 65, 70001):
        for moved in (None, T):
            p = tr.redraw(draw(N), lambda q: tr.crop_bad(q if moved is None else tr.transform(q, moved), vol), draw)
            if moved is None and N:                                                        # on the two bounds, inside the polygon: kept
                p[0, u], p[0, v], p[0, w] = 1.0, 0.5, -0.5
                p[N // 2, u], p[N // 2, v], p[N // 2, w] = 1.0, 0.5, 0.75
            want_points, want = tr.crop(p, vol, moved)
            kept, keep = te.crop_points(dev(p), volume(vol), moved)
            assert keep.dtype == torch.bool and keep.shape == (N,) and np.array_equal(host(keep), want), (N, moved is not None)
            assert np.array_equal(host(kept), want_points)                                 # the transform is the same three products and sums
            if moved is None and N:
                assert want[0] and want[N // 2]
            if N == 70001:
                assert 0.1 < want.mean() < 0.5


# ------------------------------------------------------------------------------ voxels ------------------------------------------------------------------------------
def check_voxels(p, voxel):
    import tnt_eval as te
    means, counts = te.voxel_down_sample(dev(p), voxel)
    want_means, want_counts, _ = tr.voxel_down_sample(p, voxel)
    assert means.dtype == torch.float64 and counts.dtype == torch.int32 and means.shape == (want_counts.shape[0], 3)
    assert np.array_equal(host(counts), want_counts)
    assert np.array_equal(host(means), want_means)                                         # bit-equal: the same additions in the same order
    return want_counts


def test_voxel_down_sample_sizes_and_negative_coordinates():
    rng = np.random.default_rng(31)
    import tnt_eval as te
    means, counts = te.voxel_down_sample(torch.zeros((0, 3), dtype=torch.float64, device=DEV), 0.1)
    assert means.shape == (0, 3) and counts.shape == (0,) and counts.dtype == torch.int32
    assert np.array_equal(check_voxels(np.array([[-3.25, 0.5, 11.0]]), 0.1), [1])
    voxel = 0.2
    draw = lambda n: rng.uniform(-2.0, 2.0, (n, 3)) * [1.0, 0.5, 0.25] - [0.0, 5.0, 0.0]
    p = tr.redraw(draw(70001), lambda q: tr.voxel_bad(q, voxel), draw)
    counts = check_voxels(p, voxel)
    assert counts.sum() == 70001 and counts.max() > 20 and counts.shape[0] > 500


def test_voxel_down_sample_one_voxel_and_distant_clusters():
    rng = np.random.default_rng(32)
    voxel = 0.5
    p = np.array([7.0, -3.0, 0.25]) + rng.uniform(0.0, 0.2, (1000, 3))                      # a span of 0.4 voxel: one cell
    assert np.array_equal(check_voxels(p, voxel), [1000])
    voxel = 1e-3
    a = rng.uniform(0.0, 0.004, (300, 3))
    far = a + np.array([2 ** 20 * voxel, 0.0, 0.0])
    draw = lambda n: rng.uniform(0.0, 0.004, (n, 3))
    p = np.concatenate([a, far])[rng.permutation(600)]
    p = tr.redraw(p, lambda q: tr.voxel_bad(q, voxel), lambda n: draw(n) + np.array([2 ** 20 * voxel, 0.0, 0.0]) * rng.integers(0, 2, (n, 1)))
    counts = check_voxels(p, voxel)
    assert counts.sum() == 600 and np.ptp(p[:, 0]) / voxel > 2 ** 20


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_voxel_down_sample_refuses_more_than_2_21_cells(axis):
    import tnt_eval as te
    p = np.zeros((3, 3))
    p[2, axis] = (2 ** 21 + 3) * 0.01
    with pytest.raises(RuntimeError, match=r"2\^21"):
        te.voxel_down_sample(dev(p), 0.01)
    p[2, axis] = (2 ** 21 - 3) * 0.01
    assert te.voxel_down_sample(dev(p), 0.01)[0].shape == (2, 3)


# -------------------------------------------------------------------------------- ICP --------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 257, 262145])
def test_pair_sums_equal_the_fixed_order_restatement_bit_for_bit(Q):
    """One block, two blocks, and the first size with a second stride (1024 blocks of 256 threads, one query more); about one index in twenty
    is -1 or past the target and adds nothing.  All 18 outputs with ==: the sums are the same additions in the same order."""
    import tnt_eval as te
    from diff_gaussian_rasterization import _C
    rng = np.random.default_rng(100 + Q)
    NT = 1000
    target = rng.normal(0.0, 3.0, (NT, 3)) + [40.0, -25.0, 7.0]
    index = rng.integers(0, NT, Q)
    skipped = rng.random(Q) < 0.05
    index[skipped] = np.where(rng.random(Q) < 0.5, -1, NT + rng.integers(0, 5, Q))[skipped]
    if Q == 1:
        index[0] = 3
    moved = target[np.clip(index, 0, NT - 1)] + rng.normal(0.0, 0.05, (Q, 3))
    want = tr.pair_sums(moved, target, index)
    assert want[0] == np.count_nonzero((index >= 0) & (index < NT)) > 0
    L = te._lib()
    nbytes = L.radegs_tnteval_sums_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.full((18,), float("nan"), dtype=torch.float64, device=DEV)
    m, t, i = dev(moved), dev(target), dev(index)
    rc = L.radegs_tnteval_pair_sums(Q, m.data_ptr(), NT, t.data_ptr(), i.data_ptr(), ws.data_ptr(), nbytes, out.data_ptr(), _C._stream(torch.device(DEV)))
    assert rc == 0
    got = host(out)
    assert np.array_equal(got, want), (np.flatnonzero(got != want), got, want)


def check_icp(got, want, init=None):
    assert got["iterations"] == want["iterations"] and len(got["history"]) == len(want["history"])
    assert [h["count"] for h in got["history"]] == [h["count"] for h in want["history"]]
    for g, w in zip(got["history"], want["history"]):
        assert g["fitness"] == w["fitness"] and math.isclose(g["inlier_rmse"], w["inlier_rmse"], rel_tol=1e-9)
    assert got["fitness"] == want["fitness"] and math.isclose(got["inlier_rmse"], want["inlier_rmse"], rel_tol=1e-9)
    T = got["transformation"] if init is None else got["transformation"] @ init
    assert np.array_equal(T[3], [0, 0, 0, 1]) and close(T[:3], want["transformation"][:3], 1e-9)
    assert np.array_equal(host(got["correspondence"]), want["correspondence"])


@pytest.mark.parametrize("tag", REG_TAGS)
def test_icp_on_the_pipeline_fixture(pipeline_fx, run, tag):
    import tnt_eval as te
    tau = float(pipeline_fx["tau"])
    max_dist = {"r2": 80 * tau, "r3": 20 * tau, "r": 2 * tau}[tag]
    init = {"r2": pipeline_fx["init"], "r3": pipeline_fx["r2_transformation"], "r": pipeline_fx["r3_transformation"]}[tag]
    want = run[tag]
    got = te.icp(dev(want["s"]), dev(want["t"]), max_dist, max_iter=20)
    assert [h["count"] for h in got["history"]] == list(pipeline_fx[tag + "_count"])       # the fixture's own record
    check_icp(got, want, init)


def test_icp_with_a_narrow_threshold_loses_and_gains_pairs(pipeline_fx, run):
    import tnt_eval as te
    tau = float(pipeline_fx["tau"])
    s, t = run["r2"]["s"], run["r2"]["t"]                                                   # still off by the initial error
    want = tr.icp(s, t, 1.5 * tau, max_iter=6)
    counts = [h["count"] for h in want["history"]]
    assert len(set(counts)) > 2 and 0 < min(counts) and max(counts) < s.shape[0]
    check_icp(te.icp(dev(s), dev(t), 1.5 * tau, max_iter=6), want)


def test_icp_is_independent_of_the_cell_and_repeatable(pipeline_fx, run):
    import tnt_eval as te
    tau = float(pipeline_fx["tau"])
    s, t = dev(run["r3"]["s"]), dev(run["r3"]["t"])
    a = te.icp(s, t, 20 * tau, max_iter=5)
    for other in (te.icp(s, t, 20 * tau, max_iter=5, cell=0.11), te.icp(s, t, 20 * tau, max_iter=5)):
        assert np.array_equal(a["transformation"], other["transformation"]) and a["history"] == other["history"]
        assert torch.equal(a["correspondence"], other["correspondence"])


def test_icp_without_correspondences_and_on_identical_clouds():
    import tnt_eval as te
    rng = np.random.default_rng(41)
    t = rng.uniform(0.0, 1.0, (700, 3))
    none = te.icp(dev(t + 10.0), dev(t), 0.05)
    assert np.array_equal(none["transformation"], np.eye(4)) and none["fitness"] == 0.0 and none["inlier_rmse"] == 0.0 and none["iterations"] == 1
    assert [h["count"] for h in none["history"]] == [0, 0] and bool((none["correspondence"] == -1).all())
    same = te.icp(dev(t), dev(t), 0.05)
    assert same["iterations"] == 1 and same["fitness"] == 1.0 and same["inlier_rmse"] < 1e-12
    assert np.abs(same["transformation"] - np.eye(4)).max() < 1e-12
    assert np.array_equal(host(same["correspondence"]), np.arange(700))
    empty = te.icp(torch.zeros((0, 3), dtype=torch.float64, device=DEV), dev(t), 0.05)
    assert empty["iterations"] == 0 and empty["fitness"] == 0.0


# ----------------------------------------------------------------------------- the scores -----------------------------------------------------------------------------
def test_precision_recall_equals_the_reference_run(fscore_fx):
    import tnt_eval as te
    fx = fscore_fx
    got = te.precision_recall(dev(fx["dist1"]), dev(fx["dist2"]), float(fx["tau"]), int(fx["plot_stretch"]))
    check_scores(got, fx)                                                                   # counts exact (the curves are count / N), scores 1e-15


def test_precision_recall_edge_cases(fscore_fx):
    import tnt_eval as te
    tau = 0.01
    edges = np.arange(0, tau * 5, tau / 100)
    empty = torch.zeros(0, dtype=torch.float64, device=DEV)
    d = dev(fscore_fx["dist1"])
    for a, b in ((d, empty), (empty, d), (empty, empty)):
        got = te.precision_recall(a, b, tau)
        assert [float(np.asarray(e).reshape(-1)[0]) for e in got] == list(fscore_fx["empty"])
        assert [np.asarray(e).size for e in got] == list(fscore_fx["empty_sizes"])
    cases = [np.array([0.4 * tau]), np.array([np.inf]),
             np.array([edges[-1], np.nextafter(edges[-1], 1), np.nextafter(edges[-1], 0), edges[-2], 0.0, edges[1], np.nextafter(edges[1], 0), 1.0, np.inf]),
             np.concatenate([edges, [np.inf] * 5, [tau, np.nextafter(tau, 0)]])]
    for d1 in cases:
        for d2 in cases:
            want = tr.precision_recall(d1, d2, tau, check=False)
            got = te.precision_recall(dev(d1), dev(d2), tau)
            for g, w_ in zip(got, want):
                assert np.array_equal(np.asarray(g), np.asarray(w_), equal_nan=True), (d1, d2)


def test_the_cut_changes_no_score(pipeline_fx, run):
    import tnt_eval as te
    tau = float(pipeline_fx["tau"])
    s, t = dev(run["s"]), dev(run["t"])
    cut = te.distance_cut(tau, 5)
    near = [te.cloud_distances(s, t, cut), te.cloud_distances(t, s, cut)]
    wide = [te.cloud_distances(s, t, 10 * cut), te.cloud_distances(t, s, 10 * cut)]
    assert sum(int(torch.isinf(d).sum()) for d, _ in near) > sum(int(torch.isinf(d).sum()) for d, _ in wide)      # the cut does bite
    for (dn, jn), (dw, jw) in zip(near, wide):
        kept = torch.isfinite(dn)
        assert torch.equal(dn[kept], dw[kept]) and torch.equal(jn[kept], jw[kept]) and bool((dw[~kept] >= cut).all())
    a = te.precision_recall(near[0][0], near[1][0], tau)
    b = te.precision_recall(wide[0][0], wide[1][0], tau)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


# ------------------------------------------------------------------------------ evaluate ------------------------------------------------------------------------------
def check_final(got, fx, want, same_transformation):
    """same_transformation: the clouds were moved by the fixture's own matrix, so a distance is the same few operations on the same numbers
    and holds 1e-12 of itself.  End to end the matrix is the GPU's own (1e-9, and in practice some 1e-15, from the fixture's): a distance is
    then a difference of coordinates that each hold 1e-12 of THEMSELVES, so it is held to 1e-12 of the coordinates' magnitude."""
    cut = fx["edges"][-1]
    for d_key, i_key in (("dist1", "idx1"), ("dist2", "idx2")):
        far = fx[d_key] > cut
        want_d, want_i = np.where(far, np.inf, fx[d_key]), np.where(far, -1, fx[i_key].astype(np.int64))
        assert np.array_equal(host(got[i_key]), want_i), i_key
        if same_transformation:
            assert close(host(got[d_key]), want_d, 1e-12), d_key
        else:
            got_d = host(got[d_key])
            assert np.array_equal(np.isinf(got_d), far) and np.abs(got_d[~far] - want_d[~far]).max() <= 1e-12 * np.abs(want["s"]).max(), d_key
    assert close(host(got["s"]), want["s"], 1e-12) and close(host(got["t"]), want["t"], 1e-12)
    for key in ("precision", "recall", "fscore"):
        assert math.isclose(got[key], float(fx[key]), rel_tol=1e-12), key
    assert np.array_equal(got["cum_source"], fx["cum_source"]) and np.array_equal(got["cum_target"], fx["cum_target"])
    assert np.array_equal(got["edges_source"], fx["edges"]) and np.array_equal(got["edges_target"], fx["edges"])


def test_evaluate_stage_by_stage(pipeline_fx, run):
    """every stage starts from the fixture's own intermediate, so that one stage's last-bit difference cannot hide in the next"""
    import tnt_eval as te
    fx, a = pipeline_fx, pipeline_inputs(pipeline_fx)
    tau, vol = a["tau"], volume(a["volume"])
    pcd = te.mesh_points(dev(a["vertices"]), dev(a["faces"]))
    assert np.array_equal(host(pcd), run["pcd"])
    gt = dev(a["gt"])
    inits = {"r2": fx["init"], "r3": fx["r2_transformation"], "r": fx["r3_transformation"]}
    for tag in REG_TAGS:
        want = run[tag]
        s_crop, s_keep = te.crop_points(pcd, vol, inits[tag])
        t_crop, t_keep = te.crop_points(gt, vol)
        assert np.array_equal(np.packbits(host(s_keep)), fx[tag + "_s_keep"]) and np.array_equal(np.packbits(host(t_keep)), fx[tag + "_t_keep"]), tag
        if tag == "r":
            assert close(host(s_crop), want["s"], 1e-12) and np.array_equal(host(t_crop), want["t"])
            continue
        voxel = tau if tag == "r2" else tau / 2.0
        for crop_, key in ((want["s_crop"], "s"), (want["t_crop"], "t")):
            means, counts = te.voxel_down_sample(dev(crop_), voxel)
            assert np.array_equal(host(counts), want[key + "_counts"]) and close(host(means), want[key], 1e-12), (tag, key)
    reg = te.registration_vol_ds(pcd, gt, fx["init"], vol, tau, tau * 80, 20)
    check_icp(reg, run["r2"])
    assert close(host(reg["s"]), run["r2"]["s"], 1e-12) and close(host(reg["t"]), run["r2"]["t"], 1e-12)
    reg = te.registration_unif(pcd, gt, fx["r3_transformation"], vol, 2 * tau, 20)
    check_icp(reg, run["r"])
    final = te.evaluate_histo(pcd, gt, fx["r_transformation"], vol, tau / 2.0, tau)
    check_final(final, fx, run, True)


def test_evaluate_end_to_end_and_recovery(pipeline_fx, run):
    import tnt_eval as te
    fx, a = pipeline_fx, pipeline_inputs(pipeline_fx)
    got = te.evaluate(dev(a["vertices"]), dev(a["faces"].astype(np.int32)), dev(a["gt"]), a["init"], volume(a["volume"]), a["tau"])
    for tag in REG_TAGS:
        check_icp(got[tag], run[tag])
        assert close(got[tag]["transformation"][:3], fx[tag + "_transformation"][:3], 1e-9), tag
        assert tuple(fx[tag + "_sizes"]) == (got[tag]["s"].shape[0], got[tag]["t"].shape[0]), tag
    assert np.array_equal(got["transformation"], got["r"]["transformation"])
    check_final(got, fx, run, False)
    # the known transformation is recovered as well as the restatement recovers it on the CPU (its own error is in the fixture)
    assert np.abs(got["transformation"] - fx["known"]).max() <= float(fx["recovery_error"]) + 1e-9
