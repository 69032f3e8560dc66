"""CPU tier of evaluation from files, part one: eval_io's host readers return what the reference's own code returned for the
committed input files (tests/golden/make_golden_evalio.py ran it), and tests/evalio_restatement.py -- the expectation of the GPU tier -- is
checked on its own: the RANSAC against the host-side tnt_eval.umeyama, by brute force, and on data with a known similarity; the PLY reader on
files in every layout the readers must take; merge_vertices against np.unique."""
import os

import numpy as np
import pytest

import evalio_restatement as er
import tnteval_restatement as tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return os.path.join(GOLDEN, name)


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(golden("evalio_reference.npz")))


# --------------------------------------------------------------------- the host readers ---------------------------------------------------------------------
def test_read_trajectory_returns_the_references_poses(ref):
    import eval_io
    poses, meta = eval_io.read_trajectory(golden("evalio_traj.log"))
    assert poses.dtype == np.float64 and np.array_equal(poses, ref["log_poses"])
    assert np.array_equal(np.array(meta), ref["log_meta"])


def test_read_mapping_and_sparse_trajectory_are_the_references(ref):
    import eval_io
    n_sampled, n_total, mapping = eval_io.read_mapping(golden("evalio_mapping.txt"))
    assert (n_sampled, n_total) == (int(ref["n_sampled"]), int(ref["n_total"])) and np.array_equal(mapping, ref["mapping"])
    poses, _ = eval_io.read_trajectory(golden("evalio_traj.log"))
    assert np.array_equal(eval_io.gen_sparse_trajectory(mapping, poses), ref["sparse"])
    with pytest.raises(RuntimeError, match="names frame"):
        eval_io.gen_sparse_trajectory(np.array([[0.0, 13.0]]), poses)


def test_get_traj_reads_log_and_npy_as_the_reference(ref, tmp_path):
    import eval_io
    got = eval_io.get_traj(golden("evalio_traj.log"))
    assert got.dtype == np.float64 and np.array_equal(got, ref["get_traj_log"])
    got = eval_io.get_traj(golden("evalio_traj34.npy"))
    assert got.shape == (5, 4, 4) and np.array_equal(got, ref["get_traj_npy"]) and np.array_equal(got[:, 3], np.tile([0.0, 0, 0, 1], (5, 1)))
    with pytest.raises(RuntimeError, match="json.*not supported"):
        eval_io.get_traj(str(tmp_path / "transforms.json"))
    np.save(tmp_path / "bad.npy", np.zeros((3, 2, 4)))
    with pytest.raises(RuntimeError, match="4x4 or 3x4"):
        eval_io.get_traj(str(tmp_path / "bad.npy"))


def test_load_transform_reads_the_trans_file(tmp_path):
    import eval_io
    assert np.array_equal(eval_io.load_transform(golden("evalio_trans.txt")), np.loadtxt(golden("evalio_trans.txt")))
    np.savetxt(tmp_path / "t.txt", np.eye(3))
    with pytest.raises(RuntimeError, match="4x4"):
        eval_io.load_transform(str(tmp_path / "t.txt"))


def test_best_fit_transform_and_the_scale_rule_are_the_references(ref):
    import eval_io
    scale_gt, scale, r, t = eval_io.dtu_alignment(ref["fit_points"], ref["fit_gt_points"])
    assert np.array_equal(scale, ref["fit_scale_points"]) and np.array_equal(scale_gt, ref["fit_scale_gt_points"])
    assert np.array_equal(r, ref["fit_r"]) and np.array_equal(t, ref["fit_t"])
    T, R, tt = eval_io.best_fit_transform(ref["fit_points"].astype(np.float64), ref["fit_gt_points"].astype(np.float64))
    assert np.array_equal(T, ref["fit_T64"]) and np.array_equal(T[:3, :3], R) and np.array_equal(T[:3, 3], tt)
    assert abs(np.linalg.det(R) - 1) < 1e-12
    with pytest.raises(RuntimeError, match="same shape"):
        eval_io.best_fit_transform(np.zeros((4, 3)), np.zeros((5, 3)))


def test_dtu_camera_centres_are_the_centres_the_projections_were_built_from(ref, tmp_path):
    """cv2 is not installed where the fixture was made: the files hold K R [I | -C] for known C, printed with six decimals and read as
    float32.  The entries of p4 reach 3e6 (half an ulp: 0.125) and are divided by f = 2.9e3: 5e-5; those of M reach 2.9e3 (1.2e-4), times
    |C| < 1e3, divided by f: 5e-5; float32 storage of C: 3e-5.  5e-4 covers their sum with a margin of three."""
    import eval_io
    got = eval_io.dtu_camera_centres(golden("evalio_dtu"), n=3)
    assert got.dtype == np.float32 and got.shape == (3, 3)
    assert np.abs(got - ref["dtu_centres"]).max() < 5e-4 and np.abs(ref["dtu_centres"]).max() < 1e3
    with pytest.raises(OSError):
        eval_io.dtu_camera_centres(golden("evalio_dtu"), n=4)
    np.savetxt(tmp_path / "pos_001.txt", np.zeros((3, 4)))
    with pytest.raises(RuntimeError, match="at infinity"):
        eval_io.dtu_camera_centres(str(tmp_path), n=1)


def test_load_dtu_masks_reads_mat_files(tmp_path):
    import eval_io
    from scipy.io import savemat
    os.makedirs(tmp_path / "ObsMask")
    obs = (np.arange(24).reshape(2, 3, 4) % 3 == 0)
    savemat(tmp_path / "ObsMask" / "ObsMask24_10.mat", dict(ObsMask=obs, BB=np.array([[0.0, 1, 2], [3, 4, 5]]), Res=np.array([[10.0]])))
    savemat(tmp_path / "ObsMask" / "Plane24.mat", dict(P=np.array([[0.0], [0.0], [1.0], [-2.0]])))
    mask, BB, Res, P = eval_io.load_dtu_masks(str(tmp_path), 24)
    assert np.array_equal(mask != 0, obs) and BB.shape == (2, 3) and float(Res.reshape(-1)[0]) == 10.0 and np.array_equal(P.reshape(-1), [0, 0, 1, -2])


# ----------------------------------------------------------------------- the RANSAC restatement -----------------------------------------------------------------------
def test_the_generator_draws_distinct_indices_and_depends_on_seed_and_hypothesis_alone():
    a = er.sample_indices(0, 500, 6, 24)
    assert a.min() >= 0 and a.max() < 24 and all(len(set(row)) == 6 for row in a.tolist())
    assert np.array_equal(a[100:200], er.sample_indices(0, 200, 6, 24)[100:])            # hypothesis h does not depend on K
    assert np.array_equal(er.sample_indices(0, 50, 8, 8).sum(1), np.full(50, 28))       # N == n: a permutation
    assert not np.array_equal(a, er.sample_indices(1, 500, 6, 24))
    counts = np.bincount(er.sample_indices(3, 20000, 3, 10).reshape(-1), minlength=10)
    assert counts.min() > 5400 and counts.max() < 6600                                   # 6000 each when uniform; sigma = 73
    assert int(er.draw_u32(0, np.array([0]), 0)[0]) == ((_mix(0x2545F4914F6CDD1D)) >> 32)


def _mix(z):
    m = (1 << 64) - 1
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & m
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_the_per_sample_similarity_is_tnt_evals_umeyama():
    import tnt_eval as te
    src, tgt, _ = er.noisy_pairs(40, 5)
    samples = er.sample_indices(0, 64, 6, 40)
    sums = er.sample_sums(src[samples], tgt[samples])
    T, ok, ratio = er.umeyama_batch(sums)
    assert ok.all() and (ratio > er.SCOPE).all()
    for h in range(64):
        assert np.allclose(T[h], te.umeyama(sums[h]), rtol=1e-12, atol=1e-13)
        assert np.allclose(T[h], tr.umeyama(src[samples[h]], tgt[samples[h]]), rtol=1e-10, atol=1e-11)
    flat = er.sample_sums(np.ones((1, 6, 3)), tgt[None, :6])                              # no extent
    assert not er.umeyama_batch(flat)[1][0]


def test_no_hypothesis_beats_the_winner_and_the_known_similarity_is_recovered():
    src, tgt, known, res = er.fixture(300, 4097)
    w = res["hypothesis"]
    assert res["scope"].mean() >= 0.95 and res["count"] >= 200
    for h in range(4097):                                                                 # brute force under the rule
        if h != w and res["counts"][h] > 0:
            assert er.better(res["count"], res["inlier_rmse"], w, int(res["counts"][h]), float(res["rmse"][h]), h)
    assert np.abs(res["transformation"] - known).max() < 0.02                             # noise 0.015 over a cloud of extent 6
    moved = tr.transform(src, res["transformation"])
    d = np.sqrt(((moved - tgt) ** 2).sum(1))
    assert int((d < 0.2).sum()) == res["count"] and np.isclose(np.sqrt((d[d < 0.2] ** 2).mean()), res["inlier_rmse"], rtol=1e-12)
    again = er.ransac(src, tgt, 0.2, 6, 4097, 0)
    assert again["hypothesis"] == w and np.array_equal(again["sumsq"], res["sumsq"])
    assert er.ransac(src, tgt, 0.2, 6, 4097, 1)["hypothesis"] != w


def test_exact_data_gives_every_pair_and_the_transformation():
    rng = np.random.default_rng(2)
    known = er.similarity(rng)
    src = rng.uniform(-3, 3, (6, 3))
    res = er.ransac(src, tr.transform(src, known), 0.2, 6, 64, 0, check=False)            # every rmse is rounding noise: no margin to ask for
    assert res["count"] == 6 and (res["counts"] == 6).all() and np.allclose(res["transformation"], known, rtol=0, atol=1e-12)


def test_margins_are_raised_not_narrowed():
    src, tgt, _, res = er.fixture(24, 256)
    w = res["hypothesis"]
    moved = tr.transform(src, res["T"][w])
    d = np.sqrt(((moved - tgt) ** 2).sum(1))
    j = int(np.argmax(d > 0.2))
    tgt2 = tgt.copy()
    tgt2[j] = moved[j] + (tgt[j] - moved[j]) / d[j] * (0.2 + 2e-10)                       # an outlier moved to within the margin
    if j in res["samples"][w]:
        pytest.fail("the moved pair is in the winner's sample; choose another fixture seed")
    with pytest.raises(er.Margin):
        er.ransac(src, tgt2, 0.2, 6, 256, 0)
    dup = np.concatenate([src, src]), np.concatenate([tgt, tgt])                          # all-outlier and degenerate inputs run through
    assert er.ransac(*dup, 0.2, 6, 64, 0, check=False)["count"] >= 0
    line = np.outer(np.arange(12.0), [1.0, 2.0, -1.0])
    res = er.ransac(line, line * 2.0, 0.2, 6, 128, 0, check=False)
    assert np.isfinite(res["transformation"]).all() and not res["scope"].any()


# ------------------------------------------------------------------------------- PLY -------------------------------------------------------------------------------
def test_ply_restatement_reads_its_writers_in_every_layout(tmp_path):
    v, f = er.mesh_data(37, 50, seed=3)
    for name, build in er.LAYOUTS.items():
        for fmt in ("binary_little_endian", "binary_big_endian", "ascii"):
            path = str(tmp_path / f"{name}_{fmt}.ply")
            elements, exp_v, exp_f = build(v, f)
            er.write_ply(path, elements, fmt)
            got_v = er.ply_points(path)
            assert got_v.dtype == np.float64 and np.array_equal(got_v, exp_v), (name, fmt)
            if exp_f is not None:
                gv, gf = er.ply_mesh(path)
                assert np.array_equal(gf, exp_f) and gf.dtype == np.int64, (name, fmt)


def test_ply_restatement_reads_what_the_projects_writers_write(tmp_path):
    import tetmesh
    v, f = er.mesh_data(20, 30, seed=4)
    path = str(tmp_path / "t.ply")
    tetmesh.write_ply(path, v.astype(np.float32), f)
    gv, gf = er.ply_mesh(path)
    rv, rf = tetmesh.read_ply(path)
    assert np.array_equal(gv, rv.astype(np.float64)) and np.array_equal(gf, rf)


def test_merge_vertices_restatement():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 4e-9], [np.nan, 0, 0], [5, 5, 5], [0, 1, 0], [2, 2, 2]], np.float64)
    f = np.array([[0, 1, 2], [3, 6, 7], [4, 0, 1], [6, 3, 0]])
    mv, mf = er.merge_vertices(v, f)
    assert np.array_equal(mv, v[[0, 1, 2, 7]]) and np.array_equal(mf, [[0, 1, 2], [1, 2, 3], [2, 1, 0]])   # 3 welds to 1, 6 to 2; 5 is unreferenced
    assert er.merge_vertices(v, f, digits=9)[0].shape[0] == 5                                               # 4e-9 apart at nine digits
    rng = np.random.default_rng(0)
    base = rng.uniform(-1, 1, (30, 3))
    pick = rng.integers(0, 30, 200)
    vv, ff = base[pick], rng.integers(0, 200, (150, 3))
    mv, mf = er.merge_vertices(vv, ff)
    assert mv.shape[0] == np.unique(pick[np.unique(ff)]).shape[0] and np.array_equal(mv[mf], vv[ff])
    first = [int(np.nonzero((vv == row).all(1))[0][0]) for row in mv]
    assert first == sorted(first)                                                                           # first-occurrence order
    assert er.merge_vertices(vv, np.zeros((0, 3), np.int64))[0].shape == (0, 3)
