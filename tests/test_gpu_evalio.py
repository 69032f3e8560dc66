"""GPU tier of evaluation from files, the kernels of csrc/radegs_evalio.hip against tests/evalio_restatement.py.
RANSAC: per-hypothesis counts are compared exactly and sumsq, rmse and the transformation at 1e-9 relative -- the band of "what passes
through a sum over the pairs and an SVD" (tests/test_gpu_tnteval.py) -- on the hypotheses whose sample covariance has sigma_2 / sigma_1 >
1e-3 (elsewhere the rotation is ill-determined and two SVDs may differ); every noisy fixture keeps at least 95 % of its hypotheses in that
scope, and the restatement has checked that no distance lies within 1e-9 of max_dist and that the winner's rmse is 1e-9 clear of the
runner-up's, so the winning hypothesis must be the same index.  A matrix is compared by max |a - b| <= 1e-9 max |b|.
Unpack kernels: every value exactly (F8 bit for bit, F4 and the integers widened exactly)."""
import numpy as np
import pytest
import torch

import evalio_restatement as er
import tnteval_restatement as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 1e-9
CHUNK = 256
_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def near(a, b, rel=REL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.abs(a - b).max() <= rel * np.abs(b).max())


def fixture(N, K, n=6, **kw):
    """computed once, shared, never changed"""
    key = (N, K, n, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = er.fixture(N, K, n, **kw)
    return _cache[key]


def run(src, tgt, K, n=6, seed=0):
    import tnt_eval as te
    return te.ransac_correspondence(dev(src), dev(tgt), 0.2, n, K, seed=seed, return_all=True)


def check_against_restatement(got, exp, N, min_scope=0.95):
    scope = exp["scope"]
    assert scope.mean() >= min_scope
    counts, sumsq = host(got["counts"]), host(got["sumsq"])
    assert counts.dtype == np.int32 and sumsq.dtype == np.float64 and counts.shape == exp["counts"].shape
    assert np.array_equal(counts[scope], exp["counts"][scope])
    hit = scope & (exp["counts"] > 0)
    assert np.all(np.abs(sumsq[hit] - exp["sumsq"][hit]) <= REL * exp["sumsq"][hit]) and np.all(sumsq[scope & (exp["counts"] == 0)] == 0)
    dead = ~exp["ok"]                                                # a sample without extent counts nothing
    assert np.all(counts[dead] == 0) and np.all(sumsq[dead] == 0)
    assert got["hypothesis"] == exp["hypothesis"] and got["count"] == exp["count"] and got["fitness"] == exp["count"] / N
    assert near(got["transformation"], exp["transformation"]) and np.array_equal(got["transformation"][3], [0, 0, 0, 1])
    assert abs(got["inlier_rmse"] - exp["inlier_rmse"]) <= REL * exp["inlier_rmse"]
    if exp["hypothesis"] >= 0:
        assert counts[exp["hypothesis"]] == got["count"]


# ------------------------------------------------------------------------------ RANSAC ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,n", [(7, 65, 6), (24, 2048, 6), (64, 4096, 6), (300, 4097, 6), (CHUNK + 1, 64, 6), (40, 63, 6), (40, 64, 3), (40, 64, 8)],
                         ids=["7x65", "24x2048", "64x4096", "300x4097", "second_chunk", "wave_tail", "ransac_n3", "ransac_n8"])
def test_ransac_equals_the_restatement_on_noisy_pairs(N, K, n):
    import eval_io
    assert CHUNK == eval_io.RANSAC_CHUNK
    src, tgt, known, exp = fixture(N, K, n)
    got = run(src, tgt, K, n)
    check_against_restatement(got, exp, N)
    if N >= 64:                                                      # most inliers found, the known similarity recovered to the noise
        assert got["count"] >= 0.7 * N and np.abs(got["transformation"] - known).max() < 0.02


@pytest.mark.parametrize("N,K", [(6, 1), (6, 64)], ids=["one_lane", "6x64"])
def test_ransac_on_exact_data_finds_every_pair(N, K):
    """every rmse is rounding noise here, so which hypothesis wins is not compared: count == N and the transformation are"""
    rng = np.random.default_rng(2)
    known = er.similarity(rng)
    src = rng.uniform(-3, 3, (N, 3))
    tgt = tr.transform(src, known)
    exp = er.ransac(src, tgt, 0.2, 6, K, 0, check=False)
    got = run(src, tgt, K)
    assert exp["scope"].all() and exp["closest"] > 0.1
    assert got["count"] == N and got["fitness"] == 1.0 and np.array_equal(host(got["counts"]), np.full(K, N, np.int32))
    assert 0 <= got["hypothesis"] < K and near(got["transformation"], known) and got["inlier_rmse"] < 1e-12


def test_ransac_degenerate_inputs_never_give_nan():
    line = np.outer(np.arange(12.0), [1.0, 2.0, -1.0]) + [0.5, 0.0, 3.0]
    got = run(line, line * 2.0 + 1.0, 128)                           # 12 collinear points: no sample spans a rotation
    T = got["transformation"]
    assert np.isfinite(T).all() and np.isfinite(got["inlier_rmse"]) and np.isfinite(host(got["sumsq"])).all()
    if got["count"] == 0:
        assert np.array_equal(T, np.eye(4)) and got["fitness"] == 0.0 and got["hypothesis"] == -1
    same = np.tile([[1.0, 2.0, 3.0]], (9, 1))                        # no extent at all: every hypothesis counts 0
    got = run(same, same + 1.0, 70)
    assert got["count"] == 0 and got["hypothesis"] == -1 and np.array_equal(got["transformation"], np.eye(4)) and got["fitness"] == 0.0
    assert not host(got["counts"]).any() and not host(got["sumsq"]).any()


def test_ransac_on_outliers_alone_and_on_duplicated_points():
    src, tgt, _, exp = fixture(30, 256, outliers=1.0)
    got = run(src, tgt, 256)
    check_against_restatement(got, exp, 30)
    assert np.isfinite(got["transformation"]).all()
    src, tgt, _, _ = fixture(24, 2048)
    s2, t2 = np.concatenate([src[:12], src[:12]]), np.concatenate([tgt[:12], tgt[:12]])      # a sample may hold the same point twice
    exp = None
    for seed in range(20):                                           # the first seed at which the restatement keeps its margins
        try:
            exp = er.ransac(s2, t2, 0.2, 6, 512, seed)
            break
        except er.Margin:
            continue
    assert exp is not None
    check_against_restatement(run(s2, t2, 512, seed=seed), exp, 24, min_scope=0.0)


def test_two_runs_give_the_same_bits_and_a_second_seed_another_hypothesis():
    src, tgt, _, exp = fixture(24, 2048)
    a, b = run(src, tgt, 2048), run(src, tgt, 2048)
    assert torch.equal(a["counts"], b["counts"]) and torch.equal(a["sumsq"].view(torch.int64), b["sumsq"].view(torch.int64))
    assert a["transformation"].tobytes() == b["transformation"].tobytes() and a["hypothesis"] == b["hypothesis"] and a["inlier_rmse"] == b["inlier_rmse"]
    part = run(src, tgt, 700)                                        # hypothesis h does not depend on how many are launched
    assert torch.equal(part["counts"], a["counts"][:700]) and torch.equal(part["sumsq"].view(torch.int64), a["sumsq"][:700].view(torch.int64))
    other = er.ransac(src, tgt, 0.2, 6, 2048, 1)
    c = run(src, tgt, 2048, seed=1)
    check_against_restatement(c, other, 24)
    assert c["hypothesis"] != a["hypothesis"] and c["count"] == a["count"] == exp["count"]


def test_ransac_refuses_what_it_cannot_pair():
    import tnt_eval as te
    a = torch.zeros(10, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="5 pairs are fewer than `ransac_n` = 6"):
        te.ransac_correspondence(a[:5], a[:5])
    with pytest.raises(RuntimeError, match="must be paired"):
        te.ransac_correspondence(a, a[:9])
    bad = a.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(RuntimeError, match="`target` holds non-finite values"):
        te.ransac_correspondence(a, bad)
    with pytest.raises(RuntimeError, match="`source` holds non-finite values"):
        te.ransac_correspondence(bad, a)


# --------------------------------------------------------------------------- unpack kernels ---------------------------------------------------------------------------
COUNTS = (0, 1, 63, 64, 65, 4097)
POINT_LAYOUTS = {                                                    # record dtype; the columns of x, y, z
    "f4": [("x", "<f4"), ("y", "<f4"), ("z", "<f4")],                                                       # 12 bytes
    "f8_odd": [("pad", "u1"), ("x", "<f8"), ("y", "<f8"), ("tag", "<u2"), ("z", "<f8")],                     # 27 bytes, nothing aligned
    "ints": [("z", "<i4"), ("a", "u1"), ("x", "i1"), ("y", "<u2"), ("b", "u1")],                             # 9 bytes
    "mixed": [("y", "<u4"), ("c", "u1"), ("z", "<i2"), ("x", "u1"), ("d", "<f4"), ("e", "u1")],             # 13 bytes
    "mixed_f": [("q", "<i2"), ("x", "<f4"), ("y", "<f8"), ("z", "<f4"), ("r", "u1")],                        # 19 bytes
}


def records(dtype, n, seed):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, np.dtype(dtype))
    raw = rng.integers(0, 256, rec.view(np.uint8).shape, dtype=np.uint8)     # every bit pattern of the integers
    rec.view(np.uint8)[:] = raw
    for name in rec.dtype.names:
        if rec.dtype[name].kind == "f":                                      # finite floats with all their digits, and the edge values
            vals = rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)
            vals[:min(n, 6)] = [0.0, -0.0, 1e-310 if rec.dtype[name].itemsize == 8 else 1e-40, -np.inf, 1.0 + 2.0 ** -52, 3.4e38][:min(n, 6)]
            rec[name] = vals
    return rec


def padded(raw, lead=0):
    """the bytes on the device behind `lead` leading bytes, padded as include/radegs.h asks"""
    n = lead + raw.shape[0]
    buf = np.zeros((n + 3) // 4 * 4 + 8, np.uint8)
    buf[lead:n] = raw
    return dev(buf)


@pytest.mark.parametrize("layout", sorted(POINT_LAYOUTS))
def test_unpack_points_is_exact_for_every_type_stride_and_count(layout):
    import eval_io
    dtype = np.dtype(POINT_LAYOUTS[layout])
    cols = [(dtype.fields[c][1], dtype.fields[c][0].str[1:]) for c in "xyz"]
    for n in COUNTS:
        for lead in (0, 3):                                                  # the records start at any byte
            rec = records(dtype, n, seed=n + lead)
            got = eval_io.unpack_points(padded(rec.view(np.uint8).reshape(-1), lead), lead, n, dtype.itemsize, cols)
            exp = np.stack([rec[c].astype(np.float64) for c in "xyz"], 1) if n else np.zeros((0, 3))
            assert got.dtype == torch.float64 and tuple(got.shape) == (n, 3)
            assert np.array_equal(host(got).view(np.int64), exp.view(np.int64)), (layout, n, lead)      # bit for bit, -0.0 and subnormals too


FACE_LAYOUTS = {
    "u1_i4": ([("n", "u1"), ("v", "<i4", (3,))], "u1", "i4"),                                               # 13 bytes: tetmesh, trimesh
    "u1_u4": ([("n", "u1"), ("v", "<u4", (3,))], "u1", "u4"),                                               # Open3D
    "i1_lead": ([("m", "<i2"), ("n", "i1"), ("v", "<i4", (3,))], "i1", "i4"),                               # 15 bytes, a leading property
    "u2_trail": ([("n", "<u2"), ("v", "<u4", (3,)), ("q", "u1")], "u2", "u4"),                              # 15 bytes, a trailing one
    "i2_both": ([("a", "u1"), ("n", "<i2"), ("v", "<i4", (3,)), ("b", "<f4"), ("c", "u1")], "i2", "i4"),    # 20 bytes
    "u4": ([("n", "<u4"), ("v", "<u4", (3,))], "u4", "u4"),                                                 # 16 bytes
    "i4_odd": ([("a", "u1"), ("n", "<i4"), ("v", "<i4", (3,))], "i4", "i4"),                                # 17 bytes
}


@pytest.mark.parametrize("layout", sorted(FACE_LAYOUTS))
def test_unpack_faces_reads_every_layout_and_counts_what_it_refuses(layout):
    import eval_io
    fields, ct, it = FACE_LAYOUTS[layout]
    dtype = np.dtype(fields)
    V = 1000
    args = (dtype.itemsize, dtype.fields["n"][1], ct, dtype.fields["v"][1], it, V)
    for n in COUNTS:
        rng = np.random.default_rng(n)
        rec = np.zeros(n, dtype)
        rec.view(np.uint8)[:] = rng.integers(0, 256, rec.view(np.uint8).shape, dtype=np.uint8)          # the properties to be skipped: noise
        rec["n"] = 3
        rec["v"] = rng.integers(0, V, (n, 3))
        if n:
            rec["v"][n // 2] = [0, V - 1, V // 2]                                                        # both ends of the range
        lead = n % 4
        faces, bad = eval_io.unpack_faces(padded(rec.view(np.uint8).reshape(-1), lead), lead, n, *args)
        assert faces.dtype == torch.int64 and tuple(faces.shape) == (n, 3) and int(bad.item()) == 0
        assert np.array_equal(host(faces), rec["v"].astype(np.int64).reshape(n, 3)), (layout, n)
    n = 4097
    for where, what in ((0, "quad"), (2048, "index"), (4096, "quad"), (63, "index"), (64, "negative")):
        spoiled = rec.copy()
        if what == "quad":
            spoiled["n"][where] = 4
        elif what == "index":
            spoiled["v"][where, 2] = V                                                                   # one past the last vertex
        else:
            spoiled["v"][where, 0] = -1 if it == "i4" else 2 ** 32 - 1
        faces, bad = eval_io.unpack_faces(padded(spoiled.view(np.uint8).reshape(-1)), 0, n, *args)
        assert int(bad.item()) == 1, (layout, where, what)
    spoiled = rec.copy()
    spoiled["n"][10:75] = 2
    spoiled["v"][70:80, 1] = V + 5                                                                       # 65 + 5 records, some bad twice over
    assert int(eval_io.unpack_faces(padded(spoiled.view(np.uint8).reshape(-1)), 0, n, *args)[1].item()) == 70
