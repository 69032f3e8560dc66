"""GPU tier of the Delaunay tetrahedralisation at scale: delaunay.triangulate and the kernels of csrc/radegs_delaunay.hip
where tests/test_gpu_delaunay.py (at most 1000 points, an 8-cell grid that kShellMax nearly covers) does not reach -- the shell termination
on a 30-cell grid, a (side, 1, 1) grid, a cell of 18 000 points, the slow kernel's block skip over hundreds of blocks, bounds that are not
the bounding box, the record-capacity regrow, the drop past record_capacity / out_capacity, the cell-capacity refusal and the retry ladder.
The verdict is tests/delaunay_certificate.py (exact, reference-free; tests/test_delaunay_certificate.py holds it to account); scipy is a
cross-check where its own rows pass that certificate.  X is always delaunay.perturbed(points, jitter 10^retries, seed + retries) with the
`retries` the call reported.  Wall times in the docstrings are of one run on an MI355X, host work included."""
import time

import numpy as np
import pytest
import torch

import delaunay_cases as dc
import delaunay_certificate as cert
from delaunay_cases import load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def coordinates(points, jitter, seed, retries):
    """the float64 coordinates the call that reported `retries` triangulated, as NumPy"""
    import delaunay
    for _ in range(retries):
        jitter = jitter * 10.0                                                 # as triangulate steps it
    return delaunay.perturbed(points, jitter, seed + retries).cpu().numpy()


def triangulate_and_certify(points, jitter=1e-9, seed=0):
    """(cells tensor, info, X, certify's result)"""
    import delaunay
    cells, info = delaunay.triangulate(points, jitter=jitter, seed=seed, return_info=True)
    X = coordinates(points, jitter, seed, info["retries"])
    return cells, info, X, cert.certify(X, cells.cpu().numpy())


def sorted_set(cells):
    q = np.sort(np.asarray(cells, dtype=np.int64), axis=1)
    return q[np.lexsort(q.T[::-1])]


def scipy_cross_check(name, X, cells):
    """Where scipy's rows on the same X pass the certificate they are the same set as ours.  Equal sets need no second certificate: ours
    passed.  Where they differ scipy's rows are certified: passing, two different certified triangulations of points in general position
    would exist, a failure of the kernels or of the certificate; failing, Qhull's tolerance is at fault and the certificate alone stands."""
    from scipy.spatial import Delaunay
    theirs = np.unique(np.sort(Delaunay(X).simplices, axis=1), axis=0).astype(np.int64)
    mine = sorted_set(cells)
    if mine.shape == theirs.shape and np.array_equal(mine, theirs):
        print(name, "scipy: the same", mine.shape[0], "tetrahedra")
        return True
    import delaunay_restatement as dr
    d = cert.defects(cert.certify(X, dr.orient(X, theirs)))
    print(name, "scipy differs:", theirs.shape[0], "rows against", mine.shape[0], "; scipy's defects:", d)
    assert d != {}, f"{name}: scipy's rows pass the certificate and differ from the kernels'"
    return False


# ------------------------------------------------------------------------- a. clouds -------------------------------------------------------------------------
def _cloud_points(name):
    if name != "boxes2000":
        return dev(dc.cloud(name))
    import tetmesh
    xyz, scales, rot = dc.box_gaussians(*dc.BOXES2000)
    return tetmesh.tetra_points(dev(xyz), dev(scales), dev(rot))[0]


SCIPY_MUST_AGREE = ("uniform50k", "surface20k", "boxes2000")                   # tests/test_delaunay_certificate.py certifies scipy on these
CLOUDS = ["uniform50k", "slab20k", "clustered20k", "surface20k", "boxes2000", "dup200"]
_first = {}


def first_call(name):
    """(points, cells, info, X) of a cloud's first triangulate: computed once, shared by the two tests below, never modified"""
    if name not in _first:
        import delaunay
        points = _cloud_points(name)
        cells, info = delaunay.triangulate(points, return_info=True)
        _first[name] = (points, cells, info, coordinates(points, 1e-9, 0, info["retries"]))
    return _first[name]


@pytest.mark.parametrize("name", CLOUDS)
def test_cloud_certifies(name):
    """Printed on an MI355X: wall seconds of the test (first triangulate, certificate, scipy) / deferred / uncertain / retries / scipy:
        uniform50k    2.8   3 146   0   0   the same 335 305 tetrahedra
        slab20k       1.5   3 077   0   0   the same 127 532
        clustered20k  4.9     582   0   0   133 383 rows, 7 faces of them not locally Delaunay; ours 133 382 and certified
        surface20k    1.5   6 936   0   0   the same 128 934
        boxes2000     1.9     891   0   0   the same 124 634
        dup200        0.1     133   0   0   the same 1 246
    clustered20k's triangulate alone is 4.1 s: the 18 000 points of its one crowded cell all clip one another in the fast kernel.  Before
    in_sphere_recentred (rg_delaunay_cell.h) dup200 was refused after two retries, 154 of 1 354 tetrahedra inconsistent and 481 predicate
    values uncertain, clustered20k met 1 uncertain value and lines200b below went through a retry."""
    t0 = time.perf_counter()
    points, cells, info, X = first_call(name)
    res = cert.certify(X, cells.cpu().numpy())
    t1 = time.perf_counter()
    print(name, "N", points.shape[0], "rows", cells.shape[0], "deferred", info["deferred"], "uncertain", info["uncertain"], "retries", info["retries"],
          "exact evaluations", res["exact"], "hull faces", res["hull_faces"])
    assert cert.defects(res) == {}, cert.defects(res)
    assert info["inconsistent"] == 0 and info["overflow"] == 0 and info["tets"] == cells.shape[0]
    assert cells.dtype == torch.int32 and cells.is_contiguous()
    agrees = scipy_cross_check(name, X, cells.cpu().numpy())
    assert agrees or name not in SCIPY_MUST_AGREE
    print(name, "seconds: triangulate + certify %.2f, scipy %.2f" % (t1 - t0, time.perf_counter() - t1))


@pytest.mark.parametrize("name", CLOUDS)
def test_cloud_second_call_gives_the_same_bits(name):
    """Printed on an MI355X, wall seconds of the second call: uniform50k 0.32, slab20k 1.15, clustered20k 4.07, surface20k 1.10, boxes2000 1.46,
    dup200 0.05"""
    import delaunay
    points, cells, info, X = first_call(name)
    t0 = time.perf_counter()
    again, info2 = delaunay.triangulate(points, return_info=True)
    torch.cuda.synchronize()
    print(name, "second call %.2f s" % (time.perf_counter() - t0))
    assert torch.equal(cells, again) and info2 == info


# ------------------------------------------------------------------------- b. bounds -------------------------------------------------------------------------
def _plan_emit(p, bounds):
    import delaunay
    ws, nbytes, capacity, counts = delaunay._plan(p, [float(b) for b in bounds], 0.0, 0)
    records, deferred, uncertain, overflow = counts
    assert overflow == 0 and uncertain == 0 and records > 0
    cells, unique, inconsistent = delaunay._emit(p.shape[0], ws, nbytes, capacity, records)
    assert inconsistent == 0 and 4 * unique == records == 4 * cells.shape[0]
    return cells, deferred


@pytest.mark.parametrize("name", ["uniform", "slab"])
def test_the_bounds_only_lay_the_grid(name):
    """include/radegs.h: "any finite box gives the same result".  3000 points in general position, no jitter; the true bounding box against
    one ten times as large, one half as large (points outside it land in border cells), a box of no extent (one cell of no size: the fast
    kernel's stop test never holds and every point is deferred) and the true box five diagonals away (every point in one corner cell).
    Printed on an MI355X, deferred for true / grown / shrunk / degenerate / shifted: uniform 502 / 183 / 720 / 3000 / 502 in 1.2 s, slab
    1101 / 597 / 1288 / 3000 / 1101 in 1.8 s.  While the box of no extent still had cells of size 1 the uniform cloud, whose cells are far
    smaller than 1, deferred 354 points and not 3000: which kernel finished a point depended on the units of the cloud."""
    import delaunay
    t0 = time.perf_counter()
    N = 3000
    p = dev((dc.uniform if name == "uniform" else dc.slab)(N, 60)).double()
    true, diag = delaunay._bounds(p)
    lo, hi = np.array(true[:3]), np.array(true[3:])
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    shift = 5.0 * diag * np.ones(3) / np.sqrt(3.0)
    boxes = {"true": true, "grown": list(mid - 10 * half) + list(mid + 10 * half), "shrunk": list(mid - 0.5 * half) + list(mid + 0.5 * half),
             "degenerate": list(mid) + list(mid), "shifted": list(lo + shift) + list(hi + shift)}
    want, deferred = _plan_emit(p, true)
    res = cert.certify(p.cpu().numpy(), want.cpu().numpy())
    assert cert.defects(res) == {}, cert.defects(res)
    seen = {"true": deferred}
    for key, box in boxes.items():
        if key != "true":
            cells, seen[key] = _plan_emit(p, box)
            assert torch.equal(cells, want), key
    print(name, "deferred:", seen, "seconds %.2f" % (time.perf_counter() - t0))
    assert seen["degenerate"] == N


# ------------------------------------------------------------------------- c. scale and offset -------------------------------------------------------------------------
def test_scale_by_a_power_of_two_changes_nothing_and_an_offset_still_certifies():
    """The predicates are homogeneous, and the jitter scales with the diagonal, exactly so for a power of two: 2^20 and 2^-20 times the
    points give the same rows bit for bit.  An offset of (1e6, -2e6, 3e6) leaves float64 30 bits for the differences: the rows certify.
    Printed on an MI355X: the three runs identical, rows, info (231 deferred) and coordinates; the offset cloud certifies with no exact
    evaluation; 0.56 s."""
    import delaunay
    t0 = time.perf_counter()
    p = load("random1000")["points"].astype(np.float64)
    cells, info, X, res = triangulate_and_certify(dev(p))
    assert cert.defects(res) == {} and info["retries"] == 0
    for factor in (2.0 ** 20, 2.0 ** -20):
        scaled, sinfo, sX, sres = triangulate_and_certify(dev(p * factor))
        print("scale", factor, sinfo, cert.defects(sres))
        assert np.array_equal(sX, X * factor)
        assert cert.defects(sres) == {}
        assert torch.equal(scaled, cells) and sinfo == info
    moved, minfo, mX, mres = triangulate_and_certify(dev(p + np.array([1e6, -2e6, 3e6])))
    print("offset", minfo, cert.defects(mres), "exact evaluations", mres["exact"], "seconds %.2f" % (time.perf_counter() - t0))
    assert cert.defects(mres) == {} and minfo["overflow"] == 0 and minfo["inconsistent"] == 0


# ------------------------------------------------------------------------- d. record capacity -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lines200a", "lines200b"])
def test_records_beyond_the_first_capacity_regrow_the_workspace(name, monkeypatch):
    """two skew lines: 4 T is several times the 32 N + 1024 = 7424 records of the first plan, which therefore runs twice an attempt.
    Printed on an MI355X: lines200a 4 320 rows, capacities asked for [7424, 17280], 199 deferred, 0.27 s; lines200b 10 416 rows,
    [7424, 41664], 200 deferred, 0.37 s; no retry, no uncertain value."""
    import delaunay
    t0 = time.perf_counter()
    L = delaunay._lib()
    real, asked = L.radegs_delaunay_bytes, []

    def spy(N, capacity):
        asked.append(capacity)
        return real(N, capacity)
    monkeypatch.setattr(L, "radegs_delaunay_bytes", spy)
    cells, info, X, res = triangulate_and_certify(dev(dc.cloud(name)))
    print(name, "rows", cells.shape[0], info, "capacities asked for:", asked, "seconds %.2f" % (time.perf_counter() - t0))
    assert cert.defects(res) == {}, cert.defects(res)
    assert info["overflow"] == 0 and info["inconsistent"] == 0 and 4 * cells.shape[0] > 7424
    assert asked[-2:] == [7424, 4 * cells.shape[0]] and len(asked) == 2 * (info["retries"] + 1)


def _guarded(nbytes, fill=0xA5):
    big = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
    return big, big[GUARD:GUARD + nbytes]


def _guards_intact(big, nbytes, fill=0xA5):
    return bool((big[:GUARD] == fill).all()) and bool((big[GUARD + nbytes:] == fill).all())


def _plan_direct(p, bounds, capacity):
    """radegs_delaunay_plan on a workspace of exactly radegs_delaunay_bytes(N, capacity) bytes between two guards"""
    import delaunay
    import geom_host as gh
    from diff_gaussian_rasterization import _C
    L, N = delaunay._lib(), p.shape[0]
    nbytes = L.radegs_delaunay_bytes(N, capacity)
    assert nbytes > 0 and nbytes % 16 == 0
    big, ws = _guarded(nbytes)
    counts4 = torch.zeros(4, dtype=torch.int64, device=DEV)
    gh.check(L.radegs_delaunay_plan(N, _C._ptr(p), gh.doubles(bounds), 0.0, 0, capacity, _C._ptr(ws), nbytes, _C._ptr(counts4), _C._stream(p.device)), "plan")
    counts = counts4.tolist()
    assert _guards_intact(big, nbytes), capacity
    return big, ws, nbytes, counts


def test_records_past_the_capacity_are_counted_and_not_written():
    """radegs_delaunay_plan on random1000 (4 T = 25 520) with room for 1, 25 519 and 25 520 records, the workspace between two guards.
    On an MI355X: 0.39 s."""
    import delaunay
    fx = load("random1000")
    p = dev(fx["points"]).double()
    bounds, _ = delaunay._bounds(p)
    T = fx["cells"].shape[0]
    assert 4 * T == 25520
    for capacity in (1, 25519, 25520):
        big, ws, nbytes, counts = _plan_direct(p, bounds, capacity)
        assert counts[0] == 25520 and counts[2] == 0 and counts[3] == 0, (capacity, counts)
    cells, unique, inconsistent = delaunay._emit(p.shape[0], ws, nbytes, 25520, counts[0])
    assert _guards_intact(big, nbytes)
    assert unique == T and inconsistent == 0 and np.array_equal(np.sort(cells.cpu().numpy(), axis=1), fx["cells"])
    assert cert.defects(cert.certify(fx["perturbed"], cells.cpu().numpy())) == {}


# ------------------------------------------------------------------------- e. output capacity -------------------------------------------------------------------------
def test_rows_past_the_output_capacity_are_counted_and_not_written():
    """radegs_delaunay_emit on random1000 with room for 0, 1, T - 1 and T rows in a guarded buffer.  On an MI355X: 0.63 s."""
    import delaunay
    import geom_host as gh
    from diff_gaussian_rasterization import _C
    fx = load("random1000")
    p = dev(fx["points"]).double()
    bounds, _ = delaunay._bounds(p)
    N, T, L = p.shape[0], fx["cells"].shape[0], delaunay._lib()
    want = delaunay.triangulate(p, jitter=0.0)
    assert want.shape[0] == T
    margin = 64
    for out_capacity in (0, 1, T - 1, T):
        big, ws, nbytes, counts = _plan_direct(p, bounds, 25520)              # a fresh plan every time: emit is not asked to run twice on one
        buf = torch.full((T + 2 * margin, 4), -7, dtype=torch.int32, device=DEV)
        counts2 = torch.zeros(2, dtype=torch.int64, device=DEV)
        gh.check(L.radegs_delaunay_emit(N, counts[0], 25520, _C._ptr(ws), nbytes, out_capacity, _C._ptr(buf[margin:]), _C._ptr(counts2), _C._stream(p.device)), "emit")
        assert counts2.tolist() == [T, 0], out_capacity
        assert _guards_intact(big, nbytes)
        assert torch.equal(buf[margin:margin + out_capacity], want[:out_capacity]), out_capacity
        assert bool((buf[:margin] == -7).all()) and bool((buf[margin + out_capacity:] == -7).all()), out_capacity


# ------------------------------------------------------------------------- f. cell capacity -------------------------------------------------------------------------
OUTGREW = "outgrew the 256 faces / 508 triangles"


def _shell(k):
    """("ok", info) with certified rows, or ("refused", None) by the error the API specifies; anything else fails"""
    import delaunay
    points = dev(dc.shell(k))
    try:
        cells, info, X, res = triangulate_and_certify(points)
    except RuntimeError as e:
        assert OUTGREW in str(e), str(e)
        return "refused", None
    assert cert.defects(res) == {}, (k, cert.defects(res))
    assert info["overflow"] == 0 and info["retries"] == 0 and info["inconsistent"] == 0 and info["tets"] == cells.shape[0] == 2 * k - 4
    return "ok", info


def test_slow_cell_capacity_is_a_refusal_never_a_wrong_answer():
    """k unit vectors round the origin: the centre's cell has k faces and 2 k - 4 triangles.  Up to 200 it must be returned, from 257 it must
    be refused (more faces than a byte numbers); between, either: while a clip runs the hole's rim edges share the triangle array, so a
    cell can be refused a little below its nominal 256 / 508.  That is capacity, not correctness.
    Printed on an MI355X: returned and certified up to k = 255, refused at 256, 257 and 300; 1.06 s for the ten."""
    t0 = time.perf_counter()
    outcome = {k: _shell(k)[0] for k in dc.SHELL_LADDER}
    print("shell ladder:", outcome, "largest returned:", max(k for k, v in outcome.items() if v == "ok"), "seconds %.2f" % (time.perf_counter() - t0))
    for k, v in outcome.items():
        assert v == "ok" or k > 200, k
        assert v == "refused" or k < 257, k


def test_fast_cell_capacity_defers_the_centre():
    """the same round the fast kernel's 48 faces / 92 triangles: every shell point is a hull point and deferred, the centre is deferred once
    its cell outgrows the fast kernel's, and the rows certify either way.
    Printed on an MI355X: deferred 40, 47, 49, 50, 61 for k = 40, 47, 48, 49, 60: the centre is deferred from k = 48; 0.07 s."""
    t0 = time.perf_counter()
    deferred = {}
    for k in dc.FAST_LADDER:
        outcome, info = _shell(k)
        assert outcome == "ok", k
        deferred[k] = info["deferred"]
        assert info["deferred"] in (k, k + 1), (k, info)
    print("fast ladder, deferred:", deferred, "centre deferred from k =", min([k for k, d in deferred.items() if d == k + 1], default=None),
          "seconds %.2f" % (time.perf_counter() - t0))


# ------------------------------------------------------------------------- g. retry ladder -------------------------------------------------------------------------
RUNGS = (1e-18, 1e-17, 1e-16, 1e-15, 1e-14, 1e-13, 1e-12)


def test_retry_ladder_returns_strictly_delaunay_rows_or_refuses_after_two_retries():
    """the exact 4 x 4 x 4 grid under jitters from below the coordinates' last bit upwards: every call returns rows that are strictly
    Delaunay (no cospherical neighbour either) on the coordinates its `retries` names, or raises after exactly two retries.
    Printed on an MI355X: 1e-18 to 1e-14 refused after two retries; 1e-13 and 1e-12 returned after one retry (8 and 2 uncertain values in
    the attempt returned) and certified; 0.46 s.  No rung or seed had to be added."""
    import delaunay
    t0 = time.perf_counter()
    points = dev(load("grid64")["points"])
    outcome = {}
    for jitter in RUNGS:
        try:
            cells, info, X, res = triangulate_and_certify(points, jitter=jitter)
        except RuntimeError as e:
            assert "degenerate at this jitter" in str(e) and ", 2 retries)" in str(e), str(e)
            outcome[jitter] = "refused"
            continue
        outcome[jitter] = (info["retries"], info["uncertain"], cert.defects(res))
        assert info["inconsistent"] == 0 and info["overflow"] == 0 and info["tets"] == cells.shape[0] and 0 <= info["retries"] <= 2
    print("retry ladder:", outcome, "seconds %.2f" % (time.perf_counter() - t0))
    for jitter, v in outcome.items():
        assert v == "refused" or v[2] == {}, (jitter, v)
    assert any(v == "refused" or v[0] >= 1 for v in outcome.values())


# ------------------------------------------------------------------------- h. order -------------------------------------------------------------------------
def test_a_permuted_cloud_of_5000_gives_the_same_tetrahedra():
    """On an MI355X: 33 034 tetrahedra either way, both certified; 0.49 s."""
    import delaunay
    t0 = time.perf_counter()
    p = dc.uniform(5000, 61)
    perm = np.random.default_rng(9).permutation(5000)
    first = delaunay.triangulate(dev(p), jitter=0.0).cpu().numpy()
    second = delaunay.triangulate(dev(p[perm]), jitter=0.0).cpu().numpy()
    assert cert.defects(cert.certify(p.astype(np.float64), first)) == {}
    assert cert.defects(cert.certify(p[perm].astype(np.float64), second)) == {}
    assert np.array_equal(sorted_set(perm[second]), sorted_set(first))
    print("permuted 5000: rows", first.shape[0], "seconds %.2f" % (time.perf_counter() - t0))
