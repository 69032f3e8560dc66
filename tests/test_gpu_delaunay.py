"""GPU tier of the Delaunay tetrahedralisation: delaunay.triangulate and the HIP kernels under it against the scipy fixtures
(tests/golden/make_golden_delaunay.py).  Exact throughout: the perturbed coordinates bit for bit, the cells as a set of index quadruples, no
inconsistent tetrahedron and no uncertain predicate; a Delaunay triangulation of points in general position is unique, so no tolerance applies."""
import numpy as np
import pytest
import torch

from delaunay_cases import CASES, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_results = {}


def run(name):
    """(cells as numpy, info, cells tensor) of a fixture: computed once, shared, never modified"""
    import delaunay
    if name not in _results:
        fx = load(name)
        cells, info = delaunay.triangulate(dev(fx["points"]), jitter=float(fx["jitter"]), seed=int(fx["seed"]), return_info=True)
        _results[name] = (cells.cpu().numpy(), info, cells)
    return _results[name]


def check_rows(cells, X):
    """unique, in lexicographic order of the ascending quadruple, that quadruple with at most the last two exchanged, positively oriented"""
    asc = np.sort(cells, axis=1)
    assert np.array_equal(cells[:, :2], asc[:, :2]) and np.array_equal(np.sort(cells[:, 2:], axis=1), asc[:, 2:])
    assert (asc[:, :-1] < asc[:, 1:]).all()
    order = np.lexsort(asc.T[::-1])
    assert np.array_equal(order, np.arange(asc.shape[0])) and np.unique(asc, axis=0).shape[0] == asc.shape[0]
    a, b, c, d = (X[cells[:, k]] for k in range(4))
    assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), d - a) > 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_perturbed_equals_the_fixture_bit_for_bit(name):
    import delaunay
    fx = load(name)
    got = delaunay.perturbed(dev(fx["points"]), float(fx["jitter"]), int(fx["seed"]))
    assert got.dtype == torch.float64 and got.device == torch.device(DEV)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), fx["perturbed"].view(np.uint64))


@pytest.mark.parametrize("name", list(CASES))
def test_cells_equal_scipy(name):
    fx = load(name)
    cells, info, tensor = run(name)
    print(name, info)
    assert tensor.dtype == torch.int32 and tensor.device == torch.device(DEV) and tensor.is_contiguous()
    assert set(info) == {"tets", "inconsistent", "uncertain", "deferred", "overflow", "retries"}
    assert info["inconsistent"] == 0 and info["uncertain"] == 0 and info["overflow"] == 0 and info["retries"] == 0
    assert info["tets"] == cells.shape[0] == CASES[name][1]
    assert np.array_equal(np.sort(cells, axis=1), fx["cells"])
    check_rows(cells, fx["perturbed"])
    assert 0 <= info["deferred"] <= CASES[name][0]


def test_which_kernel_finished_the_points():
    assert run("shell151")[1]["deferred"] >= 1              # the centre's 150-face cell outgrows the fast kernel's 48
    assert run("sphere120")[1]["deferred"] == 120           # every point is on the hull
    for name in ("random4", "random5", "random8"):
        assert run(name)[1]["deferred"] == CASES[name][0]
    assert run("random1000")[1]["deferred"] < 1000          # the fast kernel finishes interior points


def test_two_calls_give_the_same_bits_and_the_dtype_of_the_input_does_not_matter():
    import delaunay
    fx = load("random1000")
    first = run("random1000")[2]
    again = delaunay.triangulate(dev(fx["points"]), jitter=0.0)
    assert torch.equal(first, again)
    assert torch.equal(first, delaunay.triangulate(dev(fx["points"].astype(np.float64)), jitter=0.0))
    box = load("boxes270")
    assert torch.equal(run("boxes270")[2], delaunay.triangulate(dev(box["points"])))                     # the defaults are the fixture's jitter and seed
    assert torch.equal(run("boxes270")[2], delaunay.triangulate(dev(box["points"]).double()))


def test_a_permuted_input_gives_the_same_tetrahedra():
    import delaunay
    fx = load("random200")
    perm = np.random.default_rng(9).permutation(200)
    cells = delaunay.triangulate(dev(fx["points"][perm]), jitter=0.0).cpu().numpy()
    back = np.unique(np.sort(perm[cells], axis=1), axis=0)
    assert np.array_equal(back, fx["cells"])
    check_rows(cells, fx["points"][perm].astype(np.float64))


def test_exactly_degenerate_input_is_refused_without_jitter():
    """The unperturbed box-corner cloud is exactly degenerate: the restatement's cells disagree on it (tests/test_delaunay_restatement.py) and
    so do the same cells clipped in index order on the host (tests/test_delaunay_api.py).  In the kernels' clipping order 1 039 predicate
    values are within their error bound, and the cells happen to fit together all the same; a refusal that depended on that luck would
    depend on the order of the points, so jitter=0 refuses any input on which a tie was met, in whatever order it is given.  The 4 x 4 x 4
    grid without jitter is inconsistent outright."""
    import delaunay
    box = load("boxes270")["points"]
    perm = np.random.default_rng(5).permutation(box.shape[0])
    for points in (box, box[perm], load("grid64")["points"]):
        with pytest.raises(RuntimeError, match="degenerate"):
            delaunay.triangulate(dev(points), jitter=0.0)
    # the same clouds with the default jitter are fine, and jitter=0 on points in general position is too
    assert delaunay.triangulate(dev(box[perm])).shape[0] > 1500


def test_too_few_points_and_non_finite_values_are_refused():
    import delaunay
    good = load("random8")["points"]
    for fn in (delaunay.triangulate, delaunay.perturbed):
        with pytest.raises(RuntimeError, match="at least 4 points"):
            fn(dev(good[:3]))
        for bad in (np.nan, np.inf, -np.inf):
            p = good.copy()
            p[5, 1] = bad
            with pytest.raises(RuntimeError, match="non-finite"):
                fn(dev(p))
            with pytest.raises(RuntimeError, match="non-finite"):
                fn(dev(p.astype(np.float64)))


def test_the_shim_returns_the_same_cells():
    from tetranerf.utils.extension import cpp
    got = cpp.triangulate(dev(load("boxes270")["points"]))
    assert got.dtype == torch.int32 and got.device == torch.device(DEV) and torch.equal(got, run("boxes270")[2])


def test_route_tetra_points_to_triangulate_to_marching_tetrahedra():
    """40 synthetic Gaussians -> their 360 box points -> tetrahedra -> marching tetrahedra on the signed distance to a sphere"""
    import delaunay
    import tetmesh
    rng = np.random.default_rng(11)
    xyz = dev((rng.random((40, 3)) * 2 - 1).astype(np.float32))
    scales = dev((0.05 + 0.1 * rng.random((40, 3))).astype(np.float32))
    rot = dev(rng.normal(size=(40, 4)).astype(np.float32))
    points, points_scale = tetmesh.tetra_points(xyz, scales, rot)
    assert points.shape == (360, 3)
    cells, info = delaunay.triangulate(points, return_info=True)
    assert info["inconsistent"] == 0 and cells.shape[0] == info["tets"] > 360
    X = delaunay.perturbed(points).cpu().numpy()
    check_rows(cells.cpu().numpy(), X)
    a, b, c, d = (X[cells.cpu().numpy()[:, k]] for k in range(4))
    from scipy.spatial import ConvexHull
    hull = ConvexHull(X).volume
    assert abs(np.einsum("ij,ij->i", np.cross(b - a, c - a), d - a).sum() / 6.0 - hull) <= 1e-9 * hull      # the tetrahedra fill the hull exactly once
    sdf = points.norm(dim=1) - 0.7
    out = tetmesh.marching_tetrahedra(points[None], cells, sdf[None], points_scale[None])
    faces, n_vertices = out[2][0], out[0][0][0].shape[0]
    assert faces.shape[0] > 0 and faces.shape[1] == 3 and int(faces.min()) >= 0 and int(faces.max()) < n_vertices
