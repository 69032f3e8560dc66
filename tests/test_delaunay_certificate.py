"""CPU tier of the Delaunay scale tests: tests/delaunay_certificate.py, the exact reference-free certificate the GPU tier
(tests/test_gpu_delaunay_scale.py) holds the kernels to, is itself held to account here -- it accepts what is Delaunay (the twelve
fixtures; scipy's result on the clouds where Qhull is exact), rejects six kinds of wrong rows each by the counter that names the fault, and
its two predicates agree with brute-force rational arithmetic; and the generated clouds of tests/delaunay_cases.py have the properties
the GPU tests rely on (grid shape, cell population, record count, degree).  scipy is a cross-check, never the verdict: on the clustered
cloud Qhull's own rows fail the certificate, which this file prints and does not assert (DESIGN 11 N13 records the counts)."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.spatial as scipy_spatial

import delaunay_cases as dc
import delaunay_certificate as cert
import delaunay_restatement as dr

JITTER, SEED = 1e-9, 0
_scipy = {}


def scipy_result(name):
    """(X, scipy's rows oriented on X, certify's result) of a generated cloud: computed once, shared, never modified"""
    if name not in _scipy:
        X = dr.perturbed(dc.cloud(name), JITTER, SEED)
        cells = dr.orient(X, np.unique(np.sort(scipy_spatial.Delaunay(X).simplices, axis=1), axis=0))
        res = cert.certify(X, cells, cross_check=True)
        print(name, "scipy:", cells.shape[0], "rows, defects", cert.defects(res), "exact evaluations", res["exact"], "hull faces", res["hull_faces"],
              "ConvexHull agrees", res["scipy_hull_agrees"])
        X.setflags(write=False), cells.setflags(write=False)
        _scipy[name] = (X, cells, res)
    return _scipy[name]


# ------------------------------------------------------------------------- the predicates -------------------------------------------------------------------------
def test_filtered_signs_equal_rational_arithmetic_and_the_circumcentre_is_inside():
    rng = np.random.default_rng(3)
    X = rng.random((40, 3))
    X[20:] = X[:20] + 1e-15 * rng.normal(size=(20, 3))                       # near-copies: determinants below the filter
    X[30:] += np.array([1e6, -2e6, 3e6])
    idx = rng.integers(0, 40, size=(400, 5))
    idx = idx[[len(set(r)) == 5 for r in idx.tolist()]]
    sg = cert.Signs(X)
    o = sg.orient(*idx[:, :4].T)
    s = sg.insphere(*idx.T)
    for r, oo, ss in zip(idx.tolist(), o, s):
        F = [[Fraction(float(v)) for v in X[i]] for i in r]
        det4 = _det([[1] + F[k] for k in range(4)])
        assert oo == (det4 > 0) - (det4 < 0)
        det5 = _det([[1] + F[k] + [sum(v * v for v in F[k])] for k in range(5)])      # the textbook lifted determinant, expanded independently
        assert ss == ((det5 * det4 < 0) - (det5 * det4 > 0)), r
    assert sg.exact > 0                                                        # both paths ran
    # an exactly cospherical point and the exact circumcentre of an integer tetrahedron
    Y = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0, 0, -1.0], [0, 0, 0], [0, 0, 1.5]])
    sg = cert.Signs(Y)
    assert sg.insphere([0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 5, 6]).tolist() == [0, 1, -1]
    assert sg.orient([0], [1], [2], [5]).tolist() == [0]


def _det(m):
    """Laplace expansion along the first column, in whatever arithmetic the entries bring"""
    if len(m) == 1:
        return m[0][0]
    return sum((-1) ** i * m[i][0] * _det([row[1:] for k, row in enumerate(m) if k != i]) for i in range(len(m)) if m[i][0] != 0)


# ------------------------------------------------------------------------- acceptance -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.CASES))
def test_certificate_accepts_every_fixture(name):
    fx = dc.load(name)
    res = cert.certify(fx["perturbed"], dr.orient(fx["perturbed"], fx["cells"]), cross_check=True)
    print(name, res)
    assert cert.defects(res) == {} and res["scipy_hull_agrees"] is not False
    assert abs(res["volume"] - float(fx["hull_volume"])) <= 1e-9 * float(fx["hull_volume"])


@pytest.mark.parametrize("name", ["uniform50k", "surface20k", "boxes2000", "lines200a", "lines200b"])
def test_certificate_accepts_scipy_where_qhull_is_exact(name):
    assert cert.defects(scipy_result(name)[2]) == {}


# ------------------------------------------------------------------------- rejection -------------------------------------------------------------------------
def _canonical(X, quads):
    """rows as triangulate writes them: ascending, in lexicographic order, oriented"""
    q = np.sort(np.asarray(quads, dtype=np.int64), axis=1)
    return dr.orient(X, q[np.lexsort(q.T[::-1])])


def _good():
    fx = dc.load("random1000")
    X = fx["perturbed"]
    return X, dr.orient(X, fx["cells"]).astype(np.int64)


def _flip23(X, cells):
    """the rows with one interior face (a, b, c) between (a, b, c, d) and (a, b, c, e) replaced by the edge d e: three tetrahedra filling
    the same convex region.  A valid triangulation of the same hull that is not Delaunay."""
    sg = cert.Signs(X)
    asc = np.sort(cells, axis=1)
    face, opp, row = cert._faces(asc)
    order, start, length = cert._group([face[:, 0], face[:, 1], face[:, 2]], X.shape[0])
    for s in start[length == 2]:
        i, j = order[s], order[s + 1]
        (a, b, c), d, e = face[i], opp[i], opp[j]
        sides = sg.orient([d, d, d], [e, e, e], [a, b, c], [b, c, a])
        if abs(int(sides.sum())) == 3:                                         # the segment d e passes through the inside of the triangle
            rest = np.delete(asc, [row[i], row[j]], axis=0)
            return _canonical(X, np.concatenate([rest, [[a, b, d, e], [b, c, d, e], [a, c, d, e]]]))
    raise AssertionError("no flippable face")


def test_certificate_rejects_a_bistellar_flip_by_the_local_delaunay_counter_alone():
    X, cells = _good()
    flipped = _flip23(X, cells)
    assert flipped.shape[0] == cells.shape[0] + 1
    d = cert.defects(cert.certify(X, flipped))
    print(d)
    assert set(d) == {"not_delaunay"} and 1 <= d["not_delaunay"] <= 9          # the three faces at the new edge, perhaps the six round it


def _interior_row(X, cells):
    """a row none of whose faces is on the hull and whose corners all have other rows"""
    face, opp, row = cert._faces(np.sort(cells, axis=1))
    order, start, length = cert._group([face[:, 0], face[:, 1], face[:, 2]], X.shape[0])
    on_hull = np.zeros(cells.shape[0], dtype=bool)
    on_hull[row[order[start[length == 1]]]] = True
    return int(np.nonzero(~on_hull)[0][len(cells) // 3])


def test_certificate_rejects_a_missing_row():
    """the hole's four faces occur once: they close a surface of their own and the volumes still agree, but the missing row's fourth corner
    is strictly outside each of them"""
    X, cells = _good()
    d = cert.defects(cert.certify(X, np.delete(cells, _interior_row(X, cells), axis=0)))
    print(d)
    assert set(d) == {"outside"} and d["outside"] >= 4
    d = cert.defects(cert.certify(X, cells[1:]))                               # a row at the hull: the surface dents inwards
    print(d)
    assert "outside" in d and set(d) <= {"outside", "uncovered"}


def test_certificate_rejects_a_duplicated_row():
    X, cells = _good()
    k = _interior_row(X, cells)
    assert cert.defects(cert.certify(X, np.insert(cells, k, cells[k], axis=0))) == {"duplicate": 1}


def test_certificate_rejects_a_row_with_its_last_two_entries_exchanged():
    X, cells = _good()
    bad = cells.copy()
    bad[77, 2:] = bad[77, [3, 2]]
    assert cert.defects(cert.certify(X, bad)) == {"orientation": 1}
    bad = cells.copy()
    bad[77, :2] = bad[77, [1, 0]]                                              # the first two: the format forbids it
    assert cert.defects(cert.certify(X, bad)) == {"format": 1, "orientation": 1}


def test_certificate_rejects_the_triangulation_of_all_points_but_one():
    X, _ = _good()
    X = np.concatenate([X, [[0.5, 0.5, 0.5]]])                                 # the last point is interior: the hull and the rows stay valid
    fewer = dr.orient(X, np.unique(np.sort(scipy_spatial.Delaunay(X[:-1]).simplices, axis=1), axis=0))
    assert cert.defects(cert.certify(X[:-1], fewer)) == {}
    assert cert.defects(cert.certify(X, fewer)) == {"uncovered": 1}
    X[-1] = [2.0, 0.5, 0.5]                                                    # a hull point left out is outside what the rows cover, too
    d = cert.defects(cert.certify(X, fewer))
    assert set(d) == {"uncovered", "outside"} and d["uncovered"] == 1 and d["outside"] >= 1


def test_certificate_rejects_the_cells_of_a_permuted_cloud():
    """rows in perfect format that belong to the same points in another order: every geometric counter fires, no format counter does"""
    X, cells = _good()
    perm = np.random.default_rng(9).permutation(X.shape[0])
    d = cert.defects(cert.certify(X[perm], cells))
    print(d)
    assert not set(d) & {"format", "range", "order", "duplicate", "uncovered", "face_multiplicity", "hull_open"}
    assert {"orientation", "face_sides", "outside", "cover", "not_delaunay"} <= set(d)
    assert d["orientation"] > cells.shape[0] // 4 and d["not_delaunay"] > cells.shape[0] // 4


def test_certificate_counts_format_faults():
    X, cells = _good()
    bad = cells.copy()
    bad[5, 3] = X.shape[0]
    d = cert.defects(cert.certify(X, bad))
    assert d["range"] == 1 and set(d) <= {"range", "order"}                    # nothing geometric is said of such rows
    swapped = cells.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    assert cert.defects(cert.certify(X, swapped)) == {"order": 1}
    assert cert.defects(cert.certify(X, np.zeros((0, 4), dtype=np.int32)))["uncovered"] == X.shape[0]
    grid = dc.load("grid64")                                                   # the exact 4 x 4 x 4 grid with any rows: ties are exact zeros
    res = cert.certify(grid["points"].astype(np.float64), dr.orient(grid["perturbed"], grid["cells"]))
    print("grid64 rows on the unperturbed grid:", cert.defects(res), res["exact"])
    assert res["cospherical"] > 0 and res["exact"] > 0


# ------------------------------------------------------------------------- the clouds' properties -------------------------------------------------------------------------
def _bounds(X):
    return list(X.min(axis=0)) + list(X.max(axis=0))


def test_uniform50k_fits_the_first_record_capacity():
    X, cells, _ = scipy_result("uniform50k")
    N = X.shape[0]
    assert N == 50000 and 4 * cells.shape[0] <= 32 * N + 1024
    lo, h, dim = dc.make_grid(N, _bounds(X))
    assert dim == [30, 30, 30]                                                 # 30 > 2 kShellMax + 1: the shell termination decides, not the grid's end


def test_slab20k_has_a_one_dimensional_grid():
    X = dr.perturbed(dc.cloud("slab20k"), JITTER, SEED)
    lo, h, dim = dc.make_grid(20000, _bounds(X))
    assert dim == [22, 1, 1] and dim[0] == int(np.ceil(np.cbrt(10000)))
    assert np.bincount(dc.cell_keys(X, (lo, h, dim)), minlength=22).min() > 500


def test_clustered20k_has_one_crowded_cell_and_scipy_is_printed_not_trusted():
    p = dc.cloud("clustered20k")
    X = dr.perturbed(p, JITTER, SEED)
    grid = dc.make_grid(20000, _bounds(X))
    assert grid[2] == [22, 22, 22] and np.bincount(dc.cell_keys(X, grid)).max() >= 17000
    X, cells, res = scipy_result("clustered20k")
    print("clustered20k: scipy", scipy_spatial.__name__, "defects:", cert.defects(res))


def test_slab_and_duplicates_print_what_scipy_gives():
    for name in ("slab20k", "dup200"):
        scipy_result(name)
    p = dc.cloud("dup200")
    assert p.shape == (200, 3) and np.array_equal(p[0::2], p[1::2]) and np.unique(p, axis=0).shape[0] == 100


def test_boxes2000_restated_is_18000_exactly_degenerate_points():
    p = dc.cloud("boxes2000")
    assert p.shape == (18000, 3) and p.dtype == np.float32
    corners = p[:16000].reshape(2000, 8, 3).astype(np.float64)
    assert np.abs(corners.mean(axis=1) - p[16000:]).max() < 1e-6             # eight corners about their centre


@pytest.mark.parametrize("name", ["lines200a", "lines200b"])
def test_two_lines_outgrow_the_first_record_capacity(name):
    X, cells, _ = scipy_result(name)
    degree = dc.vertex_degrees(200, cells)
    print(name, "4T =", 4 * cells.shape[0], "largest degree", int(degree.max()))
    assert 4 * cells.shape[0] > 32 * 200 + 1024 == 7424 and degree.max() <= 200


@pytest.mark.parametrize("k", dc.SHELL_LADDER + dc.FAST_LADDER)
def test_shell_centre_has_k_neighbours(k):
    p = dc.shell(k)
    X = dr.perturbed(p, JITTER, SEED)
    cells = dr.orient(X, np.unique(np.sort(scipy_spatial.Delaunay(X).simplices, axis=1), axis=0))
    assert cert.defects(cert.certify(X, cells)) == {}
    assert dc.vertex_degrees(k + 1, cells)[k] == k and int((cells == k).any(axis=1).sum()) == 2 * k - 4 == cells.shape[0]
