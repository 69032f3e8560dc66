"""CPU tier of the Delaunay tetrahedralisation: tests/delaunay_restatement.py, the NumPy restatement of the perturbation and
of the cell clipping with the four ghost generators, against the scipy fixtures -- the same set of cells, every tetrahedron found by exactly
four cells, and the summed volume equal to the hull's.  The GPU tier compares the kernels with the same fixtures."""
import numpy as np
import pytest

import delaunay_restatement as dr
from delaunay_cases import CASES, load


def test_hash_known_answers():
    """pins the counter hash: the kernel, include/radegs.h and the restatement state the same function"""
    assert [dr.hash_u53(0, c) for c in range(3)] == [0x1C4415072F63B9, 0xDCF13CD54372C, 0xD88BA3100128]
    assert dr.hash_u53(7, 12345) == 0x1908E7D0567681
    assert dr.hash_u53(2 ** 63 - 1, 3 * (2 ** 31 - 9) + 2) == 0xE3F8544C965CC


def test_ghost_directions_are_a_regular_tetrahedron():
    d = dr.GHOST_DIRECTIONS
    assert np.allclose(d @ d.T, np.full((4, 4), -1.0 / 3.0) + np.eye(4) * 4.0 / 3.0, atol=1e-15)
    assert np.abs(d).min() > 0.01                 # none parallel to a coordinate plane


@pytest.mark.parametrize("name", list(CASES))
def test_perturbation_matches_the_fixture(name):
    fx = load(name)
    got = dr.perturbed(fx["points"], float(fx["jitter"]), int(fx["seed"]))
    assert got.dtype == np.float64 and np.array_equal(got, fx["perturbed"])
    if float(fx["jitter"]) == 0:
        assert np.array_equal(got, fx["points"].astype(np.float64))
    else:
        diag = dr.diagonal(fx["points"].astype(np.float64))
        moved = np.abs(got - fx["points"])
        assert 0 < moved.max() <= 0.5 * float(fx["jitter"]) * diag * (1 + 1e-6) + np.abs(fx["points"]).max() * 2.0 ** -52


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_scipy(name):
    fx = load(name)
    X = fx["perturbed"]
    cells, found = dr.triangulate(X)
    assert cells.dtype == np.int32 and (found == 4).all()
    assert np.array_equal(np.sort(cells, axis=1), fx["cells"])
    a, b, c, d = (X[cells[:, k]] for k in range(4))
    assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), d - a) > 0).all()
    hull = float(fx["hull_volume"])
    assert abs(dr.volume(X, cells) - hull) <= 1e-9 * hull


def test_box_corners_are_exactly_degenerate_without_jitter():
    """why the jitter exists: the unperturbed box-corner cloud holds exact degeneracies (the corners of a box are cospherical, its faces
    exact parallelograms in float32), its cells do not agree on the tetrahedra, and triangulate(points, jitter=0) has to refuse it"""
    _, found = dr.triangulate(load("boxes270")["points"].astype(np.float64))
    assert (found != 4).any()
