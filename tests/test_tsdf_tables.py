"""The generated marching-cubes table of the TSDF extraction (rade-gs_amd/csrc/rg_mc_tables.h, scripts/make_mc_tables.py): the committed
header is what the generator writes, and every one of the 256 cases obeys the face rule -- restated here from the table's own edge
list, not through the generator's code."""
import importlib.util
import os

import numpy as np
import pytest

import tsdf_restatement as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    return tr.load_tables()


def edge_corners(T, e):
    dx, dy, dz, axis = (int(v) for v in T["edge_info"][e])
    far = [dx, dy, dz]
    far[axis] += 1
    return (dx, dy, dz), tuple(far)


def negative(case, corner):
    return (case >> (corner[0] | (corner[1] << 1) | (corner[2] << 2))) & 1 == 1


def cut_edges(T, case):
    return {e for e in range(12) if negative(case, edge_corners(T, e)[0]) != negative(case, edge_corners(T, e)[1])}


def face_rule(T, case):
    """per face (axis, side): the set of undirected segments {edge, edge} the rule prescribes"""
    out = {}
    for axis in range(3):
        for side in (0, 1):
            on_face = [e for e in range(12) if all(c[axis] == side for c in edge_corners(T, e))]
            assert len(on_face) == 4
            cut = [e for e in on_face if e in cut_edges(T, case)]
            segs = set()
            if len(cut) == 2:
                segs.add(frozenset(cut))
            elif len(cut) == 4:
                corners = {c for e in on_face for c in edge_corners(T, e)}
                for c in corners:
                    if negative(case, c):
                        segs.add(frozenset(e for e in on_face if c in edge_corners(T, e)))
            else:
                assert not cut
            assert all(len(s) == 2 for s in segs)
            out[(axis, side)] = segs
    return out


def case_triangles(T, case):
    row = [int(v) for v in T["tri"][case]]
    n = int(T["ntri"][case])
    assert all(v >= 0 for v in row[:3 * n]) and all(v == -1 for v in row[3 * n:]), case
    return [tuple(row[3 * t:3 * t + 3]) for t in range(n)]


def test_header_is_what_the_generator_writes():
    spec = importlib.util.spec_from_file_location("make_mc_tables", os.path.join(ROOT, "scripts", "make_mc_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(tr.TABLE_HEADER) as fh:
        assert fh.read() == gen.render()
    assert gen.tables()[1] * 3 + 1 == tr.load_tables()["tri"].shape[1]


def test_edge_list_is_the_ownership_the_kernels_assume(T):
    """edge e = 4 * axis + a + 2 * b leaves the corner whose other two coordinates are (a, b), along `axis`"""
    for e in range(12):
        dx, dy, dz, axis = (int(v) for v in T["edge_info"][e])
        assert axis == e // 4 and (dx, dy, dz)[axis] == 0
        others = [c for k, c in enumerate((dx, dy, dz)) if k != axis]
        assert others == [e & 1, (e >> 1) & 1]
    assert len({edge_corners(T, e) for e in range(12)}) == 12


def test_empty_cases(T):
    assert T["ntri"][0] == 0 and T["ntri"][255] == 0
    assert (T["tri"][0] == -1).all() and (T["tri"][255] == -1).all()
    assert T["edge_mask"][0] == 0 and T["edge_mask"][255] == 0


def test_every_case_uses_exactly_its_cut_edges(T):
    for case in range(256):
        cut = cut_edges(T, case)
        assert int(T["edge_mask"][case]) == sum(1 << e for e in cut), case
        used = {e for t in case_triangles(T, case) for e in t}
        assert used == cut, case
        assert all(len(set(t)) == 3 for t in case_triangles(T, case)), case


def test_open_boundary_is_the_face_rule(T):
    """the edges of a case's triangles that belong to one triangle only are exactly the segments the rule draws on the six faces (each
    once); every other edge joins two triangles that run along it in opposite directions"""
    for case in range(256):
        directed = [(t[k], t[(k + 1) % 3]) for t in case_triangles(T, case) for k in range(3)]
        assert len(set(directed)) == len(directed), case
        boundary = [d for d in directed if (d[1], d[0]) not in directed]
        prescribed = [s for segs in face_rule(T, case).values() for s in segs]
        assert len(set(prescribed)) == len(prescribed), case          # no segment on two faces
        assert sorted(sorted(s) for s in prescribed) == sorted(sorted(d) for d in boundary), case


def test_complementary_cases(T):
    """The complement draws the same segment on every face with two cuts, in the opposite direction.  On a face with four cuts it draws the
    other pairing: the rule cuts off the negative corners, and the complement's negative corners are the other diagonal.  (Both cells at
    such a face see the same four signs, so they still agree with each other.)"""
    for case in range(256):
        mine, other = face_rule(T, case), face_rule(T, 255 - case)
        d_mine = {(t[k], t[(k + 1) % 3]) for t in case_triangles(T, case) for k in range(3)}
        d_other = {(t[k], t[(k + 1) % 3]) for t in case_triangles(T, 255 - case) for k in range(3)}
        for face, segs in mine.items():
            if len(segs) == 1:
                assert other[face] == segs, (case, face)
                a, b = sorted(next(iter(segs)))
                assert ((a, b) in d_mine) != ((a, b) in d_other) and ((b, a) in d_mine) != ((b, a) in d_other), (case, face)
            elif len(segs) == 2:
                assert len(other[face]) == 2 and not (other[face] & segs), (case, face)
                assert set().union(*segs) == set().union(*other[face]), (case, face)


def test_loops_face_the_positive_side(T):
    """a single negative corner: its triangle's normal points away from it"""
    mid = lambda e: np.mean(np.array(edge_corners(T, e), np.float64), 0)
    for corner in range(8):
        (t,) = case_triangles(T, 1 << corner)
        a, b, c = (mid(e) for e in t)
        inside = np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1], np.float64)
        assert np.dot(np.cross(b - a, c - a), a - inside) > 0, corner
        # and the complement, a single positive corner: towards it
        (t,) = case_triangles(T, 255 - (1 << corner))
        a, b, c = (mid(e) for e in t)
        assert np.dot(np.cross(b - a, c - a), inside - a) > 0, corner
