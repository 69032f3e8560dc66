"""CPU tier of the mesh simplification: tests/simplify_restatement.py, which the GPU tests hold the kernels to bit for bit, checked here against
things that are not it -- plain Python loops for the cells, the per-cell sums and the faces, np.linalg for the eigenvalues, and the geometry the
quadric position is there for: it never has more quadric error than the mean, it finds a crease, and it keeps a plane planar."""
import math

import numpy as np
import pytest

import simplify_cases as sc
import simplify_restatement as sr


def _cells_by_dict(c):
    v = c.vertices
    origin = [v[:, a].min() - c.h / 2.0 for a in range(3)] if c.origin is None else list(c.origin)
    coords = [tuple(math.floor((float(p[a]) - origin[a]) / c.h) for a in range(3)) for p in v]
    number = {t: k for k, t in enumerate(sorted(set(coords)))}
    return [number[t] for t in coords], sorted(set(coords))


@pytest.mark.parametrize("name", sc.NAMES)
def test_cells_equal_a_dictionary_loop(name):
    c, want = sc.CASES[name], sc.reference(name)
    cell, coords = _cells_by_dict(c)
    assert want["K"] == len(coords) and want["vertex_cell"].tolist() == cell
    assert want["cell_key"].tolist() == [x << 42 | y << 21 | z for x, y, z in coords]


@pytest.mark.parametrize("name", sc.NAMES)
def test_per_cell_sums_equal_a_sequential_loop(name):
    c, want = sc.CASES[name], sc.reference(name)
    K, cell = want["K"], want["vertex_cell"].tolist()
    sums, counts = [[0.0, 0.0, 0.0] for _ in range(K)], [0] * K
    for i, p in enumerate(c.vertices.tolist()):
        counts[cell[i]] += 1
        for a in range(3):
            sums[cell[i]][a] += p[a]
    assert want["averages"].tolist() == [[s / n for s in row] for row, n in zip(sums, counts)]
    fq = sr.face_quadrics(c.vertices, c.faces).tolist()
    Q = [[0.0] * 10 for _ in range(K)]
    for t, row in enumerate(c.faces.tolist()):
        for corner in row:                                   # ascending (triangle, corner)
            for e in range(10):
                Q[cell[corner]][e] += fq[t][e]
    assert want["quadrics"].tolist() == Q
    if c.attributes is not None:
        A = c.attributes.shape[1]
        sums = [[0.0] * A for _ in range(K)]
        for i, p in enumerate(c.attributes.tolist()):
            for a in range(A):
                sums[cell[i]][a] += p[a]
        assert want["attributes"].tolist() == [[s / n for s in row] for row, n in zip(sums, counts)]


def test_face_quadrics_are_the_weighted_plane_products():
    c = sc.CASES["bumpy_coloured"]
    fq = sr.face_quadrics(c.vertices, c.faces)
    a, b, d = (c.vertices[c.faces[:, k]] for k in range(3))
    n = np.cross(b - a, d - a)
    area = 0.5 * np.linalg.norm(n, axis=1)
    plane = np.concatenate([n / np.linalg.norm(n, axis=1)[:, None], -np.einsum("ij,ij->i", n / np.linalg.norm(n, axis=1)[:, None], a)[:, None]], 1)
    full = area[:, None, None] * plane[:, :, None] * plane[:, None, :]
    want = np.stack([full[:, i, j] for i, j in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))], 1)
    assert np.allclose(fq, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    c = sc.CASES["degenerate_triangles"]
    fq = sr.face_quadrics(c.vertices, c.faces)
    assert (fq[-5:-1] == 0.0).all() and (fq[-1] != 0.0).any() and np.isfinite(fq).all()         # zero area, equal indices: nothing


@pytest.mark.parametrize("name", sc.NAMES)
def test_jacobi_finds_the_eigenvalues_and_an_orthonormal_basis(name):
    """against np.linalg.eigvalsh: both are backward stable, so the eigenvalues agree to a few roundings of the largest, 1e-14 of it here"""
    Q = sc.reference(name)["quadrics"]
    A = np.stack([Q[:, [0, 1, 2]], Q[:, [1, 4, 5]], Q[:, [2, 5, 7]]], 1)
    lam, R = sr.jacobi(Q)
    R = np.stack([np.stack(row, 1) for row in R], 1)                                             # [K,3,3], columns the eigenvectors
    scale = np.abs(A).max((1, 2))[:, None] + 1e-300
    assert (np.abs(np.sort(lam, 1) - np.linalg.eigvalsh(A)) <= 1e-14 * scale).all()
    assert np.abs(np.einsum("kji,kjl->kil", R, R) - np.eye(3)).max() <= 1e-14
    assert (np.abs(np.einsum("kij,kjl->kil", A, R) - R * lam[:, None, :]) <= 1e-14 * scale[:, :, None]).all()


def _error_scale(Q, x):
    A = np.abs(np.stack([Q[:, [0, 1, 2]], Q[:, [1, 4, 5]], Q[:, [2, 5, 7]]], 1))
    return np.einsum("ki,kij,kj->k", np.abs(x), A, np.abs(x)) + 2.0 * (np.abs(Q[:, [3, 6, 8]]) * np.abs(x)).sum(1) + np.abs(Q[:, 9])


def test_the_quadric_position_never_has_more_error_than_the_mean():
    """E(x) <= E(m) up to the rounding of E itself.  Margin: 8e-16 of sum |terms of E(m)|.  Measured on the restatement over all cases: the worst
    E(x) - E(m) is 1.32e-16 of that scale (fans); the margin is six times the measured worst, rounded."""
    worst = 0.0
    for name in sc.NAMES:
        s = sc.reference(name)
        Q, m, x = s["quadrics"], s["averages"], s["positions"]
        excess = (sr.quadric_error(Q, x) - sr.quadric_error(Q, m)) / np.maximum(_error_scale(Q, m), 1e-300)
        worst = max(worst, float(excess.max()))
        assert (excess <= 8e-16).all(), (name, float(excess.max()))
    print("worst E(x) - E(m) over the scale of E(m):", worst)
    moved = sum(int((sc.reference(n)["positions"] != sc.reference(n)["averages"]).any(1).sum()) for n in sc.NAMES)
    assert moved > 500                                                                            # the property is not vacuous


def _roof_distances(p):
    up, down = 3.2 + 0.5 * (p[:, 0] - sc.ROOF_RIDGE), 3.2 - 0.5 * (p[:, 0] - sc.ROOF_RIDGE)
    return np.abs(p[:, 2] - up) / math.sqrt(1.25), np.abs(p[:, 2] - down) / math.sqrt(1.25)


def test_on_a_roof_the_quadric_position_finds_the_crease_and_the_mean_does_not():
    """Margin 4e-14: measured on the restatement, the farthest quadric position of a straddling cell is 9.2e-15 from a plane (coordinates up to
    24, so a few roundings of them); the margin is four times that.  The means of the same cells are 0.298 and more from one of the planes."""
    c, s = sc.CASES["roof"], sc.reference("roof")
    lo, hi = sr.cell_box(s["cell_key"], c.h, s["origin"])
    straddles = (lo[:, 0] < sc.ROOF_RIDGE) & (hi[:, 0] > sc.ROOF_RIDGE)
    assert straddles.sum() == 5
    d_up, d_down = _roof_distances(s["positions"][straddles])
    print("roof: farthest quadric position from a plane:", float(max(d_up.max(), d_down.max())))
    assert d_up.max() <= 4e-14 and d_down.max() <= 4e-14
    assert np.abs(s["positions"][straddles][:, 0] - sc.ROOF_RIDGE).max() <= 4e-14                 # on both planes: on the ridge
    m_up, m_down = _roof_distances(s["averages"][straddles])
    assert np.maximum(m_up, m_down).min() > 0.25
    d_up, d_down = _roof_distances(s["positions"][~straddles])                                    # the other cells stay on their own plane
    assert np.minimum(d_up, d_down).max() <= 4e-14


def test_a_planar_sheet_stays_planar():
    """Margin 4e-14: the farthest position measured on the restatement is 8.0e-15 from the plane (coordinates up to 24); four times that."""
    s = sc.reference("plane")
    for part in ("positions", "averages"):
        p = s[part]
        off = np.abs(p[:, 2] - (0.25 * p[:, 0] - 0.4 * p[:, 1] + 7.0)) / math.sqrt(1.0 + 0.25 ** 2 + 0.4 ** 2)
        print("plane:", part, "farthest from the plane:", float(off.max()))
        assert off.max() <= 4e-14
    assert (s["positions"] != s["averages"]).any()


def test_the_solve_that_leaves_its_cell_falls_back_to_the_mean():
    c, s = sc.CASES["leaves_the_box"], sc.reference("leaves_the_box")
    out, x, solved, kept = sr.solve(s["quadrics"], s["averages"], s["cell_key"], c.h, s["origin"], details=True)
    assert solved.all() and not kept.any() and np.allclose(x[:, 0], 1.55) and np.array_equal(out, s["averages"])
    fallen = 0
    for name in sc.NAMES:                                   # elsewhere both outcomes occur
        c, s = sc.CASES[name], sc.reference(name)
        _, _, solved, kept = sr.solve(s["quadrics"], s["averages"], s["cell_key"], c.h, s["origin"], details=True)
        fallen += int((solved & ~kept).sum())
    assert fallen > 10
    s = sc.reference("unreferenced_cell")                  # a cell without a record: no eigenvalue is positive
    assert (~sr.solve(s["quadrics"], s["averages"], s["cell_key"], 2.0, s["origin"], details=True)[2]).sum() == 1


@pytest.mark.parametrize("remove_duplicates", (True, False))
@pytest.mark.parametrize("name", sc.NAMES)
def test_faces_equal_a_loop_with_a_set(name, remove_duplicates):
    c, s = sc.CASES[name], sc.reference(name)
    cell = s["vertex_cell"].tolist()
    seen, faces, source = set(), [], []
    for t, row in enumerate(c.faces.tolist()):
        a, b, d = (cell[i] for i in row)
        if a == b or b == d or d == a:
            continue
        k = (a, b, d).index(min(a, b, d))
        triple = ((a, b, d) * 2)[k:k + 3]
        if remove_duplicates and triple in seen:
            continue
        seen.add(triple)
        faces.append(triple)
        source.append(t)
    cf, remove = sr.cell_faces(c.faces, s["vertex_cell"], s["K"], remove_duplicates)
    assert np.flatnonzero(~remove).tolist() == source and [tuple(r) for r in cf[~remove].tolist()] == faces
    for drop in (True, False):
        kept, out_f, src = sr.compact(s["K"], cf, remove, drop)
        used = sorted({i for t in faces for i in t}) if drop else list(range(s["K"]))
        assert kept.tolist() == used and src.tolist() == source
        assert [tuple(used[i] for i in r) for r in out_f.tolist()] == faces


def test_the_whole_call_rounds_once_and_maps_every_vertex():
    c = sc.CASES["bumpy_coloured"]
    v32, a32 = c.vertices.astype(np.float32), c.attributes.astype(np.float32)
    out_v, out_f, vmap, source, attr = sr.simplify_vertex_clustering(v32, c.faces, c.h, attributes=a32)
    assert out_v.dtype == np.float32 and attr.dtype == np.float32 and out_f.dtype == np.int64 and vmap.shape == (v32.shape[0],)
    assert 0 < out_f.shape[0] < c.faces.shape[0] / 5 and out_f.max() == out_v.shape[0] - 1
    s = sr.stages(v32, c.faces, c.h, attributes=a32)
    assert np.array_equal(out_v[vmap[vmap >= 0]], s["positions"].astype(np.float32)[s["vertex_cell"][vmap >= 0]])
    assert np.array_equal(vmap[c.faces[source]].min(1), out_f[:, 0])                             # an output face is its source's cells, smallest first
