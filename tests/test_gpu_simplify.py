"""GPU tier of the mesh simplification: mesh_simplify.py and the kernels of csrc/radegs_meshsimplify.hip against
tests/simplify_restatement.py on the meshes of tests/simplify_cases.py.  Cell numbers, faces, face sources and vertex maps are integers and
compared exactly.  Averages, quadrics, positions and attributes are compared bit for bit: the kernels and the restatement do the same float64
operations in the same order, one rounding each, and float64 sqrt and divide are correctly rounded on both sides (include/radegs.h, "Mesh
simplification")."""
import collections

import numpy as np
import pytest
import torch

import mesh_simplify as ms
import simplify_cases as sc
import simplify_restatement as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ON_DEVICE = {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def gpu_case(name):
    """(vertices float64, faces int64, attributes float64 or None) of a case on the device, uploaded once"""
    if name not in _ON_DEVICE:
        c = sc.CASES[name]
        _ON_DEVICE[name] = (dev(c.vertices), dev(c.faces), dev(c.attributes))
    return _ON_DEVICE[name]


def assert_result(got, want, what):
    got = tuple(host(t) for t in got)
    for g, w, part in zip(got[1:4], want[1:4], ("faces", "vertex_map", "face_source")):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (what, part)
    assert same_bits(got[0], want[0]), (what, "vertices", int((got[0] != want[0]).sum()))
    assert (got[4] is None) == (want[4] is None) and (want[4] is None or same_bits(got[4], want[4])), (what, "attributes")


# ---------------------------------------------------------------------------- the stages ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES)
def test_every_stage_equals_the_restatement(name):
    c = sc.CASES[name]
    v, f, a = gpu_case(name)
    want = sc.reference(name)
    origin, max_key = ms._grid(c.vertices.min(0).tolist(), c.vertices.max(0).tolist(), c.h, c.origin)
    assert np.array_equal(np.asarray(origin), want["origin"])
    cells = ms._cells(v, origin, c.h, max_key)
    K = cells.K
    assert K == want["K"]
    assert np.array_equal(host(cells.vertex_cell), want["vertex_cell"]) and np.array_equal(host(cells.cell_key)[:K], want["cell_key"])
    starts = host(cells.cell_start)[:K + 1]
    assert starts[0] == 0 and starts[K] == v.shape[0] and np.array_equal(np.diff(starts), np.bincount(want["vertex_cell"], minlength=K))
    assert np.array_equal(host(cells.order).astype(np.int64), np.argsort(want["vertex_cell"], kind="stable"))
    positions, attr, averages, quadrics = ms._cell_vertices(v, f, a, cells, origin, c.h, 1)
    for g, w, part in ((averages, want["averages"], "averages"), (quadrics, want["quadrics"], "quadrics"), (positions, want["positions"], "positions"),
                       (attr, want["attributes"], "attributes")):
        if w is not None:
            differing = int((host(g) != w).sum())
            print(name, part, "entries that differ:", differing)
            assert same_bits(host(g), w), (name, part, differing)
    positions, _, averages, quadrics = ms._cell_vertices(v, f, a, cells, origin, c.h, 0)
    assert quadrics is None and positions is averages and same_bits(host(averages), want["averages"])
    for remove_duplicates in (True, False):
        cf, remove = ms._cell_faces(f, v.shape[0], cells, remove_duplicates)
        wf, wr = sr.cell_faces(c.faces, want["vertex_cell"], K, remove_duplicates)
        assert np.array_equal(host(cf), wf) and np.array_equal(host(remove).astype(bool), wr), (name, remove_duplicates)


@pytest.mark.parametrize("contraction", sc.CONTRACTIONS)
@pytest.mark.parametrize("name", sc.NAMES)
def test_the_public_call_equals_the_restatement(name, contraction):
    c = sc.CASES[name]
    v, f, a = gpu_case(name)
    for remove_duplicates in (True, False):
        for drop_unreferenced in (True, False):
            want = sr.simplify_vertex_clustering(c.vertices, c.faces, c.h, contraction, c.origin, c.attributes, remove_duplicates, drop_unreferenced)
            got = ms.simplify_vertex_clustering(v, f, c.h, contraction, c.origin, a, remove_duplicates, drop_unreferenced)
            assert_result(got, want, (name, contraction, remove_duplicates, drop_unreferenced))
    v32, a32 = c.vertices.astype(np.float32), None if c.attributes is None else c.attributes.astype(np.float32)     # float32 in, int32 faces
    want = sr.simplify_vertex_clustering(v32, c.faces, c.h, contraction, c.origin, a32)
    got = ms.simplify_vertex_clustering(dev(v32), f.int(), c.h, contraction, c.origin, dev(a32))
    assert got[0].dtype == torch.float32 and (a32 is None or got[4].dtype == torch.float32)
    assert_result(got, want, (name, contraction, "float32"))


@pytest.mark.parametrize("name", ("fans", "degenerate_triangles", "bumpy_coloured"))
def test_two_calls_return_the_same_bits(name):
    c = sc.CASES[name]
    v, f, a = gpu_case(name)
    for contraction in sc.CONTRACTIONS:
        for x, y in zip(ms.simplify_vertex_clustering(v, f, c.h, contraction, c.origin, a), ms.simplify_vertex_clustering(v, f, c.h, contraction, c.origin, a)):
            assert (x is None and y is None) or same_bits(host(x), host(y))


# ------------------------------------------------------------------------ the named edge cases ------------------------------------------------------------------------
def test_cells_of_1_63_64_65_255_256_257_vertices_and_records():
    c = sc.CASES["fans"]
    want = sc.reference("fans")
    members = np.bincount(want["vertex_cell"])
    records = np.bincount(want["vertex_cell"][c.faces.reshape(-1)], minlength=want["K"])
    assert sorted(members[members > 1].tolist() + [1]) == list(sc.COUNTS) and set(sc.COUNTS) <= set(records.tolist())
    v, f, a = gpu_case("fans")
    out_v, out_f, vmap, source, _ = ms.simplify_vertex_clustering(v, f, c.h, "quadric", c.origin, a)
    assert out_v.shape[0] == 3 * len(sc.COUNTS) and out_f.shape[0] == len(sc.COUNTS)            # every fan folds into one triangle
    assert host(source).tolist() == np.concatenate([[0], np.cumsum(sc.COUNTS)[:-1]]).tolist()    # the first face of each fan survives
    assert ms.simplify_vertex_clustering(v, f, c.h, "quadric", c.origin, a, remove_duplicates=False)[1].shape[0] == c.faces.shape[0]


def test_a_cell_no_face_references_and_a_mesh_in_one_cell():
    c = sc.CASES["unreferenced_cell"]
    v, f, _ = gpu_case("unreferenced_cell")
    dropped = ms.simplify_vertex_clustering(v, f, c.h)
    kept = ms.simplify_vertex_clustering(v, f, c.h, drop_unreferenced=False)
    lone = c.vertices.shape[0] - 1
    assert int(dropped[2][lone]) == -1 and int(kept[2][lone]) >= 0 and kept[0].shape[0] > dropped[0].shape[0]
    assert np.array_equal(host(kept[0])[int(kept[2][lone])], c.vertices[lone])                   # alone in its cell: its own position
    c = sc.CASES["one_cell"]
    v, f, _ = gpu_case("one_cell")
    out = ms.simplify_vertex_clustering(v, f, c.h, drop_unreferenced=False)
    assert out[0].shape == (1, 3) and out[1].shape == (0, 3) and out[3].shape == (0,) and bool((out[2] == 0).all())
    out = ms.simplify_vertex_clustering(v, f, c.h)
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and bool((out[2] == -1).all())


def test_vertices_on_cell_faces_fall_in_the_upper_cell():
    c = sc.CASES["on_cell_faces"]
    v, _, _ = gpu_case("on_cell_faces")
    cells = ms._cells(v, c.origin, c.h, (2 ** 21 - 1) << 42 | (2 ** 21 - 1) << 21 | (2 ** 21 - 1))
    key = host(cells.cell_key)[:cells.K][host(cells.vertex_cell)]
    exact = (c.vertices / c.h).astype(np.int64)                                                  # k h / 2 over h: exact, and floor rounds down
    assert np.array_equal(key, exact[:, 0] << 42 | exact[:, 1] << 21 | exact[:, 2])
    assert (c.vertices[:, 0] / c.h == exact[:, 0]).sum() > 100                                   # many of them sit exactly on a face


def test_the_last_cell_is_accepted_and_one_more_is_refused():
    c = sc.CASES["last_cell"]
    v, f, _ = gpu_case("last_cell")
    out_v, out_f, vmap, _, _ = ms.simplify_vertex_clustering(v, f, c.h, origin=c.origin)
    assert out_f.shape[0] == 1 and host(vmap).tolist() == [2, 2, 2, 0, 0, 1, 1]
    beyond = v.clone()
    beyond[0, 0] += 1.0
    with pytest.raises(RuntimeError, match=r"outside \[0, 2\^21\)"):
        ms.simplify_vertex_clustering(beyond, f, c.h, origin=c.origin)
    with pytest.raises(RuntimeError, match=r"outside \[0, 2\^21\)"):
        ms.simplify_vertex_clustering(v, f, c.h, origin=(1.0, 0.0, 1.0))                         # a vertex below the origin: a negative cell


def test_duplicates_of_equal_and_of_opposite_orientation():
    c = sc.CASES["duplicates"]
    v, f, a = gpu_case("duplicates")
    out = ms.simplify_vertex_clustering(v, f, c.h, origin=c.origin, attributes=a)
    # faces 0-3 are one triple in four rotations, 4 its mirror image, 5 collapses, 6-8 a second triple, its rotation and its mirror image
    assert host(out[3]).tolist() == [0, 4, 6, 8] and host(out[1]).tolist() == [[0, 2, 1], [0, 1, 2], [0, 2, 3], [0, 3, 2]]
    out = ms.simplify_vertex_clustering(v, f, c.h, origin=c.origin, remove_duplicates=False)
    assert host(out[3]).tolist() == [0, 1, 2, 3, 4, 6, 7, 8]


def test_ranks_one_two_three_and_the_fallback_to_the_mean():
    for name, ranks in (("plane", {1}), ("roof", {1, 2}), ("corner", {1, 2, 3})):
        c, want = sc.CASES[name], sc.reference(name)
        Q = want["quadrics"]
        ev = np.linalg.eigvalsh(np.stack([Q[:, [0, 1, 2]], Q[:, [1, 4, 5]], Q[:, [2, 5, 7]]], 1))
        assert set(((ev > 1e-3 * ev.max(1, keepdims=True)).sum(1)).tolist()) == ranks, name
        v, f, _ = gpu_case(name)
        got = ms.simplify_vertex_clustering(v, f, c.h, origin=c.origin, drop_unreferenced=False)
        assert same_bits(host(got[0]), want["positions"])
    c, want = sc.CASES["leaves_the_box"], sc.reference("leaves_the_box")
    _, x, solved, kept = sr.solve(want["quadrics"], want["averages"], want["cell_key"], c.h, want["origin"], details=True)
    assert solved.all() and not kept.any() and (x[:, 0] > 1.0).all()                             # the planes meet at x = 1.5, outside [0, 1]
    v, f, _ = gpu_case("leaves_the_box")
    got = ms.simplify_vertex_clustering(v, f, c.h, origin=c.origin, drop_unreferenced=False)
    assert same_bits(host(got[0]), want["averages"])


def _face_set(vertices, faces):
    return collections.Counter(tuple(map(tuple, vertices[row].tolist())) for row in faces)


def test_a_shuffled_face_order_gives_the_same_vertices_and_the_same_set_of_faces():
    """The average depends on the vertices alone: the same bits.  The quadric sums take their records in another order, so their roundings
    differ: a sum of n <= 257 terms moves by at most n 2^-53 of the sum of magnitudes, and the solve divides by eigenvalues no smaller than
    1e-3 of the largest, so a position moves by at most about 257 x 2^-53 x 1e3 = 3e-11 of the coordinates' scale (below 30 here): 1e-9."""
    c = sc.CASES["fans"]
    v, f, a = gpu_case("fans")
    fs = gpu_case("fans_shuffled")[1]
    for contraction in sc.CONTRACTIONS:
        one = [host(t) for t in ms.simplify_vertex_clustering(v, f, c.h, contraction, c.origin, a, remove_duplicates=False)]
        two = [host(t) for t in ms.simplify_vertex_clustering(v, fs, c.h, contraction, c.origin, a, remove_duplicates=False)]
        assert np.array_equal(one[2], two[2]) and same_bits(one[4], two[4])
        if contraction == "average":
            assert same_bits(one[0], two[0])
        else:
            print("largest move of a quadric position under the shuffle:", float(np.abs(one[0] - two[0]).max()))
            assert np.abs(one[0] - two[0]).max() <= 1e-9
        assert collections.Counter(map(tuple, one[1].tolist())) == collections.Counter(map(tuple, two[1].tolist()))


def test_a_closed_oriented_surface_stays_closed():
    """independent of the restatement: with every face kept, each directed edge (a, b) of the output has as many (b, a)"""
    c = sc.CASES["sphere"]
    v, f, _ = gpu_case("sphere")
    for contraction in sc.CONTRACTIONS:
        faces = host(ms.simplify_vertex_clustering(v, f, c.h, contraction, remove_duplicates=False)[1])
        assert 0 < faces.shape[0] < c.faces.shape[0]
        edges = collections.Counter(zip(faces.reshape(-1).tolist(), np.roll(faces, -1, axis=1).reshape(-1).tolist()))
        assert all(edges[(b, a)] == n for (a, b), n in edges.items())


# ------------------------------------------------------------------------------- at size -------------------------------------------------------------------------------
def test_a_sheet_past_the_smallest_instantiation_of_the_sort():
    """3.15 M corner records: the sorts run their 16-items-per-thread kernels.  The answer is known without the restatement: the 726 x 726
    vertices of a regular sheet at unit spacing, cells of 6 from -0.5, are 121 x 121 cells of 36 vertices whose mean is the cell's centre in x
    and y; the faces that survive are those of a 120 x 120 sheet of quads, two each, whatever the order of the input faces."""
    import meshclean_cases as mc
    n, h = 725, 6.0
    v, f = mc.sheet(n, n, np.random.default_rng(0))
    v = np.round(v)                                                                              # the grid without its jitter: integers
    assert 3 * f.shape[0] > 3 << 20
    order = np.random.default_rng(9).permutation(f.shape[0])
    colours = np.stack([v[:, 0], v[:, 1], v[:, 0] + v[:, 1]], 1)
    out_v, out_f, vmap, source, attr = ms.simplify_vertex_clustering(dev(v), dev(f[order]), h, "average", (-0.5, -0.5, -0.5), dev(colours))
    side = (n + 1) // 6
    assert out_v.shape[0] == side * side and out_f.shape[0] == 2 * (side - 1) ** 2
    cell = (v[:, 0] + 0.5) // h * side + (v[:, 1] + 0.5) // h                                     # the key's order: x first, then y
    assert np.array_equal(host(vmap), cell.astype(np.int64))
    centre = np.stack([np.repeat(np.arange(side), side) * h + 2.5, np.tile(np.arange(side), side) * h + 2.5, np.zeros(side * side)], 1)
    assert np.array_equal(host(out_v), centre) and np.array_equal(host(attr)[:, :2], centre[:, :2])   # sums of 36 small integers are exact
    assert bool((source[1:] > source[:-1]).all())
    rows = host(out_f)
    assert (rows[:, 0] < rows[:, 1]).all() and (rows[:, 0] < rows[:, 2]).all() and np.unique(rows, axis=0).shape[0] == rows.shape[0]
    quads = collections.Counter(int(r[0]) for r in rows)
    assert set(quads.values()) == {2} and len(quads) == (side - 1) ** 2
    got = ms.simplify_vertex_clustering(dev(v), dev(f[order]), h, "quadric", (-0.5, -0.5, -0.5))                      # a plane: the quadric position stays on it
    assert got[1].shape[0] == out_f.shape[0] and torch.equal(got[2], vmap) and float(got[0][:, 2].abs().max()) <= 1e-9


# ------------------------------------------------------------------------------ the route ------------------------------------------------------------------------------
def test_the_composed_recipe_ends_in_a_file_that_reads_back(tmp_path):
    """post_process_mesh -> simplify_vertex_clustering -> compute_vertex_normals -> write_ply(normals=), read back with eval_io.read_ply_mesh"""
    import eval_io
    import mesh_clean as mcl
    import tsdf
    c = sc.CASES["bumpy_coloured"]
    floater = sc.surface(2, 2, lambda x, y: 9.0 + 0.0 * x, None, 0.0)
    v, f = sc.join((c.vertices, c.faces), floater)
    colours = np.concatenate([c.attributes, np.zeros((floater[0].shape[0], 3))])
    v1, f1, kept = mcl.post_process_mesh(dev(v.astype(np.float32)), dev(f), cluster_to_keep=1, min_triangles=0)
    assert f1.shape[0] == c.faces.shape[0]
    v2, f2, _, _, colours2 = ms.simplify_vertex_clustering(v1, f1, c.h, attributes=dev(colours.astype(np.float32))[kept])
    want = sr.simplify_vertex_clustering(host(v1), host(f1), c.h, attributes=colours.astype(np.float32)[host(kept)])
    assert np.array_equal(host(f2), want[1]) and same_bits(host(v2), want[0]) and same_bits(host(colours2), want[4])
    normals = mcl.compute_vertex_normals(v2, f2)
    path = str(tmp_path / "simplified.ply")
    tsdf.write_ply(path, v2, f2, colors=colours2, normals=normals)
    rv, rf = eval_io.read_ply_mesh(path, DEV)[:2]
    assert np.array_equal(host(rf).astype(np.int64), host(f2)) and np.array_equal(host(rv).astype(np.float32), host(v2))


def test_simplify_to_face_count_on_a_sheet(monkeypatch):
    c = sc.CASES["bumpy_coloured"]
    v, f, a = gpu_case("bumpy_coloured")
    tried = []
    count_only = ms._count_only
    monkeypatch.setattr(ms, "_count_only", lambda v64, f_, lo, hi, h, *rest: tried.append(h) or count_only(v64, f_, lo, hi, h, *rest))
    target = 400
    out = ms.simplify_to_face_count(v, f, target, attributes=a)
    used = out[5]
    assert 0 < out[1].shape[0] <= target and used in tried and 1 < len(tried) <= 16
    direct = ms.simplify_vertex_clustering(v, f, used, attributes=a)
    for x, y in zip(out[:5], direct):
        assert same_bits(host(x), host(y))
    finer = [h for h in tried if h < used]
    assert all(ms.simplify_vertex_clustering(v, f, h)[1].shape[0] > target for h in finer)       # the finest size TRIED that qualifies
    with pytest.raises(RuntimeError, match="no voxel size tried"):
        ms.simplify_to_face_count(v, f, 1, remove_duplicates=False, max_tries=3)
