"""GPU tier of the mesh clean-up: mesh_clean.py and the kernels of csrc/radegs_meshclean.hip against
tests/meshclean_restatement.py on the meshes of tests/meshclean_cases.py.  Labels, counts, faces and kept vertices are integers and compared
exactly.  Areas and normals are compared bit for bit: the kernels and the restatement do the same float64 operations in the same order, one
rounding each, and float64 sqrt and divide are correctly rounded on both sides (include/radegs.h, "Mesh clean-up")."""
import numpy as np
import pytest
import torch

import mesh_clean as mcl
import meshclean_cases as mc
import meshclean_restatement as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ON_DEVICE = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def gpu_case(name):
    """(vertices float64, faces int64) of a case on the device, uploaded once"""
    if name not in _ON_DEVICE:
        v, f = mc.CASES[name]
        _ON_DEVICE[name] = (dev(v), dev(f))
    return _ON_DEVICE[name]


def assert_mesh(got, want, what):
    (gv, gf, gk), (wv, wf, wk) = (tuple(host(t) for t in got)), want
    assert gf.dtype == np.int64 and gk.dtype == np.int64, what
    assert gf.shape == wf.shape and np.array_equal(gf, wf), (what, gf.shape, wf.shape)
    assert np.array_equal(gk, wk), what
    assert same_bits(gv, wv), what


# --------------------------------------------------------------------------- clusters ---------------------------------------------------------------------------
@pytest.mark.parametrize("adjacency", mr.ADJACENCY)
@pytest.mark.parametrize("name", mc.NAMES)
def test_clusters_counts_and_areas_equal_the_restatement(name, adjacency):
    v, f = gpu_case(name)
    want_labels, want_counts, want_area = mc.reference(name, adjacency)
    labels, counts, area = mcl.cluster_connected_triangles(f, v, adjacency)
    assert labels.dtype == torch.int64 and counts.dtype == torch.int64 and area.dtype == torch.float64
    assert np.array_equal(host(labels), want_labels)
    assert np.array_equal(host(counts), want_counts)
    diff = np.abs(host(area) - want_area)
    print(name, adjacency, "clusters", want_counts.shape[0], "largest area difference", float(diff.max()), "differing", int((diff != 0).sum()))
    assert same_bits(host(area), want_area)
    labels2, counts2, none = mcl.cluster_connected_triangles(f, None, adjacency)             # without vertices: no areas
    assert none is None and torch.equal(labels2, labels) and torch.equal(counts2, counts)
    labels3, _, area32 = mcl.cluster_connected_triangles(f.int(), v.float(), adjacency)      # int32 faces, float32 vertices: float64 arithmetic
    assert torch.equal(labels3, labels) and area32.dtype == torch.float64
    assert same_bits(host(area32), mr.cluster_areas(mc.CASES[name][0].astype(np.float32), mc.CASES[name][1], want_labels, want_counts.shape[0]))


@pytest.mark.parametrize("permuted, base", mc.PERMUTED)
def test_permuted_faces_give_the_same_partition(permuted, base):
    (_, fp), (_, fb) = mc.CASES[permuted], mc.CASES[base]
    at = {tuple(r): i for i, r in enumerate(fb.tolist())}
    to_base = np.array([at[tuple(r)] for r in fp.tolist()])
    for adjacency in mr.ADJACENCY:
        lp = host(mcl.cluster_connected_triangles(gpu_case(permuted)[1], None, adjacency)[0])
        lb = host(mcl.cluster_connected_triangles(gpu_case(base)[1], None, adjacency)[0])
        _, first, inverse = np.unique(lb[to_base], return_index=True, return_inverse=True)
        assert np.array_equal(np.argsort(np.argsort(first))[inverse], lp)                    # the base's partition, numbered in the permuted order


def test_a_mesh_past_the_smallest_instantiation_of_the_sort():
    """3.15 M edge records: the two-word sort runs its 16-items-per-thread kernels (above 3 * 2^20 records) and the scan its larger one.  The
    answer is known without the restatement: a shuffled 725 x 725 sheet and two strips are three clusters, numbered by first occurrence."""
    rng = np.random.default_rng(9)
    _, f = mc.join(mc.sheet(725, 725, rng), mc.strip(300, rng), mc.strip(77, rng))
    assert 3 * f.shape[0] > 3 << 20
    member = np.concatenate([np.zeros(2 * 725 * 725, np.int64), np.ones(300, np.int64), np.full(77, 2)])
    order = rng.permutation(f.shape[0])
    member = member[order]
    _, first, inverse = np.unique(member, return_index=True, return_inverse=True)
    want = np.argsort(np.argsort(first))[inverse]
    for adjacency in mr.ADJACENCY:
        labels, counts, _ = mcl.cluster_connected_triangles(dev(f[order]), None, adjacency)
        assert np.array_equal(host(labels), want) and np.array_equal(host(counts), np.bincount(want))


# -------------------------------------------------------------------------- the whole steps --------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.NAMES)
def test_post_process_mesh_equals_the_restatement(name):
    v, f = gpu_case(name)
    hv, hf = mc.CASES[name]
    clusters = mc.reference(name, "edge")
    C = clusters[1].shape[0]
    for keep in mc.cluster_to_keep_values(C):
        for floor in (50, 0):
            want = mr.post_process_mesh(hv, hf, keep, floor, clusters=clusters)
            assert_mesh(mcl.post_process_mesh(v, f, keep, floor), want, (name, keep, floor))
    want = mr.post_process_mesh(hv.astype(np.float32), hf, clusters=clusters)                 # the defaults, float32 vertices, int32 faces
    got = mcl.post_process_mesh(v.float(), f.int())
    assert got[0].dtype == torch.float32
    assert_mesh(got, want, name)


@pytest.mark.parametrize("name", mc.NAMES)
def test_get_connected_mesh_equals_the_restatement(name):
    v, f = gpu_case(name)
    hv, hf = mc.CASES[name]
    clusters = mc.reference(name, "manifold_edge")
    assert_mesh(mcl.get_connected_mesh(v, f, True), mr.get_connected_mesh(hv, hf, True, clusters=clusters), (name, "largest"))
    for thr in (0.2, 0.05, 0.0, 1.0):
        want = mr.get_connected_mesh(hv, hf, False, thr, clusters=clusters)
        assert_mesh(mcl.get_connected_mesh(v, f, False, thr), want, (name, thr))
    assert mcl.get_connected_mesh(v.float(), f)[0].dtype == torch.float32


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_three_removals_equal_the_restatement(name):
    v, f = gpu_case(name)
    hv, hf = mc.CASES[name]
    rng = np.random.default_rng(21)
    for p in (0.5, 0.0, 1.0):
        remove = rng.random(hf.shape[0]) < p
        assert_mesh(mcl.remove_triangles_by_mask(v, f, dev(remove)), mr.remove_triangles_by_mask(hv, hf, remove), (name, p))
    assert_mesh(mcl.remove_unreferenced_vertices(v, f), mr.remove_unreferenced_vertices(hv, hf), name)
    assert_mesh(mcl.remove_unreferenced_vertices(v.float(), f), mr.remove_unreferenced_vertices(hv.astype(np.float32), hf), name)
    got = mcl.remove_degenerate_triangles(f)
    assert got.dtype == torch.int64 and np.array_equal(host(got), mr.remove_degenerate_triangles(hf))


# ------------------------------------------------------------------------- vertex normals -------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.NAMES)
def test_vertex_normals_equal_the_restatement(name):
    v, f = gpu_case(name)
    hv, hf = mc.CASES[name]
    for vertices, hvertices in ((v, hv), (v.float(), hv.astype(np.float32))):
        for normalized in (True, False):
            got, want = host(mcl.compute_vertex_normals(vertices, f, normalized)), mr.compute_vertex_normals(hvertices, hf, normalized)
            assert got.dtype == hvertices.dtype and got.shape == want.shape
            differing = int((got != want).sum())
            print(name, got.dtype, "normalized" if normalized else "raw", "components that differ:", differing)
            assert same_bits(got, want)
    if name == "unused_vertex":
        assert host(mcl.compute_vertex_normals(v, f))[5].tolist() == [0.0, 0.0, 1.0]


def test_normals_of_closed_outward_surfaces_point_outward():
    v, f = gpu_case("tetrahedra_1000")
    n = host(mcl.compute_vertex_normals(v, f)).reshape(1000, 4, 3)
    hv = mc.CASES["tetrahedra_1000"][0].reshape(1000, 4, 3)
    assert ((n * (hv - hv.mean(1, keepdims=True))).sum(2) > 0).all()


# --------------------------------------------------------------------------- repeatability ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("floaters_49_50_51", "strip_pieces_shuffled", "large_shuffled"))
def test_every_public_function_called_twice_returns_the_same_bits(name):
    v, f = gpu_case(name)
    remove = dev(np.random.default_rng(2).random(f.shape[0]) < 0.3)
    calls = (lambda: mcl.cluster_connected_triangles(f, v, "edge"), lambda: mcl.cluster_connected_triangles(f, v, "manifold_edge"),
             lambda: mcl.remove_triangles_by_mask(v, f, remove), lambda: mcl.remove_unreferenced_vertices(v, f),
             lambda: (mcl.remove_degenerate_triangles(f),), lambda: mcl.post_process_mesh(v, f, 2), lambda: mcl.get_connected_mesh(v, f, False, 0.01),
             lambda: mcl.get_connected_mesh(v, f, True), lambda: (mcl.compute_vertex_normals(v, f),))
    for call in calls:
        for a, b in zip(call(), call()):
            assert same_bits(host(a), host(b))


def test_an_index_outside_the_vertices_is_refused_on_the_host():
    v, f = gpu_case("shared_edge")
    for bad in (f + 1, f - 1):
        for call in (lambda: mcl.cluster_connected_triangles(bad, v), lambda: mcl.post_process_mesh(v, bad), lambda: mcl.get_connected_mesh(v, bad),
                     lambda: mcl.compute_vertex_normals(v, bad), lambda: mcl.remove_unreferenced_vertices(v, bad)):
            with pytest.raises(RuntimeError, match="outside the 4 vertices"):
                call()
    with pytest.raises(RuntimeError, match="must be on the same device"):
        mcl.remove_triangles_by_mask(v, f, torch.zeros(2, dtype=torch.bool))


# ------------------------------------------------------------------------------ the route ------------------------------------------------------------------------------
def test_tsdf_mesh_loses_its_floater_and_is_written_with_normals(tmp_path):
    """the smallest end-to-end route: a VoxelBlockGrid holding a sphere of 10 voxels radius around the corner eight blocks share and a detached
    blob of 2 voxels radius -> extract_triangle_mesh -> post_process_mesh -> compute_vertex_normals -> write_ply"""
    import tsdf
    import tsdf_restatement as tr
    from test_gpu_tsdf import install_blocks, new_grid
    from test_meshclean_api import read_ply_with_normals
    coords = np.array([[x, y, z] for z in (-1, 0) for y in (-1, 0) for x in (-1, 0)], np.int32)
    p = (16 * coords.astype(np.int64)[:, None, :] + tr.VOXEL_OFFSETS[None]).astype(np.float64)                 # voxel coordinates [8,4096,3]
    sdf = np.minimum(np.linalg.norm(p, axis=2) - 10.0, np.linalg.norm(p - 12.0, axis=2) - 2.0)
    g = new_grid(block_count=8, with_color=False)
    install_blocks(g, coords, np.clip(sdf / 4.0, -1.0, 1.0).astype(np.float32), np.full((8, 4096), 5.0, np.float32))
    v, f, _ = g.extract_triangle_mesh(3.0)
    hv, hf = host(v), host(f)
    labels, counts, _ = mcl.cluster_connected_triangles(f, v)
    assert sorted(host(counts).tolist()) == sorted(mr.triangle_clusters(hf)[1].tolist()) and counts.shape[0] == 2 and int(counts.min()) >= 8
    blob = host(labels) == int(counts.argmin())
    assert (np.linalg.norm(hv[hf[blob].reshape(-1)] / g.voxel_size - 12.0, axis=1) < 3.0).all()              # the small cluster is the blob
    v1, f1, kept = mcl.post_process_mesh(v, f, cluster_to_keep=1, min_triangles=0)
    assert_mesh((v1, f1, kept), mr.post_process_mesh(hv, hf, 1, 0), "route")
    assert f1.shape[0] == int(counts.max()) and np.array_equal(host(v1)[host(f1)], hv[hf[~blob]])              # the blob went and nothing else
    n = mcl.compute_vertex_normals(v1, f1)
    assert n.dtype == torch.float32 and same_bits(host(n), mr.compute_vertex_normals(host(v1), host(f1)))
    centre_out = host(v1) / np.linalg.norm(host(v1), axis=1)[:, None]
    assert (np.abs((host(n) * centre_out).sum(1)) > 0.9).all()                                               # along the sphere's radius
    path = str(tmp_path / "recon.ply")
    tsdf.write_ply(path, v1, f1, normals=n)
    rv, rn, rc, rf = read_ply_with_normals(path)
    assert same_bits(rv, host(v1)) and same_bits(rn, host(n)) and rc is None and np.array_equal(rf, host(f1))
