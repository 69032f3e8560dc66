"""CPU tier of the mesh clean-up unit: the library exports the entry points and include/radegs.h declares them, the size functions and the
argument checks of the C entry points run without a device, mesh_clean.py has the call surface the issue names and refuses bad arguments
before any launch, tsdf.write_ply without `normals` writes the bytes it always wrote, and the new kernels use no scratch."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mesh_clean as mcl
import tsdf
from test_kernel_resources import code_objects  # noqa: F401  (the fixture) -- and its skip condition:
from test_kernel_resources import pytestmark as _needs_llvm_tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("radegs_meshclean_cluster_bytes", "radegs_meshclean_cluster", "radegs_meshclean_stats_bytes", "radegs_meshclean_stats",
           "radegs_meshclean_compact_bytes", "radegs_meshclean_compact_plan", "radegs_meshclean_compact_apply", "radegs_meshclean_normals_bytes",
           "radegs_meshclean_vertex_normals")
KERNELS = ("edge_records_kernel", "iota_kernel", "link_kernel", "roots_kernel", "number_kernel", "count_kernel", "counts_out_kernel",
           "group_area_kernel", "cluster_area_kernel", "total_partial_kernel", "total_final_kernel", "fill_kernel", "face_flags_kernel",
           "compact_apply_kernel", "corner_keys_kernel", "vertex_normals_kernel")
INVALID, TOO_LARGE = -1, -6


def _library():
    import diff_gaussian_rasterization._C as C
    return C, mcl._lib()


def test_library_exports_and_header_declares_the_entry_points():
    C, L = _library()
    header = open(os.path.join(ROOT, "include", "radegs.h")).read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in C.EXPORTED_SYMBOLS, sym
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % sym, header), sym
    assert "SURVEY.md 8f N12" in header
    assert set(mcl.SIGNATURES) == set(SYMBOLS)


def test_sizes_and_argument_checks_run_without_a_device():
    _, L = _library()
    fake = 0x1000
    assert L.radegs_meshclean_cluster_bytes(0) == 0 and L.radegs_meshclean_cluster_bytes(-1) == 0 and L.radegs_meshclean_cluster_bytes(2 ** 30 + 1) == 0
    small, large = L.radegs_meshclean_cluster_bytes(1), L.radegs_meshclean_cluster_bytes(100_000)
    assert 0 < small < 64 * 1024 and small % 256 == 0
    assert 36 * 300_000 <= large <= 60 * 300_000                                # 7 words and one 64-bit key per record, and the sort's temp
    assert L.radegs_meshclean_cluster_bytes(2 ** 30) > 36 * 3 * 2 ** 30          # a size_t: not cut to 32 bits
    assert L.radegs_meshclean_stats_bytes(0, 0) == 0 and L.radegs_meshclean_stats_bytes(10, 11) == 0 and L.radegs_meshclean_stats_bytes(10, 3) > 0
    assert L.radegs_meshclean_compact_bytes(0, 0) == 0 and L.radegs_meshclean_compact_bytes(-1, 4) == 0 and L.radegs_meshclean_compact_bytes(8, 4) > 0
    assert L.radegs_meshclean_compact_bytes(2 ** 31, 4) == 0 and L.radegs_meshclean_normals_bytes(0) == 0 and L.radegs_meshclean_normals_bytes(4) > 0

    def cluster(V=8, F=4, f=fake, manifold=0, ws=fake, nbytes=1 << 30, labels=fake, n=fake):
        return L.radegs_meshclean_cluster(V, F, f, manifold, ws, nbytes, labels, n, None)
    assert cluster(V=-1) == INVALID and cluster(F=-1) == INVALID and cluster(manifold=2) == INVALID and cluster(n=None) == INVALID
    assert cluster(V=2 ** 31) == TOO_LARGE and cluster(F=2 ** 30 + 1) == TOO_LARGE
    assert cluster(f=None) == INVALID and cluster(labels=None) == INVALID and cluster(ws=None) == INVALID and cluster(ws=fake + 4) == INVALID
    assert cluster(nbytes=L.radegs_meshclean_cluster_bytes(4) - 1) == INVALID

    def stats(V=8, F=4, C=2, v=fake, f=fake, labels=fake, ws=fake, nbytes=1 << 30, counts=fake, area=fake, total=fake):
        return L.radegs_meshclean_stats(V, F, C, v, f, labels, ws, nbytes, counts, area, total, None)
    assert stats(F=0, C=0, total=None) == 0                                       # no triangle: no launch
    assert stats(V=-1) == INVALID and stats(F=-1) == INVALID and stats(C=-1) == INVALID and stats(C=5) == INVALID and stats(C=0) == INVALID
    assert stats(V=2 ** 31) == TOO_LARGE and stats(F=2 ** 30 + 1, C=1) == TOO_LARGE
    assert stats(labels=None) == INVALID and stats(counts=None) == INVALID and stats(v=None) == INVALID and stats(f=None) == INVALID
    assert stats(ws=None) == INVALID and stats(ws=fake + 8) == INVALID and stats(nbytes=L.radegs_meshclean_stats_bytes(4, 2) - 1) == INVALID

    def plan(V=8, F=4, C=0, f=fake, remove=None, labels=None, keep=None, ws=fake, nbytes=1 << 30, counts2=fake):
        return L.radegs_meshclean_compact_plan(V, F, C, f, remove, labels, keep, 1, 1, ws, nbytes, counts2, None)
    assert plan(V=-1) == INVALID and plan(F=-1) == INVALID and plan(C=-1) == INVALID and plan(counts2=None) == INVALID
    assert plan(keep=fake) == INVALID                                            # cluster flags without the labels they index
    assert plan(V=2 ** 31) == TOO_LARGE and plan(F=2 ** 30 + 1) == TOO_LARGE
    assert plan(f=None) == INVALID and plan(ws=None) == INVALID and plan(ws=fake + 4) == INVALID
    assert plan(nbytes=L.radegs_meshclean_compact_bytes(8, 4) - 1) == INVALID

    def apply(V=8, F=4, f=fake, ws=fake, nv=3, nf=1, kept=fake, out=fake):
        return L.radegs_meshclean_compact_apply(V, F, f, ws, nv, nf, kept, out, None)
    assert apply(nv=0, nf=0) == 0                                                # nothing survives: no launch
    assert apply(V=-1) == INVALID and apply(nv=9) == INVALID and apply(nf=5) == INVALID and apply(nv=-1) == INVALID
    assert apply(V=2 ** 31) == TOO_LARGE and apply(F=2 ** 30 + 1) == TOO_LARGE
    assert apply(f=None) == INVALID and apply(ws=None) == INVALID and apply(kept=None) == INVALID and apply(out=None) == INVALID

    def normals(V=8, F=4, v=fake, f=fake, ws=fake, nbytes=1 << 30, out=fake):
        return L.radegs_meshclean_vertex_normals(V, F, v, f, 1, ws, nbytes, out, None)
    assert normals(V=0) == 0
    assert normals(V=-1) == INVALID and normals(F=-1) == INVALID and normals(V=2 ** 31) == TOO_LARGE and normals(F=2 ** 30 + 1) == TOO_LARGE
    assert normals(v=None) == INVALID and normals(f=None) == INVALID and normals(out=None) == INVALID and normals(ws=None) == INVALID
    assert normals(ws=fake + 4) == INVALID and normals(nbytes=L.radegs_meshclean_normals_bytes(4) - 1) == INVALID


def test_python_surface():
    sig = lambda f: list(inspect.signature(f).parameters)
    default = lambda f: [p.default for p in inspect.signature(f).parameters.values() if p.default is not inspect.Parameter.empty]
    assert sig(mcl.cluster_connected_triangles) == ["faces", "vertices", "adjacency"] and default(mcl.cluster_connected_triangles) == [None, "edge"]
    assert sig(mcl.remove_triangles_by_mask) == ["vertices", "faces", "remove"]
    assert sig(mcl.remove_unreferenced_vertices) == ["vertices", "faces"] and sig(mcl.remove_degenerate_triangles) == ["faces"]
    assert sig(mcl.post_process_mesh) == ["vertices", "faces", "cluster_to_keep", "min_triangles"] and default(mcl.post_process_mesh) == [1000, 50]
    assert sig(mcl.get_connected_mesh) == ["vertices", "faces", "get_largest_components", "remove_small_geometry_threshold"]
    assert default(mcl.get_connected_mesh) == [False, 0.2]                                     # cull_mesh.py:187, 91
    assert sig(mcl.compute_vertex_normals) == ["vertices", "faces", "normalized"] and default(mcl.compute_vertex_normals) == [True]
    assert sig(tsdf.write_ply) == ["path", "vertices", "faces", "colors", "normals"] and default(tsdf.write_ply) == [None, None]
    assert "IndexError" in mcl.post_process_mesh.__doc__ and "same mesh, not the same arrays" in mcl.get_connected_mesh.__doc__
    import tnt_cull
    assert tnt_cull.get_connected_mesh is mcl.get_connected_mesh


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2]])
    for call in (lambda: mcl.cluster_connected_triangles(f), lambda: mcl.cluster_connected_triangles(f, v), lambda: mcl.remove_unreferenced_vertices(v, f),
                 lambda: mcl.remove_triangles_by_mask(v, f, torch.zeros(1, dtype=torch.bool)), lambda: mcl.remove_degenerate_triangles(f),
                 lambda: mcl.post_process_mesh(v, f), lambda: mcl.get_connected_mesh(v.double(), f), lambda: mcl.compute_vertex_normals(v, f[:0])):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()
    for bad in ("vertex", None, 0, "Edge"):
        with pytest.raises(RuntimeError, match="`adjacency` must be one of"):
            mcl.cluster_connected_triangles(f, v, adjacency=bad)
    for bad in (0, -1, 2.0, None, True):
        with pytest.raises(RuntimeError, match="`cluster_to_keep` must be a positive integer"):
            mcl.post_process_mesh(v, f, cluster_to_keep=bad)
    for bad in (-1, 50.0, None, True):
        with pytest.raises(RuntimeError, match="`min_triangles` must be a non-negative integer"):
            mcl.post_process_mesh(v, f, min_triangles=bad)
    with pytest.raises(RuntimeError, match="`get_largest_components` must be a bool"):
        mcl.get_connected_mesh(v, f, get_largest_components=1)
    for bad in (float("nan"), float("inf"), None, "0.2", True):
        with pytest.raises(RuntimeError, match="`remove_small_geometry_threshold` must be a finite number"):
            mcl.get_connected_mesh(v, f, remove_small_geometry_threshold=bad)
    with pytest.raises(RuntimeError, match="`normalized` must be a bool"):
        mcl.compute_vertex_normals(v, f, normalized=1)
    every = (lambda v, f: mcl.cluster_connected_triangles(f, v), mcl.remove_unreferenced_vertices, mcl.post_process_mesh, mcl.get_connected_mesh,
             mcl.compute_vertex_normals, lambda v, f: mcl.remove_triangles_by_mask(v, f, torch.zeros(1, dtype=torch.bool)))
    for call in every:
        for bad in (f.float(), f.reshape(3), torch.zeros(2, 4, dtype=torch.int64), [[0, 1, 2]]):
            with pytest.raises(RuntimeError, match="`faces` must be an int32 or int64 tensor"):
                call(v, bad)
        for bad in (v.half(), v.long(), None if call is not every[0] else v.half()):
            with pytest.raises(RuntimeError, match="`vertices` must be a float32 or float64 tensor"):
                call(bad, f)
    with pytest.raises(RuntimeError, match="`faces` must be an int32 or int64 tensor"):
        mcl.remove_degenerate_triangles(f.float())
    # more than 2^30 faces: refused on the shape alone (a meta tensor has no storage)
    huge = torch.empty((2 ** 30 + 1, 3), dtype=torch.int64, device="meta")
    for call in (lambda: mcl.cluster_connected_triangles(huge), lambda: mcl.remove_degenerate_triangles(huge)):
        with pytest.raises(RuntimeError, match="more than 2\\^30 faces"):
            call()
    # the remaining checks sit behind the device check: let a CPU tensor past it.  Each refuses, or returns, before the library is called.
    import diff_gaussian_rasterization._C as C
    monkeypatch.setattr(C, "_require_gpu", lambda t, name: None)
    monkeypatch.setattr(mcl, "_lib", lambda: pytest.fail("the library was called"))
    for call in every:
        for bad in (torch.tensor([[0, 1, 4]]), torch.tensor([[0, -1, 2]])):
            with pytest.raises(RuntimeError, match="outside the 4 vertices"):
                call(v, bad)
        with pytest.raises(RuntimeError, match=r"`vertices` must be a tensor of shape \(N,3\)"):
            call(torch.zeros(4, 2), f)
    with pytest.raises(RuntimeError, match="outside the"):
        mcl.remove_degenerate_triangles(torch.tensor([[0, -1, 2]]))
    nan = v.clone()
    nan[1, 1] = float("nan")
    with pytest.raises(RuntimeError, match="`vertices` holds non-finite values"):
        mcl.get_connected_mesh(nan, f)
    for bad in (torch.zeros(1, dtype=torch.uint8), torch.zeros(2, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.bool), [False]):
        with pytest.raises(RuntimeError, match="`remove` must be a bool tensor"):
            mcl.remove_triangles_by_mask(v, f, bad)


def test_no_face_returns_empties_without_a_launch(monkeypatch):
    import diff_gaussian_rasterization._C as C
    monkeypatch.setattr(C, "_require_gpu", lambda t, name: None)
    monkeypatch.setattr(mcl, "_lib", lambda: pytest.fail("the library was called"))
    v, f = torch.zeros(4, 3), torch.zeros((0, 3), dtype=torch.int64)
    labels, counts, area = mcl.cluster_connected_triangles(f, v)
    assert labels.shape == (0,) and labels.dtype == torch.int64 and counts.shape == (0,) and area.shape == (0,) and area.dtype == torch.float64
    assert mcl.cluster_connected_triangles(f)[2] is None
    for call in (mcl.post_process_mesh, mcl.get_connected_mesh):
        v1, f1, kept = call(v, f)
        assert v1.shape == (0, 3) and v1.dtype == v.dtype and f1.shape == (0, 3) and f1.dtype == torch.int64 and kept.shape == (0,)
    assert mcl.remove_degenerate_triangles(f).shape == (0, 3)
    assert mcl.compute_vertex_normals(v[:0], f).shape == (0, 3)


# ----------------------------------------------------------------------------- write_ply -----------------------------------------------------------------------------
def _expected_ply(v, f, colors=None):
    """the documented layout, written out here: what tsdf.write_ply produced before it had the `normals` keyword"""
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(v)
    if colors is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f)
    body = b""
    for i, p in enumerate(v):
        body += np.asarray(p, "<f4").tobytes()
        if colors is not None:
            body += np.rint(np.clip(np.asarray(colors[i], np.float64), 0.0, 1.0) * 255.0).astype(np.uint8).tobytes()
    for t in f:
        body += b"\x03" + np.asarray(t, "<i4").tobytes()
    return head.encode("ascii") + body


def test_write_ply_without_normals_is_byte_identical(tmp_path):
    rng = np.random.default_rng(4)
    v, f = rng.standard_normal((7, 3)), np.array([[0, 1, 2], [2, 1, 3], [4, 5, 6]], np.int64)
    colors = rng.uniform(-0.1, 1.1, (7, 3))
    path = str(tmp_path / "m.ply")
    tsdf.write_ply(path, torch.from_numpy(v), torch.from_numpy(f))
    assert open(path, "rb").read() == _expected_ply(v, f)
    tsdf.write_ply(path, v.astype(np.float32), f, colors=torch.from_numpy(colors))
    assert open(path, "rb").read() == _expected_ply(v, f, colors)
    tsdf.write_ply(path, v, f, colors, None)
    assert open(path, "rb").read() == _expected_ply(v, f, colors)
    tsdf.write_ply(path, v[:0], f[:0])
    assert open(path, "rb").read() == _expected_ply(v[:0], f[:0])


def read_ply_with_normals(path):
    """(vertices, normals or None, colors uint8 or None, faces) of a file tsdf.write_ply wrote"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in head if l.startswith("element face")][0].split()[-1])
    props = [l.split()[1:] for l in head if l.startswith("property") and "list" not in l]
    dtype = np.dtype([(name, {"float": "<f4", "uchar": "u1"}[kind]) for kind, name in props])
    vrec = np.frombuffer(data, dtype=dtype, count=nv, offset=end)
    frec = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=nf, offset=end + dtype.itemsize * nv)
    assert end + dtype.itemsize * nv + 13 * nf == len(data) and (frec["n"] == 3).all()
    cols = lambda names: np.stack([vrec[n] for n in names], 1) if names[0] in dtype.names else None
    return cols(["x", "y", "z"]), cols(["nx", "ny", "nz"]), cols(["red", "green", "blue"]), frec["v"].astype(np.int64)


def test_write_ply_with_normals_reads_back(tmp_path):
    rng = np.random.default_rng(5)
    v, f = rng.standard_normal((7, 3)).astype(np.float32), np.array([[0, 1, 2], [2, 1, 3], [4, 5, 6]], np.int64)
    n = rng.standard_normal((7, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    colors = rng.uniform(0.0, 1.0, (7, 3))
    path = str(tmp_path / "n.ply")
    tsdf.write_ply(path, v, f, normals=torch.from_numpy(n))
    head = open(path, "rb").read().split(b"end_header\n")[0].decode("ascii")
    assert "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nelement face" in head
    v1, n1, c1, f1 = read_ply_with_normals(path)
    assert np.array_equal(v1, v) and np.array_equal(n1, n.astype(np.float32)) and c1 is None and np.array_equal(f1, f)
    tsdf.write_ply(path, v, f, colors=colors, normals=n)
    v2, n2, c2, f2 = read_ply_with_normals(path)
    assert np.array_equal(v2, v) and np.array_equal(n2, n.astype(np.float32)) and np.array_equal(f2, f)
    assert np.array_equal(c2, np.rint(colors * 255.0).astype(np.uint8))
    with pytest.raises(RuntimeError, match="`normals` must have one row per vertex"):
        tsdf.write_ply(path, v, f, normals=n[:6])


# ------------------------------------------------------------------------- packaging, resources -------------------------------------------------------------------------
def test_module_is_packaged_and_built():
    setup = open(os.path.join(ROOT, "rade-gs_amd", "setup.py")).read()
    assert '"mesh_clean"' in re.search(r"py_modules=\[([^\]]*)\]", setup).group(1)
    build = open(os.path.join(ROOT, "rade-gs_amd", "build.py")).read()
    assert '"radegs_meshclean": ["radegs_meshclean.hip"' in build
    assert "radegs_meshclean" not in re.search(r"UNIT_FLAGS = \{[^}]*\}", build).group(0)        # -ffp-contract=off stays on for this unit


@_needs_llvm_tools
def test_meshclean_kernels_use_no_scratch(code_objects):  # noqa: F811
    found = {k: v[0] for k, v in code_objects.items() if "4rgmc" in k}            # namespace rgmc: radegs_meshclean.hip
    for part in KERNELS:
        hits = [k for k in found if "4rgmc%d%sE" % (len(part), part) in k]
        assert len(hits) == 1, (part, sorted(found))
        assert found[hits[0]]["scratch"] == 0, (hits[0], found[hits[0]])
    assert len(found) == len(KERNELS), sorted(found)
