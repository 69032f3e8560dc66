"""CPU tier of mesh extraction: the library exports the new entry points and include/radegs.h declares them, the Python layer has the
reference's call surface and refuses CPU tensors, write_ply round-trips, and the new kernels use no scratch (read from the code objects
inside the in-tree library the way tests/test_kernel_resources.py reads the hot kernels)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_kernel_resources import code_objects  # noqa: F401  (the fixture) -- and its skip condition:
from test_kernel_resources import pytestmark as _needs_llvm_tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("radegs_tetmesh_plan_bytes", "radegs_tetmesh_plan", "radegs_tetmesh_emit", "radegs_tetra_points", "radegs_cull_alpha_accumulate",
           "radegs_cull_alpha_finish", "radegs_tetmesh_bisect", "radegs_tetmesh_filter_plan_bytes", "radegs_tetmesh_filter_plan",
           "radegs_tetmesh_filter_apply")
KERNELS = ("occ_pack_kernel", "classify_kernel", "emit_edges_kernel", "head_kernel", "scatter_ids_kernel", "vertex_kernel",
           "face_kernel", "tetra_points_kernel", "cull_alpha_kernel", "cull_finish_kernel", "bisect_kernel", "keep_vertex_kernel", "keep_face_kernel",
           "filter_counts_kernel", "filter_apply_kernel")


def _library():
    import diff_gaussian_rasterization._C as C
    return C, ctypes.CDLL(C._LIB_PATH)


def test_library_exports_and_header_declares_the_entry_points():
    C, L = _library()
    header = open(os.path.join(ROOT, "include", "radegs.h")).read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in C.EXPORTED_SYMBOLS, sym
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % sym, header), sym
    assert re.search(r"#define\s+RADEGS_ERR_TOO_LARGE\s+\(-6\)", header)


def test_sizes_and_argument_checks_run_without_a_device():
    """workspace sizes are host arithmetic; every rejection below returns before the first HIP call"""
    _, L = _library()
    ll, vp, sz = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_size_t
    L.radegs_tetmesh_plan_bytes.restype = sz
    L.radegs_tetmesh_plan_bytes.argtypes = [ctypes.c_int, ll]
    L.radegs_tetmesh_filter_plan_bytes.restype = sz
    L.radegs_tetmesh_filter_plan_bytes.argtypes = [ll, ll]
    L.radegs_tetmesh_plan.argtypes = [ctypes.c_int, ll, vp, vp, vp, sz, vp, vp]
    L.radegs_tetmesh_emit.argtypes = [ctypes.c_int, ll, vp, vp, vp, vp, vp, ll, ll, vp, vp, vp, vp, vp, vp]
    L.radegs_tetmesh_filter_plan.argtypes = [ll, ll, vp, vp, vp, vp, sz, vp, vp]
    assert L.radegs_tetmesh_plan_bytes(0, 10) == 0 and L.radegs_tetmesh_plan_bytes(10, 0) == 0
    b = [L.radegs_tetmesh_plan_bytes(1000, t) for t in (100, 10_000, 1_000_000)]
    assert b[0] < b[1] < b[2] and 100 * 1_000_000 < b[2] < 250 * 1_000_000          # about 180 bytes per tet: 4 instances of 9 words + 36
    assert L.radegs_tetmesh_plan_bytes(9_000_000, 1000) >= 9_000_000 // 8            # the V-bit occupancy mask
    assert L.radegs_tetmesh_filter_plan_bytes(0, 0) == 0 and L.radegs_tetmesh_filter_plan_bytes(1000, 2000) >= 2 * 3000 * 4
    fake, INVALID, TOO_LARGE = 0x1000, -1, -6
    too_many = (2 ** 32 - 65536) // 5 + 1                                            # 5 T >= 2^32 - 65 536
    assert L.radegs_tetmesh_plan(10, too_many, fake, fake, fake, 1 << 40, fake, None) == TOO_LARGE
    assert L.radegs_tetmesh_plan_bytes(10, too_many) == 0
    assert L.radegs_tetmesh_plan(-1, 10, fake, fake, fake, 1 << 40, fake, None) == INVALID
    assert L.radegs_tetmesh_plan(10, 10, fake, fake, fake, 16, fake, None) == INVALID                    # workspace too small
    assert L.radegs_tetmesh_plan(10, 10, fake + 4, fake, fake, 1 << 40, fake, None) == INVALID           # tets not 16-byte aligned
    assert L.radegs_tetmesh_plan(10, 10, fake, fake, fake, 1 << 40, None, None) == INVALID               # no counts
    assert L.radegs_tetmesh_emit(10, 10, fake, fake, fake, fake, fake, 0, 0, None, None, None, None, None, None) == 0   # nothing crossed: no launch
    assert L.radegs_tetmesh_emit(10, 10, fake, fake, fake, fake, fake, 5, 0, None, None, None, None, None, None) == INVALID
    assert L.radegs_tetmesh_filter_plan(2 ** 32, 0, fake, fake, fake, fake, 1 << 40, fake, None) == TOO_LARGE
    assert L.radegs_tetmesh_filter_plan(10, 10, fake, fake, fake, fake, 16, fake, None) == INVALID


def test_python_surface_matches_the_reference():
    import tetmesh
    assert list(inspect.signature(tetmesh.marching_tetrahedra).parameters) == ["vertices", "tets", "sdf", "scales"]
    assert list(inspect.signature(tetmesh.marching_tetrahedra_with_binary_search).parameters) == ["points", "points_scale", "cells", "evaluate_sdf",
                                                                                                  "n_binary_steps"]
    assert inspect.signature(tetmesh.marching_tetrahedra_with_binary_search).parameters["n_binary_steps"].default == 8
    assert list(inspect.signature(tetmesh.evaluate_cull_alpha).parameters) == ["points", "views", "integrate_fn", "masks"]
    assert list(inspect.signature(tetmesh.CullAlpha.add_view).parameters) == ["self", "integrate_result", "view", "extra_mask"]
    for name in ("get_tetra_points", "write_ply", "CullAlpha"):
        assert hasattr(tetmesh, name), name
    v = torch.zeros(1, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        tetmesh.marching_tetrahedra(v, torch.tensor([[0, 1, 2, 3]]), torch.zeros(1, 4), torch.zeros(1, 4))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        tetmesh.tetra_points(torch.zeros(2, 3), torch.ones(2, 3), torch.ones(2, 4))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        tetmesh.CullAlpha(10, "cpu")
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        tetmesh.evaluate_cull_alpha(torch.zeros(3, 3), [], lambda p, v: None)


def test_module_is_packaged_next_to_graphics_utils():
    setup = open(os.path.join(ROOT, "rade-gs_amd", "setup.py")).read()
    mods = re.search(r"py_modules=\[([^\]]*)\]", setup).group(1)
    assert '"tetmesh"' in mods and '"graphics_utils"' in mods
    build = open(os.path.join(ROOT, "rade-gs_amd", "build.py")).read()
    assert '"radegs_tetmesh": ["radegs_tetmesh.hip"' in build


def test_write_ply_round_trips_through_a_numpy_reader(tmp_path):
    import tetmesh
    rng = np.random.default_rng(5)
    v = rng.standard_normal((37, 3)).astype(np.float32)
    f = rng.integers(0, 37, (61, 3)).astype(np.int64)
    path = str(tmp_path / "recon.ply")
    tetmesh.write_ply(path, torch.from_numpy(v), torch.from_numpy(f))
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    assert "element vertex 37" in lines and "element face 61" in lines and "property list uchar int vertex_indices" in lines
    assert len(body) == 37 * 12 + 61 * 13
    # an independent reader: plain numpy on the body
    assert np.array_equal(np.frombuffer(body, "<f4", 37 * 3).reshape(37, 3), v)
    rec = np.frombuffer(body, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), 61, 37 * 12)
    assert (rec["n"] == 3).all() and np.array_equal(rec["v"], f)
    v2, f2 = tetmesh.read_ply(path)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and f2.dtype == np.int64
    tetmesh.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))           # the empty mesh is a valid file
    v0, f0 = tetmesh.read_ply(path)
    assert v0.shape == (0, 3) and f0.shape == (0, 3)
    with pytest.raises(RuntimeError, match="face index"):
        tetmesh.write_ply(path, v, f + 40)


@pytest.mark.parametrize("name", ["tetmesh", "mesh_eval", "tsdf", "tnt_eval", "tnt_cull"])
def test_geometry_modules_bind_their_own_table(name):
    """every geometry module binds its own signature table through geom_host, any number of times, and borrows no private name from a sibling"""
    import importlib
    mod = importlib.import_module(name)
    L = mod._lib()
    assert mod._lib() is L
    assert mod._SIGNATURES, name
    for sym, (restype, argtypes) in mod._SIGNATURES.items():
        fn = getattr(L, sym)
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), sym
        assert fn.restype is restype, sym
    src = inspect.getsource(mod)
    assert not re.search(r"\b_bound\b", src), name
    siblings = "geom_host|tetmesh|mesh_eval|tsdf|tnt_eval|tnt_cull"
    for m in re.finditer(r"^from (%s) import (.+)$" % siblings, src, re.M):
        assert not [n for n in re.split(r"[,\s()]+", m.group(2)) if n.startswith("_")], m.group(0)
    assert not re.search(r"\b(gh|%s)\._[a-z]" % siblings, src), name


@_needs_llvm_tools
def test_tetmesh_kernels_use_no_scratch(code_objects):  # noqa: F811
    found = {k: v[0] for k, v in code_objects.items() if "3rgt" in k}          # namespace rgt: radegs_tetmesh.hip
    for part in KERNELS:
        hits = [k for k in found if "3rgt%d%sE" % (len(part), part) in k]
        assert len(hits) == 1, (part, sorted(found))
        r = found[hits[0]]
        assert r["scratch"] == 0, (hits[0], r)
        assert r["vgpr"] <= 64, (hits[0], r)    # streaming kernels: nothing may cost them the 8 waves per SIMD
    assert len(found) == len(KERNELS), sorted(found)
    # the gather between the two sorts of the edge pairs and the join of the sorted words live with rg::radix_sort_order_2xu32
    # (radegs_sort.hip): the same two limits
    for part in ("13gather_kernelE", "11join_kernelE"):
        hits = [k for k in code_objects if k.startswith("_ZN2rg") and part in k]
        assert len(hits) == 1, hits
        r = code_objects[hits[0]][0]
        assert r["scratch"] == 0, (hits[0], r)
        assert r["vgpr"] <= 64, (hits[0], r)
