"""CPU tier of mesh evaluation: the library exports the new entry points and include/radegs.h declares them, the Python layer has the
call surface the issue names and refuses bad arguments before any launch, the workspace sizes are host arithmetic, and the new kernels
use no scratch (read from the code objects inside the in-tree library the way tests/test_kernel_resources.py reads the hot kernels)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from test_kernel_resources import code_objects  # noqa: F401  (the fixture) -- and its skip condition:
from test_kernel_resources import pytestmark as _needs_llvm_tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("radegs_mesheval_sample_bytes", "radegs_mesheval_sample_count", "radegs_mesheval_sample_emit", "radegs_mesheval_grid_bytes",
           "radegs_mesheval_grid_build", "radegs_mesheval_thin_rounds", "radegs_mesheval_nearest", "radegs_mesheval_sum_bytes",
           "radegs_mesheval_sum_below", "radegs_mesheval_obs_mask", "radegs_mesheval_above_plane", "radegs_mesheval_dilate",
           "radegs_mesheval_cull_vertices", "radegs_tetmesh_filter_plan_flags")
KERNELS = ("tri_count_kernel", "tri_emit_kernel", "cell_key_kernel", "reorder_kernel", "thin_round_kernel", "nearest_kernel", "below_partial_kernel",
           "below_final_kernel", "obs_mask_kernel", "plane_side_kernel", "dilate_kernel", "cull_vertices_kernel")


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
    assert "typedef struct RadegsCullCamera" in header
    import mesh_eval
    assert ctypes.sizeof(mesh_eval.RadegsCullCamera) == 64


def test_sizes_and_argument_checks_run_without_a_device():
    """workspace sizes are host arithmetic and monotone; every rejection below returns before the first HIP call"""
    _, L = _library()
    ll, vp, sz, f64, i32 = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_int
    d3 = ctypes.POINTER(ctypes.c_double)
    for fn in (L.radegs_mesheval_sample_bytes, L.radegs_mesheval_grid_bytes):
        fn.restype, fn.argtypes = sz, [ll]
    L.radegs_mesheval_sum_bytes.restype = sz
    s = [L.radegs_mesheval_sample_bytes(n) for n in (1, 1000, 1_000_000, 50_000_000)]
    assert 0 < s[0] <= s[1] < s[2] < s[3] and 4 * 1_000_000 <= s[2] < 16 * 1_000_000              # the scan of the counts + its scratch
    g = [L.radegs_mesheval_grid_bytes(n) for n in (1, 1000, 1_000_000, 50_000_000)]
    assert 0 < g[0] <= g[1] < g[2] < g[3] and 36 * 1_000_000 <= g[2] < 64 * 1_000_000             # keys, permutation, 24-byte points, sort scratch
    assert L.radegs_mesheval_sample_bytes(0) == 0 and L.radegs_mesheval_grid_bytes(0) == 0 and L.radegs_mesheval_grid_bytes(2 ** 32) == 0
    assert L.radegs_mesheval_sum_bytes() >= 2 * 8 * 256
    L.radegs_mesheval_sample_count.argtypes = [ll, ll, vp, vp, f64, vp, sz, vp, vp, vp]
    L.radegs_mesheval_sample_emit.argtypes = [ll, ll, vp, vp, f64, vp, ll, vp, vp]
    L.radegs_mesheval_grid_build.argtypes = [ll, vp, d3, f64, vp, sz, vp]
    L.radegs_mesheval_thin_rounds.argtypes = [ll, vp, d3, f64, f64, i32, vp, vp, vp]
    L.radegs_mesheval_nearest.argtypes = [ll, vp, d3, f64, ll, vp, f64, vp, vp, vp]
    L.radegs_mesheval_sum_below.argtypes = [ll, vp, f64, vp, sz, vp, vp]
    L.radegs_mesheval_obs_mask.argtypes = [ll, vp, d3, ctypes.POINTER(i32), vp, vp, vp, vp, vp]
    L.radegs_mesheval_above_plane.argtypes = [ll, vp, d3, vp, vp]
    L.radegs_mesheval_dilate.argtypes = [i32, i32, vp, i32, vp, vp]
    L.radegs_mesheval_cull_vertices.argtypes = [ll, vp, i32, vp, vp, vp, vp]
    L.radegs_tetmesh_filter_plan_flags.argtypes = [ll, ll, vp, vp, vp, sz, vp, vp]
    fake, INVALID, TOO_LARGE = 0x1000, -1, -6
    origin, nan_origin = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(0, float("nan"), 0)
    assert L.radegs_mesheval_sample_count(10, 10, fake, fake, 0.0, fake, 1 << 40, fake, fake, None) == INVALID       # density
    assert L.radegs_mesheval_sample_count(10, 10, fake, fake, 0.2, fake, 1 << 40, fake, None, None) == INVALID       # no totals
    assert L.radegs_mesheval_sample_count(10, 2 ** 32, fake, fake, 0.2, fake, 1 << 40, fake, fake, None) == TOO_LARGE
    assert L.radegs_mesheval_sample_emit(10, 10, fake, fake, 0.2, fake, 0, None, None) == 0                          # nothing sampled: no launch
    assert L.radegs_mesheval_sample_emit(10, 10, fake, fake, 0.2, fake, 5, None, None) == INVALID
    assert L.radegs_mesheval_sample_emit(10, 10, fake, fake, 0.2, fake, 2 ** 32, fake, None) == TOO_LARGE
    assert L.radegs_mesheval_grid_build(0, fake, origin, 1.0, fake, 1 << 40, None) == 0
    assert L.radegs_mesheval_grid_build(10, fake, origin, 0.0, fake, 1 << 40, None) == INVALID                       # cell
    assert L.radegs_mesheval_grid_build(10, fake, nan_origin, 1.0, fake, 1 << 40, None) == INVALID
    assert L.radegs_mesheval_grid_build(10, fake, origin, 1.0, fake, 16, None) == INVALID                            # workspace too small
    assert L.radegs_mesheval_grid_build(10, fake, origin, 1.0, fake + 4, 1 << 40, None) == INVALID                   # not 16-byte aligned
    assert L.radegs_mesheval_grid_build(2 ** 32, fake, origin, 1.0, fake, 1 << 40, None) == TOO_LARGE
    assert L.radegs_mesheval_thin_rounds(10, fake, origin, 1.0, 1.5, 4, fake, fake, None) == INVALID                 # radius larger than a cell
    assert L.radegs_mesheval_thin_rounds(10, fake, origin, 1.0, 1.0, 0, fake, fake, None) == 0                       # no rounds: no launch
    assert L.radegs_mesheval_thin_rounds(10, fake, origin, 1.0, 1.0, 4, None, fake, None) == INVALID
    assert L.radegs_mesheval_nearest(10, fake, origin, 1.0, 0, None, 20.0, None, None, None) == 0                    # no queries
    assert L.radegs_mesheval_nearest(10, fake, origin, 1.0, 5, fake, float("inf"), fake, fake, None) == INVALID
    assert L.radegs_mesheval_nearest(10, fake, origin, 0.01, 5, fake, 20.0, fake, fake, None) == INVALID             # 2 000 shells
    assert L.radegs_mesheval_nearest(0, fake, origin, 1.0, 5, fake, 20.0, fake, fake, None) == INVALID               # an empty cloud has no nearest
    assert L.radegs_mesheval_sum_below(5, fake, 20.0, fake, 16, fake, None) == INVALID
    box = (ctypes.c_double * 10)(*([0.0] * 9 + [0.5]))
    assert L.radegs_mesheval_obs_mask(5, fake, box, (i32 * 3)(4, 0, 4), fake, fake, fake, fake, None) == INVALID
    assert L.radegs_mesheval_obs_mask(5, fake, (ctypes.c_double * 10)(), (i32 * 3)(4, 4, 4), fake, fake, fake, fake, None) == INVALID   # Res = 0
    assert L.radegs_mesheval_obs_mask(0, None, box, (i32 * 3)(4, 4, 4), None, None, None, None, None) == 0
    assert L.radegs_mesheval_above_plane(5, fake, None, fake, None) == INVALID
    assert L.radegs_mesheval_dilate(0, 5, fake, 6, fake, None) == INVALID and L.radegs_mesheval_dilate(5, 5, fake, 65, fake, None) == INVALID
    assert L.radegs_mesheval_cull_vertices(5, fake, 2, None, fake, fake, None) == INVALID
    assert L.radegs_mesheval_cull_vertices(0, None, 2, None, None, None, None) == 0
    assert L.radegs_tetmesh_filter_plan_flags(10, 10, fake, fake, fake, 16, fake, None) == INVALID
    assert L.radegs_tetmesh_filter_plan_flags(2 ** 32, 0, fake, fake, fake, 1 << 40, fake, None) == TOO_LARGE


def test_python_surface():
    import mesh_eval as me
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(me.sample_mesh_points) == ["vertices", "faces", "density"] and inspect.signature(me.sample_mesh_points).parameters["density"].default == 0.2
    assert sig(me.downsample_points) == ["points", "radius", "perm", "generator"]
    assert sig(me.PointGrid.__init__) == ["self", "points", "cell"] and sig(me.PointGrid.nearest) == ["self", "queries", "max_dist"]
    assert sig(me.obs_mask_select) == ["points", "obs_mask", "BB", "Res", "patch"] and sig(me.above_plane) == ["points", "plane"]
    p = inspect.signature(me.dtu_chamfer).parameters
    assert list(p)[:7] == ["vertices", "faces", "stl_points", "obs_mask", "BB", "Res", "plane"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("density", "patch_size", "max_dist", "perm"))
    assert (p["density"].default, p["patch_size"].default, p["max_dist"].default, p["perm"].default) == (0.2, 60, 20, None)
    assert sig(me.dilate_mask) == ["mask", "radius"] and inspect.signature(me.dilate_mask).parameters["radius"].default == 6
    assert sig(me.cull_mesh) == ["vertices", "faces", "cameras", "masks", "dilation"]


def test_bad_arguments_raise_before_any_launch():
    import mesh_eval as me
    v, f = torch.zeros(4, 3, dtype=torch.float64), torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        me.sample_mesh_points(v, f)
    with pytest.raises(RuntimeError, match="must be float64"):
        me.sample_mesh_points(v.float(), f)
    with pytest.raises(RuntimeError, match=r"shape \(N,3\)"):
        me.sample_mesh_points(torch.zeros(4, 2, dtype=torch.float64), f)
    with pytest.raises(RuntimeError, match="`faces` must be"):
        me.sample_mesh_points(v, f.float())
    with pytest.raises(RuntimeError, match="`faces` must be"):
        me.sample_mesh_points(v, torch.zeros(3, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        me.downsample_points(v, 0.2)
    with pytest.raises(RuntimeError, match="must be float64"):
        me.PointGrid(v.float(), 1.0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        me.PointGrid(v, 1.0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        me.obs_mask_select(v, torch.ones(2, 2, 2, dtype=torch.uint8), [[0, 0, 0], [1, 1, 1]], 0.5)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        me.above_plane(v, [0, 0, 1, 0])
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        me.dtu_chamfer(v, f, v, torch.ones(2, 2, 2, dtype=torch.uint8), [[0, 0, 0], [1, 1, 1]], 0.5, [0, 0, 1, 0])
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        me.dilate_mask(torch.ones(5, 5))
    import geom_host
    for bad in (True, 0, -1.0, float("nan"), float("inf"), "1", None):       # density, cell, max_dist, radius: bools are no numbers here
        with pytest.raises(RuntimeError, match="`density` must be a positive finite number"):
            geom_host.positive(bad, "density")
    assert geom_host.positive(3, "density") == 3.0
    with pytest.raises(RuntimeError, match="float32 or float64"):
        me.cull_mesh(v.half(), f, [])
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        me.cull_mesh(v, f, [])


def test_module_is_packaged_and_built():
    setup = open(os.path.join(ROOT, "rade-gs_amd", "setup.py")).read()
    mods = re.search(r"py_modules=\[([^\]]*)\]", setup).group(1)
    assert '"mesh_eval"' in mods and '"tetmesh"' in mods
    build = open(os.path.join(ROOT, "rade-gs_amd", "build.py")).read()
    assert '"radegs_mesheval": ["radegs_mesheval.hip"' in build
    assert "radegs_mesheval" not in re.search(r"UNIT_FLAGS = \{[^}]*\}", build).group(0)      # -ffp-contract=off stays on for this unit


@_needs_llvm_tools
def test_mesheval_kernels_use_no_scratch(code_objects):  # noqa: F811
    found = {k: v[0] for k, v in code_objects.items() if "4rgme" in k}          # namespace rgme: radegs_mesheval.hip
    for part in KERNELS:
        hits = [k for k in found if "4rgme%d%sE" % (len(part), part) in k]
        assert len(hits) == 1, (part, sorted(found))
        assert found[hits[0]]["scratch"] == 0, (hits[0], found[hits[0]])
    assert len(found) == len(KERNELS), sorted(found)
