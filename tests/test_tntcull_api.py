"""CPU tier of the Tanks-and-Temples mesh culling: the library exports the new entry points and include/radegs.h declares them, tnt_cull.py has
the call surface the issue names and refuses bad arguments before any launch, the C entry points refuse theirs before the first HIP call,
the host-side pose handling agrees with the restatement, and the new kernels use no scratch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import tntcull_restatement as tc
from test_kernel_resources import code_objects  # noqa: F401  (the fixture) -- and its skip condition:
from test_kernel_resources import pytestmark as _needs_llvm_tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("radegs_tntcull_render_bytes", "radegs_tntcull_render_begin", "radegs_tntcull_render_finish", "radegs_tntcull_count_views")
KERNELS = ("clear_kernel", "resolve_kernel", "setup_kernel", "drain_kernel", "count_views_kernel")
K = (50.0, 50.0, 31.5, 23.5)


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
    assert "SURVEY.md 8f N11" in header


def test_sizes_and_argument_checks_run_without_a_device():
    _, L = _library()
    ll, vp, sz, f64, f32, i32 = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_float, ctypes.c_int
    L.radegs_tntcull_render_bytes.restype, L.radegs_tntcull_render_bytes.argtypes = sz, [ll, i32]
    L.radegs_tntcull_render_begin.argtypes = [ll, ll, vp, vp, i32, vp, i32, i32, f64, f64, f64, f64, f64, f64, vp, sz, vp, vp]
    L.radegs_tntcull_render_finish.argtypes = [ll, ll, vp, vp, i32, vp, i32, i32, f64, f64, f64, f64, f64, f64, vp, sz, vp, vp, vp]
    L.radegs_tntcull_count_views.argtypes = [ll, vp, i32, i32, i32, vp, vp, f32, f32, f32, f32, f32, vp, vp]
    header = L.radegs_tntcull_render_bytes(0, 0)
    assert 0 < header <= 256 and L.radegs_tntcull_render_bytes(-1, 1) == 0
    assert L.radegs_tntcull_render_bytes(10, 3) == header + 256 * 4                     # 60 entries of 16 bytes, in 256-byte steps
    assert L.radegs_tntcull_render_bytes(10_000_000, 8) == header + 16 * (1 << 20)      # capped: a chunk that finds the queue full is drawn in place
    fake, INVALID, TOO_LARGE = 0x1000, -1, -6

    def begin(V=8, F=4, v=fake, f=fake, B=2, cams=fake, H=48, W=64, znear=0.01, zfar=20.0, ws=fake, nbytes=1 << 20, depth=fake, fx=50.0):
        return L.radegs_tntcull_render_begin(V, F, v, f, B, cams, H, W, fx, 50.0, 31.5, 23.5, znear, zfar, ws, nbytes, depth, None)

    def finish(V=8, F=4, v=fake, f=fake, B=2, cams=fake, H=48, W=64, znear=0.01, zfar=20.0, ws=fake, nbytes=1 << 20, depth=fake):
        return L.radegs_tntcull_render_finish(V, F, v, f, B, cams, H, W, 50.0, 50.0, 31.5, 23.5, znear, zfar, ws, nbytes, depth, None, None)
    for call in (begin, finish):
        assert call(B=0) == 0                                                          # no view: no launch
        assert call(znear=0.0) == INVALID and call(znear=-1.0) == INVALID and call(znear=float("nan")) == INVALID
        assert call(zfar=0.01) == INVALID and call(zfar=float("inf")) == INVALID
        assert call(H=1) == INVALID and call(W=1) == INVALID and call(W=32769) == INVALID
        assert call(V=-1) == INVALID and call(F=-1) == INVALID and call(B=-1) == INVALID
        assert call(V=2 ** 31) == TOO_LARGE and call(F=2 ** 31) == TOO_LARGE and call(B=65536) == TOO_LARGE
        assert call(ws=None) == INVALID and call(nbytes=header - 1) == INVALID and call(ws=fake + 4) == INVALID
        assert call(depth=None) == INVALID and call(cams=None) == INVALID and call(v=None) == INVALID and call(f=None) == INVALID
    assert begin(fx=float("nan")) == INVALID

    def count(N=5, p=fake, B=2, H=48, W=64, d=fake, cams=fake, eps=0.005, counts=fake):
        return L.radegs_tntcull_count_views(N, p, B, H, W, d, cams, 50.0, 50.0, 31.5, 23.5, eps, counts, None)
    assert count(N=0) == 0 and count(B=0) == 0
    assert count(N=-1) == INVALID and count(B=-1) == INVALID and count(H=1) == INVALID and count(W=1) == INVALID and count(eps=float("nan")) == INVALID
    assert count(p=None) == INVALID and count(d=None) == INVALID and count(cams=None) == INVALID and count(counts=None) == INVALID


def test_python_surface():
    import tnt_cull as tcu
    sig = lambda f: list(inspect.signature(f).parameters)
    par = lambda f: inspect.signature(f).parameters
    assert sig(tcu.render_depth) == ["vertices", "faces", "c2w", "H", "W", "fx", "fy", "cx", "cy", "znear", "zfar", "pose"]
    p = par(tcu.render_depth)
    assert (p["znear"].default, p["zfar"].default, p["pose"].default) == (0.01, 20.0, "opengl")
    assert sig(tcu.point_masks) == ["points", "depths", "c2w", "fx", "fy", "cx", "cy", "eps", "min_views"]
    assert (par(tcu.point_masks)["eps"].default, par(tcu.point_masks)["min_views"].default) == (0.005, 20)
    assert sig(tcu.cull_mesh) == ["vertices", "faces", "c2w", "H", "W", "fx", "fy", "cx", "cy", "far", "eps", "min_views", "pose", "view_batch"]
    p = par(tcu.cull_mesh)
    assert [p[k].default for k in sig(tcu.cull_mesh)[3:]] == [1080, 1920, 1163.8678928442187, 1172.793101201448, 962.3120628412543, 542.0667209577691,
                                                             20.0, 0.005, 20, "opengl", None]             # cull_mesh.py:406-411, 125, 175


def test_poses_are_inverted_on_the_host_in_float64_as_the_restatement_does():
    import tnt_cull as tcu
    rng = np.random.default_rng(2)
    c2w = np.stack([tc.look_at(rng.standard_normal(3) * 3, rng.standard_normal(3)) for _ in range(5)])
    for pose in tcu.POSES:
        assert np.array_equal(tcu._world_to_camera(c2w, pose), tc.world_to_camera(c2w, pose))
        assert np.array_equal(tcu._world_to_camera([torch.from_numpy(m) for m in c2w], pose), tc.world_to_camera(c2w, pose))
    assert np.array_equal(tcu._world_to_camera(tc.to_opencv(c2w), "opencv"), tc.world_to_camera(c2w, "opengl"))
    assert tcu._world_to_camera(c2w.astype(np.float32)).dtype == np.float64 and tcu._world_to_camera([]).shape == (0, 4, 4)
    before = c2w.copy()
    tcu._world_to_camera(c2w, "opencv")
    assert np.array_equal(c2w, before)                                                                   # the caller's matrices are not written to


def test_bad_arguments_raise_before_any_launch():
    import tnt_cull as tcu
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2]])
    c2w, d = np.eye(4)[None], torch.zeros(1, 48, 64)
    for call in (lambda: tcu.render_depth(v, f, c2w, 48, 64, *K), lambda: tcu.point_masks(v, d, c2w, *K), lambda: tcu.cull_mesh(v, f, c2w),
                 lambda: tcu.render_depth(v.double(), f, c2w, 48, 64, *K), lambda: tcu.cull_mesh(v, f[:0], c2w, view_batch=3)):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()
    for bad in (0, 0.0, -0.01, float("nan"), "1"):
        with pytest.raises(RuntimeError, match="`znear` must be"):
            tcu.render_depth(v, f, c2w, 48, 64, *K, znear=bad)
    for near, far in ((0.01, 0.01), (1.0, 0.5), (0.01, float("inf"))):
        with pytest.raises(RuntimeError, match="`zfar` must be"):
            tcu.render_depth(v, f, c2w, 48, 64, *K, znear=near, zfar=far)
    with pytest.raises(RuntimeError, match="`zfar` must be"):
        tcu.cull_mesh(v, f, c2w, far=0.01)
    for H, W, name in ((1, 64, "H"), (48, 1, "W"), (48.0, 64, "H"), (48, 40000, "W")):
        with pytest.raises(RuntimeError, match=f"`{name}` must be an integer"):
            tcu.render_depth(v, f, c2w, H, W, *K)
        with pytest.raises(RuntimeError, match=f"`{name}` must be an integer"):
            tcu.cull_mesh(v, f, c2w, H=H, W=W)
    with pytest.raises(RuntimeError, match="`fx` must be a finite number"):
        tcu.render_depth(v, f, c2w, 48, 64, float("nan"), 50.0, 31.5, 23.5)
    with pytest.raises(RuntimeError, match="`cy` must be a finite number"):
        tcu.point_masks(v, d, c2w, 50.0, 50.0, 31.5, None)
    with pytest.raises(RuntimeError, match="`pose` must be one of"):
        tcu.render_depth(v, f, c2w, 48, 64, *K, pose="blender")
    with pytest.raises(RuntimeError, match="`pose` must be one of"):
        tcu.cull_mesh(v, f, c2w, pose=None)
    singular = np.eye(4)[None].copy()
    singular[0, :3, :3] = [[1, 2, 3], [2, 4, 6], [0, 0, 1]]
    projective = np.eye(4)[None].copy()
    projective[0, 3, 0] = 0.1
    nan = np.eye(4)[None].copy()
    nan[0, 0, 3] = np.nan
    for bad, what in ((singular, "not invertible"), (np.zeros((1, 4, 4)), "must be affine"), (projective, "must be affine"),
                      (nan, "non-finite"), (np.eye(3)[None], "stack of 4x4"), ("poses", "stack of 4x4")):
        for call in (lambda: tcu.render_depth(v, f, bad, 48, 64, *K), lambda: tcu.point_masks(v, d, bad, *K), lambda: tcu.cull_mesh(v, f, bad)):
            with pytest.raises(RuntimeError, match=what):
                call()
    for bad in (0, -2, 2.5, True):
        with pytest.raises(RuntimeError, match="`view_batch` must be a positive integer"):
            tcu.cull_mesh(v, f, c2w, view_batch=bad)
    for bad in (20.0, None, True):
        with pytest.raises(RuntimeError, match="`min_views` must be an integer"):
            tcu.point_masks(v, d, c2w, *K, min_views=bad)
    with pytest.raises(RuntimeError, match="`eps` must be a finite number"):
        tcu.cull_mesh(v, f, c2w, eps=float("inf"))


def test_module_is_packaged_and_built():
    setup = open(os.path.join(ROOT, "rade-gs_amd", "setup.py")).read()
    assert '"tnt_cull"' in re.search(r"py_modules=\[([^\]]*)\]", setup).group(1)
    build = open(os.path.join(ROOT, "rade-gs_amd", "build.py")).read()
    assert '"radegs_tntcull": ["radegs_tntcull.hip"' in build
    assert "radegs_tntcull" not in re.search(r"UNIT_FLAGS = \{[^}]*\}", build).group(0)          # -ffp-contract=off stays on for this unit


@_needs_llvm_tools
def test_tntcull_kernels_use_no_scratch(code_objects):  # noqa: F811
    found = {k: v[0] for k, v in code_objects.items() if "4rgtc" in k}            # namespace rgtc: radegs_tntcull.hip
    for part in KERNELS:
        hits = [k for k in found if "4rgtc%d%sE" % (len(part), part) in k]
        assert len(hits) == 1, (part, sorted(found))
        assert found[hits[0]]["scratch"] == 0, (hits[0], found[hits[0]])
    assert len(found) == len(KERNELS), sorted(found)
