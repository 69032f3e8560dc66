"""CPU tier of the Tanks-and-Temples evaluation: the library exports the new entry points and include/radegs.h declares them, tnt_eval.py has
the call surface the issue names and refuses bad arguments before any launch, the C entry points refuse theirs before the first HIP call,
umeyama (host code) agrees with the restatement, and the new kernels use no scratch."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import tnteval_restatement as tr
from test_kernel_resources import code_objects  # noqa: F401  (the fixture) -- and its skip condition:
from test_kernel_resources import pytestmark as _needs_llvm_tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("radegs_tnteval_centroids", "radegs_tnteval_transform", "radegs_tnteval_crop", "radegs_tnteval_voxel_bytes", "radegs_tnteval_voxel_plan",
           "radegs_tnteval_voxel_emit", "radegs_tnteval_sums_bytes", "radegs_tnteval_pair_sums", "radegs_tnteval_histogram")
KERNELS = ("centroid_kernel", "transform_kernel", "crop_kernel", "voxel_key_kernel", "first_kernel", "voxel_counts_kernel",
           "voxel_emit_kernel", "pair_sums_partial_kernel", "pair_sums_final_kernel", "pair_moments_partial_kernel", "pair_moments_final_kernel",
           "histogram_kernel")
POLY = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]


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
    assert "SURVEY.md 8f N10" in header


def test_sizes_and_argument_checks_run_without_a_device():
    _, L = _library()
    ll, vp, sz, f64, i32 = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_int
    d3 = ctypes.POINTER(ctypes.c_double)
    L.radegs_tnteval_voxel_bytes.restype, L.radegs_tnteval_voxel_bytes.argtypes = sz, [ll]
    L.radegs_tnteval_sums_bytes.restype = sz
    b = [L.radegs_tnteval_voxel_bytes(n) for n in (1, 1000, 1_000_000, 50_000_000)]
    assert 0 < b[0] <= b[1] < b[2] < b[3] and 36 * 1_000_000 <= b[2] < 64 * 1_000_000     # the 64-bit keys, seven word arrays, the sort's scratch
    assert L.radegs_tnteval_voxel_bytes(0) == 0 and L.radegs_tnteval_voxel_bytes(2 ** 32) == 0
    assert L.radegs_tnteval_sums_bytes() >= 10 * 8 * 1024
    L.radegs_tnteval_centroids.argtypes = [ll, ll, vp, vp, vp, vp]
    L.radegs_tnteval_transform.argtypes = [ll, vp, d3, vp, vp]
    L.radegs_tnteval_crop.argtypes = [ll, vp, i32, f64, f64, i32, vp, vp, vp]
    L.radegs_tnteval_voxel_plan.argtypes = [ll, vp, d3, f64, vp, sz, vp, vp]
    L.radegs_tnteval_voxel_emit.argtypes = [ll, vp, vp, ll, vp, vp, vp]
    L.radegs_tnteval_pair_sums.argtypes = [ll, vp, ll, vp, vp, vp, sz, vp, vp]
    L.radegs_tnteval_histogram.argtypes = [ll, vp, i32, vp, f64, vp, vp, vp]
    fake, INVALID, TOO_LARGE = 0x1000, -1, -6
    origin, nan_origin = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(0, float("nan"), 0)
    eye, nan_eye = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), (ctypes.c_double * 12)(*([float("nan")] * 12))
    assert L.radegs_tnteval_centroids(5, 0, None, None, None, None) == 0                                # no faces: no launch
    assert L.radegs_tnteval_centroids(5, 3, fake, None, fake, None) == INVALID
    assert L.radegs_tnteval_transform(0, None, eye, None, None) == 0
    assert L.radegs_tnteval_transform(5, fake, nan_eye, fake, None) == INVALID
    assert L.radegs_tnteval_transform(5, fake, None, fake, None) == INVALID
    assert L.radegs_tnteval_crop(5, fake, 3, 0.0, 1.0, 4, fake, fake, None) == INVALID                  # axis
    assert L.radegs_tnteval_crop(5, fake, 1, 0.0, 1.0, 2, fake, fake, None) == INVALID                  # two vertices are no polygon
    assert L.radegs_tnteval_crop(5, fake, 1, 0.0, 1.0, 1025, fake, fake, None) == TOO_LARGE             # the polygon is staged in LDS
    assert L.radegs_tnteval_crop(5, fake, 1, float("nan"), 1.0, 4, fake, fake, None) == INVALID
    assert L.radegs_tnteval_crop(0, None, 1, 0.0, 1.0, 4, None, None, None) == 0
    assert L.radegs_tnteval_crop(5, fake, 1, 0.0, 1.0, 4, None, fake, None) == INVALID
    assert L.radegs_tnteval_voxel_plan(10, fake, origin, 0.0, fake, 1 << 40, fake, None) == INVALID     # voxel
    assert L.radegs_tnteval_voxel_plan(10, fake, nan_origin, 1.0, fake, 1 << 40, fake, None) == INVALID
    assert L.radegs_tnteval_voxel_plan(10, fake, origin, 1.0, fake, 16, fake, None) == INVALID          # workspace too small
    assert L.radegs_tnteval_voxel_plan(10, fake, origin, 1.0, fake + 4, 1 << 40, fake, None) == INVALID
    assert L.radegs_tnteval_voxel_plan(2 ** 32, fake, origin, 1.0, fake, 1 << 40, fake, None) == TOO_LARGE
    assert L.radegs_tnteval_voxel_emit(10, fake, fake, 0, None, None, None) == 0                        # nothing to emit
    assert L.radegs_tnteval_voxel_emit(10, fake, fake, 11, fake, fake, None) == INVALID                 # more voxels than points
    assert L.radegs_tnteval_voxel_emit(10, fake, fake, 5, None, fake, None) == INVALID
    assert L.radegs_tnteval_pair_sums(5, fake, 5, fake, fake, fake, 16, fake, None) == INVALID
    assert L.radegs_tnteval_pair_sums(5, fake, 5, fake, fake, fake, 1 << 40, None, None) == INVALID
    assert L.radegs_tnteval_histogram(5, fake, 1, fake, 0.1, fake, fake, None) == INVALID               # one edge is no bin
    assert L.radegs_tnteval_histogram(5, fake, 4097, fake, 0.1, fake, fake, None) == TOO_LARGE
    assert L.radegs_tnteval_histogram(5, fake, 10, fake, 0.1, None, fake, None) == INVALID


def test_python_surface():
    import tnt_eval as te
    sig = lambda f: list(inspect.signature(f).parameters)
    par = lambda f: inspect.signature(f).parameters
    assert sig(te.mesh_points) == ["vertices", "faces"]
    assert sig(te.CropVolume.__init__) == ["self", "orthogonal_axis", "axis_min", "axis_max", "bounding_polygon"] and sig(te.CropVolume.from_json) == ["path"]
    assert sig(te.crop_points) == ["points", "volume", "transform"] and par(te.crop_points)["transform"].default is None
    assert sig(te.voxel_down_sample) == ["points", "voxel"] and sig(te.uniform_down_sample) == ["points", "k"] and sig(te.umeyama) == ["sums"]
    assert sig(te.icp) == ["source", "target", "max_dist", "max_iter", "relative_fitness", "relative_rmse", "cell"]
    p = par(te.icp)
    assert (p["max_iter"].default, p["relative_fitness"].default, p["relative_rmse"].default, p["cell"].default) == (20, 1e-6, 1e-6, None)
    assert sig(te.registration_vol_ds)[:7] == ["source", "gt_target", "init_trans", "volume", "voxel_size", "threshold", "max_itr"]
    assert sig(te.registration_unif)[:6] == ["source", "gt_target", "init_trans", "volume", "threshold", "max_itr"]
    assert sig(te.precision_recall) == ["dist_s", "dist_t", "threshold", "plot_stretch"] and par(te.precision_recall)["plot_stretch"].default == 5
    assert sig(te.evaluate)[:7] == ["vertices", "faces", "gt_points", "init_transform", "volume", "tau", "plot_stretch"]
    assert par(te.evaluate)["plot_stretch"].default == 5 and te.MAX_POINT_NUMBER == 4e6


def test_crop_volume_reads_the_selection_polygon_file(tmp_path):
    import tnt_eval as te
    path = tmp_path / "scene.json"
    path.write_text(json.dumps({"axis_max": 4.5, "axis_min": -1.25, "bounding_polygon": [[0, 9, 1], [2, 9, 0], [3, 9, 4], [1, 9, 2]],
                                "class_name": "SelectionPolygonVolume", "orthogonal_axis": "Y", "version_major": 1, "version_minor": 0}))
    vol = te.CropVolume.from_json(str(path))
    assert (vol.orthogonal_axis, vol.axis_min, vol.axis_max) == ("Y", -1.25, 4.5) and vol.bounding_polygon.shape == (4, 3) and vol.axes == (0, 2, 1)
    assert te.CropVolume("X", 0, 1, POLY).axes == (1, 2, 0) and te.CropVolume("Z", 0, 1, POLY).axes == (0, 1, 2)


def test_bad_arguments_raise_before_any_launch():
    import tnt_eval as te
    v, f = torch.zeros(4, 3, dtype=torch.float64), torch.tensor([[0, 1, 2]])
    vol = te.CropVolume("Y", 0.0, 1.0, POLY)
    with pytest.raises(RuntimeError, match="at least three vertices"):
        te.CropVolume("Y", 0.0, 1.0, POLY[:2])
    with pytest.raises(RuntimeError, match=r"shape \(n,3\)"):
        te.CropVolume("Y", 0.0, 1.0, [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    with pytest.raises(RuntimeError, match="must be finite"):
        te.CropVolume("Y", 0.0, float("inf"), POLY)
    with pytest.raises(RuntimeError, match="must be finite"):
        te.CropVolume("Y", 0.0, 1.0, [[0.0, 0.0, float("nan")]] + POLY[1:])
    for call in (lambda: te.mesh_points(v, f), lambda: te.crop_points(v, vol), lambda: te.voxel_down_sample(v, 0.1), lambda: te.uniform_down_sample(v, 2),
                 lambda: te.icp(v, v, 0.1), lambda: te.registration_vol_ds(v, v, np.eye(4), vol, 0.1, 0.5, 20),
                 lambda: te.registration_unif(v, v, np.eye(4), vol, 0.5, 20), lambda: te.precision_recall(v[:, 0], v[:, 0], 0.1),
                 lambda: te.evaluate(v, f, v, np.eye(4), vol, 0.1), lambda: te.transform_points(v, np.eye(4))):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()
    with pytest.raises(RuntimeError, match="must be float64"):
        te.mesh_points(v.float(), f)
    with pytest.raises(RuntimeError, match="`faces` must be"):
        te.mesh_points(v, f.float())
    with pytest.raises(RuntimeError, match=r"shape \(N,3\)"):
        te.crop_points(torch.zeros(4, 2, dtype=torch.float64), vol)
    with pytest.raises(RuntimeError, match="must be float64"):
        te.voxel_down_sample(v.float(), 0.1)
    with pytest.raises(RuntimeError, match="must be a CropVolume"):
        te.crop_points(v, dict(orthogonal_axis="Y"))
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "1", None):
        with pytest.raises(RuntimeError, match="`voxel` must be a positive finite number"):
            te.voxel_down_sample(v, bad)
    for bad in (0, -0.5, float("nan")):
        with pytest.raises(RuntimeError, match="`max_dist` must be"):
            te.icp(v, v, bad)
        with pytest.raises(RuntimeError, match="`tau` must be"):
            te.evaluate(v, f, v, np.eye(4), vol, bad)
        with pytest.raises(RuntimeError, match="`threshold` must be"):
            te.precision_recall(v[:, 0], v[:, 0], bad)
    with pytest.raises(RuntimeError, match="`cell` must be"):
        te.icp(v, v, 0.1, cell=0.0)
    with pytest.raises(RuntimeError, match="`max_iter` must be"):
        te.icp(v, v, 0.1, max_iter=-1)
    with pytest.raises(RuntimeError, match="`k` must be a positive integer"):
        te.uniform_down_sample(v, 0)
    bad_t = np.eye(4)
    bad_t[0, 3] = np.nan
    with pytest.raises(RuntimeError, match="finite 4x4"):
        te.crop_points(v, vol, bad_t)
    with pytest.raises(RuntimeError, match="finite 4x4"):
        te.registration_vol_ds(v, v, np.eye(3), vol, 0.1, 0.5, 20)
    proj = np.eye(4)
    proj[3, 0] = 0.1
    with pytest.raises(RuntimeError, match="must be affine"):
        te.evaluate(v, f, v, proj, vol, 0.1)
    with pytest.raises(RuntimeError, match="float64 vector"):
        te.precision_recall(v, v[:, 0], 0.1)
    with pytest.raises(RuntimeError, match="float64 vector"):
        te.precision_recall(v[:, 0].float(), v[:, 0], 0.1)
    with pytest.raises(RuntimeError, match="18 numbers"):
        te.umeyama(np.zeros(17))


def test_umeyama_from_the_sums_is_the_restatements():
    import tnt_eval as te
    rng = np.random.default_rng(11)
    s = rng.standard_normal((40, 3)) * [1.0, 2.0, 0.5] + [3.0, -1.0, 2.0]
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = 0.8 * q, [0.1, 0.2, -0.3]
    t = tr.transform(s, T) + 0.01 * rng.standard_normal((40, 3))

    def sums(s, t):
        n = s.shape[0]
        ds, dt = s - s.sum(0) / n, t - t.sum(0) / n
        return np.concatenate([[n], s.sum(0), t.sum(0), [((s - t) ** 2).sum()], (dt.T @ ds).reshape(-1), [(ds * ds).sum()]])
    got = te.umeyama(sums(s, t))
    assert np.allclose(got, tr.umeyama(s, t), rtol=1e-12, atol=1e-14) and np.array_equal(got[3], [0, 0, 0, 1])
    assert np.allclose(te.umeyama(sums(s, tr.transform(s, T))), T, rtol=0, atol=1e-12)
    assert np.array_equal(te.umeyama(sums(s[:2], t[:2])), np.eye(4)) and np.array_equal(te.umeyama(np.zeros(18)), np.eye(4))
    assert np.array_equal(te.umeyama(sums(np.ones((5, 3)), t[:5])), np.eye(4))                      # a source of no extent
    mirror = np.diag([1.0, 1.0, -1.0])                                                              # a reflected target still yields a rotation
    assert np.linalg.det(te.umeyama(sums(s, s @ mirror))[:3, :3]) > 0


def test_histogram_edges_and_the_cut():
    import tnt_eval as te
    tau = 0.003
    e = te.histogram_edges(tau, 5)
    assert np.array_equal(e, np.arange(0, tau * 5, tau / 100))
    cut = te.distance_cut(tau, 5)
    assert cut > e[-1] and np.nextafter(cut, 0) == e[-1]                                            # d == the last edge is still found (d < cut)
    assert te.distance_cut(tau, 0.5) > tau                                                          # a short histogram does not cut below tau


def test_module_is_packaged_and_built():
    setup = open(os.path.join(ROOT, "rade-gs_amd", "setup.py")).read()
    assert '"tnt_eval"' in re.search(r"py_modules=\[([^\]]*)\]", setup).group(1)
    build = open(os.path.join(ROOT, "rade-gs_amd", "build.py")).read()
    assert '"radegs_tnteval": ["radegs_tnteval.hip"' in build
    assert "radegs_tnteval" not in re.search(r"UNIT_FLAGS = \{[^}]*\}", build).group(0)          # -ffp-contract=off stays on for this unit


@_needs_llvm_tools
def test_tnteval_kernels_use_no_scratch(code_objects):  # noqa: F811
    found = {k: v[0] for k, v in code_objects.items() if "4rgte" in k}            # namespace rgte: radegs_tnteval.hip
    for part in KERNELS:
        hits = [k for k in found if "4rgte%d%sE" % (len(part), part) in k]
        assert len(hits) == 1, (part, sorted(found))
        assert found[hits[0]]["scratch"] == 0, (hits[0], found[hits[0]])
    assert len(found) == len(KERNELS), sorted(found)
