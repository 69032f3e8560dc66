"""CPU tier of evaluation from files, part two: the library exports the new entry points and include/radegs.h declares them,
the C entry points refuse bad arguments before the first HIP call, eval_io / tnt_eval / tnt_cull / mesh_eval have the call surface the issue
names, files that must be refused are refused with a message that names the reason -- all before any device call -- and the new kernels use
no scratch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import evalio_restatement as er
from test_kernel_resources import code_objects  # noqa: F401  (the fixture) -- and its skip condition:
from test_kernel_resources import pytestmark as _needs_llvm_tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("radegs_evalio_unpack_points", "radegs_evalio_unpack_faces", "radegs_evalio_ransac")
KERNELS = ("unpack_points_kernel", "unpack_faces_kernel", "ransac_eval_kernel", "ransac_select_kernel")


def _library():
    import diff_gaussian_rasterization._C as C
    return C, ctypes.CDLL(C._LIB_PATH)


def test_library_exports_and_header_declares_the_entry_points():
    import eval_io
    C, L = _library()
    header = open(os.path.join(ROOT, "include", "radegs.h")).read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in C.EXPORTED_SYMBOLS and sym in eval_io.SIGNATURES, sym
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
    assert "SURVEY.md 8f N18" in header
    for name, value in (("CHUNK", eval_io.RANSAC_CHUNK), ("MIN_N", eval_io.RANSAC_MIN_N), ("MAX_N", eval_io.RANSAC_MAX_N)):
        assert int(re.search(r"#define RADEGS_EVALIO_RANSAC_%s (\d+)" % name, header).group(1)) == value
    assert eval_io.MAX_RECORD == int(re.search(r"#define RADEGS_MODELIO_MAX_RECORD (\d+)", header).group(1))


def test_c_entry_points_refuse_bad_arguments_before_the_first_hip_call():
    import eval_io
    _, L = _library()
    for sym in SYMBOLS:
        getattr(L, sym).restype, getattr(L, sym).argtypes = eval_io.SIGNATURES[sym]
    fake, INVALID, TOO_LARGE = 0x1000, -1, -6
    i3 = ctypes.c_int * 3
    F4, F8, U1, I4, U4 = 6, 7, 1, 4, 5
    pts = lambda N, S, off, types, buf=fake, out=fake, at=0: L.radegs_evalio_unpack_points(N, S, buf, at, i3(*off), i3(*types), out, None)   # noqa: E731
    assert pts(0, 12, (0, 4, 8), (F4, F4, F4), None, None) == 0                               # nothing to do: no launch
    assert pts(5, 12, (0, 4, 9), (F4, F4, F4)) == INVALID                                     # z leaves the record
    assert pts(5, 24, (0, 8, 17), (F8, F8, F8)) == INVALID
    assert pts(5, 12, (0, 4, 8), (F4, F4, 8)) == INVALID                                      # no such type
    assert pts(5, 0, (0, 0, 0), (U1, U1, U1)) == INVALID and pts(5, 769, (0, 4, 8), (F4, F4, F4)) == INVALID
    assert pts(-1, 12, (0, 4, 8), (F4, F4, F4)) == INVALID and pts(5, 12, (0, 4, 8), (F4, F4, F4), at=-1) == INVALID
    assert pts(5, 12, (0, 4, 8), (F4, F4, F4), buf=fake + 2) == INVALID                       # the buffer itself is dword aligned
    assert pts(5, 12, (0, 4, 8), (F4, F4, F4), out=None) == INVALID
    assert pts(2 ** 38, 12, (0, 4, 8), (F4, F4, F4)) == TOO_LARGE
    faces = lambda F, S, co, ct, io, it, V=10, bad=fake, buf=fake, out=fake: L.radegs_evalio_unpack_faces(F, S, buf, 0, co, ct, io, it, V, out, bad, None)  # noqa: E731
    assert faces(5, 13, 0, U1, 1, I4, bad=None) == INVALID
    assert faces(5, 13, 0, F4, 4, I4) == INVALID and faces(5, 13, 0, U1, 1, U1) == INVALID   # a float length; byte indices
    assert faces(5, 13, 0, U1, 2, I4) == INVALID and faces(5, 13, 13, U1, 1, I4) == INVALID  # the list leaves the record
    assert faces(5, 13, 0, U1, 1, U4, V=-1) == INVALID and faces(-1, 13, 0, U1, 1, I4) == INVALID
    src = lambda N, n, K, md=0.2, s=fake, c=fake: L.radegs_evalio_ransac(N, s, fake, md, n, K, 0, c, fake, fake, None)                         # noqa: E731
    assert src(5, 6, 10) == INVALID and src(10, 2, 10) == INVALID and src(10, 9, 10) == INVALID
    assert src(10, 6, 0) == INVALID and src(10, 6, 10, md=0.0) == INVALID and src(10, 6, 10, md=float("nan")) == INVALID
    assert src(10, 6, 10, md=float("inf")) == INVALID and src(10, 6, 10, s=None) == INVALID and src(10, 6, 10, c=None) == INVALID
    assert src(2 ** 31, 6, 10) == TOO_LARGE and src(10, 6, 2 ** 31) == TOO_LARGE


def test_call_surface():
    import eval_io
    import mesh_eval
    import tnt_cull
    import tnt_eval as te
    sig = lambda fn: list(inspect.signature(fn).parameters)                                   # noqa: E731
    par = lambda fn: inspect.signature(fn).parameters                                         # noqa: E731
    assert sig(eval_io.read_ply_points) == ["path", "device"] and sig(eval_io.read_ply_mesh) == ["path", "device"]
    assert par(eval_io.read_ply_points)["device"].default == "cuda"
    assert sig(eval_io.merge_vertices) == ["vertices", "faces", "digits"] and par(eval_io.merge_vertices)["digits"].default == 8
    assert sig(eval_io.gen_sparse_trajectory) == ["mapping", "traj"] and sig(eval_io.dtu_camera_centres) == ["calib_dir", "n"]
    assert par(eval_io.dtu_camera_centres)["n"].default == 64 and sig(eval_io.best_fit_transform) == ["A", "B"]
    assert sig(eval_io.load_dtu_masks) == ["dataset_dir", "scan"]
    assert sig(te.ransac_correspondence) == ["source", "target", "max_dist", "ransac_n", "max_iteration", "seed", "with_scaling", "return_all"]
    p = par(te.ransac_correspondence)
    assert [p[k].default for k in sig(te.ransac_correspondence)[2:]] == [0.2, 6, 100000, 0, True, False]
    assert sig(te.trajectory_alignment)[:5] == ["map_file", "traj_to_register", "gt_traj_col", "gt_trans", "seed"]
    assert sig(te.run_evaluation)[:5] == ["dataset_dir", "traj_path", "ply_path", "out_dir", "seed"]
    assert sig(tnt_cull.cull_mesh_file)[:3] == ["mesh_path", "traj_path", "out_path"]
    assert sig(mesh_eval.evaluate_dtu_mesh)[:7] == ["mesh_path", "cameras", "dataset_dir", "scan", "out_dir", "perm", "generator"]
    ref = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01, "Truck": 0.005}
    assert te.SCENES_TAU == ref


def test_ransac_refuses_bad_arguments_before_any_launch():
    import tnt_eval as te
    a = torch.zeros(10, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        te.ransac_correspondence(a, a)
    for bad in (2, 9, 6.0, True):
        with pytest.raises(RuntimeError, match="`ransac_n` must be an integer in \\[3, 8\\]"):
            te.ransac_correspondence(a, a, ransac_n=bad)
    for bad in (0, -0.2, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="`max_dist` must be"):
            te.ransac_correspondence(a, a, max_dist=bad)
    with pytest.raises(RuntimeError, match="`max_iteration` must be"):
        te.ransac_correspondence(a, a, max_iteration=0)
    with pytest.raises(RuntimeError, match="`seed` must be"):
        te.ransac_correspondence(a, a, seed=-1)
    with pytest.raises(RuntimeError, match="`with_scaling` must be True"):
        te.ransac_correspondence(a, a, with_scaling=False)
    with pytest.raises(RuntimeError, match="must be float64"):
        te.ransac_correspondence(a.float(), a)
    with pytest.raises(RuntimeError, match=r"shape \(N,3\)"):
        te.ransac_correspondence(a[:, :2], a)
    with pytest.raises(RuntimeError, match="4x4"):
        te.trajectory_alignment(None, np.tile(np.eye(4), (8, 1, 1)), np.tile(np.eye(4), (8, 1, 1)), np.eye(3))
    with pytest.raises(RuntimeError, match="8 poses to register against 7"):
        te.trajectory_alignment(None, np.tile(np.eye(4), (8, 1, 1)), np.tile(np.eye(4), (7, 1, 1)), None)
    with pytest.raises(RuntimeError, match="invalid dataset_dir"):
        te.run_evaluation("/data/Nowhere", "traj.log", "mesh.ply")
    with pytest.raises(RuntimeError, match="json.*not supported"):
        te.run_evaluation("/data/Barn/", "transforms.json", "mesh.ply")


def test_merge_vertices_and_the_unpack_wrappers_refuse_cpu_tensors():
    import eval_io
    v, f = torch.zeros(4, 3, dtype=torch.float64), torch.tensor([[0, 1, 2]])
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        eval_io.merge_vertices(v, f)
    with pytest.raises(RuntimeError, match="`digits` must be"):
        eval_io.merge_vertices(v, f, digits=-1)
    with pytest.raises(RuntimeError, match="must be float64"):
        eval_io.merge_vertices(v.float(), f)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        eval_io.unpack_points(torch.zeros(64, dtype=torch.uint8), 0, 4, 12, [(0, "f4"), (4, "f4"), (8, "f4")])
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        eval_io.unpack_faces(torch.zeros(64, dtype=torch.uint8), 0, 4, 13, 0, "u1", 1, "i4", 3)


# ------------------------------------------------------------------ files that must be refused, by reason ------------------------------------------------------------------
def _refused(tmp_path, name, elements, match, mesh=True, **kw):
    import eval_io
    path = str(tmp_path / name)
    er.write_ply(path, elements, **kw)
    with pytest.raises(RuntimeError, match=match):
        (eval_io.read_ply_mesh if mesh else eval_io.read_ply_points)(path)


def test_files_are_refused_with_the_reason_before_any_device_call(tmp_path):
    v, f = er.mesh_data(9, 7, seed=1)
    xyz, cols = er._xyz(v, "f4")
    face = ("face", [("vertex_indices", ("list", "u1", "i4"))], [f])
    strip = ("tristrips", [("vertex_indices", ("list", "i4", "i4"))], [[[0, 1, 2, 3]]])
    for fmt in ("binary_little_endian", "binary_big_endian", "ascii"):
        kw = dict(fmt=fmt)
        _refused(tmp_path, "a.ply", [("vertex", xyz, cols), strip, face], "list property `vertex_indices` of element `tristrips`.*skipped", **kw)
        _refused(tmp_path, "b.ply", [("vertex", xyz, cols), face, strip], "list property `vertex_indices` of element `tristrips`.*skipped", **kw)
        _refused(tmp_path, "c.ply", [strip, ("vertex", xyz, cols), face], "list property `vertex_indices` of element `tristrips`.*fixed size", **kw)
        _refused(tmp_path, "d.ply", [("vertex", xyz[:2], cols[:2]), face], "`vertex` has no property `z`", **kw)
        _refused(tmp_path, "d.ply", [("vertex", xyz[1:], cols[1:])], "`vertex` has no property `x`", mesh=False, **kw)
        _refused(tmp_path, "e.ply", [("vertex", xyz, cols), face], "none of the three of PLY 1.0", version="1.1", **kw)
        _refused(tmp_path, "f.ply", [("vertex", xyz, cols)], "no `face` element", **kw)
        _refused(tmp_path, "g.ply", [("vertex", xyz, cols), face], "truncated|short payload", cut=60, **kw)
        _refused(tmp_path, "g.ply", [("vertex", xyz, cols)], "truncated|short payload", mesh=False, cut=60, **kw)
        _refused(tmp_path, "h.ply", [("vertex", xyz, cols), ("face", [("vertex_indices", ("list", "u1", "i2"))], [f])], "int32 and uint32 are read", **kw)
        _refused(tmp_path, "i.ply", [("vertex", xyz, cols), ("face", [("a", ("list", "u1", "i4")), ("vertex_indices", ("list", "u1", "i4"))], [f, f])],
                 "exactly one list property", **kw)
        quad = [list(r) for r in f]
        quad[3] = quad[3] + [0]                                                          # one quad: the element has four bytes too many
        _refused(tmp_path, "j.ply", [("vertex", xyz, cols), ("face", [("vertex_indices", ("list", "u1", "i4"))], [quad])], "not a triangle", **kw)
    path = tmp_path / "k.ply"
    path.write_bytes(b"ply\nformat binary_middle_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    import eval_io
    with pytest.raises(RuntimeError, match="format `binary_middle_endian` is none of"):
        eval_io.read_ply_points(str(path))
    path.write_bytes(b"not a ply")
    with pytest.raises(RuntimeError, match="not a PLY file"):
        eval_io.read_ply_points(str(path))


def test_load_dtu_masks_says_what_to_pass_without_scipy(monkeypatch, tmp_path):
    import builtins

    import eval_io
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.startswith("scipy"):
            raise ImportError(name)
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_scipy)
    with pytest.raises(RuntimeError, match="scipy is not installed.*pass them to mesh_eval.dtu_chamfer"):
        eval_io.load_dtu_masks(str(tmp_path), 24)


def test_module_is_packaged_and_built():
    setup = open(os.path.join(ROOT, "rade-gs_amd", "setup.py")).read()
    assert '"eval_io"' in re.search(r"py_modules=\[([^\]]*)\]", setup).group(1)
    build = open(os.path.join(ROOT, "rade-gs_amd", "build.py")).read()
    assert '"radegs_evalio": ["radegs_evalio.hip"' in build
    assert "radegs_evalio" not in re.search(r"UNIT_FLAGS = \{[^}]*\}", build).group(0)          # -ffp-contract=off stays on for this unit


@_needs_llvm_tools
def test_evalio_kernels_use_no_scratch(code_objects):  # noqa: F811
    found = {k: v[0] for k, v in code_objects.items() if "4rgev" in k}            # namespace rgev: radegs_evalio.hip
    for part in KERNELS:
        hits = [k for k in found if "4rgev%d%sE" % (len(part), part) in k]
        assert len(hits) == 1, (part, sorted(found))
        assert found[hits[0]]["scratch"] == 0, (hits[0], found[hits[0]])
    assert len(found) == len(KERNELS), sorted(found)
