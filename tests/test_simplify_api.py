"""CPU tier of the mesh simplification unit: the library exports the entry points and include/radegs.h declares them, the size functions and
the argument checks of the C entry points run without a device, mesh_simplify.py has the call surface the header's block is written for and
refuses bad arguments before any launch, and the new kernels use no scratch."""
import inspect
import os
import re

import pytest
import torch

import mesh_simplify as ms
from test_kernel_resources import code_objects  # noqa: F401  (the fixture) -- and its skip condition:
from test_kernel_resources import pytestmark as _needs_llvm_tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("radegs_simplify_cells_bytes", "radegs_simplify_cells", "radegs_simplify_vertices_bytes", "radegs_simplify_vertices",
           "radegs_simplify_faces_bytes", "radegs_simplify_faces", "radegs_simplify_face_source")
KERNELS = ("cell_keys_kernel", "heads_kernel", "number_cells_kernel", "average_kernel", "corner_cells_kernel", "quadric_kernel",
           "solve_kernel", "face_cells_kernel", "gather2_kernel", "duplicates_kernel", "face_source_kernel")
INVALID, TOO_LARGE = -1, -6


def _library():
    import diff_gaussian_rasterization._C as C
    return C, ms._lib()


def test_library_exports_and_header_declares_the_entry_points():
    C, L = _library()
    header = open(os.path.join(ROOT, "include", "radegs.h")).read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in C.EXPORTED_SYMBOLS, sym
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % sym, header), sym
    assert "SURVEY.md 8f N21" in header
    assert set(ms.SIGNATURES) == set(SYMBOLS)
    assert int(re.search(r"#define RADEGS_SIMPLIFY_CELL_BITS (\d+)", header).group(1)) == ms.CELL_BITS
    import simplify_restatement as sr
    assert int(re.search(r"#define RADEGS_SIMPLIFY_JACOBI_SWEEPS (\d+)", header).group(1)) == sr.SWEEPS and sr.CELL_BITS == ms.CELL_BITS


def test_the_signature_table_agrees_with_the_header():
    """every argument of the header's prototypes against the table's ctypes, in order"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "radegs.h")).read(), flags=re.S)
    kind = {"long long": ms.ll, "int": ms.i32, "double": ms.f64, "size_t": ms.sz}
    for sym, (restype, argtypes) in ms.SIGNATURES.items():
        ret, args = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)" % sym, header).groups()
        assert restype is kind[ret], sym
        want = [ms.vp if "*" in a else kind[re.sub(r"\s+\w+$", "", a.strip().replace("const ", "").replace("unsigned ", ""))] for a in args.split(",")]
        assert list(argtypes) == want, (sym, args)


def test_sizes_and_argument_checks_run_without_a_device():
    _, L = _library()
    fake = 0x1000
    assert L.radegs_simplify_cells_bytes(0) == 0 and L.radegs_simplify_cells_bytes(-1) == 0 and L.radegs_simplify_cells_bytes(2 ** 31) == 0
    small, large = L.radegs_simplify_cells_bytes(1), L.radegs_simplify_cells_bytes(100_000)
    assert 0 < small < 64 * 1024 and small % 256 == 0
    assert 32 * 100_000 <= large <= 56 * 100_000                                    # six words and one 64-bit key per vertex, and the sort's temp
    assert L.radegs_simplify_cells_bytes(2 ** 31 - 1) > 32 * (2 ** 31 - 1)           # a size_t: not cut to 32 bits
    assert L.radegs_simplify_vertices_bytes(0) == 0 and L.radegs_simplify_vertices_bytes(2 ** 30 + 1) == 0 and L.radegs_simplify_vertices_bytes(4) > 0
    assert L.radegs_simplify_faces_bytes(0) == 0 and L.radegs_simplify_faces_bytes(2 ** 30 + 1) == 0
    assert 52 * 100_000 <= L.radegs_simplify_faces_bytes(100_000) <= 72 * 100_000   # eleven words and one 64-bit key per face, and the sort's temp

    def cells(V=8, v=fake, o=0.0, h=1.0, max_key=7, ws=fake, nbytes=1 << 30, vc=fake, order=fake, start=fake, key=fake, n=fake):
        return L.radegs_simplify_cells(V, v, o, o, o, h, max_key, ws, nbytes, vc, order, start, key, n, None)
    assert cells(V=-1) == INVALID and cells(n=None) == INVALID and cells(max_key=-1) == INVALID and cells(V=2 ** 31) == TOO_LARGE
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert cells(h=bad) == INVALID
    assert cells(o=float("nan")) == INVALID and cells(o=float("inf")) == INVALID
    assert cells(v=None) == INVALID and cells(vc=None) == INVALID and cells(order=None) == INVALID and cells(start=None) == INVALID
    assert cells(key=None) == INVALID and cells(ws=None) == INVALID and cells(ws=fake + 4) == INVALID
    assert cells(nbytes=L.radegs_simplify_cells_bytes(8) - 1) == INVALID

    def vertices(V=8, F=4, K=3, A=0, v=fake, f=fake, a=None, vc=fake, order=fake, start=fake, key=fake, h=1.0, quadric=1, ws=fake, nbytes=1 << 30,
                 avg=fake, attr=None, q=fake, pos=fake):
        return L.radegs_simplify_vertices(V, F, K, A, v, f, a, vc, order, start, key, 0.0, 0.0, 0.0, h, quadric, ws, nbytes, avg, attr, q, pos, None)
    assert vertices(K=0) == 0                                                        # no cell: no launch
    assert vertices(V=-1) == INVALID and vertices(F=-1) == INVALID and vertices(K=-1) == INVALID and vertices(K=9) == INVALID and vertices(A=-1) == INVALID
    assert vertices(quadric=2) == INVALID and vertices(h=0.0) == INVALID and vertices(h=float("nan")) == INVALID
    assert vertices(V=2 ** 31, K=1) == TOO_LARGE and vertices(F=2 ** 30 + 1) == TOO_LARGE
    assert vertices(v=None) == INVALID and vertices(order=None) == INVALID and vertices(start=None) == INVALID and vertices(avg=None) == INVALID
    assert vertices(A=3) == INVALID and vertices(A=3, a=fake) == INVALID             # attributes without their input or their output
    assert vertices(q=None) == INVALID and vertices(pos=None) == INVALID and vertices(key=None) == INVALID and vertices(f=None) == INVALID
    assert vertices(vc=None) == INVALID and vertices(ws=None) == INVALID and vertices(ws=fake + 8) == INVALID
    assert vertices(nbytes=L.radegs_simplify_vertices_bytes(4) - 1) == INVALID

    def faces(V=8, F=4, K=3, f=fake, vc=fake, dup=1, ws=fake, nbytes=1 << 30, cf=fake, remove=fake):
        return L.radegs_simplify_faces(V, F, K, f, vc, dup, ws, nbytes, cf, remove, None)
    assert faces(F=0) == 0
    assert faces(V=-1) == INVALID and faces(F=-1) == INVALID and faces(K=-1) == INVALID and faces(K=9) == INVALID and faces(dup=2) == INVALID
    assert faces(V=2 ** 31) == TOO_LARGE and faces(F=2 ** 30 + 1) == TOO_LARGE
    assert faces(f=None) == INVALID and faces(vc=None) == INVALID and faces(cf=None) == INVALID and faces(remove=None) == INVALID
    assert faces(ws=None) == INVALID and faces(ws=fake + 4) == INVALID and faces(nbytes=L.radegs_simplify_faces_bytes(4) - 1) == INVALID

    def source(K=3, F=4, ws=fake, nf=2, out=fake):
        return L.radegs_simplify_face_source(K, F, ws, nf, out, None)
    assert source(nf=0) == 0
    assert source(K=-1) == INVALID and source(F=-1) == INVALID and source(nf=-1) == INVALID and source(nf=5) == INVALID
    assert source(K=2 ** 31) == TOO_LARGE and source(F=2 ** 30 + 1) == TOO_LARGE and source(ws=None) == INVALID and source(out=None) == INVALID


def test_python_surface():
    sig = lambda f: list(inspect.signature(f).parameters)
    default = lambda f: [p.default for p in inspect.signature(f).parameters.values() if p.default is not inspect.Parameter.empty]
    assert sig(ms.simplify_vertex_clustering) == ["vertices", "faces", "voxel_size", "contraction", "origin", "attributes", "remove_duplicates",
                                                  "drop_unreferenced"]
    assert default(ms.simplify_vertex_clustering) == ["quadric", None, None, True, True]
    assert sig(ms.simplify_to_face_count) == ["vertices", "faces", "target_faces", "contraction", "max_tries", "kw"]
    assert default(ms.simplify_to_face_count) == ["quadric", 16]
    assert "need not be monotone" in ms.simplify_to_face_count.__doc__ and "hash-map order" in ms.simplify_vertex_clustering.__doc__
    assert "from memory" in ms.simplify_vertex_clustering.__doc__


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2]])
    for call in (lambda: ms.simplify_vertex_clustering(v, f, 1.0), lambda: ms.simplify_to_face_count(v, f, 10)):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), None, "1", True):
        with pytest.raises(RuntimeError, match="`voxel_size` must be a positive finite number"):
            ms.simplify_vertex_clustering(v, f, bad)
    for bad in ("Quadric", "linear", None, 1):
        with pytest.raises(RuntimeError, match="`contraction` must be one of"):
            ms.simplify_vertex_clustering(v, f, 1.0, contraction=bad)
        with pytest.raises(RuntimeError, match="`contraction` must be one of"):
            ms.simplify_to_face_count(v, f, 10, contraction=bad)
    for bad in (0, -1, 2.0, None, True):
        with pytest.raises(RuntimeError, match="`target_faces` must be a positive integer"):
            ms.simplify_to_face_count(v, f, bad)
        with pytest.raises(RuntimeError, match="`max_tries` must be a positive integer"):
            ms.simplify_to_face_count(v, f, 10, max_tries=bad)
    with pytest.raises(RuntimeError, match="unknown arguments"):
        ms.simplify_to_face_count(v, f, 10, voxel_size=1.0)
    for bad in ((0.0, 0.0), (0.0, 0.0, float("nan")), "000", (0.0, None, 0.0), torch.zeros(2)):
        with pytest.raises(RuntimeError, match="`origin` must be three finite numbers"):
            ms.simplify_vertex_clustering(v, f, 1.0, origin=bad)
    for name in ("remove_duplicates", "drop_unreferenced"):
        with pytest.raises(RuntimeError, match="`%s` must be a bool" % name):
            ms.simplify_vertex_clustering(v, f, 1.0, **{name: 1})
    for bad in (f.float(), f.reshape(3), torch.zeros(2, 4, dtype=torch.int64), [[0, 1, 2]]):
        with pytest.raises(RuntimeError, match="`faces` must be an int32 or int64 tensor"):
            ms.simplify_vertex_clustering(v, bad, 1.0)
    for bad in (v.half(), v.long(), None):
        with pytest.raises(RuntimeError, match="`vertices` must be a float32 or float64 tensor"):
            ms.simplify_vertex_clustering(bad, f, 1.0)
    # the remaining checks sit behind the device check: let a CPU tensor past it.  Each refuses before the library is called.
    import diff_gaussian_rasterization._C as C
    import mesh_clean
    monkeypatch.setattr(C, "_require_gpu", lambda t, name: None)
    monkeypatch.setattr(ms, "_lib", lambda: pytest.fail("the library was called"))
    monkeypatch.setattr(mesh_clean, "_lib", lambda: pytest.fail("the library was called"))
    huge = torch.empty((2 ** 30 + 1, 3), dtype=torch.int64, device="meta")           # refused on the shape alone
    with pytest.raises(RuntimeError, match="more than 2\\^30 faces"):
        ms.simplify_vertex_clustering(v, huge, 1.0)
    for bad in (torch.tensor([[0, 1, 4]]), torch.tensor([[0, -1, 2]])):
        with pytest.raises(RuntimeError, match="outside the 4 vertices"):
            ms.simplify_vertex_clustering(v, bad, 1.0)
    with pytest.raises(RuntimeError, match=r"`vertices` must be a tensor of shape \(N,3\)"):
        ms.simplify_vertex_clustering(torch.zeros(4, 2), f, 1.0)
    for value in (float("nan"), float("inf")):
        broken = v.clone()
        broken[1, 1] = value
        with pytest.raises(RuntimeError, match="`vertices` holds non-finite values"):
            ms.simplify_vertex_clustering(broken, f, 1.0)
        with pytest.raises(RuntimeError, match="`vertices` holds non-finite values"):
            ms.simplify_to_face_count(broken, f, 10)
    for bad in (torch.zeros(3, 3), torch.zeros(4), torch.zeros(4, 3, dtype=torch.int64), [[0.0]] * 4):
        with pytest.raises(RuntimeError, match="`attributes` must be a float32 or float64 tensor of shape"):
            ms.simplify_vertex_clustering(v, f, 1.0, attributes=bad)
    with pytest.raises(RuntimeError, match="`attributes` holds non-finite values"):
        ms.simplify_vertex_clustering(v, f, 1.0, attributes=torch.full((4, 1), float("nan")))
    # the extent over the voxel size: 2^21 cells along an axis are one too many, whichever way they are reached
    wide = torch.tensor([[0.0, 0.0, 0.0], [2.0 ** 21, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    for call in (lambda: ms.simplify_vertex_clustering(wide, f, 1.0), lambda: ms.simplify_vertex_clustering(wide.float(), f, 1.0),
                 lambda: ms.simplify_vertex_clustering(wide / 2.0 ** 21, f, 2.0 ** -21), lambda: ms.simplify_vertex_clustering(wide, f, 1e-300),
                 lambda: ms.simplify_vertex_clustering(wide, f, 1.0, origin=(0.5, 0.0, 0.0))):
        with pytest.raises(RuntimeError, match=r"outside \[0, 2\^21\)"):
            call()
    with pytest.raises(RuntimeError, match="no extent to bisect"):
        ms.simplify_to_face_count(v, f, 10)


def test_the_grid_accepts_the_last_cell_and_states_the_key_bound():
    origin, max_key = ms._grid([0.0, 0.0, 0.0], [2.0 ** 21 - 0.5, 3.5, 0.5], 1.0, (0.0, 0.0, 0.0))
    assert origin == (0.0, 0.0, 0.0) and max_key == (2 ** 21 - 1) << 42 | 3 << 21
    origin, max_key = ms._grid([1.0, 2.0, 3.0], [2.0, 2.0, 7.0], 0.5, None)
    assert origin == (0.75, 1.75, 2.75) and max_key == 2 << 42 | 0 << 21 | 8


def test_empty_inputs_return_empties_without_a_launch(monkeypatch):
    import diff_gaussian_rasterization._C as C
    import mesh_clean
    monkeypatch.setattr(C, "_require_gpu", lambda t, name: None)
    monkeypatch.setattr(ms, "_lib", lambda: pytest.fail("the library was called"))
    monkeypatch.setattr(mesh_clean, "_lib", lambda: pytest.fail("the library was called"))
    none = torch.zeros((0, 3), dtype=torch.int32)
    for v, f, a in ((torch.zeros(0, 3), none, None), (torch.zeros(4, 3, dtype=torch.float64), none, torch.zeros(4, 2)), (torch.zeros(0, 3), none, torch.zeros(0, 5))):
        for out in (ms.simplify_vertex_clustering(v, f, 0.5, attributes=a), ms.simplify_to_face_count(v, f, 10, attributes=a)[:5]):
            assert out[0].shape == (0, 3) and out[0].dtype == v.dtype and out[1].shape == (0, 3) and out[1].dtype == torch.int64
            assert out[2].shape == (v.shape[0],) and out[2].dtype == torch.int64 and bool((out[2] == -1).all())
            assert out[3].shape == (0,) and out[3].dtype == torch.int64
            assert (out[4] is None) == (a is None) and (a is None or (out[4].shape == (0, a.shape[1]) and out[4].dtype == a.dtype))


# ------------------------------------------------------------------------- packaging, resources -------------------------------------------------------------------------
def test_module_is_packaged_and_built():
    setup = open(os.path.join(ROOT, "rade-gs_amd", "setup.py")).read()
    assert '"mesh_simplify"' in re.search(r"py_modules=\[([^\]]*)\]", setup).group(1)
    build = open(os.path.join(ROOT, "rade-gs_amd", "build.py")).read()
    assert '"radegs_meshsimplify": ["radegs_meshsimplify.hip"' in build
    assert "radegs_meshsimplify" not in re.search(r"UNIT_FLAGS = \{[^}]*\}", build).group(0)      # -ffp-contract=off stays on for this unit
    source = open(os.path.join(ROOT, "rade-gs_amd", "csrc", "radegs_meshsimplify.hip")).read()
    assert "atomicAdd" not in source and "atomic" not in re.sub(r"//.*", "", source)              # no atomics at all, float or otherwise


@_needs_llvm_tools
def test_simplify_kernels_use_no_scratch(code_objects):  # noqa: F811
    found = {k: v[0] for k, v in code_objects.items() if "4rgms" in k}            # namespace rgms: radegs_meshsimplify.hip
    for part in KERNELS:
        hits = [k for k in found if "4rgms%d%sE" % (len(part), part) in k]
        assert len(hits) == 1, (part, sorted(found))
        assert found[hits[0]]["scratch"] == 0, (hits[0], found[hits[0]])
        print(part, found[hits[0]])
    assert len(found) == len(KERNELS), sorted(found)
    solve = [v for k, v in found.items() if "solve_kernel" in k][0]
    assert solve["vgpr"] <= 128, solve                                           # the Jacobi step's live doubles: four waves per SIMD at the least
