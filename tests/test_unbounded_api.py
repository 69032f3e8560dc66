"""unbounded_mesh.py's argument checks and the C ABI's (no GPU needed: every refusal comes before the first device call)."""
import ctypes

import numpy as np
import pytest
import torch

import unbounded_mesh as um

INVALID, TOO_LARGE = -1, -6
SYMBOLS = ("radegs_unbounded_fuse", "radegs_unbounded_uncontract", "radegs_densemc_bytes", "radegs_densemc_plan", "radegs_densemc_emit")


class View:
    full_proj_transform = torch.eye(4)
    world_view_transform = torch.eye(4)


def test_signatures_cover_the_units_symbols():
    from diff_gaussian_rasterization import _C
    assert set(um._SIGNATURES) == set(SYMBOLS) and set(SYMBOLS) <= set(_C.EXPORTED_SYMBOLS)
    L = um._lib()
    for name, (restype, argtypes) in um._SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    assert L.radegs_densemc_bytes.restype is ctypes.c_size_t
    assert ctypes.sizeof(ctypes.c_float) * 16 + 2 * ctypes.sizeof(ctypes.c_int) + 2 * ctypes.sizeof(ctypes.c_void_p) == um._VIEW.itemsize == 88


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        um.ViewStack([View()], [torch.ones((12, 16))])
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        um.dense_marching_cubes(torch.ones((3, 3, 3)), torch.ones(3), torch.ones(3), torch.ones(3))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        um.world_points(torch.zeros((4, 3)), (0, 0, 0), 1.0)
    empty = um.ViewStack([], [])
    assert len(empty) == 0 and empty.table is None
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        um.fuse_samples(empty, torch.zeros((4, 3)), 0.01, (0, 0, 0), 1.0)
    with pytest.raises(RuntimeError, match="ViewStack"):
        um.fuse_samples([View()], torch.zeros((4, 3)), 0.01, (0, 0, 0), 1.0)

    class Gaussians:
        get_xyz = torch.zeros((4, 3))
    ex = um.GaussianExtractor(Gaussians(), lambda view, g, pipe, bg_color: dict(render=torch.zeros((3, 12, 16)), median_depth=torch.ones((1, 12, 16))), None)
    with pytest.raises(RuntimeError, match="reconstruction"):
        ex.extract_mesh_unbounded(32, 16)


def test_view_stack_checks_its_lists():
    with pytest.raises(RuntimeError, match="one depth map"):
        um.ViewStack([View()], [])
    with pytest.raises(RuntimeError, match="one depth map"):
        um.ViewStack([View()], [torch.ones((12, 16))], [])


def test_resolution_must_be_a_multiple_of_the_crop():
    empty, xyz = um.ViewStack([], []), torch.zeros((4, 3))
    for res, crop in ((32, 12), (1024, 500), (16, 32)):
        with pytest.raises(RuntimeError, match="multiple"):
            um.extract_mesh_unbounded(empty, xyz, res, crop)
    for res, crop in ((32.0, 16), (32, 1), (0, 16), (True, 1)):
        with pytest.raises(RuntimeError, match="integer"):
            um.extract_mesh_unbounded(empty, xyz, res, crop)
    with pytest.raises(RuntimeError, match="max_range"):
        um.extract_mesh_unbounded(empty, xyz, 32, 16, max_range=0.0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):      # the defaults are upstream's: 1024 in crops of 512
        um.extract_mesh_unbounded(empty, xyz)


def test_scene_normalisation_needs_views():
    with pytest.raises(RuntimeError, match="at least one view"):
        um.scene_normalisation([])
    with pytest.raises(RuntimeError, match="at least one view"):
        um.scene_normalisation([np.eye(3)])


def test_c_abi_refuses_bad_arguments_before_touching_the_device():
    """pointers are never dereferenced here: every call below returns before the first HIP call"""
    L = um._lib()
    fake = 0x1000
    c3 = (ctypes.c_float * 3)(0, 0, 0)

    def fuse(**over):
        kw = dict(M=8, samples=fake, ax=None, ay=None, az=None, nx=0, ny=0, nz=0, mapping=0, V=2, views=fake, contract=1, radius=1.0, center=c3, trunc5=0.1,
                  tsdf=fake, rgb=None)
        kw.update(over)
        return L.radegs_unbounded_fuse(kw["M"], kw["samples"], kw["ax"], kw["ay"], kw["az"], kw["nx"], kw["ny"], kw["nz"], kw["mapping"], kw["V"], kw["views"],
                                       kw["contract"], kw["radius"], kw["center"], kw["trunc5"], kw["tsdf"], kw["rgb"], None)
    assert fuse(M=0) == 0 and fuse(M=0, V=0, views=None) == 0                    # nothing to do, nothing launched
    for over in (dict(M=-1), dict(V=-1), dict(views=None), dict(center=None), dict(trunc5=0.0), dict(trunc5=float("nan")), dict(radius=0.0),
                 dict(radius=float("inf")), dict(mapping=2), dict(tsdf=None),
                 dict(samples=None), dict(samples=None, ax=fake, ay=fake, az=fake, nx=2, ny=2, nz=0), dict(samples=None, ax=fake, ay=fake, az=None, nx=2, ny=2, nz=2),
                 dict(samples=None, ax=fake, ay=fake, az=fake, nx=2, ny=2, nz=2, M=7)):
        assert fuse(**over) == INVALID, over
    assert fuse(M=2 ** 31) == TOO_LARGE
    assert fuse(samples=None, ax=fake, ay=fake, az=fake, nx=2048, ny=2048, nz=2048, M=2 ** 33) == TOO_LARGE
    assert fuse(contract=0, radius=0.0, M=0) == 0                                # the colouring pass does not use the radius

    un = L.radegs_unbounded_uncontract
    assert un(0, None, 1.0, c3, 32.0, None, None) == 0
    assert un(-1, fake, 1.0, c3, 32.0, fake, None) == INVALID and un(4, None, 1.0, c3, 32.0, fake, None) == INVALID
    assert un(4, fake, 1.0, c3, 32.0, None, None) == INVALID and un(4, fake, 0.0, c3, 32.0, fake, None) == INVALID
    assert un(4, fake, 1.0, None, 32.0, fake, None) == INVALID and un(4, fake, 1.0, c3, 0.0, fake, None) == INVALID

    assert L.radegs_densemc_bytes(1, 8, 8) == 0 and L.radegs_densemc_bytes(8, 8, 0) == 0 and L.radegs_densemc_bytes(2048, 2048, 2048) == 0
    small, large = L.radegs_densemc_bytes(2, 2, 2), L.radegs_densemc_bytes(512, 512, 512)
    assert 0 < small < large and large >= 512 ** 3 * 17
    assert L.radegs_densemc_bytes(1290, 1290, 1290) > 2 ** 32                   # a size_t: not cut to 32 bits
    counts = fake
    plan = lambda values=fake, n=(8, 8, 8), ws=fake, nbytes=None: L.radegs_densemc_plan(values, n[0], n[1], n[2], ws, L.radegs_densemc_bytes(*n) if nbytes is None else nbytes, counts, None)
    assert plan(values=None) == INVALID and plan(n=(1, 8, 8)) == INVALID and plan(ws=None) == INVALID and plan(ws=fake + 4) == INVALID
    assert plan(nbytes=L.radegs_densemc_bytes(8, 8, 8) - 1) == INVALID
    assert L.radegs_densemc_plan(fake, 8, 8, 8, fake, L.radegs_densemc_bytes(8, 8, 8), None, None) == INVALID
    off = (ctypes.c_int * 3)(0, 0, 0)

    def emit(n=(8, 8, 8), offset=off, G=8, V=3, F=1, values=fake, ws=fake, vertices=fake, keys=fake, faces=fake):
        return L.radegs_densemc_emit(values, fake, fake, fake, n[0], n[1], n[2], offset, G, ws, V, F, vertices, keys, faces, None)
    assert emit(V=0, F=0) == 0
    for over in (dict(n=(8, 1, 8)), dict(offset=None), dict(G=0), dict(G=7), dict(G=2 ** 20 + 1), dict(offset=(ctypes.c_int * 3)(1, 0, 0)),
                 dict(offset=(ctypes.c_int * 3)(0, -1, 0)), dict(V=-1), dict(F=-1), dict(values=None), dict(ws=None), dict(vertices=None), dict(keys=None),
                 dict(faces=None)):
        assert emit(**over) == INVALID, over
    assert emit(V=2 ** 32) == TOO_LARGE
