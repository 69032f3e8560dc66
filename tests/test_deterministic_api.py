"""The deterministic (fixed-order) backward's surface, without a GPU: the scratch formula of include/radegs.h, the Python switch, the bound
symbols, and the argument checks of radegs_backward_ordered that run before anything touches a device.  What the mode computes is checked on
the GPU (tests/test_gpu_deterministic.py)."""
import ctypes
import os

import pytest


def _r256(x):
    return (x + 255) // 256 * 256


def _sort_temp(n):
    """csrc/radegs_sort.hip::sort_temp_bytes as include/radegs.h restates it"""
    return 2 * (4 * n + 256) + 2048 * ((n + 2047) // 2048 + 1) + 3072


def _scratch_bytes(R, coord):
    """include/radegs.h: r256(R * REC * 4) + 2 * r256(R * 4) + r256(sort_temp(R)); nothing for R == 0"""
    if R <= 0:
        return _r256(_sort_temp(0))
    return _r256(R * (32 if coord else 16) * 4) + 2 * _r256(R * 4) + _r256(_sort_temp(R))


def _lib():
    import diff_gaussian_rasterization._C as C
    return C, C.library()


@pytest.mark.parametrize("coord", [0, 1])
def test_scratch_bytes_formula(coord):
    C, L = _lib()
    prev = 0
    for R in (1, 2, 63, 64, 65, 2047, 2048, 2049, 100_000, 1_000_003, 8 << 20):
        got = int(L.radegs_backward_ordered_scratch_bytes(1000, R, coord))
        assert got == _scratch_bytes(R, bool(coord)), (R, got)
        assert got % 256 == 0                     # every piece is carved at a 256-byte step, so the total is a multiple too
        assert got >= prev                        # monotonic in R
        assert got >= R * (128 if coord else 64)  # the partial records dominate: 64 | 128 B per instance
        prev = got
    # P does not enter (the sort's key width does not change its temporary); R <= 0 asks for no partial records
    assert L.radegs_backward_ordered_scratch_bytes(1, 5000, coord) == L.radegs_backward_ordered_scratch_bytes(1 << 24, 5000, coord)
    assert int(L.radegs_backward_ordered_scratch_bytes(10, 0, coord)) == int(L.radegs_backward_ordered_scratch_bytes(10, -3, coord)) < 8192


def test_switch_returns_previous_and_context_manager_restores():
    import diff_gaussian_rasterization as dgr
    import diff_gaussian_rasterization._C as C
    start = C.DETERMINISTIC
    try:
        assert dgr.set_deterministic_backward(True) is start
        assert dgr.set_deterministic_backward(False) is True
        assert C.DETERMINISTIC is False
        with dgr.deterministic_backward():
            assert C.DETERMINISTIC is True
            with dgr.deterministic_backward(False):
                assert C.DETERMINISTIC is False
            assert C.DETERMINISTIC is True
        assert C.DETERMINISTIC is False
        with pytest.raises(ZeroDivisionError):
            with dgr.deterministic_backward():
                1 / 0
        assert C.DETERMINISTIC is False           # restored on the way out of an exception too
    finally:
        C.DETERMINISTIC = start


def test_reload_env_reads_the_switch(monkeypatch):
    import diff_gaussian_rasterization._C as C
    start = C.DETERMINISTIC
    try:
        monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
        C.reload_env()
        assert C.DETERMINISTIC is True
        monkeypatch.setenv("RADEGS_DETERMINISTIC", "0")
        C.reload_env()
        assert C.DETERMINISTIC is False
        C.set_deterministic_backward(True)
        monkeypatch.delenv("RADEGS_DETERMINISTIC")
        C.reload_env()                            # like the library's own switches: absent = the default, whatever was set by hand
        assert C.DETERMINISTIC is False
    finally:
        C.DETERMINISTIC = start


def test_symbols_are_bound_with_their_argument_types():
    C, L = _lib()
    assert "radegs_backward_ordered" in C.EXPORTED_SYMBOLS and "radegs_backward_ordered_scratch_bytes" in C.EXPORTED_SYMBOLS
    assert L.radegs_backward_ordered.restype is ctypes.c_int
    assert L.radegs_backward_ordered.argtypes == [ctypes.POINTER(C.RadegsBwdArgs), C._ALLOC_FN, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_size_t, ctypes.c_void_p]
    assert L.radegs_backward_ordered_scratch_bytes.restype is ctypes.c_size_t
    assert L.radegs_backward_ordered_scratch_bytes.argtypes == [ctypes.c_int] * 3
    # radegs_backward's own binding is as it was
    assert L.radegs_backward.argtypes == [ctypes.POINTER(C.RadegsBwdArgs), C._ALLOC_FN, ctypes.c_void_p, ctypes.c_void_p]


def _args(C, R, struct_size=None):
    """RadegsBwdArgs whose pointers are non-NULL but never dereferenced: every call below must be refused before the first device call"""
    a = C.RadegsBwdArgs()
    a.struct_size = ctypes.sizeof(C.RadegsBwdArgs) if struct_size is None else struct_size
    a.P, a.D, a.M, a.R, a.width, a.height = 10, 0, 0, R, 32, 32
    fake = ctypes.c_void_p(0x1000)
    for f in ("geom_buffer", "binning_buffer", "image_buffer", "dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D",
              "dL_dscale", "dL_drot"):
        setattr(a, f, fake)
    return a


def test_bad_arguments_are_refused_before_a_device_is_touched():
    C, L = _lib()
    INVALID = -1
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "radegs.h")).read()
    assert "#define RADEGS_ERR_INVALID_ARG (%d)" % INVALID in hdr
    asked = []

    def _alloc(_user, nbytes):
        asked.append(int(nbytes))
        return 0
    cb = C._ALLOC_FN(_alloc)
    need = int(L.radegs_backward_ordered_scratch_bytes(10, 100, 0))
    scratch = ctypes.c_void_p(0x2000)   # never dereferenced
    # a struct of another size
    assert L.radegs_backward_ordered(ctypes.byref(_args(C, 100, struct_size=8)), cb, None, scratch, need, None) == INVALID
    assert b"struct_size" in L.radegs_last_error()
    # NULL scratch with R > 0
    assert L.radegs_backward_ordered(ctypes.byref(_args(C, 100)), cb, None, None, need, None) == INVALID
    assert b"scratch" in L.radegs_last_error()
    # a scratch one byte short
    assert L.radegs_backward_ordered(ctypes.byref(_args(C, 100)), cb, None, scratch, need - 1, None) == INVALID
    assert b"scratch" in L.radegs_last_error()
    # NULL arguments / allocator, as radegs_backward
    assert L.radegs_backward_ordered(None, cb, None, scratch, need, None) == INVALID
    assert L.radegs_backward_ordered(ctypes.byref(_args(C, 100)), ctypes.cast(None, C._ALLOC_FN), None, scratch, need, None) == INVALID
    assert asked == []                  # nothing was allocated, hence nothing queued, by any of the refused calls
    # P == 0: nothing to do, whatever the scratch
    a = _args(C, 0)
    a.P = 0
    assert L.radegs_backward_ordered(ctypes.byref(a), cb, None, None, 0, None) == 0


# ---- the new kernels' resources (the fixture and the tools' skip rule of tests/test_kernel_resources.py) ----
from test_kernel_resources import code_objects, waves_per_simd  # noqa: E402,F401  (code_objects is a fixture)
from test_kernel_resources import pytestmark as _needs_llvm_tools  # noqa: E402


@_needs_llvm_tools
def test_ordered_kernels_do_not_spill_and_keep_the_atomic_kernels_names_unique(code_objects):
    ordered = {k: v[0] for k, v in code_objects.items() if "blend_bwd_ordered_kernel" in k}
    assert len(ordered) == 4, sorted(ordered)            # COORD x DEPTH
    sums = {k: v[0] for k, v in code_objects.items() if "ordered_sums_kernel" in k}
    assert len(sums) == 2, sorted(sums)                  # REC = 16, 32
    for k, r in {**ordered, **sums}.items():
        assert "blend_bwd_packed_kernel" not in k and "blend_bwd_streams_kernel" not in k
        assert r["scratch"] == 0, (k, r)
    for flags in ("ILb0ELb0E", "ILb0ELb1E", "ILb1ELb0E", "ILb1ELb1E"):
        new = [r for k, r in ordered.items() if "blend_bwd_ordered_kernel" + flags in k]
        old = [v[0] for k, v in code_objects.items() if "blend_bwd_packed_kernel" + flags + "Li4E" in k]
        assert len(new) == 1 and len(old) == 1
        # the same body: the same static LDS, and the occupancy step of the one-wave-per-tile atomic kernel
        assert new[0]["lds"] == old[0]["lds"], (flags, new[0], old[0])
        assert waves_per_simd(new[0]["vgpr"]) >= waves_per_simd(old[0]["vgpr"]), (flags, new[0], old[0])


def test_the_numpy_restatement_adds_in_list_order():
    """tests/test_gpu_deterministic.py::restated_sums (the GPU test's yardstick) against the plainest possible loop, on a list with empty,
    single and long segments and values whose sum depends on the order"""
    import numpy as np
    from test_gpu_deterministic import restated_sums
    rng = np.random.default_rng(3)
    P, R, rec = 37, 900, 16
    pl = rng.integers(0, P - 5, R)                      # the last Gaussians have no instance
    pl[rng.integers(0, R, 300)] = 7                     # one long segment
    part = (rng.standard_normal((R, rec)) * 10.0 ** rng.integers(-6, 6, (R, 1))).astype(np.float32)
    got, count = restated_sums(pl, part, P)
    want = np.zeros((P, rec), np.float32)
    for r in range(R):                                  # ascending position = the stable order within every Gaussian
        want[pl[r]] = want[pl[r]] + part[r]
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(count, np.bincount(pl, minlength=P)) and count[-5:].sum() == 0 and not got[-5:].any()
    rev = np.zeros((P, rec), np.float32)
    for r in reversed(range(R)):
        rev[pl[r]] = rev[pl[r]] + part[r]
    assert not np.array_equal(rev.view(np.uint32), want.view(np.uint32))     # the data can tell two orders apart
