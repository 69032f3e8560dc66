"""CPU tier of the decoupled appearance loss's native surface: the library exports the entry points and include/radegs.h
declares them, bad arguments are refused before any device is touched, the scratch sizes are host arithmetic, the Python layer refuses
what it cannot do, and every appearance_* kernel is free of scratch with its static LDS inside what DESIGN 11 "N8" states (read from the
code objects of the in-tree library as tests/test_kernel_resources.py does)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from test_kernel_resources import code_objects  # noqa: F401  (the fixture) -- and its skip condition:
from test_kernel_resources import pytestmark as _needs_llvm_tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("radegs_appearance_downsample_forward", "radegs_appearance_downsample_backward", "radegs_appearance_head_scratch_bytes",
           "radegs_appearance_head_forward", "radegs_appearance_head_backward")
# kernel -> the most static LDS DESIGN 11 "N8" allows it (bytes)
KERNELS = {"appearance_pack_weights_kernel": 0, "appearance_head_fwd_kernel": 141040, "appearance_loss_final_kernel": 2048,
           "appearance_head_bwd_kernel": 151776, "appearance_wgrad_final_kernel": 2048, "appearance_dfeat_kernel": 150304,
           "appearance_downsample_fwd_kernel": 0, "appearance_downsample_bwd_kernel": 0}


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


def test_bad_arguments_are_refused_before_any_device_is_touched():
    """no GPU on this tier: a call that got as far as a launch or a memset would fail differently (RADEGS_ERR_HIP) or crash"""
    _, L = _library()
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.radegs_appearance_downsample_forward.argtypes = [ci, ci, vp, vp, vp]
    L.radegs_appearance_downsample_backward.argtypes = [ci, ci, vp, vp, vp]
    L.radegs_appearance_head_scratch_bytes.restype = sz
    L.radegs_appearance_head_scratch_bytes.argtypes = [ci, ci, ci]
    L.radegs_appearance_head_forward.argtypes = [ci] * 4 + [vp] * 8 + [sz, vp, vp, vp]
    L.radegs_appearance_head_backward.argtypes = [ci] * 4 + [vp] * 9 + [sz] + [vp] * 7
    fake, INVALID, big = 0x1000, -1, 1 << 40
    nbytes = L.radegs_appearance_head_scratch_bytes
    # scratch sizes: the repacked weights + 256 partial rows; the backward adds the one full-resolution tensor, 16 floats per crop pixel
    assert nbytes(31, 64, 0) == 0 and nbytes(64, 31, 1) == 0 and nbytes(0, 0, 0) == 0 and nbytes(-5, 64, 1) == 0 and nbytes(40000, 64, 1) == 0
    f, b = nbytes(70, 101, 0), nbytes(70, 101, 1)
    assert 0 < f < 64 * 1024 and f == nbytes(1200, 1600, 0)
    assert b - nbytes(37, 45, 1) == 16 * 4 * (64 * 96 - 32 * 32)
    assert nbytes(1200, 1600, 1) - 16 * 4 * 1184 * 1600 == b - 16 * 4 * 64 * 96 < 4 * 1024 * 1024
    assert L.radegs_appearance_downsample_forward(31, 64, fake, fake, None) == INVALID
    assert L.radegs_appearance_downsample_forward(64, 64, None, fake, None) == INVALID
    assert L.radegs_appearance_downsample_forward(64, 64, fake, None, None) == INVALID
    assert L.radegs_appearance_downsample_backward(64, 20, fake, fake, None) == INVALID
    assert L.radegs_appearance_downsample_backward(64, 64, None, fake, None) == INVALID
    assert L.radegs_appearance_downsample_backward(64, 64, fake, None, None) == INVALID

    def fwd(oh=70, ow=101, fh=32, fw=48, ptrs=None, scratch=fake, n=big, loss=fake):
        ptrs = [fake] * 7 if ptrs is None else ptrs
        return L.radegs_appearance_head_forward(oh, ow, fh, fw, *ptrs, scratch, n, loss, None, None)

    def bwd(oh=70, ow=101, fh=32, fw=48, ptrs=None, gl=fake, scratch=fake, n=big, outs=None):
        ptrs = [fake] * 7 if ptrs is None else ptrs
        outs = [fake] * 6 if outs is None else outs
        return L.radegs_appearance_head_backward(oh, ow, fh, fw, *ptrs, gl, scratch, n, *outs, None)

    for call in (fwd, bwd):
        assert call(oh=31) == INVALID and call(ow=31) == INVALID                          # the crop would be empty
        assert call(fh=31) == INVALID and call(fw=47) == INVALID and call(fh=33, fw=49) == INVALID    # odd F sizes
        assert call(fh=16) == INVALID and call(fw=96) == INVALID                          # even, but not H/2 x W/2
        assert call(scratch=None) == INVALID
        assert call(n=0) == INVALID and call(n=f - 1) == INVALID                          # too-small scratch
        assert call(scratch=fake + 4) == INVALID                                          # not 16-byte aligned
        for i in range(7):
            assert call(ptrs=[None if j == i else fake for j in range(7)]) == INVALID, i
    assert fwd(loss=None) == INVALID
    assert bwd(n=b - 1) == INVALID and bwd(gl=None) == INVALID
    for i in range(6):
        assert bwd(outs=[None if j == i else fake for j in range(6)]) == INVALID, i


class _Gaussians:
    def __init__(self, net):
        self.appearance_network = net
        self._appearance_embeddings = torch.zeros(4, 64)

    def get_apperance_embedding(self, idx):
        return self._appearance_embeddings[idx]


def test_python_surface_and_its_refusals():
    import gaussian_model_ops as gmo
    import loss_utils as lu
    from appearance_network import AppearanceNetwork
    assert list(inspect.signature(lu.l1_loss_appearance).parameters) == ["image", "gt_image", "gaussians", "view_idx", "return_transformed_image"]
    assert inspect.signature(lu.l1_loss_appearance).parameters["return_transformed_image"].default is False
    p = inspect.signature(gmo.patch_gaussian_model).parameters
    assert list(p) == ["cls", "appearance_network"] and p["appearance_network"].default is False
    assert lu.appearance_crop(37, 45) == (32, 32, 2, 6) and lu.appearance_crop(1200, 1600) == (1184, 1600, 8, 0)
    g = _Gaussians(AppearanceNetwork(67, 3))
    img = torch.zeros(3, 64, 64)
    with pytest.raises(RuntimeError, match="must be a GPU tensor"):
        lu.l1_loss_appearance(img, img, g, 0)
    wide = _Gaussians(AppearanceNetwork(67, 3))
    wide.appearance_network.conv2 = torch.nn.Conv2d(16, 16, 5, padding=2)
    with pytest.raises(NotImplementedError, match="3x3 16->16"):
        lu.l1_loss_appearance(img, img, wide, 0)
    four = _Gaussians(AppearanceNetwork(67, 4))
    with pytest.raises(NotImplementedError):
        lu.l1_loss_appearance(img, img, four, 0)


def test_patch_gaussian_model_swaps_the_network_after_training_setup():
    import gaussian_model_ops as gmo
    from appearance_network import AppearanceNetwork

    class Upstream(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = torch.nn.Conv2d(67, 256, 3, padding=1)
            for i, (a, b) in enumerate(((64, 128), (32, 64), (16, 32), (8, 16))):
                blk = torch.nn.Module()
                blk.conv = torch.nn.Conv2d(a, b, 3, padding=1)
                setattr(self, f"up{i + 1}", blk)
            self.conv2, self.conv3 = torch.nn.Conv2d(16, 16, 3, padding=1), torch.nn.Conv2d(16, 3, 3, padding=1)

    def make():
        class Model:
            def __init__(self):
                self.appearance_network = Upstream()

            def training_setup(self, training_args):
                self.optimizer = torch.optim.Adam([{"params": self.appearance_network.parameters(), "lr": training_args, "name": "appearance_network"}])
                return "done"

            def add_densification_stats(self, *a):
                pass

            def densify_and_prune(self, *a):
                pass
        return Model

    plain = gmo.patch_gaussian_model(make())()                 # the default leaves training_setup and the network alone
    assert plain.training_setup(1e-3) == "done" and isinstance(plain.appearance_network, Upstream)
    m = gmo.patch_gaussian_model(make(), appearance_network=True)()
    before = list(m.appearance_network.parameters())
    assert m.training_setup(1e-3) == "done"
    assert isinstance(m.appearance_network, AppearanceNetwork)
    group = m.optimizer.param_groups[0]["params"]
    after = list(m.appearance_network.parameters())
    assert len(group) == len(after) == 14 and all(a is b for a, b in zip(group, after)) and all(a is b for a, b in zip(before, after))


def test_unit_is_in_the_build_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("radegs_build_table", os.path.join(ROOT, "rade-gs_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert build.UNITS["radegs_appearance"][0] == "radegs_appearance.hip"
    assert all(os.path.exists(os.path.join(build.CSRC, f)) for f in build.UNITS["radegs_appearance"])


@_needs_llvm_tools
def test_appearance_kernels_use_no_scratch_and_stay_inside_their_lds(code_objects):  # noqa: F811
    found = {k: v[0] for k, v in code_objects.items() if "appearance_" in k}
    assert all("4rgap" in k for k in found), sorted(found)                       # namespace rgap: radegs_appearance.hip
    for part, max_lds in KERNELS.items():
        hits = [k for k in found if "4rgap%d%sE" % (len(part), part) in k]
        assert len(hits) == 1, (part, sorted(found))
        r = found[hits[0]]
        assert r["scratch"] == 0, (part, r)
        assert r["lds"] <= max_lds, (part, r)
    assert len(found) == len(KERNELS), sorted(found)
