"""Parity tests proper (run on the MI355X box with -m gpu): the HIP path, called through the drop-in
Python API -> ctypes -> C ABI, against the CPU oracle on the same seeded inputs.

Bar (BASELINE.json north_star): bit-exact tile/sort indices (radii, num_rendered, point_list,
ranges, n_contrib); images and gradients within 1e-5 abs / 1e-4 rel in fp32.  Gradients are sums
of up to thousands of fp32 atomics whose order differs run to run (the reference's are too,
SURVEY A18), so the gradient check allows the fp32 reordering error of the per-Gaussian
accumulation on top of the tolerance and reports the fraction inside the strict bound.
"""
import os

import numpy as np
import pytest
import torch

from synth_scene import make_scene, upstream_grads
from util import ATOL, RTOL, close, cov3d_of, frac_close, grad_noise_floor, oracle_backward, oracle_for

pytestmark = pytest.mark.gpu

NAMES = ["color", "radii", "coord", "mcoord", "depth", "mdepth", "alpha", "normal"]


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X box"
    return "cuda:0"


def check_forward(s, colors=None, cov3D=None, scale_modifier=1.0):
    from gpu_util import HipRun, outputs_numpy
    o = oracle_for(s, colors=colors, cov3D=cov3D, scale_modifier=scale_modifier)
    R_ref = o.forward()
    ref = o.outputs()
    h = HipRun(s, _dev(), colors=colors, cov3D=cov3D, scale_modifier=scale_modifier)
    st = h.forward_native()
    torch.cuda.synchronize()
    P, H, W = h.P, s.H, s.W
    # ---- index parity: exact ----
    assert st[0] == R_ref, "num_rendered"
    assert np.array_equal(st[8].cpu().numpy(), ref[1]), "radii"
    assert np.array_equal(h.export("tiles_touched", torch.int32, P).view(np.uint32), o.get("tiles_touched"))
    if R_ref:
        assert np.array_equal(h.export("point_list", torch.int32, R_ref).view(np.uint32), o.get("point_list")), "point_list"
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    assert np.array_equal(h.export("ranges", torch.int32, 2 * ntiles).view(np.uint32), o.get("ranges")), "ranges"
    nc = h.export("n_contrib", torch.int32, 2 * H * W).view(np.uint32)
    nc_ref = o.get("n_contrib")
    geo = s.require_coord or s.require_depth
    assert np.array_equal(nc[: H * W], nc_ref[: H * W]), "n_contrib (last contributor)"
    if geo:
        assert np.array_equal(nc[H * W:], nc_ref[H * W:]), "n_contrib (median contributor)"
    # ---- images: tolerance ----
    got = [st[1], None, st[2], st[3], st[6], st[7], st[4], st[5]]  # -> operator order color,_,coord,mcoord,depth,mdepth,alpha,normal
    for k in (0, 2, 3, 4, 5, 6, 7):
        a, b = got[k].cpu().numpy(), ref[k]
        assert not np.isnan(a).any(), NAMES[k]
        assert close(a, b).all(), f"{NAMES[k]}: max abs diff {np.abs(a - b).max():.3e}"
    return o, h


def check_backward(s, o, colors=None, cov3D=None, seed=0, ill_mask=None, min_strict=0.99, scale_modifier=1.0, rms_factor=1.1,
                   max_factor=1.25, band_factor=1.0, collect=None):
    """ill_mask: rows (Gaussians) whose covariance is (nearly) singular.  Their per-Gaussian chain rule
    multiplies the accumulated sums by ~1/lambda_min (backward.cu:333-350), so the 1e-7 relative fp32
    reordering noise of the sums is amplified without bound; for those rows the check moves to where the
    noise enters -- the blend backward's per-Gaussian sums -- and only requires finite outputs after the
    chain rule (which is bit-exact given identical sums: tests/test_hostcheck.py)."""
    import diff_gaussian_rasterization._C as C
    from gpu_util import HipRun

    def chk(ok, name, criterion, measured, allowed, msg):   # collect is a list: record every failed criterion instead of raising
        if ok:
            return
        if collect is None:
            raise AssertionError(msg)
        collect.append((name, criterion, float(measured), float(allowed)))
    g = upstream_grads(s, seed)
    ref = oracle_backward(o, g)
    h = HipRun(s, _dev(), colors=colors, cov3D=cov3D, scale_modifier=scale_modifier)
    h.forward()
    C.KEEP_ACC = True
    try:
        got = h.backward(g)
        acc = C.LAST_ACC.cpu().numpy()
    finally:
        C.KEEP_ACC = False
    P = s.means3D.shape[0]
    # ---- the blend backward's sums (SplatAcc order), all rows ----
    rec = 32 if s.require_coord else 16
    acc = acc[: P * rec].reshape(P, rec)
    dc = o.get("acc_dconic", (P, 4))
    ref_acc = np.concatenate([o.get("acc_dcolors", (P, 3)), o.get("dL_dts", (P, 1)), o.get("dL_dray_planes", (P, 2)),
                              o.get("dL_dnormals", (P, 3)), o.get("acc_dmeans2D", (P, 3)), dc[:, [0, 1, 3]],
                              o.get("acc_dopacity", (P, 1)), o.get("dL_dview_points", (P, 3)), o.get("dL_dcamera_planes", (P, 6))], 1)
    vis = o.get("radii") > 0
    # the kernel leaves constant factors to the per-Gaussian stage: 1/focal on plane sums, W/2, H/2 on mean2D
    fx, fy = s.W / (2 * s.tanfovx), s.H / (2 * s.tanfovy)
    acc = acc.astype(np.float64)
    acc[:, 4] /= fx; acc[:, 5] /= fy; acc[:, 9] *= 0.5 * s.W; acc[:, 10] *= 0.5 * s.H
    if rec == 32:
        acc[:, 19:25:2] /= fx; acc[:, 20:25:2] /= fy
    for c in range(rec if rec == 16 else 25):
        a, b = acc[vis, c], ref_acc[vis, c]
        scale = float(np.abs(b).max()) + 1e-30
        chk(close(a, b, atol=ATOL + 1e-4 * scale, rtol=1e-3).all(), f"acc[{c}]", "band", np.abs(a - b).max(), ATOL + 1e-4 * scale,
            f"acc[{c}] max abs diff {np.abs(a - b).max():.3e} (scale {scale:.3e})")
        chk(frac_close(a, b) > min_strict, f"acc[{c}]", "strict fraction", frac_close(a, b), min_strict, f"acc[{c}]")
    # ---- returned gradients ----
    # Criterion 1 (direct): >= 99 % of all elements inside the strict 1e-5 abs / 1e-4 rel bar vs the fp32
    # oracle, the rest inside a band set by the fp32 noise floor of the algorithm (util.grad_noise_floor).
    # Criterion 2 (accuracy): against the fp64 oracle the HIP gradients are as accurate as the fp32 oracle.
    report = {}
    rows = np.ones(P, bool) if ill_mask is None else ~ill_mask
    nf = grad_noise_floor(s, g, colors=colors, cov3D=cov3D, scale_modifier=scale_modifier) if P <= 20000 else None
    floor, g64 = nf if nf is not None else ({}, {})
    for k, b in ref.items():
        a = got[k]
        if a is None:
            continue
        b = b.reshape(a.shape)
        assert not np.isnan(a).any(), k
        a, b = a[rows], b[rows]
        strict = frac_close(a, b)
        scale = float(np.abs(b).max()) + 1e-30
        band = ATOL + band_factor * max(2e-6 * scale, 0.25 * floor.get(k, 0.0))
        report[k] = strict
        chk(strict > min_strict, k, "strict fraction", strict, min_strict, f"{k}: only {strict:.4f} within 1e-5/1e-4")
        chk(close(a, b, atol=band, rtol=1e-3).all(), k, "band", np.abs(a - b).max(), band,
            f"{k}: max abs diff {np.abs(a - b).max():.3e} (scale {scale:.3e}, fp32 floor {floor.get(k)})")
        if k in g64 and ill_mask is None:
            c = g64[k].reshape(got[k].shape)[rows]
            e_hip, e_ref = np.abs(a.astype(np.float64) - c), np.abs(b.astype(np.float64) - c)
            r_hip, r_ref = np.sqrt((e_hip ** 2).mean()), np.sqrt((e_ref ** 2).mean())
            chk(r_hip <= rms_factor * r_ref + 1e-7, k, "rms vs fp64 / oracle32's", r_hip / (r_ref + 1e-30), rms_factor, f"{k}: rms error vs fp64 worse than the fp32 oracle's")
            chk(e_hip.max() <= max_factor * e_ref.max() + ATOL, k, "max vs fp64 / oracle32's", e_hip.max() / (e_ref.max() + 1e-30), max_factor,
                f"{k}: max error vs fp64 {e_hip.max():.3e} vs oracle's {e_ref.max():.3e}")
    return report


MODES = [(False, False), (False, True), (True, False), (True, True)]


@pytest.mark.parametrize("coord,depth", MODES)
def test_small_scene_all_modes(coord, depth):
    s = make_scene(3000, 200, 136, sh_degree=3, mu_px=3.0, seed=21, kernel_size=0.1, require_coord=coord, require_depth=depth,
                   pose="random", bg=(0.2, 0.5, 0.9))
    o, _ = check_forward(s)
    check_backward(s, o, seed=21)


def test_config_C1():
    # BASELINE.json configs[0]: 10k Gaussians, 256x256, SH degree 0
    from synth_scene import make_config
    s = make_config("C1")
    o, _ = check_forward(s)
    check_backward(s, o, seed=0)


def test_heavy_overdraw_and_ragged_image():
    # big splats (long per-tile lists, early termination, multi-batch staging) on an image whose size
    # is not a multiple of the tile: exercises the tail tiles and `done` handling
    s = make_scene(6000, 203, 117, sh_degree=2, mu_px=14.0, seed=33, kernel_size=0.0, require_coord=True, require_depth=True,
                   pose="identity")
    o, _ = check_forward(s)
    check_backward(s, o, seed=33)


def test_precomputed_colors_and_covariance():
    s = make_scene(2500, 160, 120, sh_degree=0, mu_px=2.5, seed=5, kernel_size=0.1, pose="random", require_coord=False, require_depth=True)
    cov, colors = cov3d_of(s), torch.rand(s.means3D.shape[0], 3, generator=torch.Generator().manual_seed(1))
    o, _ = check_forward(s, colors=colors, cov3D=cov)
    check_backward(s, o, colors=colors, cov3D=cov, seed=5)


@pytest.mark.parametrize("streams", [0, 1])
def test_flat_gaussians_ill_conditioned_branch(streams, monkeypatch):
    """Flat (needle-like on screen) Gaussians: the eigen-solver's ill-conditioned branch, conics whose quadratic form is a
    difference of huge terms -- both blend paths must evaluate it in the reference's order of operations."""
    monkeypatch.setenv("RADEGS_STREAMS", str(streams))
    from test_hostcheck import _flat_scene
    s = _flat_scene(make_scene(2500, 160, 120, sh_degree=1, mu_px=3.0, seed=12, kernel_size=0.0, pose="random", require_coord=True,
                               require_depth=True))
    o, _ = check_forward(s)
    sc = s.scales.numpy()
    check_backward(s, o, seed=12, ill_mask=(sc.min(1) / sc.max(1)) < 1e-2)


def test_empty_culled_and_single():
    from gpu_util import HipRun
    from test_oracle_kat import _single
    # all culled: colour = bg, everything else 0, num_rendered 0
    s = _single(zs=[0.1], n=1)
    check_forward(s)
    # P == 0: nothing launched, all outputs zero (rasterize_points.cu:90)
    s0 = s._replace(means3D=torch.zeros(0, 3), shs=torch.zeros(0, 16, 3), rotations=torch.zeros(0, 4), scales=torch.zeros(0, 3),
                    opacities=torch.zeros(0, 1))
    h = HipRun(s0, _dev())
    out = h.forward()
    assert all(float(t.abs().sum()) == 0 for t in out)
    # one on-axis Gaussian (closed-form KAT of test_oracle_kat.py) and the hidden-third case
    check_forward(_single())
    check_forward(_single(n=3, zs=[3.0, 4.0, 5.0], opac=[5.0, 5.0, 5.0], scale=0.2))
    o, _ = check_forward(_single(n=4, zs=[4.0, 4.0, 4.0, 4.0], opac=[0.3] * 4))  # equal depth keys: index order


def test_mark_visible():
    from diff_gaussian_rasterization import GaussianRasterizer
    from gpu_util import settings_for
    from oracle import oracle as orc
    s = make_scene(5000, 64, 64, seed=3, pose="random")
    r = GaussianRasterizer(settings_for(s, _dev()))
    got = r.markVisible(s.means3D.to(_dev())).cpu().numpy()
    assert np.array_equal(got, orc.mark_visible(s.means3D, s.viewmatrix, s.projmatrix))


@pytest.mark.parametrize("bwd_ppl", [2, 4])
def test_pixels_per_lane_variants_agree(bwd_ppl, monkeypatch):
    """the tile-wide backward exists with one wave per 16x8 strip (2 pixels per lane) and one wave per tile (4; chosen for heavy overdraw)"""
    monkeypatch.setenv("RADEGS_STREAMS", "0")   # these are variants of the tile-wide kernels
    monkeypatch.setenv("RADEGS_BWD_PPL", str(bwd_ppl))
    s = make_scene(3000, 200, 136, sh_degree=3, mu_px=4.0, seed=44, kernel_size=0.1, require_coord=True, require_depth=True, pose="random")
    o, _ = check_forward(s)
    check_backward(s, o, seed=44)


@pytest.mark.parametrize("coord,depth", MODES)
@pytest.mark.parametrize("streams", [0, 1])
def test_blend_paths_agree_with_oracle(coord, depth, streams, monkeypatch):
    """The blend stage exists twice: tile-wide kernels (one wave per strip walks the tile's list) and sub-tile entry streams
    (csrc/rg_streams.inc: exactly culled per-block lists, the backward replays the forward's contribution bits).  The launcher
    picks by splat size; both must pass the same parity checks on the same scene whatever the default is."""
    monkeypatch.setenv("RADEGS_STREAMS", str(streams))
    s = make_scene(6000, 203, 131, sh_degree=2, mu_px=2.0, seed=62, kernel_size=0.1, require_coord=coord, require_depth=depth, pose="random",
                   bg=(0.3, 0.1, 0.7))
    o, _ = check_forward(s)
    check_backward(s, o, seed=62)


@pytest.mark.parametrize("coord,depth", MODES)
def test_stream_backward_long_lists(coord, depth, monkeypatch):
    """The stream backward in every mode on lists many rounds long and a ragged image.  In the coord-map modes a (block, entry)'s 32-float
    record leaves as two atomic instructions, one per 64-byte line (lane l: components l and 16 + l) -- first run on hardware in round 5
    (profiles/r05_ab_linewise.txt), the default of those modes since."""
    monkeypatch.setenv("RADEGS_STREAMS", "1")
    s = make_scene(5000, 203, 131, sh_degree=2, mu_px=5.0, seed=64, kernel_size=0.1, require_coord=coord, require_depth=depth, pose="random",
                   bg=(0.3, 0.1, 0.7))
    o, _ = check_forward(s)
    check_backward(s, o, seed=64)


@pytest.mark.parametrize("streams", [0, 1])
def test_trained_scene_shape_both_paths(streams, monkeypatch):
    """The shape of a trained scene (synth_scene CONFIGS["C2H"]: heavy-tailed footprints -- sub-pixel splats next to splats covering
    dozens of tiles -- clustered on blobs, tile lists from empty to thousands of entries) through either blend formulation."""
    monkeypatch.setenv("RADEGS_STREAMS", str(streams))
    s = make_scene(40_000, 480, 270, sh_degree=3, mu_px=1.0, seed=11, kernel_size=0.0, require_coord=False, require_depth=True,
                   sigma_ln=1.3, big_frac=0.02, big_px=48.0, clusters=30)
    o, _ = check_forward(s)
    check_backward(s, o, seed=11)


@pytest.mark.parametrize("streams", [0, 1])
def test_mixed_scene_shape_both_paths(streams, monkeypatch):
    """VERDICT r5's "C2M" (synth_scene CONFIGS["C2M"]) at a reduced size: C2's small splats plus 0.5 % splats of 50-150 px confined to the left
    third of the image -- two thirds of the tiles the entry streams' case, one third the tile-wide kernels' -- through either formulation."""
    monkeypatch.setenv("RADEGS_STREAMS", str(streams))
    s = make_scene(40_000, 480, 270, sh_degree=3, mu_px=1.5, seed=12, kernel_size=0.0, require_coord=False, require_depth=True,
                   big_frac=0.005, big_px=50.0, big_band=(-1.0, -1.0 / 3.0))
    o, _ = check_forward(s)
    check_backward(s, o, seed=12)


def test_entry_streams_heavy_overdraw_termination_and_ragged_image(monkeypatch):
    """Forced entry streams on big splats: lists of hundreds of entries per block, rows of pixels that terminate early (their
    block stops consuming its list) next to rows that do not, partial rounds, tail tiles of a ragged image."""
    monkeypatch.setenv("RADEGS_STREAMS", "1")
    s = make_scene(6000, 203, 117, sh_degree=2, mu_px=14.0, seed=33, kernel_size=0.0, require_coord=True, require_depth=True,
                   pose="identity")
    o, _ = check_forward(s)
    check_backward(s, o, seed=33)
    s = make_scene(4000, 320, 200, sh_degree=1, mu_px=1.5, seed=3, kernel_size=0.0, require_coord=False, require_depth=True)   # sparse
    o, _ = check_forward(s)
    check_backward(s, o, seed=3)


def test_tile_wide_backward_after_stream_forward(monkeypatch):
    """The tile-wide backward only needs the tile lists and n_contrib, so it is the fallback whenever the image state's entry
    streams cannot be trusted (e.g. the buffer was copied): it must accept the state a stream forward left."""
    monkeypatch.setenv("RADEGS_STREAMS", "1")
    monkeypatch.setenv("RADEGS_STREAMS_BWD", "0")
    s = make_scene(5000, 200, 136, sh_degree=1, mu_px=2.0, seed=64, kernel_size=0.1, require_coord=False, require_depth=True, pose="random")
    o, _ = check_forward(s)
    check_backward(s, o, seed=64)


def test_stream_backward_on_an_overwritten_image_state_reports_an_error_instead_of_trapping(monkeypatch):
    """The library remembers by address which image buffers hold entry streams; the buffer's own tag is the device-side double check.
    A caller that overwrites the state between forward and backward (here: zeroes it) gets no kernel trap -- the stream backward
    finds the wrong tag, touches nothing and raises a flag in the host's mapped words; the NEXT call into the library returns
    RADEGS_ERR_STATE, and the device context keeps working (a trap kills the process's HIP context)."""
    import diff_gaussian_rasterization._C as C
    from synth_scene import to_device
    monkeypatch.setenv("RADEGS_STREAMS", "1")
    C.reload_env()
    dev = torch.device(_dev())
    s_cpu = make_scene(4000, 176, 120, sh_degree=1, mu_px=2.0, seed=97, kernel_size=0.0, require_coord=False, require_depth=True)
    s = to_device(s_cpu, dev)
    g = {k: v.to(dev) for k, v in upstream_grads(s_cpu, 97).items()}
    e = torch.Tensor([])

    def forward():
        return C.rasterize_gaussians(s.bg, s.means3D, e, s.opacities, s.scales, s.rotations, 1.0, e, s.viewmatrix, s.projmatrix, s.tanfovx,
                                     s.tanfovy, s.kernel_size, s.H, s.W, s.shs, s.sh_degree, s.campos, False, s.require_coord, s.require_depth, False)

    def backward(fw):
        R, color, coord, mcoord, alpha, normal, depth, mdepth, radii, geom, binning, img = fw
        return C.rasterize_gaussians_backward(s.bg, s.means3D, radii, e, s.scales, s.rotations, 1.0, e, s.viewmatrix, s.projmatrix, s.tanfovx,
                                              s.tanfovy, s.kernel_size, g["color"], g["coord"], g["mcoord"], g["depth"], g["mdepth"], g["alpha"],
                                              g["normal"], normal, s.shs, s.sh_degree, s.campos, geom, R, binning, img, alpha, s.require_coord,
                                              s.require_depth, False)
    fw = forward()
    assert C.last_forward_used_streams() is True
    good = [t.clone() for t in backward(fw) if t is not None]
    fw = forward()
    fw[11].zero_()                       # the image state, tag included, is gone
    bad = backward(fw)                   # queues the stream backward on it: no trap, no exception yet ...
    torch.cuda.synchronize(dev)
    # ... but nothing a caller could mistake for a gradient either: the kernel poisons the accumulator, every visible
    # Gaussian's row comes back NaN -- the error itself is only reported by the NEXT call, which may be somebody else's
    vis = fw[8] > 0
    assert bool(vis.any()) and all(bool(torch.isnan(t[vis]).all()) for t in (bad[0], bad[3]))   # dL_dmeans2D, dL_dmeans3D
    with pytest.raises(RuntimeError, match="does not hold the entry streams"):
        forward()                        # the next call into the library on this thread reports it ...
    fw = forward()                       # ... once; the context is alive and the following calls are right again
    again = [t for t in backward(fw) if t is not None]
    torch.cuda.synchronize(dev)
    for a, b in zip(again, good):
        scale = float(b.abs().max()) + 1e-30
        assert float((a - b).abs().max()) <= 1e-3 * scale


def test_forward_is_deterministic_and_backward_stable():
    from gpu_util import HipRun
    s = make_scene(20000, 320, 240, sh_degree=3, mu_px=2.0, seed=8, require_coord=False, require_depth=True)
    a = HipRun(s, _dev()).forward_native()
    b = HipRun(s, _dev()).forward_native()
    for x, y in zip(a[1:9], b[1:9]):
        assert torch.equal(x, y)


def test_debug_flag_and_stream():
    # debug=True synchronises after every launch (CHECK_CUDA analogue); a non-default stream must work
    from gpu_util import HipRun
    s = make_scene(2000, 128, 128, sh_degree=1, seed=2, require_depth=True)
    ref = HipRun(s, _dev()).forward_native()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = HipRun(s, _dev(), debug=True).forward_native()
    st.synchronize()
    assert torch.equal(ref[1], got[1]) and ref[0] == got[0]


def test_sparse_scene_pixels_without_contributors():
    """Few small splats: most pixels of a strip have no contributor at all (alpha = 0, n_contrib = 0) while their neighbours do.
    The 1/alpha factors of the depth/normal cotangents are undefined there and must not leak into the wave-wide sums."""
    s = make_scene(4000, 320, 200, sh_degree=1, mu_px=1.5, seed=3, kernel_size=0.0, require_coord=False, require_depth=True)
    o, h = check_forward(s)
    assert (h.state[4].cpu().numpy() == 0).sum() > 0             # pixels with no contributor exist (a handful is enough to poison a sum)
    check_backward(s, o, seed=3)
    s = make_scene(3000, 640, 424, sh_degree=0, mu_px=1.5, seed=8, kernel_size=0.1, require_coord=True, require_depth=True)
    o, h = check_forward(s)
    assert (h.state[4].cpu().numpy() == 0).mean() > 0.1          # here a large part of the image is empty
    # few pixels per Gaussian: the sums are short and cancel, so a slightly larger share sits at the fp32 noise floor
    # (98.9 % inside the strict bar on this scene; the band and fp64-arbiter checks are unchanged)
    check_backward(s, o, seed=8, min_strict=0.98)


def test_image_wider_than_255_tiles():
    """gx = 258 tiles: the packed 8-bit tile rectangle of the instance emission does not apply and the rectangle is recomputed."""
    s = make_scene(3000, 4120, 40, sh_degree=0, mu_px=6.0, seed=17, kernel_size=0.1, require_coord=False, require_depth=True, fovx_deg=100.0)
    o, _ = check_forward(s)
    check_backward(s, o, seed=17, min_strict=0.97)


def test_handwritten_sort_matches_device_library():
    """The hand-written radix sort / scan (csrc/radegs_sort.hip) against rocPRIM's (RADEGS_PRIMS=rocprim, read once
    per process, hence the subprocess): identical point_list and ranges on a scene big enough for several blocks."""
    import hashlib
    import os
    import subprocess
    import sys
    code = (
        "import sys, hashlib, numpy as np, torch\n"
        "sys.path[:0] = [%r, %r, %r]\n"
        "from gpu_util import HipRun\n"
        "from synth_scene import make_scene\n"
        "s = make_scene(150000, 640, 360, sh_degree=1, mu_px=2.5, seed=77, require_depth=True)\n"
        "h = HipRun(s, 'cuda:0'); st = h.forward_native(); torch.cuda.synchronize()\n"
        "pl = h.export('point_list', torch.int32, st[0]); rg = h.export('ranges', torch.int32, 2 * 40 * 23)\n"
        "print('HASH', st[0], hashlib.sha1(pl.tobytes() + rg.tobytes()).hexdigest())\n"
    ) % tuple(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), p) for p in ("", "rade-gs_amd", "tests"))
    outs = []
    for over in (dict(), dict(RADEGS_PRIMS="rocprim")):
        env = dict(os.environ, **over)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([l for l in r.stdout.splitlines() if l.startswith("HASH")][0])
    assert outs[0] == outs[1], outs


def test_forced_sort_instantiations_give_the_same_lists():
    """The 16- and 32-items-per-thread sort kernels, which the size rule picks only above 3 M and 32 M items, forced onto the same
    scene (RADEGS_SORT_ITEMS, read once per process, hence the subprocesses): point_list and ranges identical to the rule's 8-item
    kernels.  Two forwards in a row under RADEGS_SPECULATE=1: the second tile sort runs at a predicted capacity with the count read on
    the device (n_dev).  The primitives on their own: tests/test_gpu_sort_scan.py."""
    import os
    import subprocess
    import sys
    code = (
        "import sys, hashlib, numpy as np, torch\n"
        "sys.path[:0] = [%r, %r, %r]\n"
        "import diff_gaussian_rasterization._C as C\n"
        "from gpu_util import HipRun\n"
        "from synth_scene import make_scene\n"
        "s = make_scene(150000, 640, 360, sh_degree=1, mu_px=2.5, seed=77, require_depth=True)\n"
        "C.binning_stats(reset=True)\n"
        "for it in range(2):\n"
        "    h = HipRun(s, 'cuda:0'); st = h.forward_native(); torch.cuda.synchronize()\n"
        "    pl = h.export('point_list', torch.int32, st[0]); rg = h.export('ranges', torch.int32, 2 * 40 * 23)\n"
        "    print('HASH', it, st[0], hashlib.sha1(pl.tobytes() + rg.tobytes()).hexdigest())\n"
        "print('SPEC', C.binning_stats())\n"
    ) % tuple(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), p) for p in ("", "rade-gs_amd", "tests"))
    outs = []
    for items in (None, "16", "32"):      # one process after the other
        env = dict(os.environ, RADEGS_SPECULATE="1")
        env.pop("RADEGS_SORT_ITEMS", None)
        if items:
            env["RADEGS_SORT_ITEMS"] = items
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert [l for l in lines if l.startswith("SPEC")] == ["SPEC (1, 0)"], lines     # the second forward was speculative and was not redone
        outs.append([l for l in lines if l.startswith("HASH")])
    assert len(outs[0]) == 2 and outs[0][0].split()[2:] == outs[0][1].split()[2:], outs[0]
    assert outs[0] == outs[1] == outs[2], outs


def test_depths_beyond_the_three_pass_sort_window(monkeypatch):
    """The depth sort runs three 9-bit passes over (key - bits(0.2f)), valid while every visible depth is below 13 107; the per-Gaussian
    kernel flags a key outside that window and the forward is redone with the four-pass sort (rg_launch.inc).  A scene scaled 3 000x
    (depths 6 000 ... 30 000) takes that path on its first frame, the remembered 4-pass sort on the next; both must equal the oracle.
    At a (W, H) whose history the unscaled scene seeded, the first far frame is speculative: it is redone straight with the 4-pass sort
    and must equal the RADEGS_SPECULATE=0 forward."""
    import diff_gaussian_rasterization._C as C
    from gpu_util import HipRun
    s = make_scene(3000, 176, 144, sh_degree=1, mu_px=3.0, seed=77, kernel_size=0.0, require_coord=False, require_depth=True)
    s = s._replace(means3D=s.means3D * 3000.0, scales=s.scales * 3000.0)
    C.binning_stats(reset=True)
    o, _ = check_forward(s)
    check_backward(s, o, seed=77)
    o, _ = check_forward(s)          # the (device, W, H) remembers: no redo any more, same result

    near = make_scene(3000, 192, 144, sh_degree=1, mu_px=3.0, seed=77, kernel_size=0.0, require_coord=False, require_depth=True)
    far = near._replace(means3D=near.means3D * 3000.0, scales=near.scales * 3000.0)
    monkeypatch.setenv("RADEGS_SPECULATE", "1")
    C.reload_env()
    HipRun(near, _dev()).forward_native()   # history at 192 x 144: a prediction that holds far's instances, the 3-pass sort
    C.binning_stats(reset=True)
    spec = HipRun(far, _dev()).forward_native()
    torch.cuda.synchronize()
    assert C.binning_stats() == (1, 1)     # one speculative forward, redone
    monkeypatch.setenv("RADEGS_SPECULATE", "0")
    C.reload_env()
    exact = HipRun(far, _dev()).forward_native()
    assert spec[0] == exact[0]
    for a, b in zip(spec[1:9], exact[1:9]):
        assert torch.equal(a, b)


def test_very_long_tile_lists():
    """Every Gaussian covers the whole 48x32 image, so each of the 6 tiles lists all 9000 of them (hundreds of staging rounds per
    block, every block list as long as the tile list), twice in a row (exact sizes, then the speculative capacity)."""
    s = make_scene(9000, 48, 32, sh_degree=0, mu_px=60.0, seed=91, kernel_size=0.0, require_coord=False, require_depth=True, low_opacity=True)
    check_forward(s)
    check_forward(s)


def test_speculative_binning_matches_exact_path():
    """The sync-free binning (capacity predicted from the previous call, rg_launch.inc) must give the very same state and images
    as the exact path, both when the prediction fits and when it is too small (instances dropped -> redone).  The switches are
    read once per process, hence the subprocesses.  Each process renders three scenes of very different num_rendered in a row
    (first call exact, then over- and under-predictions), forward + backward."""
    import os
    import subprocess
    import sys
    code = (
        "import sys, hashlib, numpy as np, torch\n"
        "sys.path[:0] = [%r, %r, %r]\n"
        "from gpu_util import HipRun\n"
        "from synth_scene import make_scene, upstream_grads\n"
        "for P, mu, seed in ((30000, 1.5, 1), (30000, 6.0, 2), (4000, 1.5, 3), (60000, 3.0, 4), (60000, 3.0, 4)):\n"
        "    s = make_scene(P, 320, 200, sh_degree=1, mu_px=mu, seed=seed, require_depth=True)\n"
        "    h = HipRun(s, 'cuda:0'); st = h.forward_native(); torch.cuda.synchronize()\n"
        "    pl = h.export('point_list', torch.int32, st[0]); rg = h.export('ranges', torch.int32, 2 * 20 * 13)\n"
        "    nc = h.export('n_contrib', torch.int32, 2 * 320 * 200)\n"
        "    img = b''.join(t.cpu().numpy().tobytes() for t in st[1:9])\n"
        "    out = h.forward(); g = h.backward(upstream_grads(s, seed))\n"
        "    finite = all(np.isfinite(v).all() for v in g.values() if v is not None)\n"
        "    print('HASH', st[0], finite, hashlib.sha1(pl.tobytes() + rg.tobytes() + nc.tobytes() + img).hexdigest())\n"
    ) % tuple(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), p) for p in ("", "rade-gs_amd", "tests"))
    outs = []
    for env_over in (dict(RADEGS_SPECULATE="0"), dict(RADEGS_SPECULATE="1"), dict(RADEGS_SPECULATE="1", RADEGS_SPECULATE_HINT="5000")):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env_over), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("HASH")]
        assert len(lines) == 5, lines
        outs.append(lines)
    assert outs[0] == outs[1] == outs[2], outs


@pytest.mark.gpu
def test_unproduced_maps_are_zero_call_after_call():
    """Maps a mode does not produce are FRESH zero tensors on every call, as the reference's torch.full(0) maps are
    (rasterize_points.cu:71-77): zeros also after the mode changed in between, no storage shared between two calls or between two
    maps of one call, and a caller that writes into one poisons nothing."""
    from gpu_util import HipRun
    held = []
    for rnd, (coord, depth) in enumerate([(False, True), (True, True), (False, True), (True, False), (False, False), (False, True)]):
        s = make_scene(3000, 203, 131, sh_degree=1, mu_px=2.5, seed=70 + rnd, kernel_size=0.1, require_coord=coord, require_depth=depth, pose="random")
        color, radii, co, mco, de, mde, alpha, normal = HipRun(s, _dev()).forward()
        if not coord:
            assert not bool(co.any()) and not bool(mco.any())
            co.detach().add_(1.0)                       # a caller scribbling over its map ...
            assert not bool(mco.any())                  # ... touches neither its sibling ...
            for old in held:                            # ... nor what earlier calls handed out
                assert not bool(old.any())
            held.append(mco.detach())
        if not depth:
            assert not bool(de.any()) and not bool(mde.any())
        if not (coord or depth):
            assert not bool(normal.any())


@pytest.mark.gpu
@pytest.mark.parametrize("streams", [0, 1])
def test_c_abi_zero_fills_the_unproduced_maps_it_is_handed_and_only_those(streams, monkeypatch):
    """include/radegs.h (round 6): a map the flags do not produce is zero-filled by the forward when its pointer is non-NULL -- every pixel, by
    the blend kernel of either formulation, also in a ragged image -- and not touched at all when it is NULL.  Through ctypes, past the binding."""
    import ctypes
    import diff_gaussian_rasterization._C as C
    monkeypatch.setenv("RADEGS_STREAMS", str(streams))
    C.reload_env()
    dev = torch.device(_dev())
    s = make_scene(3000, 203, 131, sh_degree=1, mu_px=2.5, seed=91, kernel_size=0.1, require_coord=False, require_depth=False, pose="random")
    from synth_scene import to_device
    d = to_device(s, dev)
    P, H, W = 3000, s.H, s.W
    L = C.library()

    def run(hand_over):
        f = dict(dtype=torch.float32, device=dev)
        color, alpha = torch.empty((3, H, W), **f), torch.empty((1, H, W), **f)
        extra = {k: torch.full((c, H, W), float("nan"), **f) for k, c in (("coord", 3), ("mcoord", 3), ("depth", 1), ("mdepth", 1), ("normal", 3))}
        radii = torch.empty(P, dtype=torch.int32, device=dev)
        geom, binning, img = C._Resizable(dev), C._Resizable(dev), C._Resizable(dev, image=True)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        opt = (lambda k: ptr(extra[k])) if hand_over else (lambda k: None)
        a = C.RadegsFwdArgs(P, s.sh_degree, int(d.shs.size(1)), W, H, ptr(d.bg), ptr(d.means3D), ptr(d.shs), None, ptr(d.opacities), ptr(d.scales),
                            ptr(d.rotations), None, ptr(d.viewmatrix), ptr(d.projmatrix), ptr(d.campos), 1.0, float(s.tanfovx), float(s.tanfovy),
                            float(s.kernel_size), 0, 0, 0, 0, ptr(color), opt("coord"), opt("mcoord"), opt("depth"), opt("mdepth"), ptr(alpha),
                            opt("normal"), ptr(radii))
        rc = L.radegs_forward(ctypes.byref(a), geom.cb, None, binning.cb, None, img.cb, None, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
        for r in (geom, binning, img):
            r.release()
        assert rc > 0, L.radegs_last_error()
        return color, alpha, extra
    color_a, alpha_a, ex_a = run(True)
    for k, t in ex_a.items():
        assert not bool(torch.isnan(t).any()) and not bool(t.any()), k          # handed over: all zeros, no pixel left out
    color_b, alpha_b, ex_b = run(False)
    for k, t in ex_b.items():
        assert bool(torch.isnan(t).all()), k                                     # NULL: never touched
    assert torch.equal(color_a, color_b) and torch.equal(alpha_a, alpha_b)
    assert C.last_forward_used_streams() is bool(streams)


def test_stream_byte_budget_falls_back_to_the_tile_wide_kernels(monkeypatch):
    """RADEGS_STREAMS_MAX_MB: above the budget the launcher does not ask for entry-stream storage;
    the tile-wide kernels then run on the plain image state -- same results."""
    import diff_gaussian_rasterization._C as C
    monkeypatch.setenv("RADEGS_STREAMS_MAX_MB", "0")
    s = make_scene(6000, 232, 168, sh_degree=2, mu_px=2.0, seed=66, kernel_size=0.1, require_coord=False, require_depth=True, pose="random")
    o, h = check_forward(s)
    assert h.state[11].numel() == C.library().radegs_image_bytes(s.W, s.H)      # no stream storage behind the image state
    check_backward(s, o, seed=66)


def test_a_view_that_exceeded_the_stream_budget_does_not_ban_the_streams_for_ever(monkeypatch):
    """one view whose lists exceed RADEGS_STREAMS_MAX_MB (a densification peak before pruning) makes the launcher stop asking for
    entry streams at that (device, W, H) -- for 64 forwards, not for the rest of the run: afterwards they are tried again."""
    import diff_gaussian_rasterization._C as C
    from gpu_util import HipRun
    monkeypatch.setenv("RADEGS_SPECULATE", "1")
    s = make_scene(20000, 344, 216, sh_degree=0, mu_px=1.5, seed=72, kernel_size=0.0, require_coord=False, require_depth=True)
    for _ in range(2):                                  # history for this (device, W, H): the next forwards are speculative
        HipRun(s, _dev()).forward_native()
    assert C.last_forward_used_streams() is True
    monkeypatch.setenv("RADEGS_STREAMS_MAX_MB", "1")    # now the lists (a few MB) exceed the budget: noticed by a speculative forward
    ref = [t.clone() for t in HipRun(s, _dev()).forward_native()[1:9]]
    assert C.last_forward_used_streams() is False       # redone through the tile-wide kernels
    monkeypatch.delenv("RADEGS_STREAMS_MAX_MB")         # the budget is back (the peak is over) ...
    back = None
    for n in range(1, 80):
        out = HipRun(s, _dev()).forward_native()
        for a, b in zip(out[1:9], ref):                 # either formulation: same maps (1e-5 / 1e-4), same radii
            assert torch.equal(a, b) if a.dtype != torch.float32 else torch.allclose(a, b, rtol=RTOL, atol=ATOL)
        if C.last_forward_used_streams():
            back = n
            break
    assert back is not None and back > 8, back          # ... refused for a while, then tried again and kept


@pytest.mark.parametrize("coord,depth", [(False, True), (True, True)])
def test_block_masks_in_the_tile_keys(coord, depth, monkeypatch):
    """Scenes of 2^24 Gaussians and more cannot carry an instance's block mask next to the Gaussian index in the 32-bit value: it rides in
    the top byte of a 32-bit tile key instead (the sort only looks at the low tile bits; tile_ranges masks it off; block_lists_kernel
    <MASK_IN_KEY> reads it from the sorted keys).  RADEGS_MASK_IN_KEY=1 walks a small scene through that layout: same results."""
    monkeypatch.setenv("RADEGS_STREAMS", "1")
    monkeypatch.setenv("RADEGS_MASK_IN_KEY", "1")
    s = make_scene(6000, 232, 168, sh_degree=2, mu_px=2.5, seed=67, kernel_size=0.1, require_coord=coord, require_depth=depth, pose="random")
    o, _ = check_forward(s)
    check_backward(s, o, seed=67)
    s = make_scene(1500, 203, 131, sh_degree=1, mu_px=14.0, seed=93, kernel_size=0.1, require_coord=coord, require_depth=depth, pose="random",
                   low_opacity=True)      # splats of more than 16 tiles: the cooperative emission path
    check_forward(s)


def test_entry_stream_storage_is_sized_from_the_previous_view_and_an_overflow_is_redone():
    """The entry streams are stored compactly (block_lists_kernel counts, then takes exactly the chunks a tile's lists need); a
    speculative forward sizes that storage from what the previous forward at this resolution used (+25 %).  A view whose lists need
    far more -- same Gaussians, camera pulled in -- overflows it: the kernel drops the lists it cannot place and raises the flag, the
    host redoes the forward with the capacity that cannot overflow.  Results equal the non-speculative path's, bit for bit; and
    the image state of a steady view is far smaller than the worst-case reservation of rounds 2-4."""
    import diff_gaussian_rasterization._C as C
    from gpu_util import HipRun
    s = make_scene(30000, 328, 248, sh_degree=1, mu_px=1.2, seed=71, kernel_size=0.0, require_coord=False, require_depth=True)
    os.environ["RADEGS_STREAMS"] = "1"
    try:
        os.environ["RADEGS_SPECULATE"] = "0"
        exact = [t.clone() for t in HipRun(s, _dev()).forward_native()[1:9]]
        os.environ["RADEGS_SPECULATE"] = "1"
        C.binning_stats(reset=True)                  # the counters are process-wide: whatever earlier tests did is not this test's
        for _ in range(3):                           # seed the (device, W, H) history
            h = HipRun(s, _dev()); st = h.forward_native()
        for a, b in zip(st[1:9], exact):
            assert torch.equal(a, b)
        steady_bytes = st[11].numel()
        R_far = st[0]
        calls0, misses0 = C.binning_stats(reset=True)
        assert calls0 >= 2 and misses0 == 0, (calls0, misses0)      # steady state: the history-sized storage fitted
        os.environ["RADEGS_SPECULATE_CHUNKS"] = "40"                # storage for 40 chunks = 640 list entries: certain to overflow
        h2 = HipRun(s, _dev()); st2 = h2.forward_native()
        calls, misses = C.binning_stats()
        assert calls == 1 and misses == 1, (calls, misses)          # the chunk prediction was too small: the forward was redone
        for a, b in zip(st2[1:9], exact):
            assert torch.equal(a, b)
        h2.forward()
        g = upstream_grads(s, 71)
        assert all(np.isfinite(v).all() for v in h2.backward(g).values() if v is not None)
        # compact storage: the steady view's image state stays well under the old worst-case reservation (8 x ceil(n/16) chunks of 192 B per tile)
        tiles = ((s.W + 15) // 16) * ((s.H + 15) // 16)
        old_reservation = 8 * ((int(R_far * 1.25) >> 4) + tiles + 1) * 192
        plain = C.library().radegs_image_bytes(s.W, s.H)
        assert steady_bytes - plain < 0.5 * old_reservation, (steady_bytes - plain, old_reservation)
    finally:
        for k in ("RADEGS_STREAMS", "RADEGS_SPECULATE", "RADEGS_SPECULATE_CHUNKS"):
            os.environ.pop(k, None)
        C.reload_env()


@pytest.mark.gpu
@pytest.mark.parametrize("coord,depth", [(False, True), (True, True)])
def test_big_splats_through_the_entry_streams(coord, depth, monkeypatch):
    """Splats of more than 16 tiles are emitted by the whole wave (one lane per tile); with entry streams forced, that path computes
    the block masks too (one ellipse_block_mask per lane from the broadcast record)."""
    monkeypatch.setenv("RADEGS_STREAMS", "1")
    s = make_scene(1500, 203, 131, sh_degree=1, mu_px=14.0, seed=93, kernel_size=0.1, require_coord=coord, require_depth=depth, pose="random",
                   low_opacity=True)
    o, _ = check_forward(s)
    assert int((o.get("tiles_touched") > 16).sum()) > 200
    check_backward(s, o, seed=93)


@pytest.mark.parametrize("deg,P", [(3, 3001), (1, 2500), (3, 128), (2, 1000)])
def test_per_gaussian_backward_slab_paths_agree(deg, P, monkeypatch):
    """preprocess_bwd_kernel moves its SH slab in 16-byte pieces where rows and alignment allow (SH degree 3 and 1, aligned tensors)
    and word by word otherwise: the same SH tensor at an address 4 bytes off a 16-byte boundary takes the other path and must return
    the same bits (the per-Gaussian half alone, over fixed sums: radegs_backward_from_sums has no atomics in it)."""
    from gpu_util import HipRun, backward_from_sums
    s = make_scene(P, 160, 120, sh_degree=deg, mu_px=3.0, seed=100 + deg, kernel_size=0.1, require_coord=False, require_depth=True, pose="random")
    h = HipRun(s, _dev())
    h.forward_native()
    sums = np.random.default_rng(7).standard_normal((P, 16)).astype(np.float32)
    a = backward_from_sums(h, sums)
    shs = h.shs.detach()
    buf = torch.empty(shs.numel() + 1, dtype=torch.float32, device=shs.device)
    off = buf[1:].view(shs.shape)
    off.copy_(shs)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    h.shs = off
    c = backward_from_sums(h, sums)
    assert (a["dL_dsh"] != 0).any() and np.isfinite(a["dL_dsh"]).all()
    for k in a:
        if a[k] is None:
            continue
        assert np.array_equal(a[k].view(np.uint32), c[k].view(np.uint32)), k
