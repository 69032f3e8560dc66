"""The per-Gaussian kernels looked at directly, bit for bit (csrc/rg_per_gaussian.inc: preprocess_fwd_kernel, preprocess_bwd_kernel,
drgb_clamped_kernel, sh_grad_from_views_kernel).

a  every word the forward leaves per Gaussian (splat_a, splat_b, clamped, rect, depth_key, radii, tiles_touched) against the oracle's arrays;
b  the backward over the ORACLE'S OWN per-Gaussian sums against the oracle's gradients, both opacity modes;
c  the backward over sums the oracle never produces against the host build of the same headers;
d  the launch modes of the backward (grad_chunks, the separate dL_drgb_clamped kernel) against one plain launch;
e  sh_grad_from_views against a float64 restatement of the SH basis;
f  the ordered backward with and without keep_sums: the write-back of the records does not change what is returned;
g  the records a keep_sums backward leaves, as reference sums through backward_from_sums, against what that backward returned.

Bit equality is expected, not hoped for: the product is built with -ffp-contract=off, IEEE divide and square root, and the three headers call
nothing from a library but sqrtf and ceilf (the one exception, skip_threshold's logf, fills slot 6 of splat_a and is compared with the same
device function).  The scenes, their classes of rows and the packers are tests/per_gaussian_cases.py; tests/test_per_gaussian_cases.py shows on
the CPU that the oracle populates every class and that the packers agree with the host build."""
import numpy as np
import pytest
import torch

import per_gaussian_cases as pg
from gpu_util import HipRun, backward_from_sums
from synth_scene import make_scene, upstream_grads
from util import ATOL, RTOL, close, oracle_backward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADS = ("dL_dmeans3D", "dL_dopacity", "dL_dcov3D", "dL_dscales", "dL_drotations", "dL_dsh", "dL_dcolors", "dL_dmeans2D")


def _run(c):
    h = HipRun(c.s, DEV, colors=c.colors, cov3D=c.cov3D, scale_modifier=c.scale_modifier)
    h.forward_native()
    torch.cuda.synchronize()
    return h


def _u32(h, name, n):
    return h.export(name, torch.int32, n).view(np.uint32)


# ================================================================================================== a. forward state, bit for bit
@pytest.mark.parametrize("name", list(pg.BUILDERS))
def test_forward_state_bit_for_bit(name):
    from test_gpu_stream_lists import dev_skip_thresholds
    c = pg.get_case(name)
    o, s, P = c.o, c.s, c.P
    h = _run(c)
    want = pg.expected_state(o, s, c.colors)
    radii = o.get("radii")
    vis, every = radii > 0, np.ones(P, bool)
    got_radii = h.state[8].cpu().numpy()
    tiles, rect, key = _u32(h, "tiles_touched", P), _u32(h, "rect", P), _u32(h, "depth_key", P)
    pg.assert_fields({"radii": (got_radii, radii), "tiles_touched": (tiles, o.get("tiles_touched")), "rect": (rect, want["rect"]),
                      "depth_key": (key, want["depth_key"])}, every, c.cls, name + ": every row")
    inv = ~vis
    assert not rect[inv].any() and (key[inv] == 0xFFFFFFFF).all() and not tiles[inv].any(), name + ": an invisible row with a rectangle, a depth key or tiles"
    a = h.export("splat_a", torch.float32, 16 * P).reshape(P, 16)
    pairs = {"clamped": (h.export("clamped", torch.uint8, P), want["clamped"])}
    for k, cols in (("means2D", slice(0, 2)), ("conic", slice(2, 5)), ("opacity*coef", slice(5, 6)), ("ts", slice(7, 8)), ("rgb", slice(8, 11)),
                    ("ray_planes", slice(11, 13)), ("normals", slice(13, 16))):
        pairs["splat_a." + k] = (a[:, cols], want["splat_a"][:, cols])
    if s.require_coord:
        b = h.export("splat_b", torch.float32, 12 * P).reshape(P, 12)
        for k, cols in (("camera_planes", slice(0, 6)), ("view_points", slice(6, 9)), ("padding", slice(9, 12))):
            pairs["splat_b." + k] = (b[:, cols], want["splat_b"][:, cols])
    # slot 6 = skip_threshold(slot 5) of the same device function: the packing; its arithmetic is tests/test_gpu_stream_lists.py's
    thr = np.zeros(P, np.float32)
    thr[vis] = dev_skip_thresholds(np.ascontiguousarray(a[vis, 5]))
    pairs["splat_a.skip_threshold"] = (a[:, 6], thr)
    pg.assert_fields(pairs, vis, c.cls, name + ": visible rows")


# ========================================================================== b. backward from the oracle's own sums, bit for bit
B_CASES = ["boundary_deg3_ks0_nocoord", "boundary_deg3_ks0_coord", "boundary_deg1_ks0_nocoord", "boundary_deg1_ks0.1_coord", "precomp_colors_cov3D",
           "scale_modifier_0.7"] + pg.TAILS


def _grad_pairs(got, want, P):
    pairs = {}
    for k in GRADS:
        if got.get(k) is None:
            continue
        pairs[k] = (got[k].reshape(P, -1), np.asarray(want[k], np.float32).reshape(P, -1))
    return pairs


@pytest.mark.parametrize("name", B_CASES)
def test_backward_from_the_oracles_sums_bit_for_bit(name):
    """With identical sums there is no summation order left: every returned gradient of every row (the ill-conditioned ones included) must be the
    oracle's, in the mode the reference executes and in the intended one; invisible rows exactly zero (the hook pre-fills its outputs with NaN)."""
    import diff_gaussian_rasterization._C as C
    from oracle import oracle as orc
    c = pg.get_case(name)
    o, s, P = c.o, c.s, c.P
    h = _run(c)
    g = upstream_grads(s, 3)
    vis, every = o.get("radii") > 0, np.ones(P, bool)
    prev = C.OPACITY_GRAD_INTENDED
    try:
        for intended in (False, True):
            orc.set_opacity_slip(0 if intended else 1)
            C.OPACITY_GRAD_INTENDED = intended
            want = oracle_backward(o, g)
            sums = pg.oracle_sums(o, P, s.require_coord)
            got = backward_from_sums(h, sums)
            if c.colors is not None:     # precomputed colours: the oracle returns no SH gradient, the product none either
                assert got["dL_dsh"] is None
                want = dict(want, dL_dsh=None)
            if c.cov3D is not None:      # the zero scale / rotation gradients are the binding's; the oracle leaves them at zero too
                assert not got["dL_dscales"].any() and not got["dL_drotations"].any()
            pairs = _grad_pairs(got, want, P)
            assert set(pairs) >= {"dL_dmeans3D", "dL_dopacity", "dL_dcov3D", "dL_dcolors", "dL_dmeans2D"}
            what = "%s, opacity_grad_intended=%s" % (name, intended)
            pg.assert_fields(pairs, every, c.cls, what)
            for k, (a, _) in pairs.items():
                assert not a[~vis].any(), what + ": %s is not zero on an invisible row" % k
            if "dL_dsh" in pairs:
                K = (s.sh_degree + 1) ** 2
                assert not got["dL_dsh"][:, K:].any(), what + ": SH rows beyond the active degree"
                assert got["dL_dsh"][vis, :K].any()
    finally:
        C.OPACITY_GRAD_INTENDED = prev
        orc.set_opacity_slip(1)


# ============================================================================ c. backward from arbitrary sums, device against host build
@pytest.mark.parametrize("coord", [False, True])
def test_backward_from_arbitrary_sums_equals_the_host_build(coord):
    """What this rests on: tests/test_hostcheck.py (and tests/test_per_gaussian_cases.py on this scene) pin the host build of rg_preprocess_bwd.h
    to the oracle bit for bit.  The oracle's sums are what a blend produces; this case adds magnitudes (1e+-6), all-zero records and signed zeros
    that they never take, over the same headers compiled for the device."""
    import diff_gaussian_rasterization._C as C
    from hostcheck import hostcheck as hc
    c = pg.get_case("boundary_deg3_ks0_coord" if coord else "boundary_deg3_ks0_nocoord")
    o, s, P = c.o, c.s, c.P
    h = _run(c)
    sums = pg.arbitrary_sums(c, coord)
    radii, clb, op = o.get("radii"), pg.clamp_bits(o, P), o.get("conic_opacity", (P, 4))[:, 3]
    every = np.ones(P, bool)
    prev = C.OPACITY_GRAD_INTENDED
    try:
        for intended in (False, True):
            C.OPACITY_GRAD_INTENDED = intended
            got = backward_from_sums(h, sums)
            out, dsh = hc.preprocess_bwd(s, radii, clb, op if intended else sums[:, 14], pg.host_acc(sums))
            assert np.isfinite(out).all() and np.isfinite(dsh).all()
            for k in GRADS:
                assert np.isfinite(got[k]).all(), k
            pairs = {k: (got[k].reshape(P, -1), out[:, sl]) for k, sl in pg.GRAD_COLUMNS}
            pairs["dL_dsh"] = (got["dL_dsh"], dsh)
            pg.assert_fields(pairs, every, c.cls, "arbitrary sums, coord=%s, opacity_grad_intended=%s" % (coord, intended))
    finally:
        C.OPACITY_GRAD_INTENDED = prev


# ================================================================================================ d. launch modes return the same bits
def _native_from_sums(h, sums_t, **kw):
    C, rs, st = h.C, h.rs, h.state
    e = torch.Tensor([])
    out = C.backward_from_sums(sums_t, h.means3D.detach(), st[8], e, h.scales.detach(), h.rotations.detach(), rs.scale_modifier, e, rs.viewmatrix,
                               rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, rs.image_height, rs.image_width, h.shs.detach(),
                               rs.sh_degree, rs.campos, st[9], rs.require_coord, **kw)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def _mode_case(P):
    if P == 3001:
        s = make_scene(P, 160, 120, sh_degree=3, mu_px=3.0, seed=41, kernel_size=0.1, pose="random", require_coord=True, require_depth=True)
        return pg.Case("modes_P3001", s)
    return pg.tail_scene(P)


@pytest.mark.parametrize("P", [129, 513, 3001])
def test_launch_modes_return_the_same_bits(P):
    c = _mode_case(P)
    h = _run(c)
    rec = 32 if c.s.require_coord else 16
    sums = np.random.default_rng(P).standard_normal((P, rec)).astype(np.float32)
    sums_t = torch.from_numpy(sums).to(DEV)
    radii = h.state[8].cpu().numpy()
    vis = radii > 0
    assert vis[-1] and vis.sum() > P // 2
    clamped = h.export("clamped", torch.uint8, P)
    assert P == 129 or (clamped[vis] != 0).any()
    base = _native_from_sums(h, sums_t)
    assert len(base) == 8 and all(np.isfinite(t).all() for t in base)
    every = np.ones(P, bool)
    # dL_drgb_clamped = the colour sums with the clamped channels multiplied by zero (a zero that keeps the sum's sign), zero rows where invisible
    keep = np.stack([((clamped >> ch) & 1) == 0 for ch in range(3)], 1)
    want_drgb = np.where(vis[:, None], sums[:, :3] * np.where(keep, np.float32(1), np.float32(0)), np.float32(0)).astype(np.float32)

    def same(out, what):
        pg.assert_fields({GRADS_ORDER[i]: (out[i].reshape(P, -1), base[i].reshape(P, -1)) for i in range(8)}, every, c.cls, "P=%d, %s" % (P, what))

    for chunks in (2, 3, 7):
        calls = []
        out = _native_from_sums(h, sums_t, grad_chunks=chunks, grads_ready=lambda first, count: calls.append((first, count)))
        same(out, "grad_chunks=%d" % chunks)
        nblocks = (P + 127) // 128
        assert 2 <= len(calls) <= min(chunks, nblocks), calls
        assert calls[0][0] == 0 and all(n > 0 for _, n in calls), calls
        assert all(calls[i][0] + calls[i][1] == calls[i + 1][0] for i in range(len(calls) - 1)) and calls[-1][0] + calls[-1][1] == P, calls
        assert all(f % 128 == 0 for f, _ in calls), calls
    # the inline write of dL_drgb_clamped
    out = _native_from_sums(h, sums_t, want_drgb=True)
    assert len(out) == 9
    same(out, "want_drgb")
    pg.assert_fields({"dL_drgb_clamped": (out[8], want_drgb)}, every, c.cls, "P=%d, inline" % P)
    # ... and the separate drgb_clamped_kernel, announced exactly once, before the first chunk
    events = []
    out = _native_from_sums(h, sums_t, drgb_ready=lambda: events.append("drgb"), grad_chunks=3,
                            grads_ready=lambda first, count: events.append((first, count)))
    same(out, "drgb_ready + grad_chunks=3")
    pg.assert_fields({"dL_drgb_clamped": (out[8], want_drgb)}, every, c.cls, "P=%d, separate kernel" % P)
    assert events.count("drgb") == 1 and events[0] == "drgb" and len(events) >= 3, events
    out = _native_from_sums(h, sums_t, drgb_ready=lambda: events.append("drgb2"), keep_sums=True)
    same(out, "drgb_ready, one launch, keep_sums")
    pg.assert_fields({"dL_drgb_clamped": (out[8], want_drgb)}, every, c.cls, "P=%d, separate kernel, one launch" % P)
    assert events.count("drgb2") == 1
    assert np.array_equal(sums_t.cpu().numpy().view(np.uint32), sums.view(np.uint32)), "the hook only reads its sums"


GRADS_ORDER = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


# ============================================================================ f, g. the three kinds of accumulator record, tied together
# preprocess_bwd_kernel reads a record as one of three kinds (csrc/rg_per_gaussian.inc::RecordKind): raw moments (every blend backward), the
# reference's final sums (backward_from_sums), blend sums with the constant factors pending (no blend at all).  The ordered backward
# (RADEGS_DETERMINISTIC=1) makes the raw records bit-reproducible, so the kinds can be held against each other bit for bit.
KIND_SCENES = [257, 513, 3001]     # tail_scene(257): degree 2, the word-loop slab; tail_scene(513); _mode_case(3001): coord map, kernel_size 0.1


def _ordered_case(P, monkeypatch):
    """-> (case, HipRun after its forward, cotangents), with the ordered backward switched on"""
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    c = _mode_case(P)
    h = _run(c)
    visible = int((h.state[8] > 0).sum())
    assert h.state[0] > 0 and visible > P // 2, "R = %d, %d of %d rows visible" % (h.state[0], visible, P)
    return c, h, upstream_grads(c.s, 3)


def _same_grads(got, want, c, what):
    pairs = {k: (got[k].reshape(c.P, -1), want[k].reshape(c.P, -1)) for k in GRADS}
    assert len(pairs) == 8
    for k, (a, b) in pairs.items():
        print("%s: %s: %d of %d words differ" % (what, k, int((a.view(np.uint32) != b.view(np.uint32)).sum()), a.size))
    pg.assert_fields(pairs, np.ones(c.P, bool), c.cls, what)


@pytest.mark.parametrize("P", KIND_SCENES)
def test_keeping_the_sums_does_not_change_what_is_returned(P, monkeypatch):
    """RadegsBwdArgs::keep_sums makes the kernel write every visible record back in the reference's form; the eight gradients of the launch
    must not notice (same forward state, same fixed-order sums: bit for bit)."""
    from test_gpu_deterministic import _backward
    c, h, g = _ordered_case(P, monkeypatch)
    plain, none, _ = _backward(h, h.state, g, keep=False)
    kept, acc, _ = _backward(h, h.state, g, keep=True)
    assert none is None and acc[h.state[8].cpu().numpy() > 0].any()
    _same_grads(kept, plain, c, "P=%d, KEEP_ACC on against off" % P)


def reference_form(acc, s):
    """LAST_ACC of a backward with keep_sums -- the record in the reference's form WITHOUT the constant factors (include/radegs.h) -- with
    those factors applied in float32 exactly as preprocess_bwd_kernel applies them to a record whose factors are pending: 1/focal on the
    plane sums (slots 4, 5 and, with the coord map, 19..24 alternating), (0.5f * W) and (0.5f * H) on the mean2D sums (slots 9, 10); focal
    as rg_launch.inc::make_cam computes it."""
    f32 = np.float32
    focal_x, focal_y = f32(s.W) / (f32(2.0) * f32(s.tanfovx)), f32(s.H) / (f32(2.0) * f32(s.tanfovy))
    ifx, ify = f32(1.0) / focal_x, f32(1.0) / focal_y
    a = acc.astype(np.float32).copy()
    a[:, 4] *= ifx
    a[:, 5] *= ify
    if a.shape[1] == 32:
        a[:, 19:25:2] *= ifx
        a[:, 20:25:2] *= ify
    a[:, 9] *= f32(0.5) * f32(s.W)
    a[:, 10] *= f32(0.5) * f32(s.H)
    assert a.dtype == np.float32
    return a


@pytest.mark.parametrize("P", KIND_SCENES)
def test_raw_records_and_reference_sums_return_the_same_bits(P, monkeypatch):
    """An ordered backward with keep_sums returns its gradients from RAW records and leaves them behind in the reference's form; those, with
    the constant factors applied (reference_form), are records of the REFERENCE kind.  backward_from_sums over them must return what the
    ordered backward returned, in both opacity modes: the conversion of a raw record (rg_preprocess_bwd.h: the moments times the conic, the
    -0.5f on the second moments, W/2 and H/2 afterwards) and the pending 1/focal factors are then the only difference between the two
    paths, and each is one float32 operation on either side.
    Criterion from the parent of the commit that added this test (same scenes, same GPU): all eight gradients bit-identical in both modes,
    0 of every tensor's words differing -- so bit identity is what is asserted."""
    import diff_gaussian_rasterization._C as C
    from test_gpu_deterministic import _backward
    c, h, g = _ordered_case(P, monkeypatch)
    for intended in (False, True):
        monkeypatch.setattr(C, "OPACITY_GRAD_INTENDED", intended)
        want, acc, _ = _backward(h, h.state, g, keep=True)
        got = backward_from_sums(h, reference_form(acc, c.s))
        _same_grads(got, want, c, "P=%d, opacity_grad_intended=%s, reference kind against raw kind" % (P, intended))


# ============================================================================================================ e. sh_grad_from_views
# SH constants of the reference (cuda_rasterizer/auxiliary.h: SH_C0 .. SH_C3, used by forward.cu's computeColorFromSH)
SH_C0, SH_C1 = 0.28209479177387814, 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)


def sh_basis64(deg, pos, campos):
    """[P,16] float64: the weight of every SH coefficient in the colour of direction normalize(pos - campos); zero beyond (deg+1)^2"""
    d = pos.astype(np.float64) - campos.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    w = np.zeros((pos.shape[0], 16))
    w[:, 0] = SH_C0
    if deg > 0:
        w[:, 1], w[:, 2], w[:, 3] = -SH_C1 * y, SH_C1 * z, -SH_C1 * x
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        w[:, 4], w[:, 5], w[:, 6] = SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy)
        w[:, 7], w[:, 8] = SH_C2[3] * xz, SH_C2[4] * (xx - yy)
    if deg > 2:
        w[:, 9], w[:, 10] = SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * xy * z
        w[:, 11], w[:, 12] = SH_C3[2] * y * (4.0 * zz - xx - yy), SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy)
        w[:, 13], w[:, 14] = SH_C3[4] * x * (4.0 * zz - xx - yy), SH_C3[5] * z * (xx - yy)
        w[:, 15] = SH_C3[6] * x * (xx - 3.0 * yy)
    return w


SH_SHAPES = [(P, D, 16) for P in (1, 127, 129, 1000) for D in (0, 1, 2, 3)] + [(129, 1, 4), (1000, 1, 4), (127, 2, 9), (129, 3, 16), (1000, 3, 16)]
SH_SHAPES = list(dict.fromkeys(SH_SHAPES))


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("P,D,M", SH_SHAPES)
def test_sh_grad_from_views_direct(P, D, M, V):
    import diff_gaussian_rasterization._C as C
    rng = np.random.default_rng(1000 * P + 10 * D + V + M)
    means = (rng.standard_normal((P, 3)) * 2.0 + np.array([0.0, 0.0, 6.0])).astype(np.float32)
    campos = (rng.standard_normal((V, 3)) * 0.5).astype(np.float32)
    drgb = rng.standard_normal((V, P, 3)).astype(np.float32)
    drgb[:, rng.random(P) < 0.25] = 0.0     # all-zero rows: the kernel's skip path (not visible, or fully clamped, in that view)
    if P == 1:
        drgb[:] = rng.standard_normal((V, 1, 3)).astype(np.float32) if D % 2 else 0.0
    scale = 1.0 / 3.0
    out = torch.full((P, M, 3), float("nan"), dtype=torch.float32, device=DEV)
    C.sh_grad_from_views(torch.from_numpy(means).to(DEV), torch.from_numpy(campos).to(DEV), torch.from_numpy(drgb).to(DEV), D, M, scale, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = np.zeros((P, 16, 3))
    for v in range(V):
        want += sh_basis64(D, means, campos[v])[:, :, None] * drgb[v].astype(np.float64)[:, None, :]
    want = (want * np.float64(np.float32(scale)))[:, :M]
    K = (D + 1) ** 2
    assert not got[:, K:].any(), "rows beyond (D+1)^2 must be exactly zero"
    bad = ~close(got, want, ATOL, RTOL)
    assert not bad.any(), "%d of %d elements outside %g / %g, max |diff| %.3e" % (int(bad.sum()), bad.size, ATOL, RTOL, float(np.abs(got - want).max()))
    assert P == 1 or np.abs(got[:, :K]).max() > 0.1
