"""CPU side of the edge-case tests of the fused step kernels (tests/step_edge_cases.py): every input condition the GPU tests rely on
is asserted here, and the numpy oracles are pinned AT THESE INPUTS to what the reference's own Python returns
(tests/golden/make_golden_step_edges.py -> tests/golden/step_edges_*.npz) -- the eps branch of the normal oracle, sign(0) of the L1
gradient, the fallback of compute_3D_filter and the 0/0 rows of the activations had never been pinned.

The pin uses the acceptance form of the GPU tests (step_edge_cases.rule) with the golden in the kernel's place: the reference's float32
result must be as close to the float64 oracle as the float32 oracle is.  The few comparisons where torch's float32 evaluation is further
away than 4x / 2x are listed in PIN_BARS with twice their measured ratio and the reason; all others stay at 4 / 2."""
import functools
import os

import numpy as np
import pytest

import step_edge_cases as sec
from oracle import adam_oracle as ao
from oracle import filter3d_oracle as fo
from oracle import knn_oracle
from oracle import loss_oracle as lo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# Every pin is held at 4 / 2 but the comparisons listed here, which measured more and carry twice their measured (max, rms) ratio.
PIN_BARS = {
    # autograd sums the four 1e7-sized contributions of a pixel in another order than the oracle's `+=`, next to a cancellation of
    # up to 3.7e4: measured 3.48 / 2.44
    "holes_depth_b g2 eps-touched": dict(krms=4.9),
    # the reference blurs with the 11x11 outer-product window in one conv2d, the oracle separably: measured 6.65 / 3.74 and 1.37 / 2.53
    "C3 unequal": dict(kmax=13.3, krms=7.5),
    "C1 unequal": dict(krms=5.1),
    # autograd differentiates exp, square, prod, divide and sqrt one by one where the oracle uses the closed form: measured 2.56 / 2.18
    "act opacity g_scaling_raw plain": dict(krms=4.4),
}


@functools.lru_cache(None)
def gold(name):
    return np.load(os.path.join(GOLD, f"step_edges_{name}.npz"))


# ------------------------------------------------------------------------------------------------------------------- the rule
def test_rule_accepts_oracle_noise_and_rejects_a_wrong_term():
    rng = np.random.default_rng(0)
    ref = rng.standard_normal(1000)
    o32 = ref.astype(np.float32)
    assert sec.rule(o32, o32, ref)["ok"]
    assert sec.rule((ref * (1 + 3e-8)).astype(np.float64), o32, ref)["ok"]
    bad = o32.copy()
    bad[7] *= np.float32(1.001)
    assert not sec.rule(bad, o32, ref)["ok"]
    assert not sec.rule(o32 * np.float32(1.00001), o32, ref)["ok"]
    nan = o32.copy()
    nan[3] = np.nan
    assert not sec.rule(nan, o32, ref)["ok"]
    # relative: a reference of exactly zero admits only exactly zero
    z = np.array([0.0, 1e7, 1e-3])
    assert sec.rule(z.astype(np.float32), z.astype(np.float32), z, relative=True)["ok"]
    assert not sec.rule(np.array([1e-30, 1e7, 1e-3], np.float32), z.astype(np.float32), z, relative=True)["ok"]
    # classes are separate: an error that hides under a class of 1e7 is seen in its own class
    big = np.array([True, False] * 500)
    ref2 = np.where(big, 5e7, 1e-3) * np.sign(ref)
    o2 = ref2.astype(np.float32)
    wrong = np.where(big, o2, o2 * np.float32(2))
    assert np.abs(wrong - ref2).max() < 2e-3 * np.abs(ref2).max()             # the old form passes it
    assert not sec.rule(wrong, o2, ref2, ~big)["ok"]


# -------------------------------------------------------------------------------------------------------------------- normals
@pytest.mark.parametrize("points", [False, True])
def test_normals_holes_conditions(points):
    c = sec.normals_holes()
    H, W = c["H"], c["W"]
    assert (W, H) == (70, 21) and W > 64 and H > 4 * 5
    hole = c["hole"]
    for k in ("depth1", "depth2"):
        assert (c[k][0][hole] == 0).all() and (c[k][0][~hole] > 2).all()
    assert (c["points1"][:, hole] == 0).all() and (c["points2"][:, hole] == 0).all()
    assert hole[:, -1].all() and hole[5, 31:50].all() and not hole[5, 30] and hole[:, 40].all()     # band on the border, segment, column
    assert (c["depth2"][0, 12:16, 44:52] == 2.5).all()
    m64 = sec.normal_maps64(c, points)
    L = sec.cross_lengths(m64)
    assert not ((L > 0) & (L < 1e-6)).any()                      # float32 and float64 agree on the branch of every centre
    assert int((L == 0).sum()) == 758 and L.size == 2584
    m32 = np.stack([c["points1"], c["points2"]], 0) if points else None
    if m32 is not None:
        assert ((sec.cross_lengths(m32) <= 1e-12) == (L == 0)).all()
    deg = sec.degenerate_centres(m64)
    assert (deg[0] == deg[1]).all() and (deg <= hole[None]).all()
    assert not (deg[0] & sec.border_mask(H, W)).any()
    # variant (a): no degenerate centre carries a cotangent; variant (b): every one does
    assert not sec.eps_touched(deg, (c["rn_a"] != 0).any(0)).any()
    assert (c["rn_b"] != 0).all() and (c["cot"] != 0).all()
    t = sec.eps_touched(deg, (c["rn_b"] != 0).any(0))
    assert 300 < t[0].sum() < H * W - 300                        # both classes populated
    assert t[0][:, -1].any() and t[0][0].any()                   # the eps-touched class reaches the image border


@pytest.mark.parametrize("points", [False, True])
@pytest.mark.parametrize("variant", ["a", "b"])
def test_normal_oracle_pinned_to_reference_on_holes(points, variant):
    c, Z = sec.normals_holes(), gold("normals")
    mode = "points" if points else "depth"
    tag = f"holes_{mode}_{variant}"
    for k in ("depth1", "depth2", "points1", "points2"):
        assert np.array_equal(Z[f"holes_{k}"], c[k])             # the golden was made from these inputs
    rn = c[f"rn_{variant}"]
    r64, r32 = sec.normals_reference(c, points, rn, np.float64), sec.normals_reference(c, points, rn, np.float32)
    deg = sec.degenerate_centres(sec.normal_maps64(c, points))
    zero = deg | sec.border_mask(c["H"], c["W"])[None]
    for r in (r64, r32, dict(normals=Z[f"{tag}_normals"], g_rendered=Z[f"{tag}_g_rendered"])):
        assert (r["normals"][np.broadcast_to(zero[:, None], r["normals"].shape)] == 0).all()
        assert (r["g_rendered"][:, zero[0]] == 0).all()
    assert sec.report(f"{tag} normals", sec.rule(Z[f"{tag}_normals"], r32["normals"], r64["normals"]))
    assert sec.report(f"{tag} g_rendered", sec.rule(Z[f"{tag}_g_rendered"], r32["g_rendered"], r64["g_rendered"]))
    assert abs(float(Z[f"{tag}_loss"]) - r64["loss"]) <= 4 * abs(r32["loss"] - r64["loss"]) + np.spacing(np.float32(r64["loss"]))
    touched = sec.eps_touched(deg, (rn != 0).any(0))
    cot_touched = sec.eps_touched(deg, np.ones((c["H"], c["W"]), bool))
    c64, c32 = sec.normals_vjp(c, points, c["cot"], np.float64), sec.normals_vjp(c, points, c["cot"], np.float32)
    for k in range(2):
        shape = (-1, c["H"], c["W"])
        for what, g, o32, ref, t in ((f"g{k + 1}", Z[f"{tag}_g{k + 1}"], r32[f"g{k + 1}"], r64[f"g{k + 1}"], touched[k]),
                                     (f"c{k + 1}", Z[f"holes_{mode}_c{k + 1}"], c32[k], c64[k], cot_touched[k])):
            g, o32, ref = g.reshape(shape), o32.reshape(shape), ref.reshape(shape)
            assert np.isfinite(g).all()
            t = np.broadcast_to(t, ref.shape)
            assert sec.report(f"{tag} {what} ordinary", sec.rule(g, o32, ref, ~t))
            assert sec.report(f"{tag} {what} eps-touched", sec.rule(g, o32, ref, t, relative=True, **PIN_BARS.get(f"{tag} {what} eps-touched", {})))
    if variant == "b":
        big = np.abs(r64["g1"].reshape(-1, c["H"], c["W"]))[np.broadcast_to(touched[0], (r64["g1"].size // (c["H"] * c["W"]), c["H"], c["W"]))]
        assert big.max() > 1e7 and np.median(np.abs(r64["g1"])) < 1e-1      # 1e7 next to ordinary gradients


def test_normals_all_empty_reference():
    c, Z = sec.normals_all_empty(), gold("normals")
    assert (c["W"], c["H"]) == (65, 5) and (c["rn_b"] != 0).all()
    for points in (False, True):
        tag = f"empty_{'points' if points else 'depth'}_b"
        for r in (sec.normals_reference(c, points, c["rn_b"], np.float32), {k: Z[f"{tag}_{k}"] for k in ("normals", "loss", "g1", "g2", "g_rendered")}):
            assert np.float32(r["loss"]) == 1.0                 # (the float32 oracle adds float32(0.4) + float32(0.6) in double)
            for k in ("normals", "g1", "g2", "g_rendered"):
                assert (np.asarray(r[k]) == 0).all(), (tag, k)


# ---------------------------------------------------------------------------------------------------------------- photometric
@pytest.mark.parametrize("C", [3, 1])
def test_photometric_masked_conditions_and_oracle_pin(C):
    img, gt = sec.photometric_masked(C)
    Z = gold("losses")
    assert np.array_equal(Z[f"masked_C{C}_img"], img) and np.array_equal(Z[f"masked_C{C}_gt"], gt)
    assert img.shape == (C, 37, 131)
    eq = img == gt
    assert eq.mean() >= 0.5
    assert (img[:, :, :40] == 0).all() and (gt[:, :, :40] == 0).all() and (img[:, :, 96:] == 1).all() and (gt[:, :, 96:] == 1).all()
    assert eq[:, 26:, 40:96].all() and (img[:, 10:14, 50:60] == np.float32(1.7)).all() and img.max() > 1
    assert 0.05 < (~eq).mean()
    i64, g64 = img.astype(np.float64), gt.astype(np.float64)
    assert abs(lo.rgb_loss(i64, g64, 0.2) - float(Z[f"masked_C{C}_loss"])) < 5e-6
    assert abs(lo.l1_loss(i64, g64) - float(Z[f"masked_C{C}_l1"])) < 1e-6
    assert abs(lo.ssim(i64, g64) - float(Z[f"masked_C{C}_ssim"])) < 5e-6
    ref, o32, g = lo.rgb_loss_bwd(i64, g64, 0.2), lo.rgb_loss_bwd(img, gt, 0.2), Z[f"masked_C{C}_grad"]
    assert np.abs(g - ref).max() < 1e-4 * np.abs(ref).max()
    assert np.abs(o32 - ref).max() < 1e-4 * np.abs(ref).max()
    assert sec.report(f"C{C} equal", sec.rule(g, o32, ref, eq))
    assert sec.report(f"C{C} unequal", sec.rule(g, o32, ref, ~eq, **PIN_BARS.get(f"C{C} unequal", {})))
    # sign(0) = 0: with lambda_dssim = 0 the gradient is exactly 0 where img == gt and exactly +-1/n elsewhere
    n = img.size
    g1 = Z[f"masked_C{C}_grad_l1"]
    for a in (g1, lo.rgb_loss_bwd(img, gt, 0.0).astype(np.float32)):
        assert (a[eq] == 0).all()
        assert np.array_equal(a[~eq], (np.sign(img - gt)[~eq] * np.float32(1.0 / n)).astype(np.float32))
    # identical images
    assert float(Z[f"identical_C{C}_l1"]) == 0.0 and lo.l1_loss(gt, gt) == 0.0
    assert abs(float(Z[f"identical_C{C}_ssim"]) - 1) <= 2 ** -23 and abs(lo.ssim(gt, gt) - 1) <= 2 ** -23
    assert sec.report(f"C{C} identical", sec.rule(Z[f"identical_C{C}_grad"], lo.rgb_loss_bwd(gt, gt, 0.2), lo.rgb_loss_bwd(g64, g64, 0.2)))


# ----------------------------------------------------------------------------------------------------------------------- Adam
ADAM_UPDATE_BAR = 1e-3
"""Bar on the update p_after - p_before, relative to the largest update of the tensor.  The restatement's own deviation from
torch.optim.Adam measured here is 2.4e-4 (one ulp of a parameter of 0.25..0.5 against an update of 1.25e-4: torch's lerp / addcdiv round
differently in the last bit); times 4, rounded.  A bias correction off by one step moves the update by 40 % at step 2."""


def _adam_kw(t):
    g = sec.ADAM_GROUPS[t.group]
    return dict(beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"])


def test_adam_layout_conditions():
    lay = sec.adam_layout()
    assert len(lay) == 20 and len({t.name for t in lay}) == 20
    g0 = [t for t in lay if t.group == 0 and t.has_grad]
    assert len(g0) > 16                                            # the 16-tensor table is filled twice
    assert sum(t.numel == 0 for t in lay) == 1 and 0 < [t.numel for t in lay].index(0) < 16
    assert sum(not t.has_grad for t in lay) == 1 and lay[0].has_grad and lay[-1].has_grad
    assert {1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 2048 * 3 + 1} <= {t.numel for t in lay}
    offs = {t.offsets for t in lay}
    assert (0, 0, 0, 0) in offs and (0, 1, 0, 0) in offs
    for slot in range(4):
        assert {o[slot] for o in offs} == {0, 1, 2, 3}
    assert any(t.group == 1 for t in lay) and sec.ADAM_GROUPS[0] != sec.ADAM_GROUPS[1]
    for t in lay:
        if t.numel:
            p, g, m, v = sec.adam_data(t, 1)
            z = (g == 0) & (v == 0)
            assert z.any() and (m[z] != 0).any()                   # the eps regime: m / (0 + eps)
            assert (sec.adam_data(t, 0)[1] == 0).any()


def test_adam_restatement_against_torch():
    Z = gold("adam")
    worst = 0.0
    for t in sec.adam_layout():
        if not (t.has_grad and t.numel):
            continue
        kw = _adam_kw(t)
        p0, g, m, v = sec.adam_data(t, 0)
        p1, m1, v1 = sec.adam_step32(p0, g, m, v, 1, t.lr, **kw)
        p2, m2, v2 = sec.adam_step32(p1, sec.adam_second_grad(t), m1, v1, 2, t.lr, **kw)
        q0, g, m, v = sec.adam_data(t, 1)
        q1, _, _ = sec.adam_step32(q0, g, m, v, 1000, t.lr, **kw)
        o1, _, _ = ao.step(q0, g, m, v, 1000, t.lr, **kw)
        assert np.allclose(o1, q1, rtol=1e-5, atol=1e-7)           # the oracle and its float32-scalar restatement
        for got, ref, before, tag in ((p1, Z[f"s1_{t.name}"], p0, "s1"), (p2, Z[f"s2_{t.name}"], Z[f"s1_{t.name}"], "s2"),
                                      (q1, Z[f"s1000_{t.name}"], q0, "s1000")):
            assert got.dtype == np.float32 and np.isfinite(got).all()
            assert np.abs(got - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max()) + 2e-7, (t.name, tag)
            ua, ub = got.astype(np.float64) - before, ref.astype(np.float64) - before
            if not ub.any():
                assert not ua.any()                                 # zero gradients on fresh state: nothing moves
                continue
            dev = np.abs(ua - ub).max() / np.abs(ub).max()
            worst = max(worst, dev)
            assert dev <= ADAM_UPDATE_BAR, (t.name, tag, dev)
        if t.numel <= 1100:
            assert np.allclose(m2, Z[f"m2_{t.name}"], rtol=1e-5, atol=1e-12) and np.allclose(v2, Z[f"v2_{t.name}"], rtol=1e-5, atol=1e-20)
    print("adam restatement: worst update deviation from torch", worst)
    assert worst > 0                                               # the bar is not vacuous: torch and the restatement do differ


@pytest.mark.parametrize("mutation", ["bc2_step_minus_1", "no_bias_correction"])
def test_adam_update_bar_catches_a_wrong_bias_correction(mutation):
    import math
    Z = gold("adam")
    t = [t for t in sec.adam_layout() if t.name == "n1025"][0]
    p1 = Z["s1_n1025"]
    p0, g, m, v = sec.adam_data(t, 0)
    _, m1, v1 = sec.adam_step32(p0, g, m, v, 1, t.lr)
    g2 = sec.adam_second_grad(t)
    m2 = m1 + np.float32(0.1) * (g2 - m1)
    v2 = v1 * np.float32(0.999) + np.float32(0.001) * (g2 * g2)
    bc1 = 1 - 0.9 ** 2 if mutation == "bc2_step_minus_1" else 1.0
    bc2 = 1 - 0.999 ** (1 if mutation == "bc2_step_minus_1" else 2)
    wrong = p1 - np.float32(t.lr / bc1) * (m2 / (np.sqrt(v2) / np.float32(math.sqrt(bc2)) + np.float32(1e-15)))
    ref = Z["s2_n1025"]
    dev = np.abs((wrong.astype(np.float64) - p1) - (ref.astype(np.float64) - p1)).max() / np.abs(ref.astype(np.float64) - p1).max()
    assert dev > 100 * ADAM_UPDATE_BAR


# ------------------------------------------------------------------------------------------------------------ compute_3D_filter
@functools.lru_cache(None)
def filter_scene(name):
    g = np.load(os.path.join(GOLD, "filter3d.npz"))
    cams12 = sec.cameras_from_rows(g["cams"])
    if name == "golden":
        xyz, cams, ref = g["xyz"], cams12, g["filter_out"]
    else:
        xyz, cams, ref = sec.filter_random_xyz(), sec.cameras_cycled(cams12), gold("filter3d")["random_filter"]
    return xyz, cams, ref, sec.filter_analysis(xyz, cams)


@pytest.mark.parametrize("name,share", [("golden", 0.0), ("random", 0.01)])
def test_filter_scene_conditions_and_oracle_pin(name, share):
    xyz, cams, gref, an = filter_scene(name)
    P = xyz.shape[0]
    assert P == (4096 if name == "golden" else 20000) and len(cams) == (12 if name == "golden" else 150)
    amb = an["ambiguous"]
    print(name, "ambiguous share", amb.mean(), "seen", an["seen"].mean())
    assert amb.mean() <= share
    assert an["seen"].any() and (~an["seen"]).any()                 # the fallback is taken
    assert an["argmax"] >= 0 and not amb[an["argmax"]]              # the maximum over seen points is not in doubt ...
    maybe = np.where(np.isfinite(an["zmin_maybe"]), an["zmin_maybe"], 0.0)
    assert (maybe[amb] <= an["max_seen"]).all()                     # ... and no flip can raise it
    ok = ~amb
    for out in (fo.compute_3D_filter(xyz, cams)[:, 0], gref[:, 0]):
        rel = np.abs(out - an["ref"]) / an["ref"]
        print(name, "max rel outside the ambiguous set", rel[ok].max())
        assert (rel[ok] <= 1e-5).all()
        for i in np.flatnonzero(amb):
            assert min(abs(out[i] - v) / v for v in sec.filter_candidates(an, i)) <= 1e-5


def test_filter_fallback_scenes():
    Z = gold("filter3d")
    xyz, cams = sec.filter_scene_one_seen()
    an = sec.filter_analysis(xyz, cams)
    assert an["seen"].sum() == 1 and an["seen"][200] and xyz.shape[0] > 256
    # the point exactly on the near threshold has margin 0; under the identity camera its view z is its own z, without rounding
    assert list(np.flatnonzero(an["ambiguous"])) == [sec.EXACT_NEAR_ROW] and xyz[sec.EXACT_NEAR_ROW, 2] == np.float32(0.2)
    assert (cams[0].R == np.eye(3)).all() and not cams[0].T.any()
    for out in (Z["one_seen_filter"][:, 0], fo.compute_3D_filter(xyz, cams)[:, 0]):
        assert (out == out[200]).all() and abs(out[200] - an["ref"][200]) <= 1e-5 * an["ref"][200]
    xyz, cams = sec.filter_scene_none_seen()
    an = sec.filter_analysis(xyz, cams)
    assert not an["seen"].any() and list(np.flatnonzero(an["ambiguous"])) == [sec.EXACT_NEAR_ROW] and (an["ref"] == 0).all()
    assert bool(Z["none_seen_raises"])                              # the reference takes .max() of an empty selection
    with pytest.raises(ValueError):
        fo.compute_3D_filter(xyz, cams)                             # and so does the oracle


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257])
def test_filter_small_P_conditions(P):
    xyz, cams, _, _ = filter_scene("golden")
    an = sec.filter_analysis(xyz[:P], cams)
    assert not an["ambiguous"].any() and an["seen"].any()


# ------------------------------------------------------------------------------------------------------------------ activations
def test_activation_case_conditions_and_oracle_pin():
    c, Z = sec.activation_case(257), gold("filter3d")
    for k in ("scaling_raw", "opacity_raw", "filter_3D"):
        assert np.array_equal(Z[f"act_{k}"], c[k])
    sc, f3, cls = c["scaling_raw"], c["filter_3D"], c["cls"]
    assert sc.min() >= -9 and sc.max() <= 3
    assert (f3[cls == 1] == 0).all() and (f3[cls != 1] > 0).all()
    assert (f3[cls == 2, 0] >= 99.9 * np.exp(sc[cls == 2].astype(np.float64)).max(1)).all()
    assert (c["opacity_raw"][cls == 3] == 30).all() and (c["opacity_raw"][cls == 4] == -30).all()
    for P in (1, 255, 256, 257):
        assert len(set(sec.activation_case(P)["cls"])) == min(P, 5)
    a64 = [c[k].astype(np.float64) for k in ("scaling_raw", "opacity_raw", "filter_3D")]
    a32 = [c[k] for k in ("scaling_raw", "opacity_raw", "filter_3D")]
    s64, o64 = fo.forward(*a64)
    s32, o32 = fo.forward(*a32)
    assert np.isfinite(o64).all() and (o64 > 0).all() and (o32 > 0).all()      # no product underflows
    # filter exactly 0: the coefficient is exactly 1 and sqrt(s^2 + 0) returns s = exp(raw) to 1 ulp (s^2 rounds by 2^-24, the root
    # halves that and rounds once more).  Against the float64 exp the float32 exp's own ulp comes on top: 2 ulps.
    f0 = cls == 1
    e = np.exp(sc[f0].astype(np.float64))
    assert (np.abs(s32[f0] - np.exp(sc[f0])) <= np.spacing(np.exp(sc[f0]))).all()
    # the same for any float32 s the device's expf may return over the range of raw scales: correctly rounded multiply and root alone
    e_any = np.exp(np.random.default_rng(1).uniform(-9, 3, 1_000_000)).astype(np.float32)
    assert (np.abs(np.sqrt(e_any * e_any) - e_any) <= np.spacing(e_any)).all()
    for s in (Z["act_scales"], s32):
        assert (np.abs(s[f0] - e) <= 2 * np.spacing(e.astype(np.float32))).all()
    sg = 1 / (1 + np.exp(-c["opacity_raw"][f0].astype(np.float64)))
    assert (np.abs(Z["act_opacity"][f0] - sg) <= 2 * np.spacing(sg.astype(np.float32))).all()      # float32 exp, add, divide
    for name in sec.ACT_CLASSES:
        m = cls == sec.ACT_CLASSES.index(name)
        assert sec.report(f"act scales {name}", sec.rule(Z["act_scales"], s32, s64, m[:, None]))
        assert sec.report(f"act opacity {name}", sec.rule(Z["act_opacity"], o32, o64, m[:, None]))
        for path in ("both", "scales", "opacity"):
            cs = c["cot_scales"] * (path != "opacity")
            co = c["cot_opacity"] * (path != "scales")
            g64 = fo.backward(*a64, cs.astype(np.float64), co.astype(np.float64))
            g32 = fo.backward(*a32, cs, co)
            for k, key in enumerate(("g_scaling_raw", "g_opacity_raw")):
                if name == "filter0" and key == "g_scaling_raw" and path == "opacity":
                    # d coef / d raw = coef f^2 / (s^2 + f^2) is exactly 0 at f = 0; autograd reaches it as the difference of the det1 and
                    # det2 paths, two terms of |cot sg coef| <= max|cot| rounded separately: a residue of a few ulps of that
                    assert (g64[k][m] == 0).all() and (g32[k][m] == 0).all()
                    assert np.abs(Z[f"act_{path}_{key}"][m]).max() <= 4 * 2.0 ** -23 * np.abs(co).max()
                    continue
                r = sec.rule(Z[f"act_{path}_{key}"], g32[k], g64[k], m[:, None], **PIN_BARS.get(f"act {path} {key} {name}", {}))
                assert sec.report(f"act {path} {key} {name}", r)


def test_activation_zero_over_zero_pattern():
    """scales of exp(-30) with filter 0: det1 = det2 = 0 in float32 and the reference's coefficient is 0/0.  Only the pattern of finite
    and non-finite values is recorded: the opacity and both gradients of the rows are NaN, the scales finite."""
    c, Z = sec.activation_zero_over_zero(), gold("filter3d")
    with np.errstate(all="ignore"):
        s32, o32 = fo.forward(c["scaling_raw"], c["opacity_raw"], c["filter_3D"])
        g32 = fo.backward(c["scaling_raw"], c["opacity_raw"], c["filter_3D"], c["cot_scales"], c["cot_opacity"])
    assert np.isfinite(Z["zero_scales"]).all() and np.isnan(Z["zero_opacity"]).all()
    assert np.array_equal(np.isfinite(s32), np.isfinite(Z["zero_scales"])) and np.array_equal(np.isfinite(o32), np.isfinite(Z["zero_opacity"]))
    assert np.isnan(Z["zero_both_g_scaling_raw"]).all() and np.isnan(Z["zero_both_g_opacity_raw"]).all()
    assert np.isnan(g32[1]).all()
    assert np.isfinite(Z["zero_scales_g_scaling_raw"]).all()        # only `scales` used: the coefficient is not on the path


# ------------------------------------------------------------------------------------------------------------------------ 3-NN
@pytest.mark.parametrize("P", [1, 2, 3])
def test_knn_oracle_fewer_than_four_points(P):
    assert np.isposinf(knn_oracle.mean_dist2_3nn(sec.knn_uniform(P))).all()


def test_knn_case_conditions():
    for P in sec.KNN_UNIFORM_P:
        assert sec.knn_uniform(P).shape == (P, 3)
    assert {1023, 1024, 1025, 2049} <= set(sec.KNN_UNIFORM_P)
    assert (knn_oracle.mean_dist2_3nn(sec.knn_identical()) == 0).all()
    line, plane = sec.knn_line(), sec.knn_plane()
    assert (np.ptp(line, axis=0) == 0).sum() == 2 and (np.ptp(plane, axis=0) == 0).sum() == 1
    pts, copies = sec.knn_duplicates()
    assert copies.sum() == 2500 > 2 * 1024 and len(pts) == 4000 and len(np.unique(pts[~copies], axis=0)) == 1500
    ref = knn_oracle.mean_dist2_3nn(pts)
    assert (ref[copies] == 0).all() and (ref[~copies] > 0).all()
    d = np.abs(pts[~copies] - pts[copies][0]).max(1)
    assert (d <= 1e-3 + 1e-6).sum() == 500 and (d >= 1).sum() == 1000
    lat, interior = sec.knn_lattice()
    assert len(lat) == 1000 and interior.sum() == 512
    assert np.array_equal(lat, (lat.astype(np.float64) * 8).round() / 8)       # exact in float32
    ref = knn_oracle.mean_dist2_3nn(lat)
    assert (ref[interior] == 1 / 64).all() and (ref[~interior] >= 1 / 64).all()
    for p in (line, plane, pts, lat, sec.knn_identical()):
        assert len(p) <= 4000
