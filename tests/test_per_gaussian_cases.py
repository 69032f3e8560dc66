"""CPU tier of the direct per-Gaussian tests (tests/test_gpu_per_gaussian.py): the ORACLE ALONE populates every class of rows the GPU test
relies on, and the packers that lay its arrays out for the device agree bit for bit with the host build of the product's headers
(tests/hostcheck), which tests/test_hostcheck.py pins to the oracle.  The counts are conditions on the scenes, stated here, not measurements."""
import numpy as np
import pytest

import per_gaussian_cases as pg
from gpu_util import reference_sums
from hostcheck import hostcheck as hc
from oracle import oracle as orc
from synth_scene import upstream_grads
from util import oracle_backward


@pytest.mark.parametrize("name", pg.BOUNDARY)
def test_boundary_scene_populates_every_class(name):
    c = pg.get_case(name)
    n = c.counts
    assert c.P <= 4000 and c.s.W <= 203 and c.s.H <= 136
    assert n["near_visible"] >= 3 and n["near_culled"] >= 3, "rows within 8 ulps of the near plane: %d visible, %d culled" % (n["near_visible"], n["near_culled"])
    for e in ("edge_left", "edge_top", "edge_right", "edge_bottom"):
        assert n[e] >= 5, "%s: %d visible rows with the centre outside and the rectangle clamped" % (e, n[e])
    # The reference returns at an empty tile rectangle before it writes the radius (forward.cu:402-403 against :418), and so do the oracle and the
    # product: a row with radii > 0 and tiles_touched == 0 does not exist.  What exists, and what the far-outside rows are here for, is the row
    # beyond the near plane that is culled by its empty rectangle alone (radius 0, no tiles, rect 0, depth key all ones).
    assert n["radius_without_tiles"] == 0, "%d rows with radii > 0 and no tile" % n["radius_without_tiles"]
    assert n["empty_rect_culled"] >= 5, "%d rows beyond the near plane culled by an empty rectangle" % n["empty_rect_culled"]
    for k in range(8):
        assert n["clamp_%d" % k] >= 20, "clamp flags %d: %d visible rows" % (k, n["clamp_%d" % k])
    assert n["ill_conditioned_visible"] >= 30, "%d visible ill-conditioned rows" % n["ill_conditioned_visible"]
    assert n["cover_all"] >= 1, "no row touches every tile"
    radii = c.o.get("radii")
    zc = c.groups["zero_cov"]
    if c.s.kernel_size == 0.0:
        assert (radii[zc] == 0).all(), "zero covariance at kernel_size 0 is det == 0: culled"
    else:
        assert (radii[zc] > 0).all(), "zero covariance with a 2D filter is a visible splat"
    for g, v in (("opacity_0", 0.0), ("opacity_1", 1.0)):
        rows = c.groups[g]
        assert (radii[rows] > 0).sum() >= 10 and (c.s.opacities.numpy()[rows, 0] == v).all(), g


@pytest.mark.parametrize("name", pg.TAILS)
def test_tail_scene_has_a_visible_row_in_its_last_block(name):
    c = pg.get_case(name)
    assert c.counts["last_block_128_visible"] >= 1 and c.counts["last_block_256_visible"] >= 1, c.counts
    assert c.o.get("radii")[-1] > 0


def _host_state(c):
    f, i = hc.preprocess_fwd(c.s, colors=c.colors, cov3D=c.cov3D, scale_modifier=c.scale_modifier)
    P = c.P
    a, b = np.zeros((P, 16), np.float32), np.zeros((P, 12), np.float32)
    a[:, 0:6] = f[:, 0:6]; a[:, 7] = f[:, 6]; a[:, 8:11] = f[:, 7:10]; a[:, 11:13] = f[:, 10:12]; a[:, 13:16] = f[:, 12:15]
    b[:, 0:6] = f[:, 15:21]; b[:, 6:9] = f[:, 21:24]
    vis = i[:, 0] > 0
    depth_key = np.where(vis, pg.bits(f[:, 24]), np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return dict(splat_a=a, splat_b=b, clamped=i[:, 2].astype(np.uint8), rect=np.ascontiguousarray(f[:, 25]).view(np.uint32), depth_key=depth_key), i


@pytest.mark.parametrize("name", list(pg.BUILDERS))
def test_expected_state_equals_the_host_build(name):
    c = pg.get_case(name)
    want = pg.expected_state(c.o, c.s, c.colors)
    got, i = _host_state(c)
    radii = c.o.get("radii")
    vis = radii > 0
    every = np.ones(c.P, bool)
    assert vis.any()
    pg.assert_fields({"radii": (i[:, 0], radii), "tiles_touched": (i[:, 1].astype(np.uint32), c.o.get("tiles_touched")),
                      "rect": (got["rect"], want["rect"]), "depth_key": (got["depth_key"], want["depth_key"])}, every, c.cls, name + ": every row")
    pg.assert_fields({k: (got[k], want[k]) for k in ("splat_a", "splat_b", "clamped")}, vis, c.cls, name + ": visible rows")
    assert np.isfinite(want["splat_a"][vis]).all() and np.isfinite(want["splat_b"][vis]).all(), "a NaN's sign and payload are not the arithmetic's to keep"
    w, h = (want["rect"] >> 16) & 255, want["rect"] >> 24
    assert np.array_equal((w * h)[vis], c.o.get("tiles_touched")[vis])


def test_the_comparison_names_field_row_and_class():
    """the check must be able to fail: one flipped bit in one packed slot is found and reported"""
    c = pg.get_case("boundary_deg3_ks0_coord")
    want = pg.expected_state(c.o, c.s)
    vis = c.o.get("radii") > 0
    row = int(c.groups["edge_left"][0])
    assert vis[row]
    for field, col in (("splat_a", 12), ("splat_b", 8), ("rect", 0), ("clamped", 0), ("depth_key", 0)):
        bad = want[field].copy()
        v = pg._as_words(bad)
        v[row, col] ^= 1
        msg = pg.field_diff(field, v.reshape(pg._as_words(want[field]).shape), pg._as_words(want[field]), vis, c.cls)
        assert msg is not None and msg.startswith(field + ": 1 of") and "first row %d (class edge_left)" % row in msg, msg
        assert pg.field_diff(field, want[field], want[field], vis, c.cls) is None


@pytest.mark.parametrize("name", ["boundary_deg3_ks0_coord", "boundary_deg1_ks0.1_coord", "boundary_deg1_ks0_nocoord", "scale_modifier_0.7", "tail_P257"])
def test_oracle_sums_and_backward_through_the_host_build(name):
    """oracle_sums is gpu_util.reference_sums' record; the host build over it returns the oracle's gradients bit for bit on these scenes too
    (degenerate rows included), in both opacity modes: what the device is asked to reproduce."""
    c = pg.get_case(name)
    o, s, P = c.o, c.s, c.P
    radii = o.get("radii")
    clb = pg.clamp_bits(o, P)
    co = o.get("conic_opacity", (P, 4))
    every = np.ones(P, bool)
    for intended in (False, True):
        orc.set_opacity_slip(0 if intended else 1)
        try:
            gr = oracle_backward(o, upstream_grads(s, 3))
        finally:
            orc.set_opacity_slip(1)
        sums = pg.oracle_sums(o, P, s.require_coord)
        assert np.array_equal(pg.bits(sums), pg.bits(reference_sums(o.get, P, s.require_coord, raw_opacity="acc_dopacity")))
        assert np.abs(sums[radii > 0]).max() > 0 and not sums[~(radii > 0)].any()
        out, dsh = hc.preprocess_bwd(s, radii, clb, co[:, 3] if intended else sums[:, 14], pg.host_acc(sums), scale_modifier=c.scale_modifier)
        pairs = {k: (out[:, sl], gr[k].reshape(P, -1)) for k, sl in pg.GRAD_COLUMNS}
        pairs["dL_dsh"] = (dsh, gr["dL_dsh"])
        pg.assert_fields(pairs, every, c.cls, "%s, intended=%s: host build over the oracle's sums" % (name, intended))
        for k, v in gr.items():
            assert np.isfinite(v).all(), k


@pytest.mark.parametrize("coord", [False, True])
def test_arbitrary_sums_stay_finite_through_the_host_build(coord):
    c = pg.get_case("boundary_deg3_ks0_coord" if coord else "boundary_deg3_ks0_nocoord")
    sums = pg.arbitrary_sums(c, coord)
    radii = c.o.get("radii")
    assert (np.abs(sums) > 1e4).any() and (sums == 0).all(1).sum() > 100 and (np.signbit(sums) & (sums == 0)).any()
    for opc in (c.o.get("conic_opacity", (c.P, 4))[:, 3], sums[:, 14]):
        out, dsh = hc.preprocess_bwd(c.s, radii, pg.clamp_bits(c.o, c.P), opc, pg.host_acc(sums))
        assert np.isfinite(out).all() and np.isfinite(dsh).all()
        assert np.abs(out[radii > 0]).max() > 0


@pytest.mark.parametrize("rowf", [3, 12, 27, 48, 12 // 4, 48 // 4])
def test_slab_index_arithmetic(rowf):
    """The multiply-high division of the slab copies is exact over the whole slab, full or short, and the odd row stride keeps rows apart: every
    word of an [nrows][rowf] block lands on its own LDS word inside the block's 128 x (rowf + 1) words, at (e // rowf, e % rowf)."""
    for nrows in (1, 2, 63, 127, 128):
        e, pos, g, col = pg.slab_positions(nrows, rowf)
        assert np.array_equal(g, e // rowf) and np.array_equal(col, e % rowf)
        assert len(np.unique(pos)) == len(pos) and pos.max() < 128 * (rowf + 1) and g.max() == nrows - 1
    e, _, g, _ = pg.slab_positions(5, rowf, tail=False)     # the mutation: a copy that ignores the short last block walks past its rows
    assert g.max() == 127 and e.max() >= 5 * rowf
