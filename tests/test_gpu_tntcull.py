"""GPU tier of the Tanks-and-Temples mesh culling: tnt_cull.py and the kernels of csrc/radegs_tntcull.hip against
tests/tntcull_restatement.py and the fixture the reference's own Mesher.point_masks wrote (tests/golden/make_golden_tntcull.py).

render_depth: the set of non-zero pixels is the restatement's and every depth has the restatement's BITS -- the kernel performs the same
float64 operations in the same order under -ffp-contract=off and rounds once, and bit equality is what was observed on an MI355X, so that
(and not the one-ulp bound the same reasoning allows) is asserted.  No pixel is left out of any comparison: the seeded scenes keep a
relative margin of 1e-12 on every coverage decision (tests/test_tntcull_restatement.py).  point_masks and cull_mesh: exact."""
import numpy as np
import pytest
import torch

import tntcull_cases as cs
import tntcull_restatement as tc
from test_tntcull_restatement import fixture_inputs, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = sorted(cs.SIZES)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def same_bits(got, want):
    return got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def render(v, f, size, znear=cs.ZNEAR, zfar=cs.ZFAR, c2w=None, **kw):
    import tnt_cull as tcu
    H, W = size
    return host(tcu.render_depth(dev(v), dev(f), cs.views() if c2w is None else c2w, H, W, *cs.SIZES[size], znear=znear, zfar=zfar, **kw))


def check(key, tris, size, znear=cs.ZNEAR, zfar=cs.ZFAR):
    """one case: bit-equal to the restatement (hence the same non-zero set); returns the map"""
    v, f = cs.mesh_of(tris)
    want, _ = cs.restated(key, v, f, size, znear, zfar)
    got = render(v, f, size, znear, zfar)
    assert np.array_equal(got > 0, want > 0), (key, int(((got > 0) != (want > 0)).sum()))
    assert same_bits(got, want), (key, float(np.abs(got.astype(np.float64) - want).max()))
    return got


@pytest.fixture(scope="module")
def masks_fx():
    return load("tntcull_point_masks.npz")


# ----------------------------------------------------------------------------- render -----------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_a_triangle_over_the_whole_image_takes_the_queue(size, monkeypatch):
    import tnt_cull as tcu
    got = check(("full", size), cs.full_screen(size), size)
    assert (got[0] > 0).all() and got.dtype == np.float32 and not got[2].any()      # the third view looks away
    v, f = cs.mesh_of(cs.full_screen(size))
    stats = torch.zeros(4, dtype=torch.int64, device=DEV)
    tcu._render(dev(v), dev(f), tc.world_to_camera(cs.views()), *size, cs.SIZES[size], cs.ZNEAR, cs.ZFAR, stats=stats)
    chunks, small, queued, overflow = stats.tolist()
    assert queued >= 1 and overflow == 0 and chunks >= -(-size[0] * size[1] // 1024)
    # a queue too short for the chunks: the set-up kernel draws what does not fit, and the map is the same
    for entries in (0, 1):
        monkeypatch.setattr(tcu, "QUEUE_ENTRIES", entries)
        tcu._render(dev(v), dev(f), tc.world_to_camera(cs.views()), *size, cs.SIZES[size], cs.ZNEAR, cs.ZFAR, stats=stats)
        assert stats[3].item() == chunks - entries
        assert same_bits(render(v, f, size), got)


@pytest.mark.parametrize("size", SIZES)
def test_box_sizes_either_side_of_the_in_place_threshold(size):
    """boxes of 1 x 1 to 40 x 40 pixel centres (cut by the image where it is smaller): 16 x 16 = 256 is the last one walked in place"""
    import tnt_cull as tcu
    for n in list(range(1, 19)) + [24, 31, 32, 33, 40]:
        tri = cs.right_triangle(n, size)
        got = check(("box", size, n), tri, size)
        assert (got[0] > 0).any() and not got[2].any()
        if n in (16, 17):
            v, f = cs.mesh_of(tri)
            stats = torch.zeros(4, dtype=torch.int64, device=DEV)
            tcu._render(dev(v), dev(f), tc.world_to_camera(cs.views()[:1]), *size, cs.SIZES[size], cs.ZNEAR, cs.ZFAR, stats=stats)
            assert stats.tolist()[1:3] == ([1, 0] if n == 16 else [0, 1])


@pytest.mark.parametrize("size", SIZES)
def test_triangles_that_cover_nothing_leave_zeros(size):
    far_behind = cs.at_depths(size, [-3.0, -2.0, -4.0])
    for key, tri in (("sliver", cs.sliver(size)), ("behind", far_behind), ("near", cs.at_depths(size, [0.2, 0.3, 0.4])),
                     ("beyond", cs.at_depths(size, [21.0, 25.0, 30.0]))):
        assert not check((key, size), tri, size)[0].any(), key     # in the view the case is built in; the other two match the restatement
    flat = cs.at_depths(size, [2.0, 2.0, 2.0])
    assert not check(("zero area", size), np.stack([flat[[0, 0, 1]], flat[[0, 1, 1]], flat[[2, 2, 2]]]), size).any()
    middle = (flat[0] + 0.5 * (flat[1] - flat[0])).astype(np.float32).astype(np.float64)
    check(("collinear", size), np.stack([flat[0], middle, flat[1]])[None], size)       # collinear up to rounding: whatever it covers, both agree


@pytest.mark.parametrize("size", SIZES)
def test_triangles_across_the_planes(size):
    one = check(("straddle near, one behind", size), cs.at_depths(size, [2.0, 0.1, 3.0]), size)
    two = check(("straddle near, two behind", size), cs.at_depths(size, [0.2, 3.0, -1.0]), size)
    far = check(("straddle far", size), cs.at_depths(size, [15.0, 30.0, 18.0]), size)
    for m in (one, two, far):
        assert (m[0] > 0).any() and m[0][m[0] > 0].min() >= np.float32(cs.ZNEAR) and m[0].max() <= np.float32(cs.ZFAR)
    whole = render(*cs.mesh_of(cs.at_depths(size, [15.0, 30.0, 18.0])), size, zfar=40.0)
    assert (whole[0] > 0).sum() > (far[0] > 0).sum()           # there is no geometric far clip: fragments beyond zfar are dropped one by one


def test_two_sheets_with_shared_edges_have_no_hole():
    size = (48, 64)
    for seed, flip in ((11, False), (12, True)):
        v, f, loop = cs.jittered_grid(size, seed, flip_some=flip)
        want, _ = cs.restated(("grid", seed), v, f, size)
        got = render(v, f, size)
        assert same_bits(got, want)
        for b, w2c in enumerate(tc.world_to_camera(cs.views()[:2])):
            inside = cs.strictly_inside(v, loop, size, w2c)
            assert inside.sum() > 300 and (got[b][inside] > 0).all()


@pytest.mark.parametrize("size", SIZES)
def test_the_soup_matches_in_any_face_order_and_twice(size):
    v, f, want, margin = cs.soup_reference(size)
    assert margin > 1e-12
    got = render(v, f, size)
    assert np.array_equal(got > 0, want > 0)
    assert same_bits(got, want), float(np.abs(got.astype(np.float64) - want).max())
    perm = np.random.default_rng(1).permutation(len(f))
    assert same_bits(render(v, f[perm], size), got)
    assert same_bits(render(v, f, size), got)
    assert same_bits(render(v.astype(np.float32), f.astype(np.int32), size), got)          # float32 vertices and int32 faces are converted exactly


def test_pose_switch_and_empty_inputs():
    size = (21, 33)
    v, f = cs.mesh_of(cs.right_triangle(9, size))
    gl = render(v, f, size)
    assert same_bits(render(v, f, size, c2w=tc.to_opencv(cs.views()), pose="opencv"), gl) and gl[0].any()
    assert not render(v, f[:0], size).any() and render(v, f, size, c2w=np.zeros((0, 4, 4))).shape == (0, 21, 33)
    assert render(v, f, size, c2w=[m for m in cs.views()[:1]]).shape == (1, 21, 33)


# ------------------------------------------------------------------------ vertex visibility ------------------------------------------------------------------------
def test_point_masks_reproduce_the_reference_written_fixture(masks_fx):
    import tnt_cull as tcu
    fx = masks_fx
    p, d, c2w, *K = fixture_inputs(fx)
    mask, counts = tcu.point_masks(dev(p), dev(d), c2w, *K, eps=float(fx["eps"]), min_views=int(fx["min_views"]))
    assert mask.dtype == torch.bool and counts.dtype == torch.int32
    assert np.array_equal(host(counts), fx["counts"]) and np.array_equal(host(mask), fx["mask"])
    n = int(fx["n_hand"])                                      # the dyadic cases on their thresholds, one camera
    _, one = tcu.point_masks(dev(p[:n]), dev(d[:1]), c2w[:1], *K)
    assert np.array_equal(host(one).astype(bool), fx["seen_camera0"][:n]), dict(zip(fx["hand_names"].tolist(), host(one).tolist()))
    _, c64 = tcu.point_masks(dev(p.astype(np.float64)), dev(d), [torch.from_numpy(m) for m in c2w], *K)
    assert np.array_equal(host(c64), fx["counts"])


def test_point_masks_sizes_batches_and_min_views(masks_fx):
    import tnt_cull as tcu
    fx = masks_fx
    p, d, c2w, *K = fixture_inputs(fx)
    for n in (1, 0):
        mask, counts = tcu.point_masks(dev(p[5:5 + n]), dev(d), c2w, *K)
        assert np.array_equal(host(counts), fx["counts"][5:5 + n]) and np.array_equal(host(mask), fx["mask"][5:5 + n])
    total = torch.zeros(len(p), dtype=torch.int32, device=DEV)
    for b in range(0, 24, 7):                                  # 7 + 7 + 7 + 3 views
        total += tcu.point_masks(dev(p), dev(d[b:b + 7]), c2w[b:b + 7], *K)[1]
    assert np.array_equal(host(total), fx["counts"])
    i = int(np.flatnonzero(fx["counts"] == 20)[0])
    for m, want in ((19, True), (20, True), (21, False)):
        assert host(tcu.point_masks(dev(p), dev(d), c2w, *K, min_views=m)[0])[i] == want
    mask0, counts0 = tcu.point_masks(dev(p), dev(d[:0]), c2w[:0], *K, min_views=0)
    assert not counts0.any() and mask0.all()
    for bad, what in ((dev(d).double(), "float32 tensor of shape"), (dev(d[0]), "float32 tensor of shape"), (dev(d[:5]), "5 maps for 24 poses")):
        with pytest.raises(RuntimeError, match=what):
            tcu.point_masks(dev(p), bad, c2w, *K)
    nan = p.copy()
    nan[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="non-finite"):
        tcu.point_masks(dev(nan), dev(d), c2w, *K)


# ------------------------------------------------------------------------- the whole step -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box():
    v, f, names = cs.box_scene()
    c2w = cs.ring_cameras()
    want = {pose: tc.cull_mesh(v, f, c2w, *cs.CULL_SIZE, *cs.CULL_K, eps=0.1, pose=pose) for pose in ("opengl", "opencv")}
    return v, f, names, c2w, want


def cull(v, f, c2w, **kw):
    import tnt_cull as tcu
    H, W = cs.CULL_SIZE
    fx, fy, cx, cy = cs.CULL_K
    out_v, out_f = tcu.cull_mesh(dev(v), dev(f), c2w, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, eps=0.1, **kw)
    assert out_f.dtype == torch.int64
    return host(out_v), host(out_f)


@pytest.mark.parametrize("pose", ["opengl", "opencv"])
def test_cull_mesh_keeps_what_the_restatement_keeps(box, pose):
    v, f, names, c2w, want = box
    kept_v, kept_f, counts = want[pose]
    got_v, got_f = cull(v, f, c2w, pose=pose)
    assert got_v.dtype == np.float32 and np.array_equal(got_v, kept_v) and np.array_equal(got_f, kept_f)
    if pose == "opencv":                                       # render and vertex test agree on the camera: the culling the method intends
        assert 0 < len(got_v) < len(v) and counts[names["hidden"]].max() == 0 and 0 < counts[names["floating"]].max() < 20
    else:                                                      # upstream's executed call on OpenCV poses renders the view behind each camera
        assert counts[names["hidden"]].min() == 24 and len(got_v) >= names["hidden"].stop
    for batch in (1, 5, 24):
        bv, bf = cull(v, f, c2w, pose=pose, view_batch=batch)
        assert np.array_equal(bv, got_v) and np.array_equal(bf, got_f)
    v64, f64 = cull(v.astype(np.float64), f, c2w, pose=pose)
    assert v64.dtype == np.float64 and np.array_equal(v64, kept_v.astype(np.float64)) and np.array_equal(f64, kept_f)


def test_cull_mesh_empty_inputs_and_refusals(box):
    import tnt_cull as tcu
    v, f, names, c2w, _ = box
    ev, ef = cull(v, f[:0], c2w, pose="opencv")
    assert ef.shape == (0, 3) and ev.shape[1] == 3
    zv, zf = cull(v[:0], f[:0], c2w)
    assert zv.shape == (0, 3) and zf.shape == (0, 3)
    nv, nf = cull(v, f, c2w[:0], min_views=0)                  # no camera: nothing is seen, and nothing need be
    assert np.array_equal(nv, v) and np.array_equal(nf, f)
    bad_v = v.copy()
    bad_v[7, 2] = np.inf
    bad_f = f.copy()
    bad_f[3, 1] = len(v)
    for call, what in ((lambda: cull(bad_v, f, c2w), "non-finite"), (lambda: cull(v, bad_f, c2w), "outside the"),
                       (lambda: cull(v, -bad_f, c2w), "outside the"), (lambda: cull(v[:, :2], f, c2w), r"shape \(N,3\)"),
                       (lambda: tcu.cull_mesh(dev(v).half(), dev(f), c2w), "float32 or float64"),
                       (lambda: tcu.cull_mesh(dev(v), dev(f).float(), c2w), "`faces` must be"),
                       (lambda: tcu.cull_mesh(dev(v), torch.from_numpy(f), c2w), "no CPU implementation"),
                       (lambda: tcu.render_depth(dev(v), dev(bad_f), c2w, 48, 64, *cs.CULL_K), "outside the"),
                       (lambda: tcu.render_depth(dev(bad_v), dev(f), c2w, 48, 64, *cs.CULL_K), "non-finite")):
        with pytest.raises(RuntimeError, match=what):
            call()
