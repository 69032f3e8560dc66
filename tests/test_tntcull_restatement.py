"""CPU tier of the Tanks-and-Temples mesh culling: tests/tntcull_restatement.py against the fixture the reference's own
Mesher.point_masks wrote (tests/golden/make_golden_tntcull.py), its rasterizer against hand-computed maps, and the margins of the seeded
scenes the GPU tier compares exactly."""
import os

import numpy as np
import pytest

import tntcull_cases as cs
import tntcull_restatement as tc

HERE = os.path.dirname(os.path.abspath(__file__))
IDENTITY = np.eye(4)[None]            # an OpenGL camera at the origin looking down -z


def load(name):
    with np.load(os.path.join(HERE, "golden", name)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def masks_fx():
    return load("tntcull_point_masks.npz")


def fixture_inputs(fx):
    return fx["points"], fx["depths"], fx["c2w"].astype(np.float64), *[float(v) for v in fx["intrinsics"]]


# ------------------------------------------------------------------------ vertex visibility ------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_written_fixture(masks_fx):
    fx = masks_fx
    assert fx["depths"].shape == (24, 29, 37) and fx["points"].dtype == np.float32 and 300 < len(fx["points"]) < 600
    mask, counts = tc.point_masks(*fixture_inputs(fx), float(fx["eps"]), int(fx["min_views"]))
    assert np.array_equal(counts, fx["counts"]) and np.array_equal(mask, fx["mask"])
    assert mask.any() and not mask.all() and (counts == 20).any() and (counts == 19).any()


def test_restatement_decides_the_hand_built_threshold_cases_as_the_reference(masks_fx):
    fx = masks_fx
    n = int(fx["n_hand"])
    p, d, c2w, *K = fixture_inputs(fx)
    seen = tc.seen_by(p[:n], d[0], tc.world_to_camera(c2w[:1])[0].astype(np.float32), *K, float(fx["eps"]))
    got = dict(zip([str(s) for s in fx["hand_names"]], seen.tolist()))
    assert np.array_equal(seen, fx["seen_camera0"][:n]), got
    assert got == {"u == 0": True, "u == W - 1": True, "v == 0": True, "v == H - 1": True, "u one float32 below 0": False, "z == depth + eps": False,
                   "z one float32 below depth + eps": True, "depth_sample == 0": True}


# ----------------------------------------------------------------------------- render -----------------------------------------------------------------------------
SQUARE = np.array([[-1.5, 1.5, -2.0], [1.0, 1.5, -2.0], [1.0, -1.0, -2.0], [-1.5, -1.0, -2.0]])     # window (1,1) .. (6,6) of an 8 x 8 image
K8 = (4.0, 4.0, 4.0, 4.0)


def square_map(value=2.0):
    want = np.zeros((8, 8), np.float32)
    want[1:6, 1:6] = value
    return want


def test_square_of_two_triangles_has_no_hole_on_its_diagonal_and_the_exact_depth():
    faces = np.array([[0, 1, 2], [0, 2, 3]])                       # the diagonal (1,1)-(6,6) passes through five pixel centres
    depth, _ = tc.render_depth(SQUARE, faces, IDENTITY, 8, 8, *K8, 0.5, 20.0)
    assert depth.dtype == np.float32 and np.array_equal(depth[0], square_map())
    other = np.array([[0, 1, 3], [1, 2, 3]])                       # the other diagonal, (6,1)-(1,6), does too
    assert np.array_equal(tc.render_depth(SQUARE, other, IDENTITY, 8, 8, *K8, 0.5, 20.0)[0][0], square_map())


def test_a_triangle_facing_away_gives_the_same_map():
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    a = tc.render_depth(SQUARE, faces, IDENTITY, 8, 8, *K8, 0.5, 20.0)[0]
    b = tc.render_depth(SQUARE, faces[:, ::-1], IDENTITY, 8, 8, *K8, 0.5, 20.0)[0]
    mixed = tc.render_depth(SQUARE, np.array([[0, 1, 2], [3, 2, 0]]), IDENTITY, 8, 8, *K8, 0.5, 20.0)[0]
    assert np.array_equal(a, b) and np.array_equal(a, mixed) and (a > 0).sum() == 25


def test_a_nearer_triangle_occludes_a_farther_one():
    wall = np.array([[-4.0, 4.0, -4.0], [4.0, 4.0, -4.0], [4.0, -4.0, -4.0], [-4.0, -4.0, -4.0]])  # window (0,0) .. (8,8) at depth 4
    v = np.concatenate([wall, SQUARE])
    f = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])
    want = np.full((8, 8), 4.0, np.float32)
    want[1:6, 1:6] = 2.0
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        assert np.array_equal(tc.render_depth(v, f[order], IDENTITY, 8, 8, *K8, 0.5, 20.0)[0][0], want)
    assert np.array_equal(tc.render_depth(v, f, IDENTITY, 8, 8, *K8, 0.5, 3.0)[0][0], square_map())            # the wall lies beyond zfar
    assert not tc.render_depth(v, f, IDENTITY, 8, 8, *K8, 5.0, 20.0)[0].any()                                  # both nearer than znear


def test_a_near_clipped_triangle_gives_the_map_of_the_hand_clipped_quad():
    K16 = (8.0, 8.0, 8.0, 8.0)
    A, B, C = [-1.0, -1.0, -3.0], [1.0, -1.0, -3.0], [0.0, 1.0, 1.0]               # C is behind the camera; znear = 1 cuts AC and BC at t = 1/2
    I12, I20 = [0.5, 0.0, -1.0], [-0.5, 0.0, -1.0]
    clipped = tc.clip_near(tc.camera_space(np.array([A, B, C]), np.eye(4)), 1.0)
    assert np.array_equal(np.array(clipped), np.array([[-1, -1, 3], [1, -1, 3], [0.5, 0, 1], [-0.5, 0, 1]], np.float64))
    got = tc.render_depth(np.array([A, B, C]), np.array([[0, 1, 2]]), IDENTITY, 16, 16, *K16, 1.0, 20.0)[0]
    quad = tc.render_depth(np.array([A, B, I12, I20]), np.array([[0, 1, 2], [0, 2, 3]]), IDENTITY, 16, 16, *K16, 1.0, 20.0)[0]
    assert np.array_equal(got, quad) and (got > 0).sum() > 10 and got[got > 0].min() >= 1.0
    # two vertices behind: the same plane, the triangle that is left
    D = [0.5, 1.0, 1.0]
    two = tc.render_depth(np.array([A, C, D]), np.array([[0, 1, 2]]), IDENTITY, 16, 16, *K16, 1.0, 20.0)[0]
    left = tc.clip_near(tc.camera_space(np.array([A, C, D]), np.eye(4)), 1.0)
    assert len(left) == 3 and (two > 0).any()
    hand = tc.render_depth(np.array(left) * [1, 1, -1], np.array([[0, 1, 2]]), IDENTITY, 16, 16, *K16, 1.0, 20.0)[0]
    assert np.array_equal(two, hand)


def test_the_meeting_point_does_not_depend_on_the_direction_of_the_edge():
    rng = np.random.default_rng(3)
    for _ in range(50):
        a, b = rng.standard_normal(3), rng.standard_normal(3)
        a[2], b[2] = 0.1 + abs(a[2]), 0.9 - abs(b[2]) * 2
        assert np.array_equal(tc.meet(a, b, 0.5), tc.meet(b, a, 0.5))


def test_permuting_the_faces_changes_nothing():
    size = (21, 33)
    v, f, depth, _ = cs.soup_reference(size)
    perm = np.random.default_rng(5).permutation(300)
    a = tc.render_depth(v, f[:300], cs.views(), *size, *cs.SIZES[size], cs.ZNEAR, cs.ZFAR)[0]
    b = tc.render_depth(v, f[:300][perm], cs.views(), *size, *cs.SIZES[size], cs.ZNEAR, cs.ZFAR)[0]
    assert np.array_equal(a, b) and (a > 0).any() and not (a > 0).all()


@pytest.mark.parametrize("size", sorted(cs.SIZES))
def test_the_seeded_soups_keep_their_margin(size):
    """the GPU tier compares these scenes pixel for pixel and leaves none out: no coverage decision may be near a tie"""
    v, f, depth, margin = cs.soup_reference(size)
    print("smallest relative edge-function margin", margin)
    assert margin > 1e-12
    assert len(f) == 2000 and (depth[0] > 0).sum() > 0.5 * depth[0].size
    cam = tc.camera_space(v, tc.world_to_camera(cs.views()[:1])[0])[:, 2][f]
    straddle_near = ((cam < cs.ZNEAR).any(1) & (cam >= cs.ZNEAR).any(1)).sum()
    straddle_far = ((cam > cs.ZFAR).any(1) & (cam <= cs.ZFAR).any(1)).sum()
    assert straddle_near > 20 and straddle_far > 20 and (cam < cs.ZNEAR).all(1).sum() > 20 and (cam > cs.ZFAR).all(1).sum() > 20


def test_shared_edges_leave_no_hole():
    size = (48, 64)
    for seed, flip in ((11, False), (12, True)):
        v, f, loop = cs.jittered_grid(size, seed, flip_some=flip)
        depth, _ = cs.restated(("grid", seed), v, f, size)
        for b, w2c in enumerate(tc.world_to_camera(cs.views()[:2])):
            inside = cs.strictly_inside(v, loop, size, w2c)
            assert inside.sum() > 300 and (depth[b][inside] > 0).all()
        assert not depth[2].any()


def test_the_whole_step_on_the_box_scene():
    v, f, names = cs.box_scene()
    kept_v, kept_f, counts = tc.cull_mesh(v, f, cs.ring_cameras(), *cs.CULL_SIZE, *cs.CULL_K, eps=0.1, pose="opencv")
    assert counts[names["hidden"]].max() == 0 and 0 < counts[names["floating"]].max() < 20 and counts[names["box"]].max() == 24
    assert 0 < len(kept_v) < len(v) and 0 < len(kept_f) < len(f) and kept_f.max() == len(kept_v) - 1
    assert np.array_equal(kept_v[kept_f], v[f[(counts >= 20)[f].all(1)]])
