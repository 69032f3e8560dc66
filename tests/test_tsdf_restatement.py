"""tests/tsdf_restatement.py checked against properties that do not depend on it: the GPU tier holds the kernels to the restatement bit
for bit, so a misreading shared by both would pass there.  A closed surface fused from depth maps must come out watertight, oriented
and on the sphere it came from.

Measured on the scene (ten views, voxel 0.01, sdf_trunc 0.08): 17 056 vertices, 34 108 faces, V - E + F = 2, volume 0.11336 against
4/3 pi r^3 = 0.11310, max | |v - c| - r | = 0.0037."""
import math

import numpy as np
import pytest

import tsdf_restatement as tr

SDF_TRUNC = 8 * tr.VOXEL


@pytest.fixture(scope="module")
def fused():
    return tr.fused_scene()


def test_roundf_is_half_away_from_zero():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999997, -0.49999997, 8388609.0, 0.0, -0.0, 2.4999998], np.float32)
    want = np.array([1, 2, 3, -1, -2, -3, 0, -0.0, 8388609, 0, -0.0, 2], np.float32)
    got = tr.roundf(x)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert not np.array_equal(np.rint(x), want)


def test_block_key_order_and_floor():
    c = np.array([[0, 0, 0], [-1, 0, 0], [5, -3, 2], [0, 0, -1], [-1, 0, 0], [(1 << 20) - 1, 0, 0], [-(1 << 20), 0, 0]])
    u = tr.unique_blocks(c)
    assert u.dtype == np.int32
    assert [tuple(r) for r in u.tolist()] == sorted({tuple(r) for r in c.tolist()}, key=lambda r: (r[2], r[1], r[0]))
    assert u.tolist()[0] == [0, 0, -1] and u.tolist()[1] == [-(1 << 20), 0, 0]
    with pytest.raises(ValueError):
        tr.block_key(np.array([[1 << 20, 0, 0]]))
    # a point just below zero lies in block -1, not 0
    K, E = tr.intrinsic(8, 8, 4.0), np.eye(4)
    E[:3, 3] = [-0.001, -0.001, 0.0]                      # the camera sits at (+0.001, +0.001, 0) and looks along +z
    depth = np.zeros((8, 8), np.float32)
    depth[4, 4] = 0.5                                     # the principal ray: x = y = 0.001 in the world
    depth[0, 0] = 0.5                                     # x = y = 0.001 - 0.5 < 0
    got = {tuple(r) for r in tr.touch(depth, K, E, tr.VOXEL).tolist()}
    assert (0, 0, 2) in got and (-3, -3, 2) in got and (-4, -4, 3) in got and all(r[0] in (0, -4, -3) for r in got)


def test_scene_covers_what_it_claims(fused):
    views = tr.scene_views()
    assert len(views) == 10 and all(v[0].shape == (tr.HEIGHT, tr.WIDTH) and v[1].shape == (tr.HEIGHT, tr.WIDTH, 3) for v in views)
    for depth, colour, K, E in views:
        assert (depth == 0).any() and (depth > 0).any() and depth.max() < 1.0 and depth[depth > 0].min() > 0.69
        assert colour.min() >= 0 and colour.max() <= 1
        assert 1.0 / K[0, 0] < tr.VOXEL                   # the pixel footprint at depth <= 1 is below the voxel
    coords = fused["grid"].coords()
    assert (coords.min(0) < 0).all() and (coords.max(0) > 0).all()      # blocks on both sides of the origin on every axis
    assert fused["grid"].weight.max() >= 3


def test_sphere_mesh_is_closed_and_oriented(fused):
    v, f, c = fused["mesh"]
    assert v.dtype == np.float32 and f.dtype == np.int64 and c.dtype == np.float32 and c.shape == v.shape
    assert len(v) > 10000 and len(f) > 20000
    rep = tr.mesh_report(v, f)
    assert rep["all_vertices_used"] and rep["no_collapsed_face"]
    assert rep["edges_in_two_faces"], "an undirected edge is not in exactly two faces"
    assert rep["directed_once"], "a directed edge occurs twice: two faces disagree on the orientation"
    assert rep["euler"] == 2
    assert rep["volume"] > 0
    assert abs(rep["volume"] - 4 / 3 * math.pi * tr.RADIUS ** 3) < 0.02 * rep["volume"]


def test_sphere_mesh_lies_on_the_sphere(fused):
    v, f, c = fused["mesh"]
    dev = np.abs(np.linalg.norm(v.astype(np.float64) - tr.CENTRE, axis=1) - tr.RADIUS)
    print("max | |v - c| - r | =", dev.max())
    assert dev.max() < SDF_TRUNC
    # the colours are the scene's smooth function of the position, averaged over a few views of neighbouring pixels
    assert np.abs(c - tr.hit_colour(v.astype(np.float64))).max() < 0.1


def test_mesh_crosses_block_borders_on_every_axis(fused):
    v, f, c = fused["mesh"]
    block = np.floor(v.astype(np.float64) / (16 * tr.VOXEL)).astype(np.int64)
    per_face = block[f]
    for axis in range(3):
        assert (per_face[:, :, axis].min(1) != per_face[:, :, axis].max(1)).any()
        assert (block[:, axis] < 0).any() and (block[:, axis] >= 0).any()


def test_vertex_and_face_order_is_canonical(fused):
    """vertices ascend by (block key, voxel, axis): recomputed here from the positions alone"""
    v, f, c = fused["mesh"]
    q = v.astype(np.float64) / tr.VOXEL
    axis = np.argmax(np.abs(q - np.round(q)) > 1e-4, axis=1)          # the one coordinate that is not a whole voxel (0 when all are)
    X = np.where(np.arange(3)[None] == axis[:, None], np.floor(q + 1e-6), np.round(q)).astype(np.int64)
    key = tr.block_key(X >> 4)
    vox = ((X[:, 2] & 15) * 16 + (X[:, 1] & 15)) * 16 + (X[:, 0] & 15)
    order = np.lexsort((vox, key))
    assert np.array_equal(key[order], key) and np.array_equal(vox[order], vox)


def test_integrate_leaves_unlisted_blocks_alone():
    g = tr.Grid(tr.VOXEL, True)
    views = tr.scene_views()
    d0, c0, K, E0 = views[0]
    tr.integrate(g, tr.touch(d0, K, E0, tr.VOXEL), d0, c0, K, E0)
    n0 = len(g.index)
    before = (g.tsdf.copy(), g.weight.copy(), g.color.copy())
    d1, c1, _, E1 = views[1]
    listed = tr.touch(d1, K, E1, tr.VOXEL)[::2]
    tr.integrate(g, listed, d1, c1, K, E1)
    named = {tuple(r) for r in listed.tolist()}
    keep = np.array([c not in named for c in list(g.index)[:n0]])           # the dict keeps insertion order: row i is its i-th key
    assert keep.any() and (~keep).any() and len(g.index) > n0
    for now, then in zip((g.tsdf, g.weight, g.color), before):
        assert np.array_equal(now[:n0][keep], then[keep])
    assert not np.array_equal(g.weight[:n0][~keep], before[1][~keep])


def test_weight_threshold_is_not_above(fused):
    """a corner whose weight equals the threshold makes its cells empty"""
    g = fused["grid"]
    at = tr.extract_grid(g, 2.0)
    below = tr.extract_grid(g, 2.0 - 2.0 ** -20)
    above = tr.extract_grid(g, 2.0 + 2.0 ** -20)
    assert len(at[1]) < len(below[1]) and len(at[1]) == len(above[1]) and np.array_equal(at[0], above[0])


def test_empty_inputs():
    v, f, c = tr.extract(np.zeros((0, 3), np.int64), np.zeros((0, 4096), np.float32), np.zeros((0, 4096), np.float32), None, tr.VOXEL)
    assert v.shape == (0, 3) and f.shape == (0, 3) and c is None
    assert tr.touch(np.zeros((70, 50), np.float32), tr.intrinsic(50, 70), np.eye(4), tr.VOXEL).shape == (0, 3)
