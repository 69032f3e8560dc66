"""GPU tier of TSDF fusion: tsdf.py and the kernels of csrc/radegs_tsdf.hip against tests/tsdf_restatement.py, bit for bit --
block lists, weights, tsdf, colours, vertices, faces.  Every float32 operation of the specification (include/radegs.h, "TSDF fusion") is
an IEEE add, multiply, divide, floor or round in a fixed order, correctly rounded on both sides, so no step needs a tolerance; none is
given.  The closedness, orientation and Euler checks of tests/test_tsdf_restatement.py run on the GPU's own mesh as well."""
import copy
import math

import numpy as np
import pytest
import torch

import tsdf_restatement as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DMAX, THRESHOLD = tr.SCENE_DEPTH_MAX, tr.SCENE_WEIGHT_THRESHOLD


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def new_grid(voxel=tr.VOXEL, block_count=50000, with_color=True):
    import tsdf
    return tsdf.VoxelBlockGrid(voxel_size=voxel, block_resolution=16, block_count=block_count, with_color=with_color, device=DEV)


def grid_arrays(g):
    """(coords, tsdf, weight, color) of a device grid in key order, on the host"""
    if g.n == 0:
        return np.zeros((0, 3), np.int32), np.zeros((0, 4096), np.float32), np.zeros((0, 4096), np.float32), (np.zeros((0, 4096, 3), np.float32) if g.with_color else None)
    s = g.slots.long()
    assert sorted(host(s).tolist()) == list(range(g.n)) and g.capacity >= g.n
    keys = host(g.keys)
    assert (np.diff(keys) > 0).all()
    return host(g.block_coordinates()), host(g.tsdf[s]), host(g.weight[s]), (host(g.color[s]) if g.with_color else None)


def assert_grid_equals(g, ref):
    """a device grid against a restatement Grid, block by block"""
    c, t, w, col = grid_arrays(g)
    rc, rt, rw, rcol = ref.sorted_arrays()
    assert np.array_equal(c, rc)
    assert np.array_equal(w, rw), "weights differ"
    assert same_bits(t, rt), f"tsdf differs in {(t.view(np.uint32) != rt.view(np.uint32)).sum()} voxels"
    if ref.with_color:
        assert same_bits(col, rcol), f"colour differs in {(col.view(np.uint32) != rcol.view(np.uint32)).sum()} values"
    else:
        assert col is None


def assert_mesh_equals(mesh, ref):
    v, f, c = (host(m) for m in mesh)
    rv, rf, rc = ref
    assert v.dtype == np.float32 and f.dtype == np.int64 and v.shape == rv.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    assert np.array_equal(f, rf), "faces differ"
    assert same_bits(v, rv), "vertices differ"
    if rc is None:
        assert c is None
    else:
        assert same_bits(c, rc), "colours differ"


def fuse_on_device(g, views, depth_max=DMAX, lists=None, colour=True):
    out = []
    for i, (depth, col, K, E) in enumerate(views):
        d = dev(depth)
        blocks = g.compute_unique_block_coordinates(d, K, E, depth_max=depth_max) if lists is None else dev(lists[i])
        out.append(host(blocks))
        g.integrate(blocks, d, dev(col) if colour else None, K, E, depth_max=depth_max)
    return out


def install_blocks(g, coords, tsdf_rows, weight_rows, color_rows=None):
    """blocks with given contents: inserted through integrate() with an empty depth map (nothing is fused), then written in key order"""
    K, E = tr.intrinsic(8, 8, 4.0), np.eye(4)
    g.integrate(dev(np.asarray(coords, np.int32)), torch.zeros((8, 8), device=DEV), torch.zeros((8, 8, 3), device=DEV) if g.with_color else None, K, E)
    order = np.argsort(tr.block_key(coords))
    assert np.array_equal(host(g.block_coordinates()), np.asarray(coords, np.int32)[order])
    assert float(g.weight[:g.n].abs().max()) == 0.0 and float(g.tsdf[:g.n].abs().max()) == 0.0
    s = g.slots.long()
    g.tsdf[s] = dev(np.asarray(tsdf_rows, np.float32)[order])
    g.weight[s] = dev(np.asarray(weight_rows, np.float32)[order])
    if g.with_color:
        g.color[s] = dev(np.asarray(color_rows, np.float32)[order])


@pytest.fixture(scope="module")
def ref():
    return tr.fused_scene()


@pytest.fixture(scope="module")
def fused(ref):
    """the scene fused on the device with the default capacity: dict(grid, lists, mesh)"""
    g = new_grid()
    lists = fuse_on_device(g, tr.scene_views())
    return dict(grid=g, lists=lists, mesh=g.extract_triangle_mesh(THRESHOLD))


# --------------------------------------------------------------------------- touch ---------------------------------------------------------------------------
def touch_both(depth, K, E, voxel=tr.VOXEL, **kw):
    got = new_grid(voxel).compute_unique_block_coordinates(dev(depth), K, E, **kw)
    assert got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 3 and got.device == torch.device(DEV)
    want = tr.touch(depth, K, E, voxel, **kw)
    assert np.array_equal(host(got), want), (got.shape, want.shape)
    return want


def test_touch_image_not_a_multiple_of_four():
    K = tr.intrinsic(50, 70, 60.0)
    E = tr.look_at(tr.CENTRE + np.array([0.5, 0.7, 0.3]))
    depth, _ = tr.render_sphere(E, K, 50, 70)
    assert depth.shape == (70, 50)
    want = touch_both(depth, K, E)
    assert len(want) > 20 and (want < 0).any()
    # the last sampled row and column are 64 and 44; what lies beyond them must not matter
    depth2 = depth.copy()
    depth2[68:, :] = 0.123
    depth2[:, 48:] = 0.123
    assert np.array_equal(touch_both(depth2, K, E), want)


def test_touch_ray_start_clamps_at_zero():
    rng = np.random.default_rng(11)
    depth = rng.uniform(0.005, 0.3, (40, 56)).astype(np.float32)       # sdf_trunc is 0.08: many samples start in front of the camera
    depth[::8, ::8] = 0.079999
    K = tr.intrinsic(56, 40, 30.0)
    E = tr.look_at(np.array([0.31, -0.2, 0.05]), target=np.array([0.0, 0.0, 0.0]))
    assert (depth[::4, ::4] < 0.08).sum() > 20
    touch_both(depth, K, E)
    depth, _, K, E = tr.close_view()                                   # the scene's own near view: every sample is closer than sdf_trunc
    assert 0 < depth.max() < 0.08
    assert len(touch_both(depth, K, E, depth_max=DMAX)) > 3


def test_touch_samples_at_and_beyond_depth_max():
    rng = np.random.default_rng(12)
    depth = rng.uniform(0.8, 3.2, (44, 60)).astype(np.float32)
    depth[::8, ::4] = 2.0                                              # depth / depth_scale == depth_max exactly: not a sample
    depth[4::8, ::4] = np.float32(2.0) - np.float32(2.0 ** -22)        # the last value below it: one
    depth[0, 0], depth[0, 4], depth[0, 8] = np.inf, np.nan, -1.0
    K = tr.intrinsic(60, 44, 50.0)
    E = tr.look_at(np.array([-0.4, 0.1, 0.6]), target=np.array([0.2, 0.0, -0.1]))
    want = touch_both(depth, K, E, depth_scale=2.0, depth_max=1.0)
    assert len(want) > 20
    only_far = np.where(depth / np.float32(2.0) >= 1.0, depth, 0).astype(np.float32)
    assert touch_both(only_far, K, E, depth_scale=2.0, depth_max=1.0).shape == (0, 3)


def test_touch_of_an_empty_depth_map():
    got = new_grid().compute_unique_block_coordinates(torch.zeros((96, 128), device=DEV), tr.intrinsic(), np.eye(4))
    assert tuple(got.shape) == (0, 3) and got.dtype == torch.int32
    tiny = new_grid().compute_unique_block_coordinates(torch.ones((3, 3), device=DEV), tr.intrinsic(3, 3, 2.0), np.eye(4))      # no sampled pixel at all
    assert tuple(tiny.shape) == (0, 3)


def test_touch_matches_the_scene_lists(fused, ref):
    assert len(fused["lists"]) == len(ref["lists"]) == 10
    for got, want in zip(fused["lists"], ref["lists"]):
        assert np.array_equal(got, want)


# --------------------------------------------------------------------------- unique ---------------------------------------------------------------------------
def unique_both(coords):
    import tsdf
    got = tsdf.unique_block_coordinates(dev(coords.astype(np.int32)))
    assert got.dtype == torch.int32
    assert np.array_equal(host(got), tr.unique_blocks(coords))
    return host(got)


def test_unique_heavy_duplication_and_negative_values():
    rng = np.random.default_rng(21)
    few = rng.integers(-3, 3, (37, 3))
    coords = few[rng.integers(0, 37, 50000)]
    assert len(unique_both(coords)) <= 37
    assert len(unique_both(np.repeat(np.array([[-7, 5, -2]]), 1000, 0))) == 1
    assert unique_both(np.zeros((0, 3), np.int64)).shape == (0, 3)
    lim = 1 << 20
    unique_both(np.array([[lim - 1, lim - 1, lim - 1], [-lim, -lim, -lim], [0, 0, 0], [-1, -1, -1], [lim - 1, -lim, 0], [-lim, -lim, -lim]]))


def test_unique_keys_that_differ_only_in_the_upper_word():
    """x and the low 11 bits of y make up the key's lower 32 bits: blocks that differ in z, or in y by a multiple of 2048, share them"""
    coords = np.array([[5, 3, 9], [5, 3, -9], [5, 3 + 2048, 9], [5, 3 - 4096, 9], [5, 3, 10], [5, 3, 9], [6, 3, 9], [5, 3, -9]])
    keys = tr.block_key(coords)
    assert len({int(k) & 0xFFFFFFFF for k in keys[:5]}) == 1 and len({int(k) >> 32 for k in keys[:5]}) == 5
    got = unique_both(coords)
    assert len(got) == 6
    rng = np.random.default_rng(22)
    many = np.stack([np.full(4000, 5), 3 + 2048 * rng.integers(-500, 500, 4000), rng.integers(-1000, 1000, 4000)], 1)
    unique_both(many)


def test_unique_more_than_65536_distinct_keys():
    rng = np.random.default_rng(23)
    coords = rng.integers(-40, 41, (200000, 3))
    got = unique_both(coords)
    assert len(got) > 1 << 16


def test_coordinate_out_of_range_raises():
    import tsdf
    lim = 1 << 20
    for bad in ([lim, 0, 0], [0, -lim - 1, 0], [0, 0, 2 ** 31 - 1]):
        with pytest.raises(RuntimeError, match="outside"):
            tsdf.unique_block_coordinates(dev(np.array([[0, 0, 0], bad, [1, 1, 1]], np.int32)))
    g = new_grid(block_count=4)
    views = tr.scene_views()
    depth, colour, K, E = views[0]
    g.integrate(dev(tr.touch(depth, K, E, tr.VOXEL)[:3]), dev(depth), dev(colour), K, E)
    before = grid_arrays(g)
    with pytest.raises(RuntimeError, match="outside"):
        g.integrate(dev(np.array([[0, 0, 0], [lim, 0, 0]], np.int32)), dev(depth), dev(colour), K, E)
    after = grid_arrays(g)
    assert all(same_bits(a, b) for a, b in zip(before, after))
    # a voxel so small that the scene's blocks leave the 21 bits: touch raises, it does not wrap
    with pytest.raises(RuntimeError, match="outside"):
        new_grid(voxel=1e-9).compute_unique_block_coordinates(dev(depth), K, E)
    with pytest.raises(ValueError):
        tr.touch(depth, K, E, 1e-9)


# -------------------------------------------------------------------------- integrate --------------------------------------------------------------------------
def test_integrate_all_views(fused, ref):
    assert_grid_equals(fused["grid"], ref["grid"])
    assert fused["grid"].n == len(ref["grid"].index) > 100 and ref["grid"].weight.max() >= 3


def test_integrate_view_inside_the_band(ref):
    """a close camera, handed every block of the grid: some lie behind it (p.z <= 0), and the image cuts others on all four sides"""
    depth, colour, K, E = tr.close_view()
    r = copy.deepcopy(ref["grid"])
    blocks = r.coords()
    X = (16 * blocks.astype(np.int64)[:, None, :] + tr.VOXEL_OFFSETS[None]).reshape(-1, 3) * tr.VOXEL
    p = X @ E[:3, :3].T + E[:3, 3]
    front = p[:, 2] > 1e-3
    u, v = K[0, 0] * p[front, 0] / p[front, 2] + K[0, 2], K[1, 1] * p[front, 1] / p[front, 2] + K[1, 2]
    assert (p[:, 2] <= 0).sum() > 1000
    assert (u < -1).any() and (u > tr.WIDTH).any() and (v < -1).any() and (v > tr.HEIGHT).any() and ((u > 0) & (u < tr.WIDTH) & (v > 0) & (v < tr.HEIGHT)).any()
    before = r.weight.sum()
    tr.integrate(r, blocks, depth, colour, K, E, depth_max=DMAX)
    assert r.weight.sum() > before + 300
    g = new_grid(block_count=64)
    fuse_on_device(g, tr.scene_views(), lists=ref["lists"])
    g.integrate(dev(blocks), dev(depth), dev(colour), K, E, depth_max=DMAX)
    assert_grid_equals(g, r)


def test_integrate_leaves_unlisted_blocks_alone(ref):
    views = tr.scene_views()
    g, r = new_grid(block_count=256), tr.Grid(tr.VOXEL, True)
    fuse_on_device(g, views[:3], lists=ref["lists"])
    for (depth, colour, K, E), blocks in zip(views[:3], ref["lists"]):
        tr.integrate(r, blocks, depth, colour, K, E, depth_max=DMAX)
    c0, t0, w0, col0 = grid_arrays(g)
    depth, colour, K, E = views[3]
    listed = ref["lists"][3][::2]                                        # every other block of view 3: some old, some new
    g.integrate(dev(listed), dev(depth), dev(colour), K, E, depth_max=DMAX)
    tr.integrate(r, listed, depth, colour, K, E, depth_max=DMAX)
    assert_grid_equals(g, r)
    c1, t1, w1, col1 = grid_arrays(g)
    named = {tuple(x) for x in listed.tolist()}
    old = {tuple(x): i for i, x in enumerate(c0.tolist())}
    rows1 = np.array([i for i, x in enumerate(c1.tolist()) if tuple(x) in old and tuple(x) not in named])
    rows0 = np.array([old[tuple(c1[i].tolist())] for i in rows1])
    changed = np.array([i for i, x in enumerate(c1.tolist()) if tuple(x) in old and tuple(x) in named])
    assert len(rows1) > 10 and len(changed) > 5 and len(c1) > len(c0)
    assert same_bits(t1[rows1], t0[rows0]) and same_bits(w1[rows1], w0[rows0]) and same_bits(col1[rows1], col0[rows0])
    assert not np.array_equal(w1[changed], w0[[old[tuple(c1[i].tolist())] for i in changed]])
    # a list with repeats counts each block once
    g2 = new_grid(block_count=256)
    fuse_on_device(g2, views[:3], lists=ref["lists"])
    g2.integrate(dev(np.concatenate([listed, listed[::-1], listed[:7]])), dev(depth), dev(colour), K, E, depth_max=DMAX)
    assert_grid_equals(g2, r)


def test_integrate_without_colour(fused, ref):
    g = new_grid(with_color=False)
    fuse_on_device(g, tr.scene_views(), colour=False)
    assert g.color is None
    c, t, w, _ = grid_arrays(g)
    fc, ft, fw, _ = grid_arrays(fused["grid"])
    assert np.array_equal(c, fc) and same_bits(t, ft) and same_bits(w, fw)
    v, f, col = g.extract_triangle_mesh(THRESHOLD)
    assert col is None
    assert_mesh_equals((v, f, None), (ref["mesh"][0], ref["mesh"][1], None))


def test_integrate_depth_scale_and_default_depth_max(ref):
    """depth in other units, the default depth_max of 8 and a different truncation: the same as the restatement"""
    views = tr.scene_views()[:2]
    g, r = new_grid(block_count=16), tr.Grid(tr.VOXEL, True)
    for depth, colour, K, E in views:
        mm = (depth * np.float32(1000)).astype(np.float32)
        kw = dict(depth_scale=1000.0, trunc_voxel_multiplier=5.0)
        blocks = g.compute_unique_block_coordinates(dev(mm), K, E, **kw)
        want = tr.touch(mm, K, E, tr.VOXEL, **kw)
        assert np.array_equal(host(blocks), want)
        g.integrate(blocks, dev(mm), dev(colour), K, E, **kw)
        tr.integrate(r, want, mm, colour, K, E, **kw)
    assert_grid_equals(g, r)


# ---------------------------------------------------------------------------- growth ----------------------------------------------------------------------------
def test_growth_from_four_blocks(fused):
    g = new_grid(block_count=4)
    fuse_on_device(g, tr.scene_views())
    assert g.capacity >= g.n > 4 and g.capacity < 50000 and fused["grid"].capacity == 50000
    for a, b in zip(grid_arrays(g), grid_arrays(fused["grid"])):
        assert same_bits(a, b)
    for a, b in zip(g.extract_triangle_mesh(THRESHOLD), fused["mesh"]):
        assert same_bits(host(a), host(b))


# --------------------------------------------------------------------------- extraction ---------------------------------------------------------------------------
def test_extract_sphere(fused, ref):
    assert_mesh_equals(fused["mesh"], ref["mesh"])
    v, f, c = (host(m) for m in fused["mesh"])
    rep = tr.mesh_report(v, f)
    assert rep["edges_in_two_faces"] and rep["directed_once"] and rep["no_collapsed_face"] and rep["all_vertices_used"]
    assert rep["euler"] == 2 and rep["volume"] > 0
    assert np.abs(np.linalg.norm(v.astype(np.float64) - tr.CENTRE, axis=1) - tr.RADIUS).max() < 8 * tr.VOXEL
    block = np.floor(v.astype(np.float64) / (16 * tr.VOXEL)).astype(np.int64)[f]
    for axis in range(3):
        assert (block[:, :, axis].min(1) != block[:, :, axis].max(1)).any() and (block[:, :, axis] < 0).any()


def test_extract_weight_threshold(fused, ref):
    """just below an actual weight, and at it: `weight <= threshold` leaves the cell out"""
    assert (ref["grid"].weight == 2.0).any()
    below, at = np.float32(2.0) - np.float32(2.0 ** -22), 2.0
    m_below, m_at = fused["grid"].extract_triangle_mesh(float(below)), fused["grid"].extract_triangle_mesh(at)
    assert_mesh_equals(m_below, tr.extract_grid(ref["grid"], float(below)))
    assert_mesh_equals(m_at, tr.extract_grid(ref["grid"], at))
    assert len(m_at[1]) < len(m_below[1]) < len(fused["mesh"][1])
    assert_mesh_equals(fused["grid"].extract_triangle_mesh(), tr.extract_grid(ref["grid"], 3.0))          # the default


def test_extract_with_a_block_missing(ref):
    """one block of the sphere removed: no face from a cell that needs it, the rest unchanged"""
    c, t, w, col = ref["grid"].sorted_arrays()
    full_v, full_f, _ = ref["mesh"]
    block_of_face = np.floor(full_v.astype(np.float64)[full_f] / (16 * tr.VOXEL) + 1e-9).astype(np.int64)
    counts = [((block_of_face == b[None, None]).all(2).any(1)).sum() for b in c]
    gone = int(np.argmax(counts))                                        # the block with the most faces
    keep = np.arange(len(c)) != gone
    want = tr.extract(c[keep], t[keep], w[keep], col[keep], tr.VOXEL, THRESHOLD)
    g = new_grid(block_count=8)
    install_blocks(g, c[keep], t[keep], w[keep], col[keep])
    got = g.extract_triangle_mesh(THRESHOLD)
    assert_mesh_equals(got, want)
    assert 0 < len(want[1]) < len(full_f) - counts[gone] // 2
    # no vertex inside the missing block's cells or the layer of cells below it that reach into it
    lo = c[gone].astype(np.float64) * 16 * tr.VOXEL
    v = want[0].astype(np.float64)[want[1]].mean(1)                      # face centres
    inside = ((v > lo - tr.VOXEL) & (v < lo + 16 * tr.VOXEL)).all(1)
    assert not inside.any()
    # the faces that remain are faces of the full mesh
    full = {tuple(np.round(full_v[tri].reshape(-1) / tr.VOXEL * 4096).astype(np.int64)) for tri in full_f}
    assert all(tuple(np.round(want[0][tri].reshape(-1) / tr.VOXEL * 4096).astype(np.int64)) in full for tri in want[1][::17])
    rep = tr.mesh_report(want[0], want[1])
    assert not rep["edges_in_two_faces"] and rep["directed_once"]


def test_extract_all_cases():
    """2 x 2 x 2 blocks of random values, weights above the threshold, some corners exactly zero (they count as positive)"""
    rng = np.random.default_rng(31)
    coords = np.array([[x, y, z] for z in (-1, 0) for y in (-1, 0) for x in (-1, 0)], np.int64)
    t = rng.uniform(-1, 1, (8, 4096)).astype(np.float32)
    t[rng.random((8, 4096)) < 0.05] = 0.0
    t[rng.random((8, 4096)) < 0.01] = -0.0
    w = rng.integers(4, 9, (8, 4096)).astype(np.float32)
    col = rng.random((8, 4096, 3)).astype(np.float32)
    want = tr.extract(coords, t, w, col, tr.VOXEL, 3.0)
    # every case occurs
    vol = np.zeros((32, 32, 32), np.float32)
    for i, b in enumerate(coords):
        o = (b + 1) * 16
        vol[o[0]:o[0] + 16, o[1]:o[1] + 16, o[2]:o[2] + 16] = t[i].reshape(16, 16, 16).transpose(2, 1, 0)
    case = np.zeros((31, 31, 31), np.int64)
    for i in range(8):
        case |= (vol[(i & 1):(i & 1) + 31, ((i >> 1) & 1):((i >> 1) & 1) + 31, (i >> 2):(i >> 2) + 31] < 0).astype(np.int64) << i
    assert set(range(1, 255)) <= set(np.unique(case).tolist())
    assert len(want[1]) == int(tr.tables()["ntri"][case].sum())
    g = new_grid(block_count=8)
    install_blocks(g, coords, t, w, col)
    got = g.extract_triangle_mesh(3.0)
    assert_mesh_equals(got, want)
    # a weight at the threshold in one voxel empties the eight cells around it, nothing else
    w2 = w.copy()
    w2[3, (5 * 16 + 6) * 16 + 7] = 3.0
    g2 = new_grid(block_count=8)
    install_blocks(g2, coords, t, w2, col)
    got2 = g2.extract_triangle_mesh(3.0)
    want2 = tr.extract(coords, t, w2, col, tr.VOXEL, 3.0)
    assert_mesh_equals(got2, want2)
    assert len(want2[1]) < len(want[1])


def test_extract_empty_grid():
    g = new_grid()
    v, f, c = g.extract_triangle_mesh()
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and tuple(c.shape) == (0, 3)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and v.device == torch.device(DEV)
    v, f, c = new_grid(with_color=False).extract_triangle_mesh()
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and c is None
    # blocks, but nothing observed in them
    g = new_grid(block_count=2)
    install_blocks(g, np.array([[0, 0, 0], [1, 0, 0], [-1, 2, 5]]), np.full((3, 4096), -0.5, np.float32), np.zeros((3, 4096), np.float32), np.zeros((3, 4096, 3), np.float32))
    v, f, c = g.extract_triangle_mesh(0.0)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and tuple(c.shape) == (0, 3)


def test_whole_pipeline_is_deterministic(fused):
    g = new_grid()
    lists = fuse_on_device(g, tr.scene_views())
    assert all(np.array_equal(a, b) for a, b in zip(lists, fused["lists"]))
    for a, b in zip(grid_arrays(g), grid_arrays(fused["grid"])):
        assert same_bits(a, b)
    again = g.extract_triangle_mesh(THRESHOLD)
    for a, b in zip(again, fused["mesh"]):
        assert same_bits(host(a), host(b))
    for a, b in zip(g.extract_triangle_mesh(THRESHOLD), again):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------- fuse_views ---------------------------------------------------------------------------
class View:
    def __init__(self, E, gt_mask):
        self.image_width, self.image_height = tr.WIDTH, tr.HEIGHT
        self.FoVx, self.FoVy = 2 * math.atan(tr.WIDTH / (2 * tr.FOCAL)), 2 * math.atan(tr.HEIGHT / (2 * tr.FOCAL))
        self.world_view_transform = torch.from_numpy(E.T.astype(np.float32)).to(DEV)
        if gt_mask is not None:
            self.gt_mask = gt_mask


def test_fuse_views():
    import tsdf
    scene = tr.scene_views()
    ys, xs = np.meshgrid(np.arange(tr.HEIGHT), np.arange(tr.WIDTH), indexing="ij")
    views, rendered, by_hand = [], {}, tr.Grid(tr.VOXEL, True)
    for i, (depth, colour, K, E) in enumerate(scene):
        alpha = np.where((xs + ys + i) % 7 == 0, 0.49, np.where((xs + 2 * ys) % 11 == 0, 0.5, 0.9)).astype(np.float32)      # 0.5 itself stays
        gt = None if i % 3 == 2 else np.where((xs // 8 + ys // 8 + i) % 5 == 0, 0.2, np.where(xs % 9 == 0, 0.5, 1.0)).astype(np.float32)
        wide = (colour * np.float32(1.5) - np.float32(0.25)).astype(np.float32)                                              # leaves [0, 1]: clamped
        view = View(E, None if gt is None else dev(gt)[None])
        views.append(view)
        rendered[id(view)] = dict(render=dev(np.concatenate([wide.transpose(2, 0, 1), np.zeros((4, tr.HEIGHT, tr.WIDTH), np.float32)])),
                                  median_depth=dev(depth)[None], mask=dev(alpha)[None])
        # the same by hand: the world_view_transform as the view holds it (float32), the intrinsics from the field of view
        masked = depth.copy()
        if gt is not None:
            masked[gt < 0.5] = 0
        masked[alpha < 0.5] = 0
        assert (masked != depth).sum() > 100
        Kv = np.array([[tr.WIDTH / (2 * math.tan(view.FoVx / 2)), 0, tr.WIDTH / 2], [0, tr.HEIGHT / (2 * math.tan(view.FoVy / 2)), tr.HEIGHT / 2], [0, 0, 1]])
        Ev = E.T.astype(np.float32).astype(np.float64).T
        blocks = tr.touch(masked, Kv, Ev, tr.VOXEL, depth_max=DMAX)
        tr.integrate(by_hand, blocks, masked, np.clip(wide, 0, 1), Kv, Ev, depth_max=DMAX)
    want = tr.extract_grid(by_hand, THRESHOLD)
    before = {k: {n: t.clone() for n, t in d.items()} for k, d in rendered.items()}
    got = tsdf.fuse_views(views, lambda v: rendered[id(v)], voxel_size=tr.VOXEL, depth_max=DMAX, alpha_thres=0.5, block_count=16, weight_threshold=THRESHOLD)
    assert_mesh_equals(got, want)
    assert len(want[1]) > 10000
    for k, d in rendered.items():                                                                                          # the renderer's maps are not modified
        assert all(torch.equal(t, before[k][n]) for n, t in d.items())
    with pytest.raises(RuntimeError, match="no views"):
        tsdf.fuse_views([], lambda v: None)
