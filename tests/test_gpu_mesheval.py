"""GPU tier of mesh evaluation: the HIP kernels and mesh_eval.py against the fixtures the reference's own code wrote
(tests/golden/make_golden_mesheval.py) and against tests/mesheval_restatement.py at sizes and edge cases the fixtures do not reach.
Exact: per-triangle counts, point order, masks, neighbour indices, the culled mesh.  Sampled coordinates and distances: 1e-12 relative
(both sides are the same few fp64 operations; the slack only allows for a square root that is not correctly rounded).  Means: 1e-9
relative (N 2^-53 at N = 10^7: any summation order fits)."""
import math

import numpy as np
import pytest
import torch

import mesheval_restatement as mr
from test_mesheval_golden import chamfer_inputs, check_chamfer, close, cull_cameras, load, projection_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHAMFER_KEYS = ("data_pcd", "counts", "keep", "inbound", "grid_inbound", "in_obs", "dist_d2s", "idx_d2s", "above", "dist_s2d", "idx_s2d")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def chamfer_fx():
    return load("mesheval_chamfer.npz")


@pytest.fixture(scope="module")
def cull_fx():
    return load("mesheval_cull.npz")


def sample(vertices, faces, density=0.2):
    import mesh_eval
    cloud, counts = mesh_eval.sample_mesh_points(dev(np.asarray(vertices, np.float64).reshape(-1, 3)), dev(np.asarray(faces, np.int64).reshape(-1, 3)), density)
    assert cloud.dtype == torch.float64 and counts.dtype == torch.int32
    return host(cloud), host(counts)


def thin(points, radius, perm=None):
    """mesh_eval.downsample_points on `points` in the given order (identity permutation unless one is passed) -> keep mask"""
    import mesh_eval
    n = len(points)
    perm = np.arange(n) if perm is None else perm
    kept, keep, used = mesh_eval.downsample_points(dev(np.asarray(points, np.float64).reshape(-1, 3)), radius, perm=dev(perm.astype(np.int64)))
    keep = host(keep)
    assert keep.dtype == bool and np.array_equal(host(used), perm) and np.array_equal(host(kept), np.asarray(points)[perm][keep])
    return keep


# ------------------------------------------------------------------------- fixture -------------------------------------------------------------------------
def test_chamfer_fixture_stage_by_stage(chamfer_fx):
    import mesh_eval as me
    fx, a = chamfer_fx, chamfer_inputs(chamfer_fx)
    cloud, counts = me.sample_mesh_points(dev(a["vertices"]), dev(a["faces"]), a["density"])
    assert np.array_equal(host(counts), fx["counts"]) and close(host(cloud), fx["data_pcd"], 1e-12)
    # from here every stage starts from the fixture's own intermediate, so that one stage's last-bit difference cannot hide in the next
    data_down, keep, _ = me.downsample_points(dev(fx["data_pcd"]), a["density"], perm=dev(a["perm"]))
    assert np.array_equal(host(keep), fx["keep"])
    want_down = fx["data_pcd"][a["perm"]][fx["keep"]]
    assert np.array_equal(host(data_down), want_down)
    masks = me.obs_mask_select(data_down, a["obs_mask"], a["BB"], a["Res"], a["patch"])
    for got, key in zip(masks, ("inbound", "grid_inbound", "in_obs")):
        assert got.dtype == torch.bool and np.array_equal(host(got), fx[key]), key
    stl = dev(a["stl"])
    cell = a["max_dist"] / me.NN_CELLS_PER_MAX_DIST
    dist, idx = me.PointGrid(stl, cell).nearest(dev(want_down[fx["in_obs"]]), a["max_dist"])
    assert idx.dtype == torch.int64 and np.array_equal(host(idx), fx["idx_d2s"]) and close(host(dist), fx["dist_d2s"], 1e-12)
    above = me.above_plane(stl, a["plane"])
    assert np.array_equal(host(above), fx["above"])
    dist, idx = me.PointGrid(dev(want_down[fx["inbound"]]), cell).nearest(stl[above], a["max_dist"])
    assert np.array_equal(host(idx), fx["idx_s2d"]) and close(host(dist), fx["dist_s2d"], 1e-12)
    assert np.isinf(host(dist)).sum() == np.isinf(fx["dist_s2d"]).sum() > 0
    s, n = host(me.mean_below(dist, a["max_dist"]))
    assert n == np.isfinite(fx["dist_s2d"]).sum() and math.isclose(s / n, float(fx["mean_s2d"]), rel_tol=1e-9)
    # another cell size changes the search, not the answer
    dist2, idx2 = me.PointGrid(dev(want_down[fx["inbound"]]), 0.7).nearest(stl[above], a["max_dist"])
    assert torch.equal(idx2, idx) and torch.equal(dist2, dist)


def test_chamfer_fixture_end_to_end(chamfer_fx):
    import mesh_eval as me
    a = chamfer_inputs(chamfer_fx)
    out = me.dtu_chamfer(dev(a["vertices"]), dev(a["faces"].astype(np.int32)), dev(a["stl"]), a["obs_mask"], a["BB"], a["Res"], a["plane"],
                         density=a["density"], patch_size=a["patch"], max_dist=a["max_dist"], perm=dev(a["perm"]))
    got = {k: host(out[k]) for k in CHAMFER_KEYS}
    got.update({k: out[k] for k in ("mean_d2s", "mean_s2d", "overall")})
    check_chamfer(got, chamfer_fx)
    assert np.array_equal(host(out["data_in"]), host(out["data_down"])[got["inbound"]]) and out["stl_above"].shape[0] == got["above"].sum()


# --------------------------------------------------------------------------- sums ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 262144, 262145, 600001])
def test_mean_below_equals_the_fixed_order_restatement_bit_for_bit(n):
    """Around the one-block boundary, the last size with one row per thread (1024 x 256), the first with a second stride, and a ragged large
    one.  Both outputs with ==: the order of the additions is the contract (tests/test_mesheval_restatement.py shows other orders differ)."""
    import mesh_eval as me
    d = mr.sum_case(n)
    got = host(me.mean_below(dev(d), mr.SUM_MAX_DIST))
    want = mr.sum_below(d, mr.SUM_MAX_DIST)
    assert got.dtype == np.float64 and got[0] == want[0] and got[1] == want[1], (got, want)


# ------------------------------------------------------------------------- sampling -------------------------------------------------------------------------
def test_sampling_empty_and_degenerate_meshes():
    cloud, counts = sample(np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    assert cloud.shape == (0, 3) and counts.shape == (0,)
    v = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0], [1.0, 2.0, 3.0]])
    cloud, counts = sample(v, np.zeros((0, 3), np.int64))
    assert np.array_equal(cloud, v) and counts.shape == (0,)
    cloud, counts = sample(v, [[0, 0, 1], [0, 1, 2], [2, 2, 2], [0, 3, 1]])             # repeated corners, collinear points, coincident points
    assert np.array_equal(cloud, v) and np.array_equal(counts, [0, 0, 0, 0])


def test_sampling_one_large_triangle_spans_workgroups():
    v = np.array([[100.0, -50.0, 600.0], [119.3, -47.1, 603.7], [98.2, -31.6, 611.9]])
    want, want_counts = mr.sample_mesh(v, [[0, 1, 2]])
    cloud, counts = sample(v, [[0, 1, 2]])
    assert want_counts[0] > 4000 and np.array_equal(counts, want_counts)
    assert cloud.shape == want.shape and close(cloud, want, 1e-12) and np.array_equal(cloud[:3], v)


def test_sampling_equal_subdivisions_keep_the_reference_ties():
    """right isosceles triangles with thr = density exactly: n1 = n2 = n puts lattice points ON k0 + k1 = 1 up to the rounding of two divisions"""
    verts, faces = [], []
    for n in (2, 3, 5, 6, 7):
        for leg in (0.2 * n + 0.1, 0.2 * n + 0.05):
            k = len(verts)
            verts += [[10.0 * n, 0.0, 0.0], [10.0 * n + leg, 0.0, 0.0], [10.0 * n, leg, 0.0]]
            faces += [[k, k + 1, k + 2], [k + 2, k, k + 1]]
    want, want_counts = mr.sample_mesh(np.array(verts), faces)
    cloud, counts = sample(verts, faces)
    assert (want_counts > 0).all() and np.array_equal(counts, want_counts) and close(cloud, want, 1e-12)
    rng = np.random.default_rng(3)
    v = rng.uniform(-0.6, 0.6, (400, 3)) + [100.0, 200.0, -300.0]                          # and random shapes, slivers included
    f = rng.integers(0, 400, (1500, 3))
    want, want_counts = mr.sample_mesh(v, f)
    cloud, counts = sample(v, f)
    assert want.shape[0] < 12000 + 400 and np.array_equal(counts, want_counts) and close(cloud, want, 1e-12)


def test_sampling_refuses_bad_meshes():
    import mesh_eval as me
    v = torch.zeros(4, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="outside the 4 vertices"):
        me.sample_mesh_points(v, torch.tensor([[0, 1, 4]], device=DEV))
    bad = v.clone()
    bad[2, 1] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        me.sample_mesh_points(bad, torch.tensor([[0, 1, 2]], device=DEV))
    for density in (True, 0.0, float("inf")):
        with pytest.raises(RuntimeError, match="`density` must be a positive finite number"):
            me.sample_mesh_points(v, torch.tensor([[0, 1, 2]], device=DEV), density)


# ------------------------------------------------------------------------- thinning -------------------------------------------------------------------------
def test_thinning_chain_of_200_rounds():
    line = np.stack([50.0 + np.arange(200) * 0.6 * 0.2, np.full(200, -7.0), np.full(200, 3.0)], 1)
    keep = thin(line, 0.2)
    assert np.array_equal(keep, mr.thin(line, 0.2)) and np.array_equal(keep, np.arange(200) % 2 == 0)


def test_thinning_duplicates_crowded_cell_and_single_point():
    rng = np.random.default_rng(5)
    assert np.array_equal(thin(np.array([[1.0, 2.0, 3.0]]), 0.2), [True])
    base = rng.uniform(0, 2, (300, 3))
    dup = np.concatenate([base, base[:100], base[:50]], 0)[rng.permutation(450)]      # exact duplicates: the first of each survives
    assert np.array_equal(thin(dup, 0.2), mr.thin(dup, 0.2))
    crowd = np.concatenate([rng.uniform(0.41, 0.59, (150, 3)), rng.uniform(0, 1, (400, 3))], 0)[rng.permutation(550)]   # 150 points in one cell
    keep = thin(crowd, 0.2)
    assert np.array_equal(keep, mr.thin(crowd, 0.2)) and 1 < keep.sum() < 550


_ORDER_CASES = {}


def _order_case(seed):
    """10 000 random points (about five neighbours within the radius) thinned under permutation `seed`: (GPU, restatement) masks by point id"""
    if seed not in _ORDER_CASES:
        pts = np.random.default_rng(6).uniform(0, 4, (10_000, 3)) + [300.0, -200.0, 650.0]
        perm = np.random.default_rng(seed).permutation(10_000)
        by_id = []
        for keep in (thin(pts, 0.2, perm), mr.thin(pts[perm], 0.2)):
            ids = np.zeros(10_000, bool)
            ids[perm[keep]] = True
            by_id.append(ids)
        _ORDER_CASES[seed] = tuple(by_id)
    return _ORDER_CASES[seed]


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_thinning_equals_the_loop_under_a_permutation(seed):
    got, want = _order_case(seed)
    assert np.array_equal(got, want) and 2000 < want.sum() < 5000


def test_thinning_depends_on_the_order():
    a, b, c = (_order_case(seed)[0] for seed in (0, 1, 2))
    assert not np.array_equal(a, b) and not np.array_equal(b, c) and not np.array_equal(a, c)


def test_thinning_clusters_one_key_period_apart():
    """cell keys wrap after 2048 cells along x and y and 1024 along z: two clusters that share keys must not see each other"""
    import mesh_eval as me
    rng = np.random.default_rng(7)
    r = 0.2
    cell = r * me.CELL_SLACK
    for axis, period in ((0, 2048), (1, 2048), (2, 1024)):
        a = rng.uniform(0, 3 * r, (120, 3))
        b = rng.uniform(0, 3 * r, (120, 3))
        b[:, axis] += period * cell
        pts = np.concatenate([a, b], 0)[rng.permutation(240)]
        assert np.array_equal(thin(pts, r), mr.thin(pts, r)), axis


# --------------------------------------------------------------------- nearest neighbour ---------------------------------------------------------------------
def test_nearest_near_far_outside_and_empty():
    import mesh_eval as me
    rng = np.random.default_rng(8)
    cloud = rng.uniform(0, 10, (3000, 3)) + [100.0, 50.0, 600.0]
    cloud[17] = cloud[4]                                                               # equal distances: the lower index
    grid = me.PointGrid(dev(cloud), 0.5)
    lo = np.array([100.0, 50.0, 600.0])
    queries = np.concatenate([rng.uniform(0, 10, (2000, 3)) + lo,                      # inside the cloud
                              rng.uniform(-3.5, 13.5, (2000, 3)) + lo,                 # around its bounding box: several shells out
                              rng.uniform(-30, 40, (500, 3)) + lo,                     # mostly beyond max_dist
                              cloud[4:5], cloud[:3] + 1e-3], 0)
    want_d, want_i = mr.nearest(cloud, queries, 4.0)
    dist, idx = grid.nearest(dev(queries), 4.0)
    assert np.array_equal(host(idx), want_i) and close(host(dist), want_d, 1e-12)
    assert (want_i == -1).sum() > 100 and (want_d[:4000] > 1.0).sum() > 100 and want_i[4500] == 4
    dist, idx = grid.nearest(torch.zeros((0, 3), dtype=torch.float64, device=DEV), 4.0)
    assert dist.shape == (0,) and idx.shape == (0,) and idx.dtype == torch.int64
    one = me.PointGrid(dev(cloud[:1]), 2.5)                                            # a cloud of one point
    dist, idx = one.nearest(dev(queries[:100]), 20.0)
    want_d, want_i = mr.nearest(cloud[:1], queries[:100], 20.0)
    assert np.array_equal(host(idx), want_i) and close(host(dist), want_d, 1e-12)
    s, n = host(me.mean_below(dev(np.array([1.0, np.inf, 3.0, 20.0, 19.5])), 20.0))
    assert (s, n) == (23.5, 3.0)


# --------------------------------------------------------------------------- masks ---------------------------------------------------------------------------
def test_observation_mask_on_every_side_of_the_box_and_the_volume():
    import mesh_eval as me
    rng = np.random.default_rng(9)
    BB = np.array([[10.0, -20.0, 30.0], [14.0, -17.0, 32.0]])
    vol = (rng.random((7, 6, 5)) < 0.6)
    res, patch = 1.0, 2.0
    pts = rng.uniform(BB[0] - patch - 1.5, BB[1] + 2 * patch + 1.5, (6000, 3))
    want = mr.obs_masks(pts, vol, BB, res, patch)
    g = np.rint((pts[want[0]] - BB[:1].astype(np.float32)) / res)
    assert (g == -1).any() and all((g[:, k] == vol.shape[k]).any() for k in range(3))  # grid indices -1 and shape occur among the inbound points
    assert 0 < want[2].sum() < want[1].sum() < want[0].sum() < 6000
    for obs in (vol, dev(vol), dev(vol.astype(np.uint8))):
        got = me.obs_mask_select(dev(pts), obs, BB, res, patch)
        for a, b in zip(got, want):
            assert np.array_equal(host(a), b)
    plane = np.array([0.3, -0.2, 0.9, -24.0])
    assert np.array_equal(host(me.above_plane(dev(pts), plane)), mr.above_plane(pts, plane))


# --------------------------------------------------------------------------- cull ---------------------------------------------------------------------------
def test_cull_fixture(cull_fx):
    import mesh_eval as me
    fx = cull_fx
    cams = [(torch.from_numpy(c[0]), c[1], c[2], c[3], c[4], dev(c[5])) for c in cull_cameras(fx)]
    for i, c in enumerate(cams):
        assert np.array_equal(host(me.dilate_mask(c[5], 6)), fx[f"dilated{i}"]), i
    v, f = me.cull_mesh(dev(fx["vertices"]), dev(fx["faces"]), cams)
    assert v.dtype == torch.float32 and f.dtype == torch.int64
    assert np.array_equal(host(v), fx["out_vertices"]) and np.array_equal(host(f), fx["out_faces"])
    v64, f64 = me.cull_mesh(dev(fx["vertices"].astype(np.float64)), dev(fx["faces"].astype(np.int64)), cams)     # as trimesh holds them
    assert v64.dtype == torch.float64 and np.array_equal(host(v64), fx["out_vertices"].astype(np.float64)) and torch.equal(f64, f)
    from types import SimpleNamespace                                                                            # the reference's camera objects
    objs = [SimpleNamespace(world_view_transform=torch.from_numpy(fx[f"w2c{i}"]).T.contiguous().to(DEV), FoVx=float(fx[f"fov{i}"][0]),
                            FoVy=float(fx[f"fov{i}"][1]), image_width=c[3], image_height=c[4], gt_mask=c[5][None].float()) for i, c in enumerate(cams)]
    v2, f2 = me.cull_mesh(dev(fx["vertices"]), dev(fx["faces"]), objs)
    assert torch.equal(v2, v) and torch.equal(f2, f)


def test_cull_edge_cases_against_the_restatement():
    import mesh_eval as me
    rng = np.random.default_rng(10)
    verts = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    verts[0] = [0.0, 0.0, -5.0]                                                        # behind the first camera
    faces = rng.integers(0, 500, (900, 3))
    W, H = 53, 37
    front = np.eye(4, dtype=np.float32)
    front[2, 3] = 3.0                                                                  # the cloud sits 3 in front
    away = np.diag([1.0, 1.0, -1.0, 1.0]).astype(np.float32)
    away[0, 3], away[2, 3] = 40.0, -3.0                                                # behind and far to the side: sees no vertex inside (-1, 1)
    blob = (rng.random((H, W)) < 0.03).astype(np.uint8) * 255
    cases = {"behind": [(front, 60.0, 50.0, W, H, blob)], "unseen": [(front, 60.0, 50.0, W, H, blob), (away, 60.0, 50.0, W, H, np.zeros((H, W), np.uint8))],
             "zeros": [(front, 60.0, 50.0, W, H, np.zeros((H, W), np.uint8))]}
    for name, cams in cases.items():
        keep = mr.cull_vertex_mask(verts, [(projection_rows(c), c[3], c[4], c[5]) for c in cams], 6)
        want_v, want_f, _ = mr.apply_vertex_mask(verts, faces, keep)
        v, f = me.cull_mesh(dev(verts), dev(faces), [(torch.from_numpy(c[0]), c[1], c[2], c[3], c[4], dev(c[5])) for c in cams])
        assert np.array_equal(host(v), want_v) and np.array_equal(host(f), want_f), name
        if name == "zeros":
            assert 0 < keep.sum() < 500                                                # only what projects outside the image survives
    v, f = me.cull_mesh(dev(verts), dev(faces), [])                                    # no camera: nothing is culled
    assert np.array_equal(host(v), verts) and np.array_equal(host(f), faces)


def test_dilation_with_set_pixels_at_the_borders():
    import mesh_eval as me
    rng = np.random.default_rng(11)
    m = np.zeros((37, 53), np.uint8)
    m[0, 0] = m[36, 52] = m[0, 30] = m[20, 0] = m[36, 7] = 1
    m[rng.integers(0, 37, 6), rng.integers(0, 53, 6)] = 200
    for radius in (0, 1, 6, 9):
        assert np.array_equal(host(me.dilate_mask(dev(m), radius)), mr.dilate(m, radius)), radius
    assert np.array_equal(host(me.dilate_mask(dev(m.astype(np.float32)))), mr.dilate(m, 6))


# ------------------------------------------------------------------------- end to end -------------------------------------------------------------------------
def test_chamfer_at_5000_triangles_repeats_bit_for_bit_on_a_side_stream():
    import mesh_eval as me
    rng = np.random.default_rng(12)
    nlat, nlon, centre = 50, 51, np.array([40.0, -120.0, 700.0])
    th, ph = np.meshgrid(np.pi * (np.arange(nlat + 1)) / nlat, 2 * np.pi * np.arange(nlon) / nlon, indexing="ij")
    rad = 8.0 * (1 + 0.02 * np.sin(5 * th) * np.cos(3 * ph))
    verts = (np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1) * rad[..., None]).reshape(-1, 3) + centre
    verts = verts.astype(np.float32).astype(np.float64)
    at = lambda a, b: a * nlon + (b % nlon)
    faces = [[at(a, b), at(a + 1, b), at(a + 1, b + 1)] for a in range(nlat) for b in range(nlon)]
    faces += [[at(a, b), at(a + 1, b + 1), at(a, b + 1)] for a in range(1, nlat - 1) for b in range(nlon)]
    faces = np.array(faces)
    assert 4900 < faces.shape[0] < 5100
    d = rng.standard_normal((6000, 3))
    stl = centre + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(7.5, 8.5, (6000, 1))
    stl[:500] += [60.0, 0.0, 0.0]
    BB = np.array([centre - [20.0, 20.0, 2.0], centre + [20.0, 20.0, 20.0]])
    vol = rng.random((81, 81, 45)) < 0.7
    plane = np.array([0.0, 0.1, 1.0, -(700.0 - 12.0 + 0.1 * -120.0)])
    stream = torch.cuda.Stream(device=DEV)
    runs = []
    with torch.cuda.stream(stream):
        v, f, s = dev(verts), dev(faces), dev(stl)
        perm = None
        for _ in range(2):
            out = me.dtu_chamfer(v, f, s, vol, BB, 0.5, plane, perm=perm, generator=torch.Generator(device=DEV).manual_seed(3))
            perm = out["perm"]
            runs.append(out)
    stream.synchronize()
    a, b = runs
    assert a["data_pcd"].shape[0] > 15_000 and 0 < a["keep"].sum() < a["keep"].shape[0] and 0 < a["in_obs"].sum() < a["inbound"].sum()
    assert math.isfinite(a["overall"]) and 0 < a["mean_d2s"] < 2 and 0 < a["mean_s2d"] < 20
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k
