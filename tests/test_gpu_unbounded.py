"""GPU tier of unbounded mesh extraction: unbounded_mesh.py and the kernels of csrc/radegs_unbounded.hip against
tests/unbounded_restatement.py, bit for bit, NaN equal to NaN.  Every float32 operation of the specification (include/radegs.h, "Unbounded
mesh extraction") is an IEEE add, multiply, divide, square root, floor, min or max in a fixed order, correctly rounded on both sides, so no
step needs a tolerance; none is given."""
import math
import os

import numpy as np
import pytest
import torch

import unbounded_restatement as ur

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
H0, W0, H2, W2 = 37, 45, 24, 31
VOXEL = 0.025                      # trunc5 = float32(5 * 0.025) = 0.125 exactly


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def same_bits(a, b):
    """bit for bit, NaN equal to NaN (the sign and payload of a NaN are not pinned: x86 and gfx950 produce different ones)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or a.dtype != np.float32:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


class View:
    def __init__(self, full_proj, world_view=None):
        self.full_proj_transform = torch.from_numpy(np.asarray(full_proj, F))
        self.world_view_transform = torch.from_numpy(np.asarray(np.eye(4) if world_view is None else world_view, F))


def stack_of(views, world_view=None, colour=True):
    import unbounded_mesh as um
    vs = [View(m, None if world_view is None else world_view[i]) for i, (m, _, _) in enumerate(views)]
    return um.ViewStack(vs, [dev(d) for _, d, _ in views], [dev(c) for _, _, c in views] if colour else None)


# ----------------------------------------------------------------------- the fuse kernel -----------------------------------------------------------------------
def fuse_views():
    """seven views.  View 0 looks along +z from the origin with px = x / z, py = y / z: a constant depth of 0.5 with one NaN pixel and a zero
    background in its first columns, so that the decisions of the specification can be hit exactly.  Views 1..6 are perspective cameras
    around the origin with rough depth maps; view 2 is 24 x 31, the others 37 x 45."""
    rng = np.random.default_rng(1701)
    axis = np.zeros((4, 4), F)
    axis[0, 0] = axis[1, 1] = axis[2, 2] = axis[2, 3] = 1
    d0 = np.full((H0, W0), 0.5, F)
    d0[18, 30] = np.nan
    d0[:, :6] = 0
    views = [(axis, d0, rng.random((3, H0, W0)).astype(F))]
    for k in range(1, 7):
        a, e = 0.9 * k, 0.5 * math.sin(1.3 * k)
        eye = 3.0 * np.array([math.cos(a) * math.cos(e), math.sin(a) * math.cos(e), math.sin(e)])
        E = ur.look_at(eye, np.array([0.1, -0.1, 0.0]))
        H, W = (H2, W2) if k == 2 else (H0, W0)
        full = (E.T @ ur.projection(0.9, 0.8).T).astype(F)
        depth = (3.0 + rng.uniform(-1.2, 1.2, (H, W)) * (rng.random((H, W)) < 0.7)).astype(F)
        depth[rng.random((H, W)) < 0.05] = 0
        views.append((full, depth, rng.random((3, H, W)).astype(F)))
    return views


def fuse_samples_list():
    """the decisions of the specification first (with center 0, radius 1, view 0), then 1000 samples all over the contracted cube"""
    one = F(1)
    special = [
        (0, 0, 0),                                        # y = 0: z = 0 for view 0, px = 0 / 0
        (0.25, 0.1, 0.25), (-0.25, 0.1, 0.25),            # px exactly +1, -1: not in view
        (0.1, 0.3, 0.3), (0.1, -0.3, 0.3),                # py exactly +1, -1
        (0, 0, 0.625),                                    # sdf = 0.5 - 0.625 = -trunc exactly: not integrated
        (0, 0, float(np.nextafter(F(0.625), F(0)))),      # the last value before it: integrated, s just above -1
        (0, 0, 0.1), (0, 0, 0.7),                         # sdf / trunc = 3.2: clamped to 1; sdf / trunc = -1.6: skipped
        (0, 0, 0.45),                                     # sdf / trunc = 0.4
        (float(np.nextafter(one, F(0))), 0, 0), (1, 0, 0), (float(np.nextafter(one, F(2))), 0, 0),      # mag just below 1, exactly 1, just above
        (1.2, 0.5, 0.3), (-0.7, 1.1, 0.9),                # mag in (1, 2)
        (2, 0, 0), (0, -2, 0),                            # mag exactly 2: 1 / 0
        (1.9, 1.9, 1.9), (-1.5, 1.4, 1.2),                # mag above 2: a negative factor
        (1.6, 0, 0), (0, 0, 1.75),                        # world norm 2.5 and 4: above 1.9, the truncation stops growing
        (0.1, 0.1, -0.5),                                 # behind view 0
        (0.18, 0, 0.5),                                   # its taps include the NaN pixel
        (-0.45, 0, 0.5), (-0.09, 0, 0.1),                 # over the zero background: skipped (sdf = -0.5), integrated (sdf = -0.1)
        (0.48, 0.35, 0.5),                                # near the map's corner
    ]
    rng = np.random.default_rng(1702)
    rest = np.where(rng.random((1000, 1)) < 0.5, rng.uniform(-1.9, 1.9, (1000, 3)), rng.normal(0, 0.4, (1000, 3)))
    return np.concatenate([np.array(special, np.float64), rest]).astype(F)


FRAMES = (((0.0, 0.0, 0.0), 1.0), ((0.1, -0.2, 0.05), 1.7))


@pytest.fixture(scope="module")
def fuse_scene():
    views = fuse_views()
    return dict(views=views, stack=stack_of(views), stack_plain=stack_of(views, colour=False), samples=fuse_samples_list())


def check_fuse(scene, y, V, contract, rgb, frame):
    import unbounded_mesh as um
    center, radius = frame
    views = scene["views"][:V]
    stack = stack_of(views) if V not in (0, 7) else (scene["stack"] if V else None)
    want = ur.fuse(y, views, VOXEL, center, radius, contract, rgb)
    if V == 0:      # a stack names its device through its maps: V = 0 goes through the C ABI directly
        t = torch.full((len(y),), 7.0, device=DEV)
        c = torch.full((len(y), 3), 7.0, device=DEV) if rgb else None
        from diff_gaussian_rasterization import _C
        import ctypes
        y_dev = dev(y)
        rc = um._lib().radegs_unbounded_fuse(len(y), _C._ptr(y_dev), None, None, None, 0, 0, 0, 0, 0, None, int(contract), float(F(radius)),
                                             (ctypes.c_float * 3)(*center), float(F(5 * VOXEL)), _C._ptr(t), _C._ptr(c), _C._stream(torch.device(DEV)))
        assert rc == 0
        got = (t, c) if rgb else t
    else:
        got = um.fuse_samples(stack, dev(y), VOXEL, center, radius, contract=contract, return_rgb=rgb)
    if rgb:
        assert same_bits(host(got[0]), want[0]) and same_bits(host(got[1]), want[1]), (len(y), V, contract, frame)
    else:
        assert same_bits(host(got), want), (len(y), V, contract, frame, int((host(got).view(np.uint32) != want.view(np.uint32)).sum()))
    return want


@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 1000])
def test_fuse_matches_the_restatement(fuse_scene, M):
    y = fuse_scene["samples"][:M]
    for V in (0, 1, 3, 7):
        for contract in (True, False):
            for rgb in (True, False):
                for frame in FRAMES:
                    want = check_fuse(fuse_scene, y, V, contract, rgb, frame)
                    t = want[0] if rgb else want
                    if V == 0:
                        assert (t == 1).all() and (not rgb or (want[1] == 0).all())


def test_fuse_decisions_of_the_specification(fuse_scene):
    """the special samples against view 0 alone, center 0 and radius 1: what each of them must come to"""
    y = fuse_scene["samples"][:26]
    t, c = check_fuse(fuse_scene, y, 1, True, True, FRAMES[0])
    untouched = [0, 1, 2, 3, 4, 5, 8, 21, 22, 23]                       # 0 / 0, px or py = +-1, sdf = -trunc, sdf < -trunc, behind, NaN tap, background
    assert (t[untouched] == 1).all() and (c[untouched] == 0).all()
    assert t[6] == (F(1) + np.maximum((F(0.5) - y[6, 2]) / F(0.125), F(-1))) / F(2) and 0 < t[6] < 1e-6       # s just above -1
    assert t[7] == 1 and (c[7] > 0).all()                                # s clamped to +1: (1 * 1 + 1) / 2, and the colour is integrated
    assert t[9] == (F(1) + (F(0.5) - y[9, 2]) / F(0.125)) / F(2) and abs(t[9] - 0.7) < 1e-6
    assert t[24] == (F(1) + (F(0) - F(0.1)) / F(0.125)) / F(2)           # over the zero background, within the truncation
    assert np.isnan(ur.uncontract(y[15:17], 1.0, (0, 0, 0))).any() or np.isinf(ur.uncontract(y[15:17], 1.0, (0, 0, 0))).any()      # mag = 2
    # with all seven views: some sample is integrated by several, and some by none
    full = check_fuse(fuse_scene, fuse_scene["samples"], 7, True, False, FRAMES[0])
    assert (full == 1).sum() > 10 and (full < 0).sum() >= 5 and ((full > 0) & (full < 1)).sum() > 10


def test_fuse_lattice_modes_agree_with_explicit_samples(fuse_scene):
    import unbounded_mesh as um
    rng = np.random.default_rng(1703)
    for dims in ((7, 5, 9), (4, 4, 4), (1, 1, 70), (13, 2, 3)):
        ax, ay, az = (np.sort(rng.uniform(-1.2, 1.2, n)).astype(F) for n in dims)
        pts = ur.lattice_points(ax, ay, az)
        for contract, frame in ((True, FRAMES[1]), (False, FRAMES[0])):
            want = ur.fuse(pts, fuse_scene["views"], VOXEL, frame[0], frame[1], contract, True)
            explicit = um.fuse_samples(fuse_scene["stack"], dev(pts), VOXEL, frame[0], frame[1], contract=contract, return_rgb=True)
            assert same_bits(host(explicit[0]), want[0]) and same_bits(host(explicit[1]), want[1])
            for mapping in (um.ZRUN, um.BRICK):
                got = um.fuse_samples(fuse_scene["stack"], (dev(ax), dev(ay), dev(az)), VOXEL, frame[0], frame[1], contract=contract, return_rgb=True, mapping=mapping)
                assert torch.equal(got[0].view(torch.int32), explicit[0].view(torch.int32)) and torch.equal(got[1].view(torch.int32), explicit[1].view(torch.int32)), (dims, mapping)
                plain = um.fuse_samples(fuse_scene["stack_plain"], (dev(ax), dev(ay), dev(az)), VOXEL, frame[0], frame[1], contract=contract, mapping=mapping)
                assert torch.equal(plain.view(torch.int32), explicit[0].view(torch.int32))


def test_world_points(fuse_scene):
    import unbounded_mesh as um
    y = fuse_scene["samples"]
    for (center, radius), max_range in ((FRAMES[1], 32.0), (FRAMES[0], 1.5)):
        got = host(um.world_points(dev(y), center, radius, max_range))
        want = ur.world_points(y, radius, center, max_range)
        assert same_bits(got, want)
        assert np.isnan(want).any() and (want == F(max_range)).any() and (want == -F(max_range)).any()


# ------------------------------------------------------------------- dense marching cubes -------------------------------------------------------------------
def mc_both(values, ax, ay, az, offset=(0, 0, 0), G=None):
    import unbounded_mesh as um
    got = um.dense_marching_cubes(dev(values), dev(ax), dev(ay), dev(az), offset, G)
    want = ur.dense_marching_cubes(values, ax, ay, az, offset, G)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[2].dtype == torch.int64
    assert np.array_equal(host(got[1]), want[1]) and np.array_equal(host(got[2]), want[2]), "keys or faces differ"
    assert same_bits(host(got[0]), want[0]), "vertices differ"
    return got, want


def test_marching_cubes_all_256_cases():
    T = ur.tables()
    ax, ay, az = np.array([0.5, 1.75], F), np.array([-2.0, -1.0], F), np.array([3.0, 3.5], F)
    for case in range(256):
        mag = F(0.25) + F(0.125) * np.arange(8, dtype=F)
        values = np.zeros((2, 2, 2), F)
        for i in range(8):
            values[i & 1, (i >> 1) & 1, i >> 2] = -mag[i] if case >> i & 1 else mag[i]
        _, want = mc_both(values, ax, ay, az, (3, 0, 5), 9)
        assert len(want[0]) == bin(int(T["edge_mask"][case])).count("1") and len(want[2]) == int(T["ntri"][case])


def test_marching_cubes_random_lattice_with_zeros_and_nan():
    rng = np.random.default_rng(1704)
    dims = (11, 6, 17)
    values = rng.uniform(-1, 1, dims).astype(F)
    values[rng.random(dims) < 0.05] = 0.0
    values[rng.random(dims) < 0.02] = -0.0
    values[rng.random(dims) < 0.01] = np.nan
    ax, ay, az = (np.sort(rng.uniform(-2, 2, n)).astype(F) for n in dims)
    _, want = mc_both(values, ax, ay, az, (2, 40, 0), 64)
    assert len(want[2]) > 1000


def test_marching_cubes_all_positive_is_empty():
    ax = np.linspace(-1, 1, 5).astype(F)
    for values in (np.ones((5, 5, 5), F), np.zeros((5, 5, 5), F)):
        got, _ = mc_both(values, ax, ax, ax)
        assert tuple(got[0].shape) == (0, 3) and tuple(got[1].shape) == (0,) and tuple(got[2].shape) == (0, 3)


def test_sphere_over_eight_crops_welds_to_a_closed_surface():
    import unbounded_mesh as um
    sphere = lambda p: (np.linalg.norm(p.astype(np.float64) - np.array([0.03, -0.02, 0.05]), axis=1) - 0.6).astype(F)
    want_parts = ur.cropped_marching_cubes(sphere, 1.0, 18, 9)
    axes = ur.crop_axes(1.0, 18, 9)
    parts = []
    for i in range(2):
        for j in range(2):
            for k in range(2):
                values = sphere(ur.lattice_points(axes[i], axes[j], axes[k]))
                parts.append(um.dense_marching_cubes(dev(values), dev(axes[i]), dev(axes[j]), dev(axes[k]), (8 * i, 8 * j, 8 * k), 17))
    for got, want in zip(parts, want_parts):
        assert same_bits(host(got[0]), want[0]) and np.array_equal(host(got[1]), want[1]) and np.array_equal(host(got[2]), want[2])
    v, f = um.weld(parts)
    wv, wf = ur.weld(want_parts)
    assert same_bits(host(v), wv) and np.array_equal(host(f), wf)
    rep = ur.mesh_report(host(v), host(f))
    assert rep["edges_in_two_faces"] and rep["directed_once"] and rep["no_collapsed_face"] and rep["all_vertices_used"]
    assert rep["volume"] > 0 and rep["euler"] == 2
    cat_v, cat_f = ur.concatenate([tuple(host(t) for t in p) for p in parts])
    assert not ur.mesh_report(cat_v, cat_f)["edges_in_two_faces"]       # without the weld the seams are open


# ----------------------------------------------------------------------------- end to end -----------------------------------------------------------------------------
def test_extract_mesh_unbounded_sphere(tmp_path):
    import unbounded_mesh as um
    s = ur.sphere_scene()
    wv, wf, wc, info = ur.sphere_mesh()
    stack = stack_of(s["views"], s["world_view"])
    v, f, c = um.extract_mesh_unbounded(stack, dev(s["xyz"]), resolution=32, crop_resolution=16)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and c.dtype == torch.float32 and v.device == torch.device(DEV)
    assert np.array_equal(host(f), wf) and same_bits(host(v), wv) and same_bits(host(c), wc)
    rep = ur.mesh_report(host(v), host(f))
    assert rep["edges_in_two_faces"] and rep["directed_once"] and rep["volume"] > 0 and rep["euler"] == 2 and len(wf) > 1000
    d = np.abs(np.linalg.norm(host(v).astype(np.float64) - ur.SPHERE_CENTRE, axis=1) - ur.SPHERE_RADIUS)
    assert d.max() < 5 * info["voxel_size"]
    col = np.asarray(ur.COLOUR, F)
    assert (host(c) >= col / 2).all() and (host(c) < col).all()
    again = um.extract_mesh_unbounded(stack, dev(s["xyz"]), resolution=32, crop_resolution=16)
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(again, (v, f, c)))
    # the same through the extractor: the renderer's package is read under this renderer's names
    views = [View(m, w) for (m, _, _), w in zip(s["views"], s["world_view"])]
    maps = {id(view): (dev(d), dev(col_)) for view, (_, d, col_) in zip(views, s["views"])}

    class Gaussians:
        get_xyz = dev(s["xyz"])

    def render(view, gaussians, pipe, bg_color):
        assert gaussians is ex.gaussians and pipe == "pipe" and tuple(bg_color.tolist()) == (0.0, 0.0, 0.0) and bg_color.is_cuda
        return dict(render=maps[id(view)][1], median_depth=maps[id(view)][0][None], mask=None)
    ex = um.GaussianExtractor(Gaussians(), render, "pipe")
    for view in views:
        view.full_proj_transform = view.full_proj_transform.to(DEV)
    ex.reconstruction(views)
    ev, ef, ec = ex.extract_mesh_unbounded(32, 16)
    assert torch.equal(ef, f) and same_bits(host(ev), wv) and same_bits(host(ec), wc)
    path = os.path.join(tmp_path, "mesh.ply")
    ex.write_ply(path, ev, ef, ec)
    assert os.path.getsize(path) > len(wv) * 15 + len(wf) * 13
