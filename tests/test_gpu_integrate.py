"""GPU parity of GaussianRasterizer.integrate against the oracle: exact indices (radii, num_rendered,
per-pixel last contributor, per-pixel point counts, projected coordinates), images / integrated opacities / sdf within
1e-5 abs / 1e-4 rel."""
import numpy as np
import pytest
import torch

from synth_scene import make_scene
from util import close, oracle_for

pytestmark = pytest.mark.gpu


def _points(s, n, seed, spread=0.05, far=0):
    rng = np.random.default_rng(seed)
    P = s.means3D.shape[0]
    pts = s.means3D.numpy()[rng.integers(0, P, n)] + rng.normal(size=(n, 3)).astype(np.float32) * np.float32(spread)
    if far:
        pts = np.concatenate([pts, rng.normal(size=(far, 3)).astype(np.float32) * 40.0])
    return np.ascontiguousarray(pts, dtype=np.float32)


def _run(s, pts, debug=False):
    import diff_gaussian_rasterization._C as C
    from diff_gaussian_rasterization import GaussianRasterizer
    from gpu_util import settings_for
    from synth_scene import to_device
    assert torch.cuda.is_available(), "these tests need the MI355X box"
    dev = torch.device("cuda:0")
    d = to_device(s, dev)
    r = GaussianRasterizer(settings_for(s, dev, debug))
    p = torch.from_numpy(pts).to(dev)
    out = r.integrate(p, d.means3D, torch.zeros_like(d.means3D), d.opacities, shs=d.shs, scales=d.scales, rotations=d.rotations)
    rs = r.raster_settings
    e = torch.Tensor([])
    st = C.integrate_gaussians_to_points(rs.bg, p, d.means3D, e, d.opacities, d.scales, d.rotations, 1.0, e, e, rs.viewmatrix,
                                         rs.projmatrix, rs.tanfovx, rs.tanfovy, 0.0, None, s.H, s.W, d.shs, s.sh_degree, rs.campos,
                                         False, debug)
    torch.cuda.synchronize()
    # the wrapper and the native entry agree, and two runs are bit-identical (no atomics on the value path)
    for a, b in zip(out, st[1:7]):
        assert torch.equal(a, b)
    P = s.means3D.shape[0]
    nc = None
    if st[9].numel():  # the state buffers stay empty when nothing was launched (P == 0 or PN == 0)
        nc = C.debug_export("n_contrib", torch.int32, 2 * s.H * s.W, P, st[0], s.W, s.H, False, st[7], st[8], st[9]).cpu().numpy()
        nc = nc.view(np.uint32)
    return st[0], [t.cpu().numpy() for t in out], nc


# kUsedBatches * 64 (csrc/rg_integrate.inc): a tile list this long still has every used bit of phase 1 in LDS, so its four strips take
# the point-major (cached) phase 2; a longer one makes them replay the 5-sample test per pixel
BITS_REACH = 12 * 64


def strips(o, ref, s):
    """Per 16x4 pixel strip (one wave of integrate_kernel), from the oracle: the length of its tile's list, the number of query points in
    the strip and in its fullest pixel."""
    gx, gy = (s.W + 15) // 16, (s.H + 15) // 16
    rg = o.get("ranges")[: 2 * gx * gy].reshape(gy, gx, 2).astype(np.int64)
    per_pixel = np.zeros((gy * 16, gx * 16), np.int64)
    per_pixel[: s.H, : s.W] = ref[0][8]
    per_pixel = per_pixel.reshape(gy * 4, 4, gx, 16)
    return np.repeat(rg[..., 1] - rg[..., 0], 4, axis=0), per_pixel.sum(axis=(1, 3)), per_pixel.max(axis=(1, 3))


def check(s, pts, min_projected=1, path=None):
    """path(*strips(...)): the test's precondition on the phase-2 form its scene reaches, asserted first"""
    assert s.kernel_size == 0.0  # the operator hard-codes kernel_size 0.0 for integrate (upstream __init__.py:283)
    o = oracle_for(s)
    ref = o.integrate(pts)
    if path:
        path(*strips(o, ref, s))
    R, got, nc = _run(s, pts)
    H, W = s.H, s.W
    assert R == o.num_rendered, "num_rendered"
    assert np.array_equal(got[5], ref[5]), "radii"
    assert np.array_equal(nc[: H * W], o.get("n_contrib")[: H * W]), "last contributor"
    assert np.array_equal(got[3].view(np.uint32), ref[3].view(np.uint32)), "projected coordinates (bit-exact)"
    assert np.array_equal(got[0][8], ref[0][8]), "points per pixel"
    proj = ref[3].any(axis=1)
    assert proj.sum() >= min_projected
    names = ["color9", "alpha_integrated", "color_integrated", "coordinate2d", "sdf"]
    for k in (0, 1, 2, 4):
        assert not np.isnan(got[k]).any(), names[k]
        assert close(got[k], ref[k]).all(), f"{names[k]}: max abs diff {np.abs(got[k] - ref[k]).max():.3e}"
    return o, got


def all_cached(length, pts, pixel_max):
    assert length.max() <= BITS_REACH, length.max()


def some_replay(length, pts, pixel_max):
    assert length.max() > BITS_REACH, length.max()


def test_integrate_random_scene():
    s = make_scene(6000, 200, 152, sh_degree=2, mu_px=4.0, seed=31, kernel_size=0.0, pose="random", require_coord=False, require_depth=True)
    o, got = check(s, _points(s, 20000, 1, far=500), min_projected=5000, path=all_cached)
    a = got[1]
    assert ((a >= 0) & (a <= 1)).all() and (a < 0.5).sum() > 100 and (a > 0.9).sum() > 100


def test_integrate_many_points_per_pixel_and_heavy_overdraw():
    # 64x48 image, 30k points -> ~10 per pixel: several 4-point passes per lane; large splats -> long tile lists
    s = make_scene(1500, 64, 48, sh_degree=0, mu_px=12.0, seed=32, kernel_size=0.0, pose="random", require_coord=False,
                   require_depth=True, low_opacity=True)
    o, got = check(s, _points(s, 30000, 2, spread=0.3), min_projected=10000, path=some_replay)
    assert got[0][8].max() > 8


@pytest.mark.parametrize("P,W,H,n,replay", [(3000, 128, 96, 40000, False), (2500, 96, 64, 25000, True)], ids=["cached", "cached_and_replay"])
def test_integrate_strips_of_more_than_64_points(P, W, H, n, replay):
    """A cached strip deals its query points to the lanes 64 at a time: here every cached strip needs several deals (up to five in the
    first scene), and in the second scene some tiles replay with up to five passes of four points per pixel next to cached ones."""
    s = make_scene(P, W, H, sh_degree=0, mu_px=3.0, seed=41, kernel_size=0.0, pose="random", require_coord=False, require_depth=True)

    def path(length, pts, pixel_max):
        cached = length <= BITS_REACH
        assert cached.any() and (pts[cached] > 64).any(), "no cached strip with a second deal"
        assert replay == (~cached).any(), length.max()
        if replay:
            assert pixel_max[~cached].max() > 4, "no replayed pixel with a second pass"   # kPointsPerPass

    check(s, _points(s, n, 9), path=path)


def test_integrate_ill_conditioned_gaussians():
    from test_hostcheck import _flat_scene
    s = _flat_scene(make_scene(3000, 160, 120, sh_degree=1, mu_px=3.0, seed=33, kernel_size=0.0, pose="random", require_coord=False,
                               require_depth=True), frac=0.4, seed=4)
    o, got = check(s, _points(s, 15000, 3), min_projected=3000)
    assert (o.get("condition")[o.get("radii") > 0] == 0).sum() > 100


def test_integrate_partial_tiles_and_identity_pose():
    s = make_scene(2000, 100, 70, sh_degree=3, mu_px=2.0, seed=34, kernel_size=0.0, pose="identity", require_coord=False, require_depth=True)
    check(s, _points(s, 8000, 4, far=100), min_projected=2000)


def test_integrate_empty_inputs():
    s = make_scene(500, 64, 48, sh_degree=0, mu_px=3.0, seed=35, kernel_size=0.0, require_coord=False, require_depth=True)
    pts = _points(s, 100, 5)
    # no points: image stays zero (the reference returns before launching anything, rasterize_points.cu:330)
    R, got, _ = _run(s, pts[:0])
    assert R == 0 and (got[0] == 0).all() and got[1].shape == (0,)
    # no Gaussians: initial point values
    s0 = s._replace(means3D=s.means3D[:0], opacities=s.opacities[:0], scales=s.scales[:0], rotations=s.rotations[:0], shs=s.shs[:0])
    R, got, _ = _run(s0, pts)
    assert R == 0 and (got[0] == 0).all() and (got[1] == 1).all() and (got[4] == -1000).all() and (got[2] == 0).all()
    # all points behind the camera / outside the image
    far = np.float32(-1.0) * np.abs(pts) - np.float32(50.0)
    o = oracle_for(s)
    ref = o.integrate(far)
    R, got, _ = _run(s, far)
    assert R == o.num_rendered and (got[1] == 1).all() and (got[4] == -1000).all()
    assert close(got[0], ref[0]).all()


def test_integrate_debug_mode_and_determinism(monkeypatch):
    """Debug mode (a sync after every launch), the exact binning and a speculative one whose forced prediction is far too small (the
    integrate is redone with exact sizes) all give the same result."""
    import diff_gaussian_rasterization._C as C
    s = make_scene(3000, 128, 96, sh_degree=1, mu_px=4.0, seed=36, kernel_size=0.0, pose="random", require_coord=False, require_depth=True)
    pts = _points(s, 10000, 6)
    R1, a, _ = _run(s, pts, debug=True)
    R2, b, _ = _run(s, pts)
    assert R1 == R2
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    runs = []
    for env in (dict(RADEGS_SPECULATE="0"), dict(RADEGS_SPECULATE="1", RADEGS_SPECULATE_HINT="1000")):   # R1 is ~30 000
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        C.reload_env()
        C.binning_stats(reset=True)
        runs.append(_run(s, pts)[:2])
        stats = C.binning_stats()
    assert stats == (2, 2), stats   # both integrate calls of _run were speculative and redone
    assert runs[0][0] == runs[1][0] == R1
    for x, y in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(x, y, equal_nan=True)


def test_integrate_C2_full_size():
    """The benchmark scene (1M Gaussians, 1920x1080) with 2M query points scattered around the Gaussians."""
    from synth_scene import make_config
    s = make_config("C2", kernel_size=0.0)
    P = s.means3D.shape[0]
    rng = np.random.default_rng(7)
    pts = s.means3D.numpy()[:, None, :] + rng.normal(size=(P, 2, 3)).astype(np.float32) * 1.5 * s.scales.numpy().max(1)[:, None, None]
    o, got = check(s, np.ascontiguousarray(pts.reshape(-1, 3), dtype=np.float32), min_projected=1_000_000)
    # size-independent properties: every projected point is counted once; integrated opacity never exceeds 1
    assert got[0][8].sum() == (got[3].any(axis=1)).sum()
    assert (got[1] <= 1.0 + 1e-6).all() and (got[1] >= 0).all()


import os  # noqa: E402

_ISPEC = os.environ.get("RADEGS_FUZZ_SEEDS", "0:6")
_ISEEDS = [int(v) for v in _ISPEC.split(",")] if "," in _ISPEC else list(range(*(int(v) for v in _ISPEC.split(":"))))


@pytest.mark.parametrize("seed", _ISEEDS)
def test_integrate_random_configuration(seed):
    """Randomised sweep of integrate(): image shapes off the tile grid, densities from empty pixels to heavy overdraw, SH degree,
    pose, opacity regime, background, point clouds from sparse to ~10 per pixel, some points outside the frustum."""
    r = np.random.default_rng(3000 + seed)
    mu = float(r.choice([0.7, 1.5, 4.0, 12.0]))
    P = int(r.integers(200, 6000)) if mu < 12 else int(r.integers(200, 1500))
    W, H = int(r.integers(33, 300)), int(r.integers(17, 220))
    s = make_scene(P, W, H, sh_degree=int(r.integers(0, 4)), mu_px=mu, seed=int(r.integers(0, 10_000)), kernel_size=0.0,
                   pose=str(r.choice(["identity", "random"])), require_coord=False, require_depth=True, low_opacity=bool(r.integers(0, 2)),
                   bg=tuple(float(v) for v in r.random(3)) if r.integers(0, 2) else (0.0, 0.0, 0.0), fovx_deg=float(r.choice([40.0, 60.0, 95.0])),
                   near_cull_frac=float(r.choice([0.0, 0.02, 0.3])))
    n = int(r.choice([50, 2000, 10 * W * H]))
    check(s, _points(s, n, seed, spread=float(r.choice([0.02, 0.3])), far=int(r.integers(0, 200))), min_projected=1)
