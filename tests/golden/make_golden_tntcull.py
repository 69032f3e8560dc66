"""Generates tests/golden/tntcull_point_masks.npz.  Build container only (needs the reference's sources).

The fixture is written by the reference's own code, RUN, not copied: eval_tnt/cull_mesh.py is imported with the modules it needs and this
container lacks (`open3d`, `trimesh`, `pyrender`, `cv2`) stubbed as empty modules, a Mesher is built with its `device` set to "cpu", and
Mesher.point_masks is called on 24 ring cameras, synthetic 29 x 37 depth maps with zero regions and a few hundred points, some behind
cameras and some outside the images.  `mask` is its first return value for all cameras.  `counts` is the sum over the cameras of its second
return value for that camera alone: at forecast_radius 0 that value is the OR over the cameras handed in of exactly the term the loop adds
to its private `valid_num`.

Margins.  float32 summation order inside torch's matmul and its float32 matrix inverse are not part of the specification, so the
generator checks in float64 that no decision can depend on them: for every (point, camera) pair every comparison -- u and v against the
image's edges, z against 0, the sampled depth against 0, z against the sampled depth + eps -- is at least 1e-4 (relative to the
quantity's scale) away from its threshold, also when the sampling position moves by 1e-3 pixel.  Points that fail are redrawn; the
margin is never narrowed.  The exception is the hand-built cases: dyadic points seen by camera 0, whose pose, intrinsics and depth values
are dyadic too, so that every product and sum is exact in any order; they sit exactly ON u == 0, u == W - 1, z == depth + eps (and one
float32 below it) and depth_sample == 0."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_mesheval import save  # noqa: E402

H, W = 29, 37
FX, FY, CX, CY = 32.0, 32.0, 16.0, 16.0          # powers of two: camera 0's projections of the hand-built points are exact
EPS, MIN_VIEWS, RADIUS, VIEWS = 0.005, 20, 4.0, 24
REL = 1e-4
F32 = np.float32


def ring_pose(k):
    """OpenCV camera-to-world pose k of the ring: at RADIUS (cos t, sin t, 0), z towards the origin, y down the world's -z"""
    t = 2 * np.pi * k / VIEWS
    c, s = (round(np.cos(t)), round(np.sin(t))) if k % 6 == 0 else (np.cos(t), np.sin(t))      # the four axis-aligned ones are exact
    r = RADIUS if k % 6 == 0 else RADIUS * (1.0 + 0.05 * np.sin(5.0 * k))
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = [-s, c, 0.0], [0.0, 0.0, -1.0], [-c, -s, 0.0], [r * c, r * s, 0.0]
    return m


def depth_map(k):
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = RADIUS + 0.7 + 0.9 * np.sin(0.4 * j + k) * np.cos(0.3 * i + 0.5 * k)
    d[(i - (6 + k % 11)) ** 2 + (j - (8 + 2 * (k % 9))) ** 2 < 14.0] = 0.0                     # a hole: nothing was rendered there
    d[:, 30 + k % 5:] *= (k % 3 != 0)                                                          # every third map has an empty right edge
    if k == 0:
        d[0:3, 0:3] = 2.0                                                                      # the hand-built cases' plateau ...
        d[3:9, 3:9] = 0.0                                                                      # ... and their hole
    return d.astype(F32)


def dyadic_points():
    """camera-0 coordinates (x_c, y_c, z_c) -> world (RADIUS - z_c, x_c, -y_c); names for the test's report"""
    t = F32(2.0) + F32(EPS)                                                                    # float32(depth + eps) on the plateau
    below = np.nextafter(t, F32(0))
    corner = lambda z: (-float(z) / 2, -float(z) / 2, float(z))                                # projects to u = v = 0 exactly: 32 x + 16 z = 0
    cases = [("u == 0", (-1.0, 0.0, 2.0)), ("u == W - 1", (1.25, 0.0, 2.0)), ("v == 0", (0.25, -1.0, 2.0)), ("v == H - 1", (0.25, 0.75, 2.0)),
             ("u one float32 below 0", (float(np.nextafter(F32(-1.0), F32(-2))), 0.0, 2.0)),
             ("z == depth + eps", corner(t)), ("z one float32 below depth + eps", corner(below)),
             ("depth_sample == 0", (-1.375, -1.375, 4.0))]                                        # pixel (5, 5) of the hole, at z = 4
    names = [c[0] for c in cases]
    cam = np.array([c[1] for c in cases])
    world = np.stack([RADIUS - cam[:, 2], cam[:, 0], -cam[:, 1]], axis=1)
    assert np.array_equal(world.astype(F32).astype(np.float64), world)
    return names, world.astype(F32)


def bilinear(D, u, v):
    x0, y0 = np.clip(np.floor(u), 0, W - 1).astype(int), np.clip(np.floor(v), 0, H - 1).astype(int)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    a, b = np.clip(u, 0, W - 1) - x0, np.clip(v, 0, H - 1) - y0
    return (D[y0, x0] * (1 - a) + D[y0, x1] * a) * (1 - b) + (D[y1, x0] * (1 - a) + D[y1, x1] * a) * b


def unsafe(points, c2w32, depths, skip=None):
    """bool [N]: points with a decision inside the margin for some camera; float64.  skip: (point, camera) pairs left out."""
    p = points.astype(np.float64)
    bad = np.zeros(len(p), bool)
    for k in range(VIEWS):
        w2c = np.linalg.inv(c2w32[k].astype(np.float64))
        cam = p @ w2c[:3, :3].T + w2c[:3, 3]
        z = cam[:, 2] + 1e-8
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = (FX * cam[:, 0] + CX * cam[:, 2]) / z, (FY * cam[:, 1] + CY * cam[:, 2]) / z
        near = np.abs(z) < 1e-3
        tests = [(u, 0.0, REL * (W - 1)), (u, W - 1.0, REL * (W - 1)), (v, 0.0, REL * (H - 1)), (v, H - 1.0, REL * (H - 1))]
        edge = np.zeros(len(p), bool)
        for q, t, m in tests:
            edge |= ~(np.abs(q - t) >= m)                                                       # NaN counts as unsafe
        inside = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z > 0)
        # a point safely behind the camera is out whatever u and v say
        behind = z < -1e-3
        this = (near | edge) & ~behind
        D = depths[k].astype(np.float64)
        for du, dv in ((0, 0), (1e-3, 1e-3), (1e-3, -1e-3), (-1e-3, 1e-3), (-1e-3, -1e-3)):
            s = bilinear(D, np.where(inside, u, 0) + du, np.where(inside, v, 0) + dv)
            zero = s == 0
            if (du, dv) == (0, 0):
                zero0 = zero
            this |= inside & ((zero != zero0) | (~zero & (s < REL * RADIUS)) | (~zero & ~(np.abs(z - (s + EPS)) >= REL * (s + EPS))))
        if skip is not None:
            this &= ~skip[:, k]
        bad |= this
    return bad


def main(seed=43):
    for name in ("open3d", "trimesh", "pyrender", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, os.path.join(REF, "eval_tnt"))
    import torch
    import cull_mesh as reference

    rng = np.random.default_rng(seed)
    c2w32 = np.stack([ring_pose(k) for k in range(VIEWS)]).astype(F32)
    assert np.array_equal(c2w32[0].astype(np.float64), ring_pose(0))
    depths = np.stack([depth_map(k) for k in range(VIEWS)])
    assert all((d == 0).any() and (d > 0).any() for d in depths)

    def draw(n):
        kind = rng.integers(0, 10, n)
        ball = rng.standard_normal((n, 3)) * [0.9, 0.9, 0.6]                                   # around the centre: inside most images
        far = rng.standard_normal((n, 3))
        far = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(4.5, 9.0, (n, 1)) * [1.0, 1.0, 0.25]   # behind some cameras
        high = ball + [0.0, 0.0, 1.0] * rng.choice([-1.0, 1.0], (n, 1)) * rng.uniform(1.5, 3.0, (n, 1))            # above / below the images
        return np.where((kind < 6)[:, None], ball, np.where((kind < 8)[:, None], far, high)).astype(F32)

    names, hand = dyadic_points()
    pts = draw(400)
    for _ in range(200):
        bad = unsafe(pts, c2w32, depths)
        if not bad.any():
            break
        pts[bad] = draw(int(bad.sum()))
    else:
        raise SystemExit("no draw keeps the margins")
    skip = np.zeros((len(hand), VIEWS), bool)
    skip[:, 0] = True                                                                          # exact by construction, on the threshold on purpose
    assert not unsafe(hand, c2w32, depths, skip).any(), "a hand-built point is inside the margin for a camera other than 0"
    points = np.concatenate([hand, pts])
    assert not unsafe(points, c2w32, depths, np.concatenate([skip, np.zeros((len(pts), VIEWS), bool)])).any()

    mesher = reference.Mesher(H, W, FX, FY, CX, CY, 20.0)
    mesher.device = "cpu"
    assert mesher.forecast_radius == 0
    poses = [torch.from_numpy(m.copy()) for m in c2w32]
    maps = [torch.from_numpy(d.copy()) for d in depths]
    mask, _ = mesher.point_masks(torch.from_numpy(points.copy()), maps, poses)
    seen = np.stack([mesher.point_masks(torch.from_numpy(points.copy()), [maps[k]], [poses[k]])[1] for k in range(VIEWS)])
    counts = seen.sum(axis=0).astype(np.int32)
    assert np.array_equal(mask, counts >= MIN_VIEWS) and 0.15 < mask.mean() < 0.85
    n = len(hand)
    print("counts: min", counts.min(), "max", counts.max(), "; kept", int(mask.sum()), "of", len(mask), "; in [18, 21]:", int(((counts >= 18) & (counts <= 21)).sum()))
    print("hand-built, camera 0:", dict(zip(names, seen[0, :n].astype(int))))
    want = dict(zip(names, [1, 1, 1, 1, 0, 0, 1, 1]))
    assert all(int(seen[0, i]) == want[nm] for i, nm in enumerate(names)), "the hand-built cases do not sit where they were built to"
    assert (counts == 0).any() and counts.max() > MIN_VIEWS + 1 and (counts == MIN_VIEWS).any() and (counts == MIN_VIEWS - 1).any()
    save("tntcull_point_masks.npz", points=points, depths=depths, c2w=c2w32, intrinsics=np.array([FX, FY, CX, CY]), eps=np.asarray(EPS),
         min_views=np.asarray(MIN_VIEWS), mask=mask, counts=counts, seen_camera0=seen[0].astype(bool), n_hand=np.asarray(n), hand_names=np.array(names))


if __name__ == "__main__":
    main()
