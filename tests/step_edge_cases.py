"""Seeded case builders and classification helpers for the edge-case tests of the fused step kernels (normals and the consistency
loss, the photometric loss, fused Adam, compute_3D_filter, the 3D-filter activations, 3-NN): test infrastructure, pure numpy, no GPU.

tests/golden/make_golden_step_edges.py runs the reference's own Python on these inputs (tests/golden/step_edges_*.npz),
tests/test_step_edge_cases.py asserts on the CPU every condition a builder promises and pins the numpy oracles to the goldens at these
inputs, tests/test_gpu_step_edges.py runs the HIP kernels on them.

The acceptance form for floating-point comparisons is `rule()`: per class of elements, the kernel must be as accurate as the float32
numpy oracle evaluated on the same float32 inputs, both measured against the float64 oracle."""
import math
from collections import namedtuple

import numpy as np

from oracle import normal_oracle as no

F32_EPS = float(np.finfo(np.float32).eps)


# --------------------------------------------------------------------------------------------------------------- acceptance rule
def _err(x, ref, relative):
    e = np.abs(np.asarray(x, dtype=np.float64) - ref)
    if relative:
        # relative to each element's own reference magnitude; an exactly zero reference admits only exactly zero
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(ref != 0, e / np.abs(ref), np.where(e == 0, 0.0, np.inf))
    return e


def rule(hip, o32, ref64, mask=None, relative=False, kmax=4.0, krms=2.0):
    """max|hip - ref| <= kmax * max|o32 - ref| + tiny and rms likewise with krms, over the class `mask`; tiny is one float32 ulp of the
    class's median magnitude (of 1 when `relative`).  Returns the figures; `ok` is the verdict."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    hip, o32 = np.broadcast_to(np.asarray(hip), ref64.shape), np.broadcast_to(np.asarray(o32), ref64.shape)
    if mask is not None:
        mask = np.broadcast_to(mask, ref64.shape)
        hip, o32, ref64 = hip[mask], o32[mask], ref64[mask]
    hip, o32, ref64 = hip.reshape(-1), o32.reshape(-1), ref64.reshape(-1)
    if ref64.size == 0:
        return dict(n=0, ok=True, ratio_max=0.0, ratio_rms=0.0, max_hip=0.0, max_32=0.0, rms_hip=0.0, rms_32=0.0, tiny=0.0)
    finite = bool(np.isfinite(hip).all())
    eh, e3 = _err(hip, ref64, relative), _err(o32, ref64, relative)
    tiny = F32_EPS if relative else float(np.spacing(np.float32(np.median(np.abs(ref64)))))
    mh, m3 = float(eh.max()), float(e3.max())
    with np.errstate(over="ignore", invalid="ignore"):
        rh, r3 = float(np.sqrt(np.mean(eh * eh))), float(np.sqrt(np.mean(e3 * e3)))
    ok = finite and mh <= kmax * m3 + tiny and rh <= krms * r3 + tiny
    ratio = lambda a, b: 0.0 if a == 0 else (float("inf") if b == 0 else a / b)
    return dict(n=int(ref64.size), ok=bool(ok), ratio_max=ratio(mh, m3), ratio_rms=ratio(rh, r3), max_hip=mh, max_32=m3, rms_hip=rh, rms_32=r3,
                tiny=tiny)


def report(label, r):
    """one line per comparison: the measured ratios go into the test docstrings and DESIGN.md from these"""
    print(f"RULE {label}: n={r['n']} max {r['max_hip']:.3e} vs {r['max_32']:.3e} (x{r['ratio_max']:.3g}) rms {r['rms_hip']:.3e} vs "
          f"{r['rms_32']:.3e} (x{r['ratio_rms']:.3g}) tiny {r['tiny']:.3e} {'ok' if r['ok'] else 'FAIL'}")
    return r["ok"]


# ------------------------------------------------------------------------------------------------------ 1. normals: "holes"
NORMALS_W, NORMALS_H, NORMALS_FOVX = 70, 21, 1.0      # crosses the 64x4 block in both directions
DEPTH_RATIO = 0.6


def fovy_of(W, H, fovx):
    return float(2 * np.arctan(np.tan(fovx / 2) * H / W))


def hole_mask(W=NORMALS_W, H=NORMALS_H):
    y, x = np.mgrid[0:H, 0:W]
    return ((x - 20) ** 2 + (y - 10) ** 2 < 36) | (x > 55) | ((y == 5) & (x > 30) & (x < 50)) | (x == 40)


def normals_holes():
    """depth maps with exact zeros (a disc, a band that touches the border, a one-pixel row segment, a one-pixel column), their
    back-projected point maps with the same holes, and two rendered-normal variants: (a) zero in the holes, (b) non-zero everywhere"""
    W, H, fovx = NORMALS_W, NORMALS_H, NORMALS_FOVX
    fovy = fovy_of(W, H, fovx)
    rng = np.random.default_rng(70021)
    y, x = np.mgrid[0:H, 0:W]
    hole = hole_mask(W, H)
    d1 = (3 + 0.5 * np.sin(x / 5.0) * np.cos(y / 3.0) + 0.05 * rng.standard_normal((H, W))).astype(np.float32)
    d2 = (d1 + np.float32(0.05)).astype(np.float32)
    d2[12:16, 44:52] = 2.5
    d1[hole] = 0.0
    d2[hole] = 0.0
    p1, p2 = no.depths_to_points(d1, d2, W, H, fovx, fovy)
    p1, p2 = p1.astype(np.float32), p2.astype(np.float32)
    p1[:, hole] = 0.0
    p2[:, hole] = 0.0
    rn = rng.standard_normal((3, H, W)).astype(np.float32)
    rn /= np.linalg.norm(rn, axis=0, keepdims=True)
    rn *= (0.3 + 0.7 * rng.random((1, H, W))).astype(np.float32)     # alpha-weighted: not unit length
    rn_a = rn.copy()
    rn_a[:, hole] = 0.0
    cot = rng.standard_normal((2, 3, H, W)).astype(np.float32)
    return dict(W=W, H=H, fovx=fovx, fovy=fovy, hole=hole, depth1=d1.reshape(1, H, W), depth2=d2.reshape(1, H, W), points1=p1, points2=p2,
                rn_a=rn_a, rn_b=rn, cot=cot)


def normals_all_empty():
    W, H, fovx = 65, 5, 1.0
    rng = np.random.default_rng(655)
    rn = rng.standard_normal((3, H, W)).astype(np.float32)
    z1, z3 = np.zeros((1, H, W), np.float32), np.zeros((3, H, W), np.float32)
    return dict(W=W, H=H, fovx=fovx, fovy=fovy_of(W, H, fovx), depth1=z1, depth2=z1.copy(), points1=z3, points2=z3.copy(), rn_b=rn,
                cot=rng.standard_normal((2, 3, H, W)).astype(np.float32))


def normal_maps64(c, points):
    """(2,3,H,W) float64 point maps of a normals case (depth mode: back-projected in float64 from the float32 depths)"""
    if points:
        return np.stack([c["points1"], c["points2"]], 0).astype(np.float64)
    q1, q2 = no.depths_to_points(c["depth1"].astype(np.float64), c["depth2"].astype(np.float64), c["W"], c["H"], c["fovx"], c["fovy"])
    return np.stack([q1, q2], 0)


def cross_lengths(maps):
    """|v| of every interior centre, (2,H-2,W-2), in the dtype of `maps`"""
    _, (_, _, _, n) = no.points_to_normal(maps)
    return n[:, 0]


def degenerate_centres(maps64):
    """(2,H,W) bool: interior centres whose cross product is exactly zero (the `len <= eps` branch)"""
    H, W = maps64.shape[-2:]
    deg = np.zeros((2, H, W), dtype=bool)
    deg[:, 1:-1, 1:-1] = cross_lengths(maps64) <= no.EPS
    return deg


def border_mask(H, W):
    b = np.ones((H, W), dtype=bool)
    b[1:-1, 1:-1] = False
    return b


def eps_touched(deg, cot_nonzero):
    """(2,H,W) bool: pixels of map k one of whose four neighbouring centres is degenerate and carries a non-zero cotangent.
    deg: (2,H,W) from degenerate_centres; cot_nonzero: (H,W) or (2,H,W) bool."""
    src = deg & np.broadcast_to(cot_nonzero, deg.shape)
    t = np.zeros_like(src)
    t[:, 1:, :] |= src[:, :-1, :]
    t[:, :-1, :] |= src[:, 1:, :]
    t[:, :, 1:] |= src[:, :, :-1]
    t[:, :, :-1] |= src[:, :, 1:]
    return t


def normals_reference(c, points, rn, dtype, upstream=1.0):
    """normals, loss and the fused-loss gradients (g_map1, g_map2, g_rendered) of a normals case by oracle/normal_oracle.py in `dtype`"""
    dt = np.dtype(dtype).type
    W, H, fovx, fovy = c["W"], c["H"], c["fovx"], c["fovy"]
    r = rn.astype(dt)
    if points:
        maps = np.stack([c["points1"], c["points2"]], 0).astype(dt)
        nm, _ = no.points_to_normal(maps)
    else:
        d1, d2 = c["depth1"].astype(dt), c["depth2"].astype(dt)
        nm = no.depth_double_to_normal(d1, d2, W, H, fovx, fovy)
    loss = no.consistency_loss(r, nm, DEPTH_RATIO)
    g_r, g_nm = no.consistency_loss_bwd(r, nm, DEPTH_RATIO, upstream)
    g1, g2 = normals_vjp(c, points, g_nm, dtype)
    return dict(normals=nm, loss=float(loss), g1=g1, g2=g2, g_rendered=g_r)


def normals_vjp(c, points, cot, dtype):
    """d<cot, normals>/d(map1, map2) by the oracle in `dtype`; cot: (2,3,H,W)"""
    dt = np.dtype(dtype).type
    W, H, fovx, fovy = c["W"], c["H"], c["fovx"], c["fovy"]
    if points:
        gp = no.points_to_normal_bwd(np.stack([c["points1"], c["points2"]], 0).astype(dt), cot.astype(dt))
        return gp[0], gp[1]
    return no.depth_double_to_normal_bwd(c["depth1"].astype(dt), c["depth2"].astype(dt), W, H, fovx, fovy, cot.astype(dt))


# ---------------------------------------------------------------------------------------------------- 2. photometric: "masked"
PHOTO_W, PHOTO_H = 131, 37           # three column tiles with a ragged last one, three row tiles


def photometric_masked(C):
    H, W = PHOTO_H, PHOTO_W
    rng = np.random.default_rng(13137 + C)
    y, x = np.mgrid[0:H, 0:W]
    gt = np.stack([0.5 + 0.4 * np.sin(x / 9.0 + c) * np.cos(y / 7.0 - c) for c in range(C)], 0).astype(np.float32)
    img = np.clip(gt + 0.1 * rng.standard_normal((C, H, W)), 0, 1).astype(np.float32)
    gt[:, :, :40] = 0.0
    img[:, :, :40] = 0.0
    gt[:, :, 96:] = 1.0
    img[:, :, 96:] = 1.0
    img[:, 26:, 40:96] = gt[:, 26:, 40:96]
    img[:, 10:14, 50:60] = 1.7           # renders are not clipped
    return img, gt


# ------------------------------------------------------------------------------------------------------------- 3. fused Adam
def adam_step32(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-15):
    """One step of radegs_adam.hip restated operation by operation in numpy float32 (the unit is built without fma contraction and with
    IEEE divide and sqrt, the host scalars are doubles rounded once): bit-exact.  oracle/adam_oracle.step on float32 arrays, but
    `lr` enters as float32(lr) widened to double before the division by bc1 (RadegsAdamTensor.lr is a float) and eps is cast to float32."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    omb1, b2, omb2, epsf = f(1.0 - beta1), f(beta2), f(1.0 - beta2), f(eps)
    bc1, bc2 = 1.0 - math.pow(beta1, float(t)), 1.0 - math.pow(beta2, float(t))
    step_size, bc2_sqrt = f(float(f(lr)) / bc1), f(math.sqrt(bc2))
    m = m + omb1 * (g - m)
    v = v * b2 + omb2 * (g * g)
    denom = np.sqrt(v) / bc2_sqrt + epsf
    return p - step_size * (m / denom), m, v


ADAM_NUMELS = (1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 2048 * 3 + 1)
# float offsets of (param, grad, exp_avg, exp_avg_sq) from a 16-byte boundary
ADAM_OFFSETS = ((0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0), (0, 0, 2, 0), (0, 0, 0, 3), (1, 1, 1, 1), (2, 3, 1, 0), (3, 2, 0, 1), (0, 2, 0, 0),
                (3, 3, 3, 3), (1, 2, 3, 0), (0, 0, 0, 0))
AdamTensor = namedtuple("AdamTensor", "name group numel offsets has_grad lr")
ADAM_GROUPS = (dict(betas=(0.9, 0.999), eps=1e-15), dict(betas=(0.8, 0.99), eps=1e-8))


def adam_layout():
    """20 tensors: 18 in the first group (17 with a gradient: two launches of the 16-tensor table), 2 in a second group with its own
    betas and eps.  One tensor has numel 0, one has no gradient."""
    lrs = (1.6e-4, 2.5e-3, 2.5e-3 / 20, 0.05, 0.005, 0.001)
    out = []
    for j, (n, off) in enumerate(zip(ADAM_NUMELS, ADAM_OFFSETS)):
        out.append(AdamTensor(f"n{n}", 0, n, off, True, lrs[j % 6]))
    out.insert(6, AdamTensor("empty", 0, 0, (0, 0, 0, 0), True, 0.01))
    out.insert(9, AdamTensor("nograd", 0, 1500, (1, 0, 2, 3), False, 0.01))
    for j, off in enumerate(((0, 0, 0, 0), (0, 1, 0, 0), (2, 0, 0, 0), (0, 0, 1, 2))):
        out.append(AdamTensor(f"off{j}", 0, 1025 + j, off, True, lrs[j]))
    out.append(AdamTensor("g2_aligned", 1, 3000, (0, 0, 0, 0), True, 0.02))
    out.append(AdamTensor("g2_ragged", 1, 2051, (3, 0, 1, 0), True, 0.003))
    return out


def adam_data(t, phase):
    """(p, g, m, v) float32 of tensor `t` for phase 0 (fresh state, steps 1 and 2 follow) or phase 1 (state of a long run, step 1000).
    Gradients span six decades; a stretch of exactly zero gradients sits on v == 0 (the eps regime: m / (0 + eps))."""
    rng = np.random.default_rng([t.numel, phase, sum(ord(ch) for ch in t.name)])
    n = t.numel
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
    if phase == 0:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
        v = np.square(rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
    z = slice(n // 3, n // 3 + max(1, n // 8))
    g[z] = 0.0
    if phase == 1:
        v[z] = 0.0
        m[z] = (1e-18 * rng.standard_normal(n)).astype(np.float32)[z]
    return p, g, m, v


def adam_second_grad(t):
    rng = np.random.default_rng([t.numel, 7, sum(ord(ch) for ch in t.name)])
    g = (rng.standard_normal(t.numel) * 10.0 ** rng.uniform(-6, 0, t.numel)).astype(np.float32)
    g[t.numel // 3: t.numel // 3 + max(1, t.numel // 8)] = 0.0       # stays zero: m == 0 and v == 0 after two steps
    return g


# ------------------------------------------------------------------------------------------------------ 4. compute_3D_filter
Cam = namedtuple("Cam", "R T image_width image_height FoVx FoVy")
AMBIGUOUS = 1e-5
FILTER_SCALE = 0.2 ** 0.5


def cameras_from_rows(rows):
    return [Cam(r[:9].reshape(3, 3), r[9:12], int(r[12]), int(r[13]), float(r[14]), float(r[15])) for r in rows]


def cameras_cycled(cams, n=150):
    return [cams[i % len(cams)]._replace(T=cams[i % len(cams)].T + 0.01 * i) for i in range(n)]


def filter_random_xyz(P=20000):
    return (np.random.default_rng(2).standard_normal((P, 3)) * 3.0).astype(np.float32)


def filter_analysis(xyz, cameras):
    """Float64 evaluation of compute_3D_filter on the float32 inputs the kernel sees (xyz, R, T, fx, fy as float32), with the margin of
    every validity test.  Returns a dict:
      ref (P,) float64 filter; seen (P,) bool; ambiguous (P,) bool (smallest margin over all cameras below 1e-5);
      zmin_sure / zmin_maybe (P,): the smallest depth over the cameras that certainly / possibly see the point (inf if none);
      max_seen: the largest distance over seen points (0 if none), argmax: its row (-1 if none)."""
    x64 = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    P = x64.shape[0]
    zmin = np.full(P, np.inf)
    zmin_sure, zmin_maybe = np.full(P, np.inf), np.full(P, np.inf)
    margin = np.full(P, np.inf)
    focal = 0.0
    amax = np.abs(x64).max(axis=1) if P else np.zeros(0)
    for cam in cameras:
        W, H = cam.image_width, cam.image_height
        fx, fy = W / (2 * math.tan(cam.FoVx / 2.)), H / (2 * math.tan(cam.FoVy / 2.))
        focal = max(focal, fx)
        R = np.asarray(cam.R, dtype=np.float32).astype(np.float64)
        T = np.asarray(cam.T, dtype=np.float32).astype(np.float64)
        pc = x64 @ R + T[None]
        z0 = pc[:, 2]
        z = np.maximum(z0, float(np.float32(0.001)))
        px = pc[:, 0] / z * float(np.float32(fx)) + W / 2.0
        py = pc[:, 1] / z * float(np.float32(fy)) + H / 2.0
        near = float(np.float32(0.2))                       # the comparison is made in float32: the threshold is 0.2f
        m_d = np.abs(z0 - near) / (amax + np.abs(T).max() + 1)
        m_x = np.minimum(np.abs(px + 0.15 * W), np.abs(px - 1.15 * W)) / (np.abs(px) + W)
        m_y = np.minimum(np.abs(py + 0.15 * H), np.abs(py - 1.15 * H)) / (np.abs(py) + H)
        margin = np.minimum(margin, np.minimum(m_d, np.minimum(m_x, m_y)))
        tests = ((z0 > near, m_d), ((px >= -0.15 * W) & (px <= 1.15 * W), m_x), ((py >= -0.15 * H) & (py <= 1.15 * H), m_y))
        valid = tests[0][0] & tests[1][0] & tests[2][0]
        sure = np.ones(P, dtype=bool)
        maybe = np.ones(P, dtype=bool)
        for ok, m in tests:
            sure &= ok & (m >= AMBIGUOUS)
            maybe &= ok | (m < AMBIGUOUS)
        zmin = np.where(valid, np.minimum(zmin, z), zmin)
        zmin_sure = np.where(sure, np.minimum(zmin_sure, z), zmin_sure)
        zmin_maybe = np.where(maybe, np.minimum(zmin_maybe, z), zmin_maybe)
    seen = np.isfinite(zmin)
    dist = np.minimum(zmin, 100000.0)
    max_seen = float(dist[seen].max()) if seen.any() else 0.0
    argmax = int(np.flatnonzero(seen)[np.argmax(dist[seen])]) if seen.any() else -1
    dist = np.where(seen, dist, max_seen)
    k = FILTER_SCALE / float(np.float32(focal))
    return dict(ref=dist * k, seen=seen, ambiguous=margin < AMBIGUOUS, zmin_sure=zmin_sure, zmin_maybe=zmin_maybe, max_seen=max_seen,
                argmax=argmax, k=k)


def filter_candidates(an, i):
    """the values an ambiguous point may take: every validity test of it decided one way or the other"""
    lo, hi = an["zmin_maybe"][i], an["zmin_sure"][i]
    vals = [min(z, 100000.0) if np.isfinite(z) else an["max_seen"] for z in (lo, hi)]
    return [v * an["k"] for v in vals]


EXACT_NEAR_ROW = 100


def filter_scene_one_seen(P=300, row=200):
    """an identity camera; every point behind it but one, and one exactly on the near threshold (not seen)"""
    rng = np.random.default_rng(300)
    xyz = rng.standard_normal((P, 3)).astype(np.float32)
    xyz[:, 2] = -1.0 - np.abs(xyz[:, 2])
    xyz[row] = (0.25, -0.5, 5.0)
    xyz[EXACT_NEAR_ROW] = (0.0, 0.0, np.float32(0.2))      # view z == 0.2f exactly under the identity camera: `z > 0.2` is false
    cams = [Cam(np.eye(3), np.zeros(3), 100, 80, 1.0, 0.8), Cam(np.eye(3), np.array([0.0, 0.0, -0.5]), 64, 64, 0.9, 0.9)]
    return xyz, cams


def filter_scene_none_seen(P=300):
    xyz, cams = filter_scene_one_seen(P)
    xyz[200, 2] = -5.0
    return xyz, cams


# ------------------------------------------------------------------------------------------------- 4b. 3D-filter activations
ACT_CLASSES = ("plain", "filter0", "filter_big", "op_hi", "op_lo")


def activation_case(P=257):
    """rows cycle through: plain; filter exactly 0 (coefficient exactly 1); filter 100 times the largest scale; opacity raw +30; -30.
    Raw scales stay in [-9, 3] so that no product underflows."""
    rng = np.random.default_rng(257)
    n = 257
    sc = rng.uniform(-9, 3, (n, 3)).astype(np.float32)
    op = (2 * rng.standard_normal((n, 1))).astype(np.float32)
    f3 = (np.exp(sc.astype(np.float64)).mean(1, keepdims=True) * rng.uniform(0.2, 2, (n, 1))).astype(np.float32)
    cls = np.arange(n) % 5
    f3[cls == 1] = 0.0
    f3[cls == 2] = (100.0 * np.exp(sc[cls == 2].astype(np.float64)).max(1, keepdims=True)).astype(np.float32)
    op[cls == 3] = 30.0
    op[cls == 4] = -30.0
    cs, co = rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, 1)).astype(np.float32)
    return dict(scaling_raw=sc[:P], opacity_raw=op[:P], filter_3D=f3[:P], cot_scales=cs[:P], cot_opacity=co[:P], cls=cls[:P])


def activation_zero_over_zero(P=16):
    """raw scales of -30 with filter 0: s^2 = 8.8e-27, the product of three underflows, the reference's float32 expression is 0/0"""
    rng = np.random.default_rng(16)
    return dict(scaling_raw=np.full((P, 3), -30.0, np.float32), opacity_raw=rng.standard_normal((P, 1)).astype(np.float32),
                filter_3D=np.zeros((P, 1), np.float32), cot_scales=rng.standard_normal((P, 3)).astype(np.float32),
                cot_opacity=rng.standard_normal((P, 1)).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ 5. 3-NN
KNN_UNIFORM_P = (4, 5, 7, 63, 64, 65, 1023, 1024, 1025, 2049)      # kBox = 1024


def knn_uniform(P):
    return np.random.default_rng(9000 + P).random((P, 3)).astype(np.float32)


def knn_identical(P=300):
    return np.tile(np.array([[0.3, -1.25, 2.0]], np.float32), (P, 1))


def knn_line(P=700):
    pts = np.zeros((P, 3), np.float32)
    pts[:, 0], pts[:, 2] = 0.5, -2.0
    pts[:, 1] = np.random.default_rng(71).random(P).astype(np.float32)
    return pts


def knn_plane(P=1500):
    pts = np.random.default_rng(72).random((P, 3)).astype(np.float32)
    pts[:, 2] = 1.5
    return pts


def knn_duplicates():
    """2500 copies of one point (the run straddles three boxes of 1024), 500 distinct points within 1e-3 of it, 1000 far points"""
    rng = np.random.default_rng(73)
    c = np.array([0.5, 0.25, -0.75], np.float32)
    near = (c + rng.uniform(-1e-3, 1e-3, (500, 3))).astype(np.float32)
    far = (c + rng.uniform(1.0, 3.0, (1000, 3)) * rng.choice([-1.0, 1.0], (1000, 3))).astype(np.float32)
    pts = np.concatenate([np.tile(c[None], (2500, 1)), near, far], 0)
    perm = rng.permutation(len(pts))
    return pts[perm], (perm < 2500)


def knn_lattice(n=10, h=0.125):
    """n^3 lattice with spacing 1/8: exact in float32, many tied distances; interior points give exactly 1/64"""
    g = np.arange(n, dtype=np.float32) * np.float32(h)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    idx = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)
    interior = ((idx > 0) & (idx < n - 1)).all(1)
    perm = np.random.default_rng(74).permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), interior[perm]
