"""NumPy float32 restatement of unbounded mesh extraction as this library specifies it (include/radegs.h, "Unbounded mesh extraction";
DESIGN 11 N17), written from that text and not from the kernels: the contraction, the per-sample truncation, the per-view projection,
bilinear gather and running average, the dense marching cubes, the crops and their weld -- every float32 operation in the order the
specification gives (numpy multiplies, then adds; no fused multiply-add).  It is the arbiter of tests/test_gpu_unbounded.py, and
tests/test_unbounded_restatement.py checks it against the reference's own run (tests/golden/unbounded_*.npz) and against properties that
do not depend on it.  Also the common scene of those tests: a sphere seen by eight cameras, analytic depth, constant colour."""
import math

import numpy as np

from tsdf_restatement import mesh_report, tables  # noqa: F401  (the table of N9 and the mesh properties, shared)

F = np.float32


# ---------------------------------------------------------------------- host helpers (float64) ----------------------------------------------------------------------
def focus_point(poses):
    """the point nearest to all optical axes of camera-to-world poses [n,3,4] (column 2: the axis, column 3: the origin)"""
    poses = np.asarray(poses, np.float64)
    d, o = poses[:, :3, 2:3], poses[:, :3, 3:4]
    m = np.eye(3) - d * np.transpose(d, [0, 2, 1])
    mt_m = np.transpose(m, [0, 2, 1]) @ m
    return np.linalg.inv(mt_m.mean(0)) @ (mt_m @ o).mean(0)[:, 0]


def scene_normalisation(world_view_transforms):
    """(center float64 [3], radius float64) of row-vector world-to-view matrices [n,4,4]; the inverse in the matrices' own type, as upstream"""
    c2w = np.array([np.linalg.inv(np.asarray(m).T) for m in world_view_transforms])
    center = focus_point(c2w[:, :3, :] @ np.diag([1.0, -1.0, -1.0, 1.0]))
    return center, np.linalg.norm(c2w[:, :3, 3] - center, axis=-1).min()


def contract_f32(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        mag = np.sqrt((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])[..., None]
        return np.where(mag < 1, x, (F(2) - F(1) / mag) * (x / mag)).astype(F)


def contracted_bound(xyz, center, radius):
    """R: the 0.95 quantile of the contracted norms of the normalised points (float32, as upstream computes them), plus 0.01, at most 1.9"""
    x = (np.asarray(xyz, F) - np.asarray(center, np.float64).astype(F)) / F(radius)
    c = contract_f32(x)
    n = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    return min(np.quantile(n, q=0.95) + 0.01, 1.9)


# --------------------------------------------------------------------------- the fuse ---------------------------------------------------------------------------
def uncontract(y, radius, center):
    """contracted y [M,3] float32 -> world x [M,3] float32"""
    y = np.asarray(y, F)
    r, c = F(radius), np.asarray(center, F)
    with np.errstate(all="ignore"):
        mag = np.sqrt((y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2])
        inv = F(1) / (F(2) - mag)
        x = np.stack([np.where(mag < 1, y[:, k], inv * (y[:, k] / mag)) for k in range(3)], -1).astype(F)
        return (x * r + c[None]).astype(F)


def truncation(x, trunc5):
    """per-sample truncation of world points x [M,3]: trunc5, divided by 2 - min(|x|, 1.9) where |x| > 1"""
    t5 = F(trunc5)
    with np.errstate(all="ignore"):
        n = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        return np.where(n > 1, t5 * (F(1) / (F(2) - np.minimum(n, F(1.9)))), t5).astype(F)


def _gather(img, ix, iy, ok):
    """bilinear, align_corners, border: img [H,W] float32, ix / iy the clamped pixel coordinates; lanes outside `ok` return 0"""
    H, W = img.shape
    x0f, y0f = np.floor(ix), np.floor(iy)
    x0, y0 = np.where(ok, x0f, 0).astype(np.int64), np.where(ok, y0f, 0).astype(np.int64)
    x1f, y1f = x0f + F(1), y0f + F(1)
    nw, ne, sw, se = (x1f - ix) * (y1f - iy), (ix - x0f) * (y1f - iy), (x1f - ix) * (iy - y0f), (ix - x0f) * (iy - y0f)
    x1, y1 = x0 + 1, y0 + 1
    xin, yin = x1 < W, y1 < H
    x1c, y1c = np.minimum(x1, W - 1), np.minimum(y1, H - 1)
    out = np.zeros(ix.shape, F)
    out = out + img[y0, x0] * nw
    out = np.where(xin, out + img[y0, x1c] * ne, out)
    out = np.where(yin, out + img[y1c, x0] * sw, out)
    out = np.where(xin & yin, out + img[y1c, x1c] * se, out)
    return np.where(ok, out, F(0)).astype(F)


def fuse(samples, views, voxel_size, center, radius, contract=True, return_rgb=False):
    """samples float32 [M,3]; views: [(full_proj_transform [4,4] row-vector convention, depth [H,W], rgb [3,H,W] or None)] ->
    tsdf [M] (and rgb [M,3]).  voxel_size is a host number: trunc5 = float32(5 voxel_size)."""
    y = np.asarray(samples, F).reshape(-1, 3)
    trunc5 = F(5.0 * float(voxel_size))
    if contract:
        x = uncontract(y, radius, center)
        trunc = truncation(x, trunc5)
    else:
        x, trunc = y, np.full(len(y), trunc5, F)
    M = len(x)
    tsdf, w, rgb = np.ones(M, F), np.ones(M, F), np.zeros((M, 3), F)
    with np.errstate(all="ignore"):
        for m, depth, colour in views:
            m, depth = np.asarray(m, F), np.asarray(depth, F)
            H, W = depth.shape
            q = [((x[:, 0] * m[0, c] + x[:, 1] * m[1, c]) + x[:, 2] * m[2, c]) + m[3, c] for c in (0, 1, 3)]
            z = q[2]
            px, py = q[0] / z, q[1] / z
            inview = (px > -1) & (px < 1) & (py > -1) & (py < 1) & (z > 0)
            ix = np.minimum(np.maximum(((px + F(1)) / F(2)) * F(W - 1), F(0)), F(W - 1))
            iy = np.minimum(np.maximum(((py + F(1)) / F(2)) * F(H - 1), F(0)), F(H - 1))
            ix, iy = np.where(inview, ix, F(0)), np.where(inview, iy, F(0))
            sdf = _gather(depth, ix, iy, inview) - z
            ok = inview & (sdf > -trunc)
            s = np.minimum(np.maximum(sdf / trunc, F(-1)), F(1))
            wp = w + F(1)
            tsdf = np.where(ok, (tsdf * w + s) / wp, tsdf)
            if return_rgb and colour is not None:
                colour = np.asarray(colour, F)
                for c in range(3):
                    rgb[:, c] = np.where(ok, (rgb[:, c] * w + _gather(colour[c], ix, iy, inview)) / wp, rgb[:, c])
            w = np.where(ok, wp, w)
    return (tsdf.astype(F), rgb) if return_rgb else tsdf.astype(F)


def lattice_points(ax, ay, az):
    """the samples of a lattice in its canonical order: index (lx * ny + ly) * nz + lz"""
    xx, yy, zz = np.meshgrid(np.asarray(ax, F), np.asarray(ay, F), np.asarray(az, F), indexing="ij")
    return np.stack([xx.ravel(), yy.ravel(), zz.ravel()], -1)


def world_points(y, radius, center, max_range):
    """after the weld: uncontract, then clamp to +-max_range (NaN stays NaN)"""
    x = uncontract(y, radius, center)
    r = F(max_range)
    return np.where(x < -r, -r, np.where(x > r, r, x)).astype(F)


# ------------------------------------------------------------------- dense marching cubes -------------------------------------------------------------------
def dense_marching_cubes(values, ax, ay, az, lattice_offset=(0, 0, 0), G=None):
    """values [nx,ny,nz] float32 over the lattice ax x ay x az -> vertices float32 [V,3] (in lattice-point, axis order), keys int64 [V],
    faces int64 [F,3] (in cell, table order; indices into these vertices)"""
    T = tables()
    ax, ay, az = (np.asarray(a, F) for a in (ax, ay, az))
    nx, ny, nz = len(ax), len(ay), len(az)
    v = np.asarray(values, F).reshape(nx, ny, nz)
    G = max(nx, ny, nz) if G is None else int(G)
    neg = v < 0
    cut = np.zeros((nx, ny, nz, 3), bool)
    cut[:-1, :, :, 0] = neg[:-1] != neg[1:]
    cut[:, :-1, :, 1] = neg[:, :-1] != neg[:, 1:]
    cut[:, :, :-1, 2] = neg[:, :, :-1] != neg[:, :, 1:]
    lx, ly, lz, la = np.nonzero(cut)                                       # row-major: lattice point, then axis
    vertex_id = np.full((nx, ny, nz, 3), -1, np.int64)
    vertex_id[lx, ly, lz, la] = np.arange(len(lx))
    step = np.eye(3, dtype=np.int64)[la]
    v_o, v_e = v[lx, ly, lz], v[lx + step[:, 0], ly + step[:, 1], lz + step[:, 2]]
    with np.errstate(all="ignore"):
        t = (F(0) - v_o) / (v_e - v_o)
        pos = [ax[lx], ay[ly], az[lz]]
        far = [ax[np.minimum(lx + 1, nx - 1)], ay[np.minimum(ly + 1, ny - 1)], az[np.minimum(lz + 1, nz - 1)]]
        vertices = np.stack([np.where(la == k, pos[k] + t * (far[k] - pos[k]), pos[k]) for k in range(3)], -1).astype(F)
    g = [lx + int(lattice_offset[0]), ly + int(lattice_offset[1]), lz + int(lattice_offset[2])]
    keys = ((g[0] * G + g[1]) * G + g[2]) * 3 + la
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for i in range(8):
        case |= neg[(i & 1):(i & 1) + nx - 1, ((i >> 1) & 1):((i >> 1) & 1) + ny - 1, (i >> 2):(i >> 2) + nz - 1].astype(np.int64) << i
    cx, cy, cz = np.nonzero(T["ntri"][case] > 0)
    if not len(cx):
        return vertices.reshape(-1, 3), keys.astype(np.int64), np.zeros((0, 3), np.int64)
    cc = case[cx, cy, cz]
    rows = T["tri"][cc].astype(np.int64)[:, :-1].reshape(len(cc), -1, 3)
    used = rows[..., 0] >= 0
    info = T["edge_info"][np.where(rows >= 0, rows, 0)]
    ids = vertex_id[cx[:, None, None] + info[..., 0], cy[:, None, None] + info[..., 1], cz[:, None, None] + info[..., 2], info[..., 3]]
    faces = ids[used].astype(np.int64).reshape(-1, 3)
    assert (faces >= 0).all()
    return vertices, keys.astype(np.int64), faces


def crop_axes(R, resolution, crop):
    """xs float64 [N+1] and, per crop index, the float32 lattice coordinates [crop]"""
    N = resolution // crop
    xs = np.linspace(-R, R, N + 1)
    return [np.linspace(xs[i], xs[i + 1], crop).astype(F) for i in range(N)]


def weld(parts):
    """parts: [(vertices, keys, faces)] crop-major -> (vertices ascending by key, duplicates removed; faces re-indexed, in the given order)"""
    if not parts:
        return np.zeros((0, 3), F), np.zeros((0, 3), np.int64)
    v = np.concatenate([p[0] for p in parts])
    k = np.concatenate([p[1] for p in parts])
    base = np.cumsum([0] + [len(p[0]) for p in parts[:-1]])
    f = np.concatenate([p[2] + b for p, b in zip(parts, base)])
    if not len(k):
        return np.zeros((0, 3), F), np.zeros((0, 3), np.int64)
    _, first, inverse = np.unique(k, return_index=True, return_inverse=True)
    return v[first], inverse.reshape(-1)[f]


def concatenate(parts):
    """the crops' meshes side by side, not welded"""
    base = np.cumsum([0] + [len(p[0]) for p in parts[:-1]])
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[2] + b for p, b in zip(parts, base)])


def cropped_marching_cubes(sdf, R, resolution, crop):
    """sdf(points [M,3] float32) -> values [M]; the N^3 crops of the cube [-R, R]^3, each crop^3 samples: the list of parts for weld()"""
    axes = crop_axes(R, resolution, crop)
    N, G = len(axes), len(axes) * (crop - 1) + 1
    parts = []
    for i in range(N):
        for j in range(N):
            for k in range(N):
                values = sdf(lattice_points(axes[i], axes[j], axes[k]))
                parts.append(dense_marching_cubes(values, axes[i], axes[j], axes[k], (i * (crop - 1), j * (crop - 1), k * (crop - 1)), G))
    return parts


def extract_mesh_unbounded(views, world_view_transforms, xyz, resolution, crop, max_range=32.0):
    """the whole route: (vertices [V,3] world, faces [F,3], colors [V,3]) and the numbers it ran with"""
    center, radius = scene_normalisation(world_view_transforms)
    voxel = radius * 2 / resolution
    R = contracted_bound(xyz, center, radius)
    parts = cropped_marching_cubes(lambda p: fuse(p, views, voxel, center, radius, True), R, resolution, crop)
    y, faces = weld(parts)
    vertices = world_points(y, radius, center, max_range)
    _, colors = fuse(vertices, views, voxel, center, radius, False, True)
    return vertices, faces, colors, dict(center=center, radius=radius, R=R, voxel_size=voxel)


# ------------------------------------------------------------------------- the scene -------------------------------------------------------------------------
SPHERE_CENTRE = np.array([0.02, -0.03, 0.01])
# The reference's voxel_size is 2 radius / resolution whatever the bound R, so at resolution 32 the truncation 5 voxel_size is 0.3125 of
# the camera distance.  The sphere's diameter stays below it: every view then integrates every interior sample (a sample deeper than the
# truncation behind a view's surface would keep its initial +1 and open a second, inner surface).  Views that see a surface point from
# behind pull its average below zero and move the level set; the cloud that sets R leaves room for it.  The background is a far wall, as
# in a rendered unbounded scene, not 0: a sample in front of it is free space for that view (s = +1).  With a zero background such a
# sample is skipped, and the samples behind the sphere's limb, negative for the one view that has them within its truncation, are
# outvoted by nobody: the mesh then carries open shells behind every silhouette.
SPHERE_RADIUS = 0.25
BACKGROUND = 6.0
CLOUD_RADIUS = 0.45
CAMERA_DISTANCE = 2.0
WIDTH, HEIGHT, FOV = 64, 48, 0.9
COLOUR = (0.8, 0.5, 0.25)
ZNEAR, ZFAR = 0.01, 100.0


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """world-to-camera 4x4, column-vector convention (x right, y down, z forward)"""
    eye, target, up = np.asarray(eye, np.float64), np.asarray(target, np.float64), np.asarray(up, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, y, z])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def projection(fovx, fovy, znear=ZNEAR, zfar=ZFAR):
    """the renderer's projection matrix, column-vector convention: w = z"""
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1] = 1.0 / math.tan(fovx / 2), 1.0 / math.tan(fovy / 2)
    P[3, 2], P[2, 2], P[2, 3] = 1.0, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    return P


def sphere_depth(E, fovx, fovy, width, height, centre=SPHERE_CENTRE, radius=SPHERE_RADIUS, background=BACKGROUND):
    """z-depth float64 [H,W] of the sphere, `background` elsewhere; pixel (i, j) looks along NDC ((2j / (W-1)) - 1, (2i / (H-1)) - 1): the
    align_corners convention of the gather"""
    Rt, o = E[:3, :3].T, -E[:3, :3].T @ E[:3, 3]
    ys, xs = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    ndx, ndy = 2 * xs / (width - 1) - 1, 2 * ys / (height - 1) - 1
    dirs = np.stack([ndx * math.tan(fovx / 2), ndy * math.tan(fovy / 2), np.ones_like(xs)], -1) @ Rt.T
    oc = o - centre
    a, b, c = (dirs * dirs).sum(-1), 2 * (dirs @ oc), oc @ oc - radius * radius
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(disc)) / (2 * a)
    return np.where((disc > 0) & (t > 0), t, background)


def pattern_colour(view, width, height, dtype=F):
    """a colour map [3,H,W] that differs from pixel to pixel and from view to view, exact in float32 (multiples of 1/64)"""
    c, i, j = np.meshgrid(np.arange(3), np.arange(height), np.arange(width), indexing="ij")
    return (((i * 7 + j * 13 + c * 29 + view * 31) % 64) / 64.0).astype(dtype)


def sphere_scene(width=WIDTH, height=HEIGHT, dtype=F, pattern=False):
    """eight views of the sphere from the corners of a cube: dict(views=[(full_proj, depth, rgb)], world_view=[row-vector 4x4], xyz);
    the colour maps are the constant COLOUR, or pattern_colour"""
    fovx = FOV
    fovy = 2 * math.atan(math.tan(fovx / 2) * height / width)
    views, wv = [], []
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                eye = SPHERE_CENTRE + CAMERA_DISTANCE * np.array([sx, sy * 1.1, sz * 0.9]) / math.sqrt(1 + 1.21 + 0.81)
                E = look_at(eye, SPHERE_CENTRE)
                world_view = E.T.astype(dtype)
                full = (world_view.astype(np.float64) @ projection(fovx, fovy).T.astype(dtype).astype(np.float64)).astype(dtype)
                depth = sphere_depth(E, fovx, fovy, width, height).astype(dtype)
                rgb = pattern_colour(len(views), width, height, dtype) if pattern else np.broadcast_to(np.asarray(COLOUR, dtype)[:, None, None], (3, height, width)).copy()
                views.append((full, depth, rgb))
                wv.append(world_view)
    rng = np.random.default_rng(17)
    d = rng.standard_normal((400, 3))
    xyz = (SPHERE_CENTRE + CLOUD_RADIUS * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    return dict(views=views, world_view=wv, xyz=xyz)


_mesh = None


def sphere_mesh():
    """the scene's mesh at resolution 32, crop 16 (computed once, shared, not to be modified)"""
    global _mesh
    if _mesh is None:
        s = sphere_scene()
        _mesh = extract_mesh_unbounded(s["views"], s["world_view"], s["xyz"], 32, 16)
    return _mesh
