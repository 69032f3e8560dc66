"""Scenes both tiers of the Tanks-and-Temples culling tests draw from (tests/test_tntcull_restatement.py, tests/test_gpu_tntcull.py).  Geometry
is built in the window space of view 0 -- so that a case can say how many pixels a triangle covers and on which side of a plane it lies --
and carried to the world by that view's pose.  Every vertex is rounded to float32, as a PLY holds it."""
import numpy as np

import tntcull_restatement as tc

SIZES = {(21, 33): (25.0, 25.0, 16.3, 10.6), (48, 64): (50.0, 50.0, 31.7, 24.2)}     # (H, W) -> fx, fy, cx, cy
ZNEAR, ZFAR = 0.5, 20.0                                                                # planes at a scale the scenes straddle
SOUP_SEEDS = {(21, 33): 7, (48, 64): 8}                                                # margins checked in the CPU tier


def views():
    """three OpenGL poses: the one the scenes are built in, one beside it, one that looks away and sees nothing"""
    a = tc.look_at([0.3, -3.0, 0.4], [0.0, 0.0, 0.1])
    b = tc.look_at([1.1, -2.6, -0.3], [0.1, 0.4, 0.0])
    c = tc.look_at([0.3, -3.0, 0.4], [0.6, -9.0, 0.7])
    return np.stack([a, b, c])


def to_world(xy, d, size):
    """window positions xy [...,2] of view 0 at depths d [...] -> world points, float32-rounded float64"""
    fx, fy, cx, cy = SIZES[size]
    X, Y = (xy[..., 0] - cx) * d / fx, (cy - xy[..., 1]) * d / fy
    cam = np.stack([X, Y, -d, np.ones_like(d)], axis=-1)
    return (cam @ views()[0].T)[..., :3].astype(np.float32).astype(np.float64)


def mesh_of(tris):
    """[T,3,3] world triangles -> (vertices [3T,3], faces [T,3])"""
    tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    return tris.reshape(-1, 3), np.arange(3 * len(tris), dtype=np.int64).reshape(-1, 3)


def right_triangle(n, size, at=(3.3, 3.3), depth=(2.0, 2.5, 3.0)):
    """a right triangle whose box holds n x n pixel centres"""
    x, y = at
    xy = np.array([[x, y], [x + n - 0.2, y], [x, y + n - 0.2]])
    return to_world(xy, np.array(depth), size)


def full_screen(size):
    H, W = size
    return to_world(np.array([[-W, -H], [3.0 * W, -H], [-W, 3.0 * H]]), np.array([3.0, 4.0, 5.0]), size)


def sliver(size):
    """thin and long, between two rows of pixel centres: covers none"""
    return to_world(np.array([[1.2, 5.9], [17.8, 6.1], [9.0, 6.05]]), np.array([2.0, 2.0, 2.0]), size)


def at_depths(size, d):
    return to_world(np.array([[4.0, 3.0], [15.5, 4.5], [7.5, 14.0]]), np.asarray(d, np.float64), size)


def soup(size, n=2000):
    """random triangles from sub-pixel to half the image, depths on both sides of both planes"""
    H, W = size
    rng = np.random.default_rng(SOUP_SEEDS[size])
    centre = rng.uniform([-0.2 * W, -0.2 * H], [1.2 * W, 1.2 * H], (n, 1, 2))
    extent = np.exp(rng.uniform(np.log(0.3), np.log(0.5 * W), (n, 1, 1)))
    xy = centre + extent * rng.standard_normal((n, 3, 2))
    kind = rng.choice(4, (n, 1), p=[0.7, 0.1, 0.1, 0.1])
    lo, hi = np.array([0.6, -2.0, 17.0, 0.2])[kind], np.array([18.0, 1.0, 24.0, 0.8])[kind]
    d = rng.uniform(lo, hi) + rng.choice([0.05, 1.0], (n, 1)) * rng.standard_normal((n, 3))
    d = np.where(np.abs(d) < 1e-3, 0.25, d)
    return mesh_of(to_world(xy, d, size))


def jittered_grid(size, seed, rows=7, cols=9, flip_some=False):
    """a sheet of 2 (rows - 1)(cols - 1) triangles over most of the image, every inner edge shared; (vertices, faces, boundary loop of window xy)"""
    H, W = size
    rng = np.random.default_rng(seed)
    gy, gx = np.meshgrid(np.linspace(2.2, H - 2.7, rows), np.linspace(1.6, W - 2.3, cols), indexing="ij")
    step = min((H - 5) / (rows - 1), (W - 4) / (cols - 1))
    xy = np.stack([gx, gy], axis=-1) + rng.uniform(-0.3, 0.3, (rows, cols, 2)) * step
    d = rng.uniform(1.5, 6.0, (rows, cols))
    world = to_world(xy, d, size).reshape(-1, 3)
    idx = np.arange(rows * cols).reshape(rows, cols)
    a, b, c, e = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([b, e, c], 1)])
    if flip_some:                                                              # both windings are drawn: a neighbour may walk the shared edge the same way
        k = rng.random(len(faces)) < 0.5
        faces[k] = faces[k][:, [0, 2, 1]]
    loop = np.concatenate([idx[0, :-1], idx[:-1, -1], idx[-1, :0:-1], idx[:0:-1, 0]])
    return world, faces.astype(np.int64), loop


def strictly_inside(world, loop, size, w2c, clearance=1e-6):
    """bool [H,W]: pixel centres inside the sheet's outline as view `w2c` sees it, at least `clearance` pixels from it"""
    H, W = size
    fx, fy, cx, cy = SIZES[size]
    cam = tc.camera_space(world[loop], w2c)
    x, y = fx * cam[:, 0] / cam[:, 2] + cx, cy - fy * cam[:, 1] / cam[:, 2]
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    inside, near = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for k in range(len(loop)):
        ax, ay, bx, by = x[k], y[k], x[(k + 1) % len(loop)], y[(k + 1) % len(loop)]
        with np.errstate(divide="ignore", invalid="ignore"):
            cross = ((ay > py) != (by > py)) & (px < ax + (py - ay) / (by - ay) * (bx - ax))
        inside ^= cross
        t = np.clip(((px - ax) * (bx - ax) + (py - ay) * (by - ay)) / ((bx - ax) ** 2 + (by - ay) ** 2), 0, 1)
        near |= np.hypot(px - (ax + t * (bx - ax)), py - (ay + t * (by - ay))) < clearance
    return inside & ~near


# ------------------------------------------------------------------------- the whole step -------------------------------------------------------------------------
CULL_SIZE = (48, 64)
CULL_K = (50.0, 50.0, 31.5, 23.5)


def ring_cameras(n=24, radius=3.0):
    """OpenCV poses (what Mesher.point_masks reads) on a ring above the box, at varying heights, looking down at its centre"""
    out = []
    for k in range(n):
        t = 2 * np.pi * (k + 0.25) / n
        out.append(tc.to_opencv(tc.look_at([radius * np.cos(t), radius * np.sin(t), 2.6 + 0.5 * np.sin(3 * t)], [0.0, 0.0, 0.0])))
    return np.stack(out)


def patch(centre, normal_axis, half, n=3):
    """an n x n vertex square patch"""
    u = np.linspace(-half, half, n)
    g = np.stack(np.meshgrid(u, u, indexing="ij"), -1).reshape(-1, 2)
    pts = np.zeros((n * n, 3))
    pts[:, [a for a in range(3) if a != normal_axis]] = g
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, e = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    return pts + np.asarray(centre), np.concatenate([np.stack([a, b, c], 1), np.stack([b, e, c], 1)])


def box_scene():
    """a closed box (six 5 x 5 vertex sides, seams not merged) whose top all ring cameras see, a patch inside it that none sees, and a patch out
    beyond the ring that the cameras with their back to it do not see.  Returns (vertices float32, faces int64, {name: vertex slice})."""
    parts, names = [], {}
    for axis in range(3):
        for sign in (-1.0, 1.0):
            c = np.zeros(3)
            c[axis] = 0.6 * sign
            parts.append(patch(c, axis, 0.6, 5))
    parts.append(patch([0.05, -0.1, 0.0], 2, 0.2))         # hidden: inside the box
    parts.append(patch([0.3, 5.5, 0.2], 1, 0.25))          # floating: outside the ring
    verts, faces, off = [], [], 0
    for k, (v, f) in enumerate(parts):
        verts.append(v)
        faces.append(f + off)
        if k >= 6:
            names["hidden" if k == 6 else "floating"] = slice(off, off + len(v))
        off += len(v)
    names["box"] = slice(0, names["hidden"].start)
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int64), names


# --------------------------------------------------------------------- references, computed once ---------------------------------------------------------------------
_cache = {}


def restated(key, vertices, faces, size, znear=ZNEAR, zfar=ZFAR, c2w=None):
    """(depth float32 [B,H,W], margin) of tntcull_restatement.render_depth for a named case, computed once per process and not to be written to"""
    if key not in _cache:
        H, W = size
        depth, margin = tc.render_depth(vertices, faces, views() if c2w is None else c2w, H, W, *SIZES[size], znear, zfar)
        depth.setflags(write=False)
        _cache[key] = (depth, margin)
    return _cache[key]


def soup_reference(size):
    v, f = soup(size)
    return (v, f) + restated(("soup", size), v, f, size)
