"""NumPy restatement of the Tanks-and-Temples mesh culling (the rule set is DESIGN 11 N11 and include/radegs.h): the depth
render in float64, Mesher.point_masks at forecast_radius 0 in float32, and the whole step.  Written from the rule set, not from the kernels;
the kernels follow the same operations in the same order, so the two are compared exactly.  NumPy multiplies, divides, adds and subtracts
IEEE doubles one rounding at a time and never fuses, which is what -ffp-contract=off gives the device code."""
import numpy as np

F32 = np.float32


# ----------------------------------------------------------------------------- poses -----------------------------------------------------------------------------
def world_to_camera(c2w, pose="opengl"):
    """float64 [B,4,4]: the inverse of every pose; "opencv" negates columns 1 and 2 of the pose first"""
    m = np.array(c2w, dtype=np.float64).reshape(-1, 4, 4)
    if pose == "opencv":
        m[:, :3, 1] *= -1
        m[:, :3, 2] *= -1
    return np.stack([np.linalg.inv(x) for x in m]) if len(m) else m


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """an OpenGL camera-to-world pose: the camera at `eye` looks down its -z at `target`, +y up"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(np.asarray(up, np.float64), back)
    right /= np.linalg.norm(right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, np.cross(back, right), back, eye
    return m


def to_opencv(c2w_gl):
    """the OpenCV pose of the same camera (x right, y down, z forward)"""
    m = np.array(c2w_gl, dtype=np.float64)
    m[..., :3, 1] *= -1
    m[..., :3, 2] *= -1
    return m


# ----------------------------------------------------------------------------- render -----------------------------------------------------------------------------
def camera_space(vertices, w2c):
    """(X, Y, d) per vertex: rows of w2c evaluated as ((m0 x + m1 y) + m2 z) + m3, d = -Z"""
    v = np.asarray(vertices, np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    row = lambda r: ((w2c[r, 0] * x + w2c[r, 1] * y) + w2c[r, 2] * z) + w2c[r, 3]
    return np.stack([row(0), row(1), -row(2)], axis=1)


def meet(a, b, znear):
    """where the edge a-b meets d = znear, from the end that is smaller in (X, Y, d)"""
    if tuple(b) < tuple(a):
        a, b = b, a
    t = (znear - a[2]) / (b[2] - a[2])
    return np.array([a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), znear])


def clip_near(p, znear):
    """Sutherland-Hodgman of the triangle p [3,3] = (X, Y, d) rows against d >= znear: the polygon's vertices in order"""
    out = []
    for i in range(3):
        k = (i + 1) % 3
        if p[i][2] >= znear:
            out.append(p[i])
        if (p[i][2] >= znear) != (p[k][2] >= znear):
            out.append(meet(p[i], p[k], znear))
    return out


def fan(poly):
    return [(poly[0], poly[k], poly[k + 1]) for k in range(1, len(poly) - 1)]


def edge_terms(ax, ay, bx, by, px, py):
    """the two rounded products of the edge function of a -> b at p, taken from the end that is smaller in (x, then y), and the sign to apply:
    value = sign * (first - second).  Arrays over triangles [T,1,1] against pixels [1,H,W]."""
    flip = (bx < ax) | ((bx == ax) & (by < ay))
    sx, sy = np.where(flip, bx, ax), np.where(flip, by, ay)
    ex, ey = np.where(flip, ax, bx), np.where(flip, ay, by)
    first, second = (ex - sx) * (py - sy), (ey - sy) * (px - sx)
    return first, second, np.where(flip, -1.0, 1.0)


def window(tris, fx, fy, cx, cy):
    """tris [T,3,3] of (X, Y, d) -> x [T,3], y [T,3], d [T,3]"""
    X, Y, d = tris[..., 0], tris[..., 1], tris[..., 2]
    return fx * X / d + cx, cy - fy * Y / d, d


def render_view(vertices, faces, w2c, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0, chunk=512):
    """One view.  Returns (depth float32 [H,W], cover bool [H,W], margin): margin is the smallest |first - second| / (|first| + |second|) over
    all (candidate pixel, edge) pairs whose value is not exactly 0 with both products equal -- how far the nearest coverage decision is
    from flipping."""
    cam = camera_space(vertices, w2c)
    tris = []
    for f in np.asarray(faces).reshape(-1, 3):
        p = cam[f]
        tris.extend(fan(clip_near(p, znear)) if (p[:, 2] < znear).any() else [tuple(p)])
    best = np.full((H, W), np.inf)
    margin = np.inf
    py, px = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    px, py = px[None], py[None]
    tris = np.array(tris, dtype=np.float64).reshape(-1, 3, 3)
    for s in range(0, len(tris), chunk):
        x, y, d = window(tris[s:s + chunk], fx, fy, cx, cy)
        col = lambda a, k: a[:, k][:, None, None]
        a1, a2, asg = edge_terms(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
        area = asg * (a1 - a2)
        with np.errstate(invalid="ignore"):
            jlo, jhi = np.maximum(np.ceil(x.min(1) - 0.5), 0.0), np.minimum(np.floor(x.max(1) - 0.5), W - 1.0)
            ilo, ihi = np.maximum(np.ceil(y.min(1) - 0.5), 0.0), np.minimum(np.floor(y.max(1) - 0.5), H - 1.0)
            draw = ((area < 0) | (area > 0)) & (jlo <= jhi) & (ilo <= ihi)
        j, i = px - 0.5, py - 0.5
        box = (draw[:, None, None] & (j >= jlo[:, None, None]) & (j <= jhi[:, None, None]) & (i >= ilo[:, None, None]) & (i <= ihi[:, None, None]))
        orient = np.where(area < 0, -1.0, 1.0)[:, None, None]
        E = []
        for a, b in ((1, 2), (2, 0), (0, 1)):                                    # the edge opposite vertex 0, 1, 2
            first, second, sg = edge_terms(col(x, a), col(y, a), col(x, b), col(y, b), px, py)
            E.append(orient * (sg * (first - second)))
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.abs(first - second) / (np.abs(first) + np.abs(second))
            rel = np.where(box & ~((first == second) & (first != 0)), rel, np.inf)   # a centre exactly on an edge is a decision, not a margin
            rel = np.where(np.isnan(rel), 0.0, rel)                                  # both products 0: a centre on a vertex -- no margin
            margin = min(margin, float(rel.min()) if rel.size else np.inf)
        E0, E1, E2 = E
        total = (E0 + E1) + E2
        covered = box & (E0 >= 0) & (E1 >= 0) & (E2 >= 0) & (total > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            depth = total / ((E0 / col(d, 0) + E1 / col(d, 1)) + E2 / col(d, 2))
        keep = covered & (depth >= znear) & (depth <= zfar)
        best = np.minimum(best, np.where(keep, depth.astype(F32).astype(np.float64), np.inf).min(axis=0, initial=np.inf))
    cover = np.isfinite(best)
    return np.where(cover, best, 0.0).astype(F32), cover, margin


def render_depth(vertices, faces, c2w, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0, pose="opengl"):
    """(depth float32 [B,H,W], margin)"""
    w2c = world_to_camera(c2w, pose)
    out = [render_view(vertices, faces, m, H, W, fx, fy, cx, cy, znear, zfar) for m in w2c]
    depth = np.stack([o[0] for o in out]) if out else np.zeros((0, H, W), F32)
    return depth, min([o[2] for o in out], default=np.inf)


# ------------------------------------------------------------------------ vertex visibility ------------------------------------------------------------------------
def sample_coord(u, size):
    s = F32(size - 1)
    g = u / s * F32(2) - F32(1)
    x = (g + F32(1)) / F32(2) * s
    return np.minimum(s, np.maximum(x, F32(0)))


def seen_by(points, depth, w2c32, fx, fy, cx, cy, eps=0.005):
    """bool [N]: which points one camera sees.  float32 throughout; w2c32: the float32 world-to-camera matrix."""
    p = np.asarray(points, F32)
    H, W = depth.shape
    fx, fy, cx, cy, eps = F32(fx), F32(fy), F32(cx), F32(cy), F32(eps)
    m = np.asarray(w2c32, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    row = lambda r: ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    xc, yc, zc = row(0), row(1), row(2)
    zz = zc + F32(1e-8)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u, v = (fx * xc + cx * zc) / zz, (fy * yc + cy * zc) / zz
        inside = (u >= 0) & (u <= F32(W - 1)) & (v >= 0) & (v <= F32(H - 1)) & (zz > 0)
        u, v = np.where(inside, u, F32(0)), np.where(inside, v, F32(0))            # the others are never sampled
        ix, iy = sample_coord(u, W), sample_coord(v, H)
    x0f, y0f = np.floor(ix), np.floor(iy)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    nw, ne = ((x0f + F32(1)) - ix) * ((y0f + F32(1)) - iy), (ix - x0f) * ((y0f + F32(1)) - iy)
    sw, se = ((x0f + F32(1)) - ix) * (iy - y0f), (ix - x0f) * (iy - y0f)
    D = np.asarray(depth, F32)
    right, below = x0 + 1 < W, y0 + 1 < H
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    s = F32(0) + D[y0, x0] * nw
    s = np.where(right, s + D[y0, x1] * ne, s)
    s = np.where(below, s + D[y1, x0] * sw, s)
    s = np.where(right & below, s + D[y1, x1] * se, s)
    assert s.dtype == F32 and zz.dtype == F32
    front = np.where(s > 0, zz < s + eps, True)
    return inside & front


def point_masks(points, depths, c2w, fx, fy, cx, cy, eps=0.005, min_views=20):
    """(mask bool [N], counts int32 [N]); c2w: OpenCV poses, inverted in float64 and rounded to float32"""
    w2c = world_to_camera(c2w).astype(F32)
    counts = np.zeros(len(points), np.int32)
    for b in range(len(w2c)):
        counts += seen_by(points, depths[b], w2c[b], fx, fy, cx, cy, eps)
    return counts >= min_views, counts


# ------------------------------------------------------------------------- the whole step -------------------------------------------------------------------------
def cull_mesh(vertices, faces, c2w, H, W, fx, fy, cx, cy, far=20.0, eps=0.005, min_views=20, pose="opengl"):
    """(kept vertices, renumbered faces int64, counts)"""
    vertices, faces = np.asarray(vertices), np.asarray(faces, np.int64).reshape(-1, 3)
    depths, _ = render_depth(vertices, faces, c2w, H, W, fx, fy, cx, cy, 0.01, far, pose)
    mask, counts = point_masks(vertices, depths, c2w, fx, fy, cx, cy, eps, min_views)
    new_index = np.cumsum(mask) - 1
    kept_faces = faces[mask[faces].all(axis=1)] if len(faces) else faces
    return vertices[mask], new_index[kept_faces].astype(np.int64), counts
