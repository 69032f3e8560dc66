"""NumPy float32 restatement of TSDF fusion as this library specifies it (include/radegs.h, "TSDF fusion"), written from
that text and not from the kernels: touch, integrate and the marching-cubes extraction, every float32 operation in the order the
specification gives (numpy multiplies, then adds; no fused multiply-add).  It is the arbiter of tests/test_gpu_tsdf.py, and
tests/test_tsdf_restatement.py checks it against properties that do not depend on it.  Also the common scene of those tests: a sphere
seen by ten cameras, analytic depth and colour."""
import math
import os
import re

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_HEADER = os.path.join(ROOT, "rade-gs_amd", "csrc", "rg_mc_tables.h")
KEY_BIAS = 1 << 20

_tables = None


def load_tables(path=TABLE_HEADER):
    """the generated header as arrays: tri [256, row] int8, ntri [256], edge_mask [256], edge_info [12,4] = dx, dy, dz, axis"""
    with open(path) as fh:
        text = re.sub(r"//[^\n]*", "", fh.read())

    def ints(name):
        body = re.search(name + r"(?:\[\w+\])+\s*=\s*\{(.*?)\};", text, re.S).group(1)
        return [int(t, 0) for t in re.findall(r"-?0x[0-9a-fA-F]+|-?\d+", body)]
    row = int(re.search(r"#define RG_MC_ROW (\d+)", text).group(1))
    return dict(tri=np.array(ints("kMcTriTable"), np.int8).reshape(256, row), ntri=np.array(ints("kMcNumTris"), np.int64),
                edge_mask=np.array(ints("kMcEdgeMask"), np.int64), edge_info=np.array(ints("kMcEdgeInfo"), np.int64).reshape(12, 4))


def tables():
    global _tables
    if _tables is None:
        _tables = load_tables()
    return _tables


def roundf(x):
    """C's roundf: half away from zero, spelled sign * floor(|x| + 0.5); the sum is taken in float64, where it is exact for a float32 x"""
    x = np.asarray(x, F)
    return (np.sign(x) * np.floor(np.abs(x).astype(np.float64) + 0.5)).astype(F)


def block_key(coords):
    """63-bit key of int block coordinates [n,3]: 21 bits per axis, bias 2^20, z in the highest bits, x in the lowest"""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    if c.size and (c.min() < -KEY_BIAS or c.max() >= KEY_BIAS):
        raise ValueError("a block coordinate is outside [-2^20, 2^20)")
    b = c + KEY_BIAS
    return (b[:, 2] << 42) | (b[:, 1] << 21) | b[:, 0]


def unique_blocks(coords):
    """the distinct rows of int coordinates [n,3], ascending by key, as int32"""
    c = np.asarray(coords, np.int64).reshape(-1, 3)
    _, first = np.unique(block_key(c), return_index=True)
    return c[first].astype(np.int32)


def _intrinsics(intrinsic):
    K = np.asarray(intrinsic, np.float64)
    return F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])


# ------------------------------------------------------------------------- touch -------------------------------------------------------------------------
def touch(depth, intrinsic, extrinsic, voxel_size, depth_scale=1.0, depth_max=8.0, trunc_voxel_multiplier=8.0):
    depth = np.asarray(depth, F)
    H, W = depth.shape
    fx, fy, cx, cy = _intrinsics(intrinsic)
    P = np.linalg.inv(np.asarray(extrinsic, np.float64)).astype(F)        # camera to world, inverted in float64
    block_size, trunc = F(float(voxel_size) * 16), F(float(voxel_size) * float(trunc_voxel_multiplier))
    ds, dmax = F(depth_scale), F(depth_max)
    ys, xs = np.meshgrid(np.arange(H // 4) * 4, np.arange(W // 4) * 4, indexing="ij")
    with np.errstate(all="ignore"):
        d = depth[ys, xs] / ds
        ok = (d > 0) & (d < dmax)
        xn, yn = (xs.astype(F) - cx) / fx, (ys.astype(F) - cy) / fy
        tmin, tmax = np.maximum(d - trunc, F(0)), np.minimum(d + trunc, dmax)
        step = (tmax - tmin) / F(3)
        out = []
        for k in range(4):
            t = tmin + F(k) * step
            px, py = xn * t, yn * t
            b = [np.floor((((P[r, 0] * px + P[r, 1] * py) + P[r, 2] * t) + P[r, 3]) / block_size) for r in range(3)]
            out.append(np.stack(b, -1)[ok])
    c = np.concatenate(out).reshape(-1, 3)
    if c.size and not (np.isfinite(c).all() and c.min() >= -KEY_BIAS and c.max() < KEY_BIAS):
        raise ValueError("a block coordinate is outside [-2^20, 2^20)")
    return unique_blocks(c.astype(np.int64))


# ------------------------------------------------------------------------ the grid ------------------------------------------------------------------------
class Grid:
    """blocks: {(bx, by, bz): index}; tsdf, weight [n,4096] and color [n,4096,3] float32; voxel index (z * 16 + y) * 16 + x"""

    def __init__(self, voxel_size, with_color=True):
        self.voxel_size, self.with_color = float(voxel_size), with_color
        self.index = {}
        self.tsdf, self.weight = np.zeros((0, 4096), F), np.zeros((0, 4096), F)
        self.color = np.zeros((0, 4096, 3), F) if with_color else None

    def insert(self, coords):
        new = [tuple(int(v) for v in c) for c in unique_blocks(coords) if tuple(int(v) for v in c) not in self.index]
        for c in new:
            self.index[c] = len(self.index)
        n = len(new)
        self.tsdf = np.concatenate([self.tsdf, np.zeros((n, 4096), F)])
        self.weight = np.concatenate([self.weight, np.zeros((n, 4096), F)])
        if self.with_color:
            self.color = np.concatenate([self.color, np.zeros((n, 4096, 3), F)])

    def coords(self):
        """the grid's block coordinates, ascending by key"""
        return unique_blocks(np.array(list(self.index), np.int64).reshape(-1, 3))

    def rows(self, coords):
        return np.array([self.index[tuple(int(v) for v in c)] for c in np.asarray(coords).reshape(-1, 3)], np.int64)

    def sorted_arrays(self):
        """(coords [n,3], tsdf [n,4096], weight, color or None) in key order: what the device grid holds, slot order removed"""
        c = self.coords()
        r = self.rows(c)
        return c, self.tsdf[r], self.weight[r], (self.color[r] if self.with_color else None)


VOXEL_OFFSETS = np.stack([np.arange(4096) & 15, (np.arange(4096) >> 4) & 15, np.arange(4096) >> 8], -1)      # [4096,3] = x, y, z


def integrate(grid, block_coords, depth, color, intrinsic, extrinsic, depth_scale=1.0, depth_max=8.0, trunc_voxel_multiplier=8.0):
    depth = np.asarray(depth, F)
    H, W = depth.shape
    assert (color is not None) == grid.with_color
    blocks = unique_blocks(block_coords)
    grid.insert(blocks)
    if not len(blocks):
        return
    rows = grid.rows(blocks)
    fx, fy, cx, cy = _intrinsics(intrinsic)
    E = np.asarray(extrinsic, np.float64)
    R, t = (E[:3, :3] * grid.voxel_size).astype(F), E[:3, 3].astype(F)      # world to camera, the rotation times voxel_size, in float64
    trunc, ds, dmax = F(grid.voxel_size * float(trunc_voxel_multiplier)), F(depth_scale), F(depth_max)
    X = (16 * blocks.astype(np.int64)[:, None, :] + VOXEL_OFFSETS[None]).astype(F)                           # [n,4096,3]
    tsdf, w = grid.tsdf[rows], grid.weight[rows]
    with np.errstate(all="ignore"):
        p = [((R[k, 0] * X[..., 0] + R[k, 1] * X[..., 1]) + R[k, 2] * X[..., 2]) + t[k] for k in range(3)]
        ok = p[2] > 0
        u, v = (fx * p[0]) / p[2] + cx, (fy * p[1]) / p[2] + cy
        ui, vi = roundf(u), roundf(v)
        ok &= (ui >= 0) & (ui < F(W)) & (vi >= 0) & (vi < F(H))
        uj, vj = np.where(ok, ui, 0).astype(np.int64), np.where(ok, vi, 0).astype(np.int64)
        d = depth[vj, uj] / ds
        sdf = d - p[2]
        ok &= (d > 0) & ~(d > dmax) & ~(sdf < -trunc)
        s = np.minimum(sdf, trunc) / trunc
        inv = F(1) / (w + F(1))
        grid.tsdf[rows] = np.where(ok, (w * tsdf + s) * inv, tsdf)
        if grid.with_color:
            c_old, c_new = grid.color[rows], np.asarray(color, F)[vj, uj]
            grid.color[rows] = np.where(ok[..., None], (w[..., None] * c_old + c_new) * inv[..., None], c_old)
        grid.weight[rows] = np.where(ok, w + F(1), w)


# ----------------------------------------------------------------------- extraction -----------------------------------------------------------------------
def extract(coords, tsdf, weight, color, voxel_size, weight_threshold=3.0):
    """coords int [n,3] (distinct), tsdf / weight [n,4096], color [n,4096,3] or None -> vertices float32 [V,3], faces int64 [F,3], colors
    float32 [V,3] or None, in the canonical order: vertices by (block key, voxel index, axis), faces by (block key, voxel index of the
    cell's lowest corner, table order)."""
    T = tables()
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    empty = (np.zeros((0, 3), F), np.zeros((0, 3), np.int64), None if color is None else np.zeros((0, 3), F))
    if not len(coords):
        return empty
    lo = coords.min(0)
    dims = (coords.max(0) - lo + 1) * 16 + 1                                # one layer of absent voxels beyond the last block
    vol_t, vol_ok = np.zeros(dims, F), np.zeros(dims, bool)
    vol_c = None if color is None else np.zeros(tuple(dims) + (3,), F)
    vol_key, vol_vox = np.zeros(dims, np.int64), np.zeros(dims, np.int64)
    keys = block_key(coords)
    for i, b in enumerate(coords):
        o = (b - lo) * 16
        sl = (slice(o[0], o[0] + 16), slice(o[1], o[1] + 16), slice(o[2], o[2] + 16))
        vol_t[sl] = np.asarray(tsdf[i], F).reshape(16, 16, 16).transpose(2, 1, 0)      # stored z, y, x -> indexed x, y, z
        vol_ok[sl] = (np.asarray(weight[i], F).reshape(16, 16, 16).transpose(2, 1, 0) > F(weight_threshold))
        if vol_c is not None:
            vol_c[sl] = np.asarray(color[i], F).reshape(16, 16, 16, 3).transpose(2, 1, 0, 3)
        vol_key[sl] = keys[i]
        vol_vox[sl] = np.arange(4096).reshape(16, 16, 16).transpose(2, 1, 0)
    nx, ny, nz = dims - 1
    corner = lambda a, i: a[(i & 1):(i & 1) + nx, ((i >> 1) & 1):((i >> 1) & 1) + ny, ((i >> 2) & 1):((i >> 2) & 1) + nz]
    valid = np.ones((nx, ny, nz), bool)
    case = np.zeros((nx, ny, nz), np.int64)
    for i in range(8):
        valid &= corner(vol_ok, i)
        case |= (corner(vol_t, i) < 0).astype(np.int64) << i
    case = np.where(valid, case, 0)
    # the owned edges that carry a vertex: marked by some valid cell
    marked = np.zeros(tuple(dims) + (3,), bool)
    for e in range(12):
        dx, dy, dz, axis = T["edge_info"][e]
        cut = (T["edge_mask"][case] >> e) & 1 == 1
        marked[dx:dx + nx, dy:dy + ny, dz:dz + nz, axis] |= cut
    vx, vy, vz, va = np.nonzero(marked)
    order = np.lexsort((va, vol_vox[vx, vy, vz], vol_key[vx, vy, vz]))
    vx, vy, vz, va = vx[order], vy[order], vz[order], va[order]
    vertex_id = np.full(tuple(dims) + (3,), -1, np.int64)
    vertex_id[vx, vy, vz, va] = np.arange(len(vx))
    step = np.eye(3, dtype=np.int64)[va]
    ex, ey, ez = vx + step[:, 0], vy + step[:, 1], vz + step[:, 2]
    t_o, t_e = vol_t[vx, vy, vz], vol_t[ex, ey, ez]
    ratio = (F(0) - t_o) / (t_e - t_o)
    X = (np.stack([vx, vy, vz], -1) + lo[None] * 16).astype(F)
    vs = F(voxel_size)
    vertices = np.stack([vs * (X[:, k] + np.where(va == k, ratio, F(0))) for k in range(3)], -1).astype(F)
    colors = None
    if vol_c is not None:
        c_o, c_e = vol_c[vx, vy, vz], vol_c[ex, ey, ez]
        colors = (c_o + ratio[:, None] * (c_e - c_o)).astype(F)
    # faces, cell by cell
    cx_, cy_, cz_ = np.nonzero(T["ntri"][case] > 0)
    order = np.lexsort((vol_vox[cx_, cy_, cz_], vol_key[cx_, cy_, cz_]))
    cx_, cy_, cz_ = cx_[order], cy_[order], cz_[order]
    cc = case[cx_, cy_, cz_]
    rows = T["tri"][cc].astype(np.int64)[:, :-1].reshape(len(cc), -1, 3)    # [cells, max tris, 3] edge numbers, -1 = none
    used = rows[..., 0] >= 0
    e = np.where(rows >= 0, rows, 0)
    info = T["edge_info"][e]                                                # [cells, tris, 3, 4]
    ids = vertex_id[cx_[:, None, None] + info[..., 0], cy_[:, None, None] + info[..., 1], cz_[:, None, None] + info[..., 2], info[..., 3]]
    faces = ids[used]
    assert (faces >= 0).all()
    return vertices, faces.astype(np.int64).reshape(-1, 3), colors


def extract_grid(grid, weight_threshold=3.0):
    c, t, w, col = grid.sorted_arrays()
    return extract(c, t, w, col, grid.voxel_size, weight_threshold)


# ------------------------------------------------------------------ properties of a mesh ------------------------------------------------------------------
def mesh_report(vertices, faces):
    """what makes a triangle mesh a closed oriented surface: every undirected edge in exactly two faces, every directed edge once,
    V - E + F, and the signed volume (positive: the normals point outward)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed = d[:, 0] * (len(v) + 1) + d[:, 1]
    u = np.sort(d, 1)
    _, per_edge = np.unique(u[:, 0] * (len(v) + 1) + u[:, 1], return_counts=True)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return dict(edges_in_two_faces=bool((per_edge == 2).all()), directed_once=len(np.unique(directed)) == len(directed),
                no_collapsed_face=bool((d[:, 0] != d[:, 1]).all()), euler=len(np.unique(f)) - len(per_edge) + len(f),
                volume=float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6), all_vertices_used=len(np.unique(f)) == len(v))


# ------------------------------------------------------------------------- the scene -------------------------------------------------------------------------
CENTRE = np.array([0.013, -0.007, 0.021])
RADIUS = 0.3
VOXEL = 0.01
WIDTH, HEIGHT, FOCAL = 128, 96, 130.0
# The scene is fused with a depth limit that leaves out each view's grazing samples.  A ray that only just enters the sphere leaves it again
# less than sdf_trunc later, so the voxels behind the limb -- outside the sphere -- receive a negative value from that view: the projective
# signed distance cannot tell them from the inside.  With the default limit of 8 this leaves 22 closed one-voxel bubbles just outside the
# surface (V - E + F = 46).  A z-depth of 1 - 0.3 cos(theta) <= 0.85 keeps the surface within 60 degrees of each view's axis; the ring
# views, 45 degrees apart, and the two polar ones still cover the whole sphere.  Few views see each point, so the scene's mesh counts every
# observed voxel (the weights are whole numbers: `weight <= 0.5` is `weight == 0`).
SCENE_DEPTH_MAX = 0.85
SCENE_WEIGHT_THRESHOLD = 0.5


def look_at(eye, target=CENTRE, up=(0.0, 0.0, 1.0)):
    """world-to-camera 4x4 (x right, y down, z forward) of a camera at `eye` looking at `target`"""
    eye, target, up = np.asarray(eye, np.float64), np.asarray(target, np.float64), np.asarray(up, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, y, z])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def intrinsic(width=WIDTH, height=HEIGHT, focal=FOCAL):
    return np.array([[focal, 0, width / 2], [0, focal, height / 2], [0, 0, 1]], np.float64)


def hit_colour(p):
    return (0.5 + 0.5 * np.sin(7.0 * p + np.array([0.0, 1.0, 2.0]))).astype(F)


def render_sphere(E, K, width=WIDTH, height=HEIGHT, centre=CENTRE, radius=RADIUS):
    """(z-depth float32 [H,W], 0 on the background; colour float32 [H,W,3]) of the sphere, one ray through each pixel's integer position"""
    Rt, o = E[:3, :3].T, -E[:3, :3].T @ E[:3, 3]
    ys, xs = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    dirs = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1) @ Rt.T
    oc = o - centre
    a, b, c = (dirs * dirs).sum(-1), 2 * (dirs @ oc), oc @ oc - radius * radius
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(disc)) / (2 * a)
    hit = (disc > 0) & (t > 0)
    t = np.where(hit, t, 0.0)
    colour = np.where(hit[..., None], hit_colour(o + t[..., None] * dirs), 0).astype(F)
    return t.astype(F), colour


def scene_views():
    """the ten views: eight on a ring of radius 1 around the centre, one above, one below: [(depth, colour, K, E)]"""
    K = intrinsic()
    eyes = [CENTRE + np.array([math.cos(a), math.sin(a), 0.0]) for a in np.arange(8) * (2 * math.pi / 8)]
    views = [(look_at(e),) for e in eyes] + [(look_at(CENTRE + np.array([0, 0, 1.0]), up=(0, 1.0, 0)),), (look_at(CENTRE - np.array([0, 0, 1.0]), up=(0, 1.0, 0)),)]
    return [render_sphere(E, K) + (K, E) for (E,) in views]


def close_view():
    """a camera 0.36 from the centre, between the surface and the outer edge of the band: the sphere leaves the image on all four sides,
    its nearest samples are closer than sdf_trunc, and many voxels of the band lie behind the camera"""
    K = intrinsic()
    E = look_at(CENTRE + np.array([0.216, -0.288, 0.0]))
    return render_sphere(E, K) + (K, E)


_fused = None


def fused_scene():
    """the sphere fused from the ten views (computed once, shared, not to be modified): dict(grid, lists, mesh)"""
    global _fused
    if _fused is None:
        g, lists = Grid(VOXEL, True), []
        for depth, colour, K, E in scene_views():
            b = touch(depth, K, E, VOXEL, depth_max=SCENE_DEPTH_MAX)
            lists.append(b)
            integrate(g, b, depth, colour, K, E, depth_max=SCENE_DEPTH_MAX)
        _fused = dict(grid=g, lists=lists, mesh=extract_grid(g, SCENE_WEIGHT_THRESHOLD))
    return _fused
