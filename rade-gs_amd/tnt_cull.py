"""HIP-backed Tanks-and-Temples mesh culling: eval_tnt/cull_mesh.py, the step between the marching-tetrahedra mesh and
tnt_eval.evaluate -- one depth map of the mesh per camera (upstream: pyrender / EGL), the per-vertex count of the cameras that see a vertex
(Mesher.point_masks at forecast_radius 0), and the faces whose three vertices at least `min_views` cameras see.  GPU only.  The rasterizer
is float64 and pinned to a written rule set (include/radegs.h); the vertex test is float32, as upstream's.  Reading the
trajectory, trimesh's load / merge_vertices and the forecast branch stay with the caller; Mesher.get_connected_mesh, the
step after cull_mesh (cull_mesh.py:283), is mesh_clean's and is passed on here under the name the reference's class has it."""
import functools
import math

import numpy as np
import torch

import geom_host as gh
import mesh_clean
import mesh_simplify
from diff_gaussian_rasterization import _C
from geom_host import f32, f64, i32, ll, sz, vp

MAX_SIDE, MAX_VIEWS = 32768, 65535
DEFAULT_VIEW_BATCH = 8            # eight 1080p maps are 66 MB
QUEUE_ENTRIES = None              # test hook: the number of queue entries render_depth's workspace holds (None: radegs_tntcull_render_bytes)
POSES = ("opengl", "opencv")

_SIGNATURES = {
    "radegs_tntcull_render_bytes": (sz, [ll, i32]),
    "radegs_tntcull_render_begin": (i32, [ll, ll, vp, vp, i32, vp, i32, i32, f64, f64, f64, f64, f64, f64, vp, sz, vp, vp]),
    "radegs_tntcull_render_finish": (i32, [ll, ll, vp, vp, i32, vp, i32, i32, f64, f64, f64, f64, f64, f64, vp, sz, vp, vp, vp]),
    "radegs_tntcull_count_views": (i32, [ll, vp, i32, i32, i32, vp, vp, f32, f32, f32, f32, f32, vp, vp]),
    "radegs_tetmesh_filter_plan_bytes": (sz, [ll, ll]),
    "radegs_tetmesh_filter_plan_flags": (i32, [ll, ll, vp, vp, vp, sz, vp, vp]),
    "radegs_tetmesh_filter_apply": (i32, [ll, ll, vp, vp, vp, ll, ll, vp, vp, vp]),
    **mesh_clean.SIGNATURES,      # get_connected_mesh below runs on them
    # mesh_simplify.py binds its own table; it is merged here, next to the clean-up whose compaction it ends in, because the check that the
    # signature tables of the host modules together cover every exported symbol reads this module's table, not mesh_simplify's
    **mesh_simplify.SIGNATURES,
}
get_connected_mesh = mesh_clean.get_connected_mesh      # cull_mesh.py:186-202


def _lib():
    return gh.bind(_SIGNATURES)


_call = functools.partial(gh.call, _SIGNATURES)


# ------------------------------------------------------------------------- arguments -------------------------------------------------------------------------
def _number(x, name):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
        raise RuntimeError(f"`{name}` must be a finite number")
    return float(x)


def _side(x, name):
    if isinstance(x, bool) or not isinstance(x, int) or not 2 <= x <= MAX_SIDE:
        raise RuntimeError(f"`{name}` must be an integer in [2, {MAX_SIDE}]")
    return x


def _intrinsics(fx, fy, cx, cy):
    return tuple(_number(v, n) for v, n in ((fx, "fx"), (fy, "fy"), (cx, "cx"), (cy, "cy")))


def _planes(znear, zfar):
    znear, zfar = _number(znear, "znear"), _number(zfar, "zfar")
    if not znear > 0:
        raise RuntimeError("`znear` must be positive")
    if not zfar > znear:
        raise RuntimeError("`zfar` must be larger than `znear`")
    return znear, zfar


def _pose(pose):
    if pose not in POSES:
        raise RuntimeError(f"`pose` must be one of {POSES}")
    return pose


def _world_to_camera(c2w, pose="opengl"):
    """[B,4,4] float64 numpy: the inverses of the camera-to-world poses (a list of 4x4 arrays / tensors, or one [B,4,4]), inverted on the host
    in float64.  `pose` "opengl": the pose is used as an OpenGL camera, as upstream executes; "opencv": columns 1 and 2 are negated first,
    the two lines upstream has commented out."""
    _pose(pose)
    if isinstance(c2w, torch.Tensor):
        c2w = c2w.detach().cpu().numpy()
    elif isinstance(c2w, (list, tuple)):
        c2w = [m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m for m in c2w]
    try:
        m = np.array(c2w, dtype=np.float64)
    except (TypeError, ValueError):
        raise RuntimeError("`c2w` must be a stack of 4x4 matrices") from None
    if m.size == 0:
        m = m.reshape(0, 4, 4)
    if m.ndim != 3 or m.shape[1:] != (4, 4):
        raise RuntimeError(f"`c2w` must be a stack of 4x4 matrices, got shape {m.shape}")
    if m.shape[0] > MAX_VIEWS:
        raise RuntimeError(f"`c2w` holds more than {MAX_VIEWS} poses")
    if not np.isfinite(m).all():
        raise RuntimeError("`c2w` holds non-finite values")
    if m.shape[0] and not (m[:, 3] == [0.0, 0.0, 0.0, 1.0]).all():
        raise RuntimeError("every pose of `c2w` must be affine: its last row must be (0, 0, 0, 1)")
    if pose == "opencv":
        m[:, :3, 1] *= -1
        m[:, :3, 2] *= -1
    out = np.empty_like(m)
    for b in range(m.shape[0]):
        try:
            if np.linalg.matrix_rank(m[b]) < 4:
                raise np.linalg.LinAlgError
            out[b] = np.linalg.inv(m[b])
        except np.linalg.LinAlgError:
            raise RuntimeError(f"pose {b} of `c2w` is not invertible") from None
        if not np.isfinite(out[b]).all():
            raise RuntimeError(f"pose {b} of `c2w` is not invertible")
    return out


def _mesh(vertices, faces):
    if not isinstance(vertices, torch.Tensor) or vertices.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("`vertices` must be a float32 or float64 tensor")
    gh.faces_type(faces)
    v = gh.points(vertices, "vertices", vertices.dtype)
    _C._require_gpu(faces, "faces")
    if faces.device != v.device:
        raise RuntimeError("`vertices` and `faces` must be on the same device")
    if v.shape[0] >= 2 ** 31 or faces.shape[0] >= 2 ** 31:
        raise RuntimeError("the mesh has 2^31 vertices or faces, or more")
    f = gh.faces(faces, v.shape[0])
    gh.finite(v, "vertices")
    return v, f


def _cameras_to(dev, w2c, dtype):
    return torch.from_numpy(np.ascontiguousarray(w2c[:, :3].reshape(-1, 12))).to(dev, dtype)


# --------------------------------------------------------------------------- render ---------------------------------------------------------------------------
def _render(v64, f, w2c, H, W, K, znear, zfar, stats=None):
    """the maps of the views `w2c` ([b,4,4] numpy) of a checked mesh; `stats`: an int64 [4] GPU tensor radegs_tntcull_render_finish fills"""
    dev, B, V, F = v64.device, w2c.shape[0], v64.shape[0], f.shape[0]
    depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    if B == 0:
        return depth
    L = _lib()
    nbytes = L.radegs_tntcull_render_bytes(F, B) if QUEUE_ENTRIES is None else L.radegs_tntcull_render_bytes(0, 0) + 16 * int(QUEUE_ENTRIES)
    ws = gh.workspace(nbytes, dev)
    cams = _cameras_to(dev, w2c, torch.float64)
    args = (V, F, v64, f, B, cams, H, W, *K, znear, zfar, ws, nbytes, depth)
    _call("radegs_tntcull_render_begin", dev, *args)
    _call("radegs_tntcull_render_finish", dev, *args, stats)
    return depth


@torch.no_grad()
def render_depth(vertices, faces, c2w, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0, pose="opengl"):
    """cull_mesh.py:17-66, extract_depth_from_mesh: the depth (distance along the viewing axis) of the nearest surface of the mesh at every
    pixel centre of every camera, 0 where there is none; both sides of a triangle are drawn.  `vertices` float32 or float64 [V,3] and
    `faces` int [F,3] on the GPU; `c2w`: B host 4x4 camera-to-world matrices.  Returns float32 [B,H,W].  The value is the exact one rounded
    to float32: the quantisation of upstream's 24-bit depth buffer is not reproduced."""
    H, W, K = _side(H, "H"), _side(W, "W"), _intrinsics(fx, fy, cx, cy)
    znear, zfar = _planes(znear, zfar)
    w2c = _world_to_camera(c2w, pose)
    v, f = _mesh(vertices, faces)
    return _render(v.double(), f, w2c, H, W, K, znear, zfar)


# ----------------------------------------------------------------------- vertex visibility -----------------------------------------------------------------------
def _count(p32, depths, w2c, K, eps, counts):
    B, H, W = depths.shape
    if B == 0 or p32.shape[0] == 0:
        return
    dev = p32.device
    cams = _cameras_to(dev, w2c, torch.float32)      # inverted in float64, rounded once: upstream inverts in float32
    _call("radegs_tntcull_count_views", dev, p32.shape[0], p32, B, H, W, depths, cams, *K, eps, counts)


def _min_views(min_views):
    if isinstance(min_views, bool) or not isinstance(min_views, int):
        raise RuntimeError("`min_views` must be an integer")
    return min_views


@torch.no_grad()
def point_masks(points, depths, c2w, fx, fy, cx, cy, eps=0.005, min_views=20):
    """cull_mesh.py:96-183, Mesher.point_masks with forecast_radius 0: per point the number of cameras for which it projects inside the image
    and is not behind that camera's depth map by `eps` or more (a map that reads 0 there hides nothing).  `points` float32 or float64 [N,3]
    (projected in float32, as upstream), `depths` float32 [B,H,W] on the same device, `c2w`: B host 4x4 matrices in the OpenCV convention
    the reference's loop uses them in.  Returns (mask bool [N]: counts >= min_views, counts int32 [N])."""
    K, eps, min_views = _intrinsics(fx, fy, cx, cy), _number(eps, "eps"), _min_views(min_views)
    w2c = _world_to_camera(c2w)
    if not isinstance(points, torch.Tensor) or points.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("`points` must be a float32 or float64 tensor")
    p = gh.points(points, "points", points.dtype)
    _C._require_gpu(depths, "depths")
    if depths.dim() != 3 or depths.dtype != torch.float32:
        raise RuntimeError("`depths` must be a float32 tensor of shape (B,H,W)")
    if depths.device != p.device:
        raise RuntimeError("`points` and `depths` must be on the same device")
    B, H, W = depths.shape
    if B != w2c.shape[0]:
        raise RuntimeError(f"`depths` holds {B} maps for {w2c.shape[0]} poses")
    _side(H, "H"), _side(W, "W")
    gh.finite(p, "points")
    gh.finite(depths, "depths")
    counts = torch.zeros(p.shape[0], dtype=torch.int32, device=p.device)
    _count(p.float(), depths.detach().contiguous(), w2c, K, eps, counts)
    return counts >= min_views, counts


# ------------------------------------------------------------------------- the whole step -------------------------------------------------------------------------
@torch.no_grad()
def cull_mesh(vertices, faces, c2w, H=1080, W=1920, fx=1163.8678928442187, fy=1172.793101201448, cx=962.3120628412543, cy=542.0667209577691,
              far=20.0, eps=0.005, min_views=20, pose="opengl", view_batch=None):
    """cull_mesh.py:205-319, Mesher.cull_mesh: renders the mesh from every camera, keeps the vertices at least `min_views` cameras see, keeps
    the faces whose three vertices are kept and renumbers them.  The defaults are the reference's Tanks-and-Temples intrinsics.  `pose`
    chooses the convention the RENDER reads `c2w` in -- "opengl" is what upstream executes, although its vertex test reads the same matrices
    as OpenCV poses; "opencv" renders with the convention the vertex test uses.  The views are rendered `view_batch` at a
    time (default 8).  Returns (vertices of the caller's precision, faces int64)."""
    H, W, K = _side(H, "H"), _side(W, "W"), _intrinsics(fx, fy, cx, cy)
    znear, zfar = _planes(0.01, far)
    eps, min_views = _number(eps, "eps"), _min_views(min_views)
    if view_batch is not None and (isinstance(view_batch, bool) or not isinstance(view_batch, int) or view_batch < 1):
        raise RuntimeError("`view_batch` must be a positive integer")
    step = DEFAULT_VIEW_BATCH if view_batch is None else min(view_batch, MAX_VIEWS)
    render_w2c, test_w2c = _world_to_camera(c2w, pose), _world_to_camera(c2w)
    v_in, f = _mesh(vertices, faces)
    dev, NV, NF = v_in.device, v_in.shape[0], f.shape[0]
    v32, v64 = v_in.float(), v_in.double()
    counts = torch.zeros(NV, dtype=torch.int32, device=dev)
    for b in range(0, render_w2c.shape[0], step):
        depths = _render(v64, f, render_w2c[b:b + step], H, W, K, znear, zfar)
        _count(v32, depths, test_w2c[b:b + step], K, eps, counts)
    flags = (counts >= min_views).to(torch.int32)
    nbytes = _lib().radegs_tetmesh_filter_plan_bytes(NV, NF)
    ws = gh.workspace(nbytes, dev)
    counts2 = torch.zeros(2, dtype=torch.int64, device=dev)
    _call("radegs_tetmesh_filter_plan_flags", dev, NV, NF, flags, f, ws, nbytes, counts2)
    nv, nf = counts2.tolist()              # the one host read
    out_v = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((nf, 3), dtype=torch.int64, device=dev)
    _call("radegs_tetmesh_filter_apply", dev, NV, NF, v32, f, ws, nv, nf, out_v, out_f)
    if v_in.dtype == torch.float64:            # the kept rows of the caller's own precision
        out_v = v_in[flags.bool()]
    return out_v, out_f


@torch.no_grad()
def cull_mesh_file(mesh_path, traj_path, out_path=None, device="cuda", **kw):
    """Mesher.__call__ from paths alone (cull_mesh.py:292-317, 403-416): eval_io.read_ply_mesh, eval_io.merge_vertices (trimesh's
    load(process=True) and merge_vertices()), eval_io.get_traj, cull_mesh with `kw`, tetmesh.write_ply to `out_path` (default: the mesh
    path with `.ply` replaced by `_cull.ply`).  Returns (vertices, faces int64, out_path)."""
    import eval_io
    import tetmesh
    v, f = eval_io.read_ply_mesh(mesh_path, device)
    v, f = eval_io.merge_vertices(v, f)
    kv, kf = cull_mesh(v, f, eval_io.get_traj(traj_path), **kw)
    out_path = mesh_path.replace(".ply", "_cull.ply") if out_path is None else out_path
    tetmesh.write_ply(out_path, kv, kf)
    return kv, kf, out_path
