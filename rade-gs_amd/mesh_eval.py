"""HIP-backed mesh evaluation: what the reference does with recon.ply -- evaluate_dtu_mesh.py's cull_mesh and the DTU
Chamfer distance of dtu_eval/eval.py (sample the triangles, thin the shuffled cloud by a radius, mask it with the observation volume,
nearest-neighbour distances to and from the scan's cloud).  GPU only.  eval.py's geometry is float64 here as there: every step is a
decision on an exact distance.  Reading DTU's .mat / .ply files, the Procrustes alignment and the coloured clouds stay with the caller
(INTEGRATION 5b)."""
import ctypes
import functools
import math

import numpy as np
import torch

import geom_host as gh
from diff_gaussian_rasterization import _C
from geom_host import f64, i32, ll, pf64, sz, vp

CELL_SLACK = 1.0 + 1e-6      # thinning grid: cell = radius * CELL_SLACK, so that rounding in floor((p - origin) / cell) cannot put two
                             # points within the radius more than one cell apart
NN_CELLS_PER_MAX_DIST = 8    # dtu_chamfer's nearest-neighbour grids: cell = max_dist / 8
ROUNDS_PER_READ = 8          # thinning rounds enqueued between two reads of the undecided counter


class RadegsCullCamera(ctypes.Structure):
    _fields_ = [("m", ctypes.c_float * 12), ("W", ctypes.c_int), ("H", ctypes.c_int), ("mask_offset", ctypes.c_longlong)]

_SIGNATURES = {
    "radegs_mesheval_sample_bytes": (sz, [ll]),
    "radegs_mesheval_sample_count": (i32, [ll, ll, vp, vp, f64, vp, sz, vp, vp, vp]),
    "radegs_mesheval_sample_emit": (i32, [ll, ll, vp, vp, f64, vp, ll, vp, vp]),
    "radegs_mesheval_grid_bytes": (sz, [ll]),
    "radegs_mesheval_grid_build": (i32, [ll, vp, pf64, f64, vp, sz, vp]),
    "radegs_mesheval_thin_rounds": (i32, [ll, vp, pf64, f64, f64, i32, vp, vp, vp]),
    "radegs_mesheval_nearest": (i32, [ll, vp, pf64, f64, ll, vp, f64, vp, vp, vp]),
    "radegs_mesheval_sum_bytes": (sz, []),
    "radegs_mesheval_sum_below": (i32, [ll, vp, f64, vp, sz, vp, vp]),
    "radegs_mesheval_obs_mask": (i32, [ll, vp, pf64, ctypes.POINTER(ctypes.c_int), vp, vp, vp, vp, vp]),
    "radegs_mesheval_above_plane": (i32, [ll, vp, pf64, vp, vp]),
    "radegs_mesheval_dilate": (i32, [i32, i32, vp, i32, vp, vp]),
    "radegs_mesheval_cull_vertices": (i32, [ll, vp, i32, vp, vp, vp, vp]),
    "radegs_tetmesh_filter_plan_flags": (i32, [ll, ll, vp, vp, vp, sz, vp, vp]),
    "radegs_tetmesh_filter_plan_bytes": (sz, [ll, ll]),
    "radegs_tetmesh_filter_apply": (i32, [ll, ll, vp, vp, vp, ll, ll, vp, vp, vp]),
}


def _lib():
    return gh.bind(_SIGNATURES)


_call = functools.partial(gh.call, _SIGNATURES)


# ------------------------------------------------------------------ triangle sampling ------------------------------------------------------------------
@torch.no_grad()
def sample_mesh_points(vertices, faces, density=0.2):
    """eval.py:50-71.  `vertices` float64 [V,3], `faces` int [F,3] on the GPU.  Returns (cloud float64 [V+M,3]: the vertices followed by the
    samples, triangles in input order, i major, j minor; counts int32 [F]: samples per triangle, 0 for a dropped one)."""
    gh.faces_type(faces)
    v = gh.points(vertices, "vertices")
    f = gh.faces(faces, v.shape[0])
    gh.positive(density, "density")
    gh.finite(v, "vertices")
    V, F, dev = v.shape[0], f.shape[0], v.device
    nbytes = _lib().radegs_mesheval_sample_bytes(F)
    ws = gh.workspace(nbytes, dev)
    counts = torch.zeros(F, dtype=torch.int32, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    _call("radegs_mesheval_sample_count", dev, V, F, v, f, float(density), ws, nbytes, counts, totals)
    M, too_fine = totals.tolist()          # the one host read
    if too_fine:
        raise RuntimeError(f"sample_mesh_points: {too_fine} triangles are subdivided more than 30 000 times along an edge at density {density}")
    if M >= 2 ** 32 - 1:
        gh.check(gh.ERR_TOO_LARGE, "sample_mesh_points")
    out = torch.empty((V + M, 3), dtype=torch.float64, device=dev)
    out[:V].copy_(v)
    _call("radegs_mesheval_sample_emit", dev, V, F, v, f, float(density), ws, M, ctypes.c_void_p(out.data_ptr() + 24 * V))
    return out, counts


# ----------------------------------------------------------------------- the grid -----------------------------------------------------------------------
class PointGrid:
    """A uniform grid of `cell` over `points` (float64 [N,3], N >= 1, kept by reference).  .nearest() answers eval.py's kneighbors calls."""

    def __init__(self, points, cell):
        self.points = gh.points(points, "points")
        gh.positive(cell, "cell")
        if self.points.shape[0] == 0:
            raise RuntimeError("`points` is empty: a grid needs at least one point")
        gh.finite(self.points, "points")
        self.cell, self.n, self.device = float(cell), self.points.shape[0], self.points.device
        self.origin = gh.doubles(self.points.amin(dim=0).tolist())
        self.nbytes = _lib().radegs_mesheval_grid_bytes(self.n)
        if self.nbytes == 0:
            gh.check(gh.ERR_TOO_LARGE, "PointGrid")
        self.ws = gh.workspace(self.nbytes, self.device)
        _call("radegs_mesheval_grid_build", self.device, self.n, self.points, self.origin, self.cell, self.ws, self.nbytes)

    @torch.no_grad()
    def nearest(self, queries, max_dist):
        """(dist float64 [Q], index int64 [Q]) of the nearest grid point where its distance is < max_dist, else (inf, -1)"""
        q = gh.points(queries, "queries")
        if q.device != self.device:
            raise RuntimeError("`queries` must be on the grid's device")
        gh.positive(max_dist, "max_dist")
        if math.ceil(max_dist / self.cell) > 511:
            raise RuntimeError("`max_dist` is more than 511 cells: build the grid with a larger cell")
        Q = q.shape[0]
        dist = torch.empty(Q, dtype=torch.float64, device=self.device)
        index = torch.empty(Q, dtype=torch.int64, device=self.device)
        _call("radegs_mesheval_nearest", self.device, self.n, self.ws, self.origin, self.cell, Q, q, float(max_dist), dist, index)
        return dist, index


@torch.no_grad()
def mean_below(dist, max_dist):
    """(sum, count) of dist < max_dist as a float64 [2] GPU tensor, summed in a fixed order"""
    _C._require_gpu(dist, "dist")
    if dist.dtype != torch.float64 or dist.dim() != 1:
        raise RuntimeError("`dist` must be a float64 vector")
    d, dev = dist.contiguous(), dist.device
    nbytes = _lib().radegs_mesheval_sum_bytes()
    ws = gh.workspace(nbytes, dev)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    _call("radegs_mesheval_sum_below", dev, d.shape[0], d, float(max_dist), ws, nbytes, out)
    return out


# -------------------------------------------------------------------- radius thinning --------------------------------------------------------------------
@torch.no_grad()
def downsample_points(points, radius, perm=None, generator=None):
    """eval.py:80-94.  Shuffles `points` (float64 [N,3]) by `perm` (int64 [N]; drawn from `generator`, or torch's global one, when None), then
    keeps the lexicographically first maximal independent set of the graph d^2 <= radius^2 in shuffled order -- what the reference's
    sequential loop keeps.  Returns (kept points in shuffled order, keep mask bool [N] in shuffled order, perm)."""
    p = gh.points(points, "points")
    gh.positive(radius, "radius")
    N, dev = p.shape[0], p.device
    if perm is None:
        g = generator
        perm = torch.randperm(N, generator=g, device=g.device if g is not None else dev).to(dev)
    else:
        _C._require_gpu(perm, "perm")
        if perm.dtype != torch.int64 or tuple(perm.shape) != (N,):
            raise RuntimeError(f"`perm` must be an int64 tensor of shape ({N},)")
        if N and not bool(torch.equal(torch.sort(perm).values, torch.arange(N, device=dev))):
            raise RuntimeError("`perm` is not a permutation of 0..N-1")
    if N == 0:
        return p.clone(), torch.zeros(0, dtype=torch.bool, device=dev), perm
    shuffled = p[perm].contiguous()
    grid = PointGrid(shuffled, float(radius) * CELL_SLACK)
    state = torch.zeros(N, dtype=torch.uint8, device=dev)
    undecided = torch.full((1,), N, dtype=torch.int64, device=dev).to(torch.int32)   # read as unsigned by the kernel; N < 2^32 - 65 536
    while True:                            # no cap: a cloud ordered along a line needs as many rounds as it has points
        _call("radegs_mesheval_thin_rounds", dev, N, grid.ws, grid.origin, grid.cell, float(radius), ROUNDS_PER_READ, state, undecided)
        if int(undecided.item()) == 0:     # one host read per batch of rounds
            break
    keep = state == 1
    return shuffled[keep], keep, perm


# ------------------------------------------------------------------------- masks -------------------------------------------------------------------------
@torch.no_grad()
def obs_mask_select(points, obs_mask, BB, Res, patch=60):
    """eval.py:102-110 on `points` (float64 [N,3]).  `obs_mask`: the ObsMask volume [d0,d1,d2] (a bool / uint8 GPU tensor, or a numpy array as
    loadmat returns it); `BB` [2,3] (taken to float32 as the reference does), `Res` a scalar.  Returns three bool [N] masks over `points`:
    inbound; inbound and inside the volume's index range; that and ObsMask set -- the reference's `inbound`, `grid_inbound` and `in_obs`
    scattered back to full length."""
    p = gh.points(points, "points")
    dev = p.device
    if isinstance(obs_mask, np.ndarray):
        obs_mask = torch.from_numpy(np.ascontiguousarray(obs_mask != 0).view(np.uint8)).to(dev)
    _C._require_gpu(obs_mask, "obs_mask")
    if obs_mask.dim() != 3 or obs_mask.dtype not in (torch.uint8, torch.bool) or 0 in obs_mask.shape:
        raise RuntimeError("`obs_mask` must be a non-empty bool or uint8 volume of three dimensions")
    vol = obs_mask.contiguous().view(torch.uint8)
    bb = np.asarray(BB.cpu() if isinstance(BB, torch.Tensor) else BB).astype(np.float32)
    res = float(np.asarray(Res.cpu() if isinstance(Res, torch.Tensor) else Res).reshape(-1)[0])
    if bb.shape != (2, 3) or not np.isfinite(bb).all() or not (math.isfinite(res) and res > 0):
        raise RuntimeError("`BB` must be a finite (2,3) array and `Res` a positive number")
    patch = float(patch)                               # a Python scalar leaves the sums below in float32, as the reference's
    lo, hi = bb[0] - patch, bb[1] + patch * 2
    box = gh.doubles(list(lo.astype(np.float64)) + list(hi.astype(np.float64)) + list(bb[0].astype(np.float64)) + [res])
    dims = (ctypes.c_int * 3)(*vol.shape)
    N = p.shape[0]
    out = torch.zeros((3, N), dtype=torch.uint8, device=dev)
    _call("radegs_mesheval_obs_mask", dev, N, p, box, dims, vol, out[0], out[1], out[2])
    return out[0].bool(), out[1].bool(), out[2].bool()


@torch.no_grad()
def above_plane(points, plane):
    """eval.py:128-130: (P . [x, y, z, 1]) > 0 as a bool [N] mask"""
    p = gh.points(points, "points")
    pl = np.asarray(plane.cpu() if isinstance(plane, torch.Tensor) else plane, dtype=np.float64).reshape(-1)
    if pl.shape != (4,) or not np.isfinite(pl).all():
        raise RuntimeError("`plane` must hold four finite numbers")
    out = torch.zeros(p.shape[0], dtype=torch.uint8, device=p.device)
    _call("radegs_mesheval_above_plane", p.device, p.shape[0], p, gh.doubles(pl), out)
    return out.bool()


# ------------------------------------------------------------------------ chamfer ------------------------------------------------------------------------
@torch.no_grad()
def dtu_chamfer(vertices, faces, stl_points, obs_mask, BB, Res, plane, *, density=0.2, patch_size=60, max_dist=20, perm=None, generator=None):
    """dtu_eval/eval.py in mesh mode, everything on the GPU.  Returns results.json's `mean_d2s`, `mean_s2d`, `overall` (Python floats) and what
    the reference's visualisation step consumes: data_pcd, perm, keep (shuffled order), data_down, inbound / grid_inbound / in_obs (over
    data_down), data_in, data_in_obs, dist_d2s / idx_d2s (over data_in_obs, indices into stl_points), above (over stl_points), stl_above,
    dist_s2d / idx_s2d (over stl_above, indices into data_in).  Distances of max_dist or more read inf, their index -1."""
    stl = gh.points(stl_points, "stl_points")
    if stl.shape[0] == 0:
        raise RuntimeError("`stl_points` is empty")
    gh.finite(stl, "stl_points")
    data_pcd, counts = sample_mesh_points(vertices, faces, density)
    data_down, keep, perm = downsample_points(data_pcd, density, perm=perm, generator=generator)
    inbound, grid_inbound, in_obs = obs_mask_select(data_down, obs_mask, BB, Res, patch_size)
    data_in, data_in_obs = data_down[inbound], data_down[in_obs]
    if data_in.shape[0] == 0:
        raise RuntimeError("dtu_chamfer: no point of the mesh lies inside the bounding box")
    cell = float(max_dist) / NN_CELLS_PER_MAX_DIST
    dist_d2s, idx_d2s = PointGrid(stl, cell).nearest(data_in_obs, max_dist)
    above = above_plane(stl, plane)
    stl_above = stl[above]
    dist_s2d, idx_s2d = PointGrid(data_in, cell).nearest(stl_above, max_dist)
    sums = torch.stack([mean_below(dist_d2s, max_dist), mean_below(dist_s2d, max_dist)]).cpu().numpy()   # one host read for both means
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_d2s, mean_s2d = float(sums[0, 0] / sums[0, 1]), float(sums[1, 0] / sums[1, 1])               # the mean of nothing is nan, as numpy's
    return dict(mean_d2s=mean_d2s, mean_s2d=mean_s2d, overall=(mean_d2s + mean_s2d) / 2, data_pcd=data_pcd, counts=counts, perm=perm, keep=keep,
                data_down=data_down, inbound=inbound, grid_inbound=grid_inbound, in_obs=in_obs, data_in=data_in, data_in_obs=data_in_obs,
                dist_d2s=dist_d2s, idx_d2s=idx_d2s, above=above, stl_above=stl_above, dist_s2d=dist_s2d, idx_s2d=idx_s2d)


# -------------------------------------------------------------------------- cull --------------------------------------------------------------------------
def _mask_u8(mask, name):
    _C._require_gpu(mask, name)
    m = mask.detach()
    if m.dim() == 3 and m.size(0) >= 1:
        m = m[0]                                # the reference reads channel 0 of gt_mask
    if m.dim() != 2 or 0 in m.shape:
        raise RuntimeError(f"`{name}` must be a non-empty [H,W] or [C,H,W] tensor")
    return (m != 0).to(torch.uint8).contiguous()


@torch.no_grad()
def dilate_mask(mask, radius=6):
    """skimage's binary_dilation(mask, disk(radius)): `mask` [H,W] (non-zero = set) -> bool [H,W]; pixels outside the image are clear"""
    m = _mask_u8(mask, "mask")
    if not isinstance(radius, int) or not 0 <= radius <= 64:
        raise RuntimeError("`radius` must be an integer in [0, 64]")
    out = torch.empty_like(m)
    _call("radegs_mesheval_dilate", m.device, m.shape[1], m.shape[0], m, radius, out)
    return out.bool()


def _camera_fields(cam, mask):
    """(w2c float32 [4,4] on the CPU, fx, fy, W, H, mask) from a tuple or from an object with the reference's camera attributes"""
    if isinstance(cam, (tuple, list)):
        w2c, fx, fy, W, H, m = cam
    else:
        W, H = int(cam.image_width), int(cam.image_height)
        fx, fy = W / (2 * math.tan(cam.FoVx / 2)), H / (2 * math.tan(cam.FoVy / 2))
        w2c, m = cam.world_view_transform.T, cam.gt_mask      # inverse(inverse(world_view_transform.T)) up to rounding
    w2c = torch.as_tensor(w2c).detach().to("cpu", torch.float32)
    if tuple(w2c.shape) != (4, 4) or not bool(torch.isfinite(w2c).all()):
        raise RuntimeError("a camera's w2c must be a finite 4x4 matrix")
    if int(W) < 2 or int(H) < 2:
        raise RuntimeError("a camera's image must be at least 2x2")
    return w2c, float(fx), float(fy), int(W), int(H), (m if mask is None else mask)


@torch.no_grad()
def cull_mesh(vertices, faces, cameras, masks=None, dilation=6):
    """evaluate_dtu_mesh.cull_mesh: keeps a vertex iff every camera either sees it outside its image or on a set pixel of its mask dilated
    by `dilation`; keeps the faces whose three vertices are kept and renumbers them.  `vertices` float32 or float64 [V,3] (projected in
    float32, as upstream), `faces` int [F,3]; `cameras`: objects with world_view_transform / FoVx / FoVy / image_width / image_height /
    gt_mask, or tuples (w2c, fx, fy, W, H, mask); `masks[i]` replaces camera i's mask.  Returns (vertices, faces int64)."""
    if not isinstance(vertices, torch.Tensor) or vertices.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("`vertices` must be a float32 or float64 tensor")
    gh.faces_type(faces)
    v_in = gh.points(vertices, "vertices", vertices.dtype)
    f = gh.faces(faces, v_in.shape[0])
    gh.finite(v_in, "vertices")
    dev, NV, NF = v_in.device, v_in.shape[0], f.shape[0]
    v32 = v_in.float()
    table, dilated, offset = (RadegsCullCamera * max(len(cameras), 1))(), [], 0
    for i, cam in enumerate(cameras):
        w2c, fx, fy, W, H, m = _camera_fields(cam, None if masks is None else masks[i])
        m = _mask_u8(m, "mask")
        if m.device != dev or tuple(m.shape) != (H, W):
            raise RuntimeError(f"camera {i}: its mask must be a ({H},{W}) tensor on the vertices' device")
        K = torch.eye(4)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, W / 2.0, H / 2.0
        table[i].m[:] = (K @ w2c)[:3].reshape(-1).tolist()
        table[i].W, table[i].H, table[i].mask_offset = W, H, offset
        dilated.append(dilate_mask(m, dilation).view(torch.uint8).reshape(-1))
        offset += W * H
    flags = torch.ones(NV, dtype=torch.int32, device=dev)
    nbytes = _lib().radegs_tetmesh_filter_plan_bytes(NV, NF)
    ws = gh.workspace(nbytes, dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    if cameras:
        cam_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        all_masks = torch.cat(dilated)
        _call("radegs_mesheval_cull_vertices", dev, NV, v32, len(cameras), cam_dev, all_masks, flags)
    _call("radegs_tetmesh_filter_plan_flags", dev, NV, NF, flags, f, ws, nbytes, counts)
    nv, nf = counts.tolist()               # the one host read
    out_v = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((nf, 3), dtype=torch.int64, device=dev)
    _call("radegs_tetmesh_filter_apply", dev, NV, NF, v32, f, ws, nv, nf, out_v, out_f)
    if v_in.dtype == torch.float64:            # the kept rows of the caller's own precision
        out_v = v_in[flags.bool()]
    return out_v, out_f


# ---------------------------------------------------------------------- from paths to the numbers ----------------------------------------------------------------------
def _camera_centre(cam):
    """evaluate_dtu_mesh.py:153-155: c2w[:3, 3] of (world_view_transform.T).inverse(), float32 as torch computes it on the host"""
    w2c = cam[0] if isinstance(cam, (tuple, list)) else cam.world_view_transform.T
    return torch.as_tensor(w2c).detach().to("cpu", torch.float32).inverse()[:3, 3].numpy()


@torch.no_grad()
def evaluate_dtu_mesh(mesh_path, cameras, dataset_dir, scan, out_dir=None, perm=None, generator=None, device="cuda"):
    """evaluate_dtu_mesh.py:141-194 with dtu_eval/eval.py from paths alone: the training cameras' centres are aligned to those of
    dataset_dir/Calibration/cal18/pos_XXX.txt (scale, then best_fit_transform), the mesh is read, culled (cull_mesh), scaled and moved, and
    scored against dataset_dir/Points/stl/stl{scan:03}_total.ply with the ObsMask and Plane files (dtu_chamfer).  `cameras` as cull_mesh
    takes them.  With `out_dir`: recon_culled.ply, recon_aligned.ply and results.json are written there.  Returns dtu_chamfer's dict with
    `scale`, `R`, `t` and the aligned `vertices` / `faces` added."""
    import json
    import os

    import eval_io
    import tetmesh
    points = np.array([_camera_centre(cam) for cam in cameras])
    if points.shape[0] < 3:
        raise RuntimeError("evaluate_dtu_mesh needs at least three cameras for the alignment")
    gt_points = eval_io.dtu_camera_centres(os.path.join(dataset_dir, "Calibration", "cal18"), n=min(64, points.shape[0]))
    scale_gt, scale, r, t = eval_io.dtu_alignment(points[:64], gt_points)
    obs_mask, BB, Res, plane = eval_io.load_dtu_masks(dataset_dir, scan)
    v, f = eval_io.read_ply_mesh(mesh_path, device)
    v, f = cull_mesh(v, f, cameras)
    dev = v.device
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        tetmesh.write_ply(os.path.join(out_dir, "recon_culled.ply"), v, f)
    v = v * float(scale_gt) / float(scale)                                                  # :180-181
    v = v @ torch.from_numpy(np.asarray(r.T, dtype=np.float64)).to(dev) + torch.from_numpy(np.asarray(t, dtype=np.float64)).to(dev)
    v = v.contiguous()
    if out_dir is not None:
        tetmesh.write_ply(os.path.join(out_dir, "recon_aligned.ply"), v, f)
    stl = eval_io.read_ply_points(os.path.join(dataset_dir, "Points", "stl", f"stl{int(scan):03}_total.ply"), device)
    res = dtu_chamfer(v, f, stl, obs_mask, BB, Res, plane, perm=perm, generator=generator)
    if out_dir is not None:
        with open(os.path.join(out_dir, "results.json"), "w") as fp:
            json.dump({"mean_d2s": res["mean_d2s"], "mean_s2d": res["mean_s2d"], "overall": res["overall"]}, fp, indent=True)
    res.update(scale=float(scale_gt) / float(scale), R=r, t=t, vertices=v, faces=f)
    return res
