"""HIP-backed unbounded mesh extraction: the reference's GaussianExtractor.extract_mesh_unbounded, utils/mesh_utils.py:162-270
with utils/mcube_utils.py and focus_point_fn of utils/render_utils.py -- the 2DGS-style route for unbounded scenes: a TSDF fused over a
contracted cube, sampled densely, meshed crop by crop, welded, uncontracted and coloured.  Upstream needs open3d, trimesh and skimage and
runs the marching cubes on the host; here the depth and colour maps stay on the GPU from the renderer to the mesh.  GPU only.  The
specification is include/radegs.h, "Unbounded mesh extraction" (DESIGN 11 N17 lists the deviations and what is restated from memory).

Not here: extract_mesh_bounded (Open3D's ScalableTSDFVolume -- tsdf.py is this project's bounded route), depth_to_normal and export_image
(no mesh depends on them), the video and trajectory helpers of render_utils.py."""
import ctypes
from functools import partial

import numpy as np
import torch

import geom_host as gh
import tsdf as _tsdf
from diff_gaussian_rasterization import _C
from geom_host import f32, i32, ll, pf32, sz, vp

ZRUN, BRICK = 0, 1          # RADEGS_UNBOUNDED_ZRUN / _BRICK: how a wave's lanes map to the samples of a lattice (same bits either way)
# the mapping of lattice-mode fuses: bricks project to compact patches of every map (DESIGN 11 N17 has the measurement)
DEFAULT_MAPPING = BRICK
pi32 = ctypes.POINTER(ctypes.c_int)

SIGNATURES = {
    "radegs_unbounded_fuse": (i32, [ll, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, f32, pf32, f32, vp, vp, vp]),
    "radegs_unbounded_uncontract": (i32, [ll, vp, f32, pf32, f32, vp, vp]),
    "radegs_densemc_bytes": (sz, [i32, i32, i32]),
    "radegs_densemc_plan": (i32, [vp, i32, i32, i32, vp, sz, vp, vp]),
    "radegs_densemc_emit": (i32, [vp, vp, vp, vp, i32, i32, i32, pi32, ll, vp, ll, ll, vp, vp, vp, vp]),
}
_SIGNATURES = SIGNATURES
# RadegsUnboundedView (include/radegs.h): 16 floats, W, H, two pointers -- 88 bytes
_VIEW = np.dtype([("m", "<f4", (16,)), ("W", "<i4"), ("H", "<i4"), ("depth", "<u8"), ("rgb", "<u8")])
assert _VIEW.itemsize == 88


def _lib():
    return gh.bind(_SIGNATURES)


_call = partial(gh.call, _SIGNATURES)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _floats3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


# ---------------------------------------------------------------------- host helpers ----------------------------------------------------------------------
# Small, not hot: float64 NumPy, once per scene.
def contract(x):
    """world (normalised) -> contracted: x if |x| < 1, else (2 - 1 / |x|) x / |x|; float64 [..., 3]"""
    x = np.asarray(_host(x), np.float64)
    with np.errstate(all="ignore"):
        mag = np.linalg.norm(x, axis=-1)[..., None]
        return np.where(mag < 1, x, (2 - 1 / mag) * (x / mag))


def uncontract(y):
    """contracted -> world (normalised): y if |y| < 1, else y / (|y| (2 - |y|)); float64 [..., 3]"""
    y = np.asarray(_host(y), np.float64)
    with np.errstate(all="ignore"):
        mag = np.linalg.norm(y, axis=-1)[..., None]
        return np.where(mag < 1, y, (1 / (2 - mag)) * (y / mag))


def focus_point(poses):
    """the point nearest to all optical axes of camera-to-world poses [n,3,4] (column 2: the axis, column 3: the origin)"""
    poses = np.asarray(poses, np.float64)
    d, o = poses[:, :3, 2:3], poses[:, :3, 3:4]
    m = np.eye(3) - d * np.transpose(d, [0, 2, 1])
    mt_m = np.transpose(m, [0, 2, 1]) @ m
    return np.linalg.inv(mt_m.mean(0)) @ (mt_m @ o).mean(0)[:, 0]


def scene_normalisation(views):
    """(center float64 [3], radius float64): the focus point of the cameras and the distance of the nearest one to it.  `views`: objects
    with a `world_view_transform` (row-vector 4x4), or such matrices."""
    mats = [np.asarray(_host(getattr(v, "world_view_transform", v))) for v in views]
    if not mats or any(m.shape != (4, 4) for m in mats):
        raise RuntimeError("scene_normalisation: needs at least one view with a 4x4 world_view_transform")
    # as upstream: the inverse is taken in the matrices' own type (float32 for the renderer's cameras), everything after it in float64
    c2w = np.array([np.linalg.inv(m.T) for m in mats])
    center = focus_point(c2w[:, :3, :] @ np.diag([1.0, -1.0, -1.0, 1.0]))
    return center, np.linalg.norm(c2w[:, :3, 3] - center, axis=-1).min()


def contracted_bound(xyz, center, radius):
    """R = min(quantile_0.95 of the contracted norms of the normalised points + 0.01, 1.9).  The norms are float32, as upstream computes
    them (its points are a float32 tensor); the quantile is np.quantile, as upstream's."""
    F = np.float32
    x = (np.asarray(_host(xyz), F).reshape(-1, 3) - np.asarray(center, np.float64).astype(F)) / F(radius)
    with np.errstate(all="ignore"):
        mag = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])[:, None]
        c = np.where(mag < 1, x, (F(2) - F(1) / mag) * (x / mag)).astype(F)
        n = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    return min(np.quantile(n, q=0.95) + 0.01, 1.9)


# ------------------------------------------------------------------------ the views ------------------------------------------------------------------------
class ViewStack:
    """The views of a fuse, resident on the device: per view the full_proj_transform (row-vector convention, float32), the depth map
    float32 [H,W] (or [1,H,W]) and optionally the colour float32 [3,H,W]; sizes may differ from view to view.  `views`: objects with
    `full_proj_transform` and `world_view_transform`."""

    def __init__(self, views, depths, rgbs=None):
        views, depths = list(views), list(depths)
        rgbs = None if rgbs is None else list(rgbs)
        if len(depths) != len(views) or (rgbs is not None and len(rgbs) != len(views)):
            raise RuntimeError("ViewStack: one depth map (and one colour map) per view")
        self.device = None
        self.depths, self.rgbs, mats = [], [], []
        table = np.zeros(len(views), _VIEW)
        for i, (view, d) in enumerate(zip(views, depths)):
            _C._require_gpu(d, "depths[%d]" % i)
            if self.device is None:
                self.device = d.device
            d = d.detach()
            if d.dim() == 3 and d.size(0) == 1:
                d = d[0]
            if d.dim() != 2 or 0 in d.shape or d.dtype != torch.float32 or d.device != self.device:
                raise RuntimeError(f"`depths[{i}]` must be a non-empty float32 (H,W) or (1,H,W) map on {self.device}, got {tuple(d.shape)} {d.dtype} on {d.device}")
            d = d.contiguous()
            H, W = d.shape
            c = None
            if rgbs is not None:
                c = rgbs[i]
                _C._require_gpu(c, "rgbs[%d]" % i)
                if c.dim() != 3 or tuple(c.shape) != (3, H, W) or c.dtype != torch.float32 or c.device != self.device:
                    raise RuntimeError(f"`rgbs[{i}]` must be float32 (3,{H},{W}) on {self.device}, got {tuple(c.shape)} {c.dtype} on {c.device}")
                c = c.detach().contiguous()
            m = np.asarray(_host(view.full_proj_transform), np.float32)
            if m.shape != (4, 4):
                raise RuntimeError(f"`views[{i}].full_proj_transform` must be 4x4")
            table[i] = (m.reshape(-1), W, H, d.data_ptr(), 0 if c is None else c.data_ptr())
            self.depths.append(d)
            self.rgbs.append(c)
            mats.append(np.asarray(_host(view.world_view_transform)))
        self.world_view = mats
        self.has_rgb = rgbs is not None
        self.n = len(views)
        self.table = None if not self.n else torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(self.device)

    def __len__(self):
        return self.n


def _stack(stack):
    if not isinstance(stack, ViewStack):
        raise RuntimeError("`stack` must be a ViewStack")
    if stack.n == 0:
        raise RuntimeError("unbounded_mesh (MI355X build): an empty ViewStack names no GPU device -- this operator has no CPU implementation")
    return stack


def _axis(a, name, dev):
    if not isinstance(a, torch.Tensor) or a.dim() != 1 or a.dtype != torch.float32 or a.numel() == 0:
        raise RuntimeError(f"`{name}` must be a non-empty float32 tensor of shape (n,)")
    _C._require_gpu(a, name)
    if a.device != dev:
        raise RuntimeError(f"`{name}` must be on {dev}, it is on {a.device}")
    return a.detach().contiguous()


@torch.no_grad()
def fuse_samples(stack, samples, voxel_size, center, radius, contract=True, return_rgb=False, mapping=None):
    """The TSDF of every sample over all views of `stack`, one kernel: `samples` is a float32 [M,3] GPU tensor, or a lattice (ax, ay, az)
    of three float32 GPU vectors whose nx ny nz points, z fastest, are never materialised.  contract=True: the samples are points of the
    contracted cube (center, radius: scene_normalisation's).  Returns tsdf [M], and rgb [M,3] with return_rgb."""
    stack = _stack(stack)
    dev = stack.device
    voxel_size = gh.positive(voxel_size, "voxel_size")
    radius = gh.positive(radius, "radius")
    center = np.asarray(center, np.float64).reshape(-1)
    if center.shape != (3,) or not np.isfinite(center).all():
        raise RuntimeError("`center` must be three finite numbers")
    if return_rgb and not stack.has_rgb:
        raise RuntimeError("return_rgb needs a ViewStack with colour maps")
    mapping = DEFAULT_MAPPING if mapping is None else mapping
    if mapping not in (ZRUN, BRICK):
        raise RuntimeError("`mapping` must be ZRUN or BRICK")
    if isinstance(samples, (tuple, list)):
        if len(samples) != 3:
            raise RuntimeError("a lattice is three coordinate vectors (ax, ay, az)")
        ax, ay, az = (_axis(a, n, dev) for a, n in zip(samples, ("ax", "ay", "az")))
        pts, dims = None, (ax.numel(), ay.numel(), az.numel())
        M = dims[0] * dims[1] * dims[2]
        if M >= 2 ** 31:
            gh.check(gh.ERR_TOO_LARGE, "fuse_samples")
    else:
        pts = gh.points(samples, "samples", torch.float32)
        if pts.device != dev:
            raise RuntimeError(f"`samples` must be on {dev}, it is on {pts.device}")
        ax = ay = az = None
        dims, M = (0, 0, 0), pts.shape[0]
    tsdf = torch.empty(M, dtype=torch.float32, device=dev)
    rgb = torch.empty((M, 3), dtype=torch.float32, device=dev) if return_rgb else None
    trunc5 = float(np.float32(5.0 * voxel_size))
    _call("radegs_unbounded_fuse", dev, M, pts, ax, ay, az, dims[0], dims[1], dims[2], mapping, stack.n, stack.table, 1 if contract else 0,
          float(np.float32(radius)), _floats3(center), trunc5, tsdf, rgb)
    return (tsdf, rgb) if return_rgb else tsdf


@torch.no_grad()
def world_points(contracted, center, radius, max_range=32.0):
    """the vertices after the weld: uncontracted, un-normalised, clamped to +-max_range; float32 [M,3] on the GPU"""
    y = gh.points(contracted, "contracted", torch.float32)
    out = torch.empty_like(y)
    _call("radegs_unbounded_uncontract", y.device, y.shape[0], y, float(np.float32(gh.positive(radius, "radius"))), _floats3(center),
          gh.positive(max_range, "max_range"), out)
    return out


# ------------------------------------------------------------------ dense marching cubes ------------------------------------------------------------------
@torch.no_grad()
def dense_marching_cubes(values, ax, ay, az, lattice_offset=(0, 0, 0), G=None):
    """marching cubes at level 0 over `values` float32 [nx,ny,nz] with the lattice coordinates ax, ay, az (each at least 2 long):
    (vertices float32 [V,3], keys int64 [V], faces int64 [F,3] into these vertices).  key = ((gx G + gy) G + gz) 3 + axis with
    g = lattice_offset + l: the same edge of two lattices that share a plane has the same key (and the same vertex bits)."""
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32:
        raise RuntimeError("`values` must be a float32 tensor")
    _C._require_gpu(values, "values")
    dev = values.device
    ax, ay, az = (_axis(a, n, dev) for a, n in zip((ax, ay, az), ("ax", "ay", "az")))
    nx, ny, nz = ax.numel(), ay.numel(), az.numel()
    if min(nx, ny, nz) < 2:
        raise RuntimeError("dense_marching_cubes: every axis of the lattice needs at least 2 points")
    if values.numel() != nx * ny * nz:
        raise RuntimeError(f"`values` must hold {nx}x{ny}x{nz} numbers, got {tuple(values.shape)}")
    off = [int(v) for v in lattice_offset]
    G = max(o + n for o, n in zip(off, (nx, ny, nz))) if G is None else int(G)
    if len(off) != 3 or min(off) < 0 or any(o + n > G for o, n in zip(off, (nx, ny, nz))) or G > 2 ** 20:
        raise RuntimeError("`lattice_offset` and `G` must satisfy 0 <= offset, offset + n <= G <= 2^20")
    v = values.detach().contiguous()
    nbytes = _lib().radegs_densemc_bytes(nx, ny, nz)
    if nbytes == 0:
        gh.check(gh.ERR_TOO_LARGE, "dense_marching_cubes")
    ws = gh.workspace(nbytes, dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    _call("radegs_densemc_plan", dev, v, nx, ny, nz, ws, nbytes, counts)
    V, F = counts.tolist()                      # the one host read: the two sizes
    vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int64, device=dev)
    _call("radegs_densemc_emit", dev, v, ax, ay, az, nx, ny, nz, (ctypes.c_int * 3)(*off), G, ws, V, F, vertices, keys, faces)
    return vertices, keys, faces


@torch.no_grad()
def weld(parts):
    """[(vertices, keys, faces)] in crop order -> (vertices ascending by key, duplicates removed; faces re-indexed, order kept).  torch.unique
    on the device sorts the keys; duplicates of a key carry the same bits (the spec's point), the first occurrence is taken."""
    parts = [p for p in parts if p[0].shape[0]]
    if not parts:
        return None, None
    v = torch.cat([p[0] for p in parts])
    k = torch.cat([p[1] for p in parts])
    base = np.cumsum([0] + [p[0].shape[0] for p in parts[:-1]])
    f = torch.cat([p[2] + int(b) for p, b in zip(parts, base)])
    uniq, inverse = torch.unique(k, sorted=True, return_inverse=True)
    first = torch.full((uniq.numel(),), k.numel(), dtype=torch.int64, device=k.device)
    first.scatter_reduce_(0, inverse, torch.arange(k.numel(), device=k.device), reduce="amin")
    return v[first], inverse[f]


def crop_axes(R, resolution, crop_resolution):
    """per crop index the float32 lattice coordinates [crop]: float32(linspace(xs[i], xs[i+1], crop)), xs = linspace(-R, R, N + 1)"""
    N = resolution // crop_resolution
    xs = np.linspace(-R, R, N + 1)
    return [np.linspace(xs[i], xs[i + 1], crop_resolution).astype(np.float32) for i in range(N)]


@torch.no_grad()
def extract_mesh_unbounded(stack, xyz, resolution=1024, crop_resolution=512, max_range=32.0, timings=None):
    """mesh_utils.py:162-270: (vertices float32 [V,3] in the world, faces int64 [F,3], colors float32 [V,3]) on the GPU.  `xyz`: the
    Gaussians' centres (they set the bound R of the contracted cube).  Upstream fixes the crop at 512 and asserts resolution % 512 == 0;
    here the crop is a parameter with that default.  `timings`: a dict that receives device-synchronised seconds per stage."""
    for name, v in (("resolution", resolution), ("crop_resolution", crop_resolution)):
        if not isinstance(v, int) or isinstance(v, bool) or v < 2:
            raise RuntimeError(f"`{name}` must be an integer >= 2")
    if resolution % crop_resolution != 0:
        raise RuntimeError(f"`resolution` ({resolution}) must be a multiple of `crop_resolution` ({crop_resolution})")
    gh.positive(max_range, "max_range")
    stack = _stack(stack)
    if not stack.has_rgb:
        raise RuntimeError("extract_mesh_unbounded needs a ViewStack with colour maps")
    dev = stack.device
    center, radius = scene_normalisation(stack.world_view)
    voxel_size = radius * 2 / resolution
    R = contracted_bound(xyz, center, radius)
    axes = [torch.from_numpy(a).to(dev) for a in crop_axes(R, resolution, crop_resolution)]
    N, step = len(axes), crop_resolution - 1
    G = N * step + 1
    clock = _Clock(dev, timings)
    parts = []
    for i in range(N):
        for j in range(N):
            for k in range(N):
                values = fuse_samples(stack, (axes[i], axes[j], axes[k]), voxel_size, center, radius, contract=True)
                clock.add("fuse")
                parts.append(dense_marching_cubes(values, axes[i], axes[j], axes[k], (i * step, j * step, k * step), G))
                clock.add("marching_cubes")
    y, faces = weld(parts)
    clock.add("weld")
    if y is None:
        e = torch.empty((0, 3), dtype=torch.float32, device=dev)
        return e, torch.empty((0, 3), dtype=torch.int64, device=dev), e.clone()
    vertices = world_points(y, center, radius, max_range)
    _, colors = fuse_samples(stack, vertices, voxel_size, center, radius, contract=False, return_rgb=True)
    clock.add("colouring")
    return vertices, faces, colors


class _Clock:
    def __init__(self, dev, out):
        self.dev, self.out = dev, out
        if out is not None:
            import time
            self.time = time.perf_counter
            torch.cuda.synchronize(dev)
            self.t = self.time()

    def add(self, name):
        if self.out is None:
            return
        torch.cuda.synchronize(self.dev)
        now = self.time()
        self.out[name] = self.out.get(name, 0.0) + (now - self.t)
        self.t = now


class GaussianExtractor:
    """mesh_utils.py:65-117, 162-270: renders every view once, keeps the colour and median-depth maps on the device, and extracts the
    unbounded mesh from them.  Upstream reads render_pkg['middepth']; this renderer's package calls that map `median_depth`."""

    def __init__(self, gaussians, render, pipe, bg_color=None):
        self.gaussians = gaussians
        self._render, self._pipe = render, pipe
        self._bg = [0, 0, 0] if bg_color is None else bg_color
        self.clean()

    def clean(self):
        self.stack, self.viewpoint_stack = None, []

    @torch.no_grad()
    def reconstruction(self, viewpoint_stack):
        self.clean()
        self.viewpoint_stack = list(viewpoint_stack)
        depths, rgbs, render = [], [], None
        for view in self.viewpoint_stack:
            if render is None:
                dev = view.full_proj_transform.device if isinstance(view.full_proj_transform, torch.Tensor) and view.full_proj_transform.is_cuda else "cuda"
                render = partial(self._render, pipe=self._pipe, bg_color=torch.tensor(self._bg, dtype=torch.float32, device=dev))
            pkg = render(view, self.gaussians)
            rgbs.append(pkg["render"][:3].detach().float().contiguous())
            depths.append(pkg["median_depth"].detach().float())
        self.stack = ViewStack(self.viewpoint_stack, depths, rgbs)

    @torch.no_grad()
    def extract_mesh_unbounded(self, resolution=1024, crop_resolution=512, max_range=32.0):
        if self.stack is None:
            raise RuntimeError("GaussianExtractor: call reconstruction(viewpoint_stack) first")
        return extract_mesh_unbounded(self.stack, self.gaussians.get_xyz, resolution, crop_resolution, max_range)

    @staticmethod
    def write_ply(path, vertices, faces, colors=None):
        _tsdf.write_ply(path, vertices, faces, colors)
