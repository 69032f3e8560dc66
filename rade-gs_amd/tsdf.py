"""HIP-backed TSDF fusion: the reference's DTU route from a trained model to recon.ply, mesh_extract.py:51-105 -- render
every training view, fuse the median depth maps into a truncated signed distance volume, extract a triangle mesh -- which upstream
hands to Open3D's VoxelBlockGrid on the CPU.  Here the volume lives on the GPU from the first depth map to the mesh: `VoxelBlockGrid`
has upstream's three calls (compute_unique_block_coordinates, integrate, extract_triangle_mesh), `fuse_views` is the loop around them.
GPU only.  The specification is include/radegs.h, "TSDF fusion" (DESIGN 11 N9 says which of its points are from memory of Open3D)."""
import ctypes
import functools
import math

import numpy as np
import torch

import geom_host as gh
from diff_gaussian_rasterization import _C
from geom_host import f32, i32, ll, pf32, sz, vp

BLOCK_RESOLUTION = 16        # the kernels' block: 16^3 voxels, one workgroup of 256 threads walks it in 16 steps
COORD_LIMIT = 1 << 20        # block coordinates live in [-2^20, 2^20): 21 bits per axis of the 63-bit key
MAX_BLOCKS = (1 << 19) - 1   # radegs_tsdf_extract_*: every voxel index below 2^31

_SIGNATURES = {
    "radegs_tsdf_unique_bytes": (sz, [ll]),
    "radegs_tsdf_touch": (i32, [i32, i32, vp, pf32, f32, f32, f32, f32, vp, sz, vp, vp]),
    "radegs_tsdf_unique_plan": (i32, [ll, vp, ll, vp, vp, sz, vp, vp]),
    "radegs_tsdf_unique_emit": (i32, [ll, vp, ll, vp, vp]),
    "radegs_tsdf_insert_apply": (i32, [ll, vp, ll, vp, vp, ll, ll, vp, vp, vp, vp, vp]),
    "radegs_tsdf_integrate": (i32, [ll, vp, vp, ll, i32, i32, vp, vp, pf32, f32, f32, f32, vp, vp, vp, vp]),
    "radegs_tsdf_extract_bytes": (sz, [ll]),
    "radegs_tsdf_extract_plan": (i32, [ll, vp, vp, vp, vp, f32, vp, sz, vp, vp]),
    "radegs_tsdf_extract_emit": (i32, [ll, vp, vp, vp, vp, f32, vp, ll, ll, vp, vp, vp, vp]),
}


def _lib():
    return gh.bind(_SIGNATURES)


_call = functools.partial(gh.call, _SIGNATURES)


def _matrix(m, name, shape):
    """a finite float64 matrix on the host, from a tensor, an array or nested lists"""
    a = np.asarray(m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m, dtype=np.float64)
    if a.shape != shape or not np.isfinite(a).all():
        raise RuntimeError(f"`{name}` must be a finite {shape[0]}x{shape[1]} matrix")
    return a


def _image(t, name, shape=None, channels=None):
    """shape and type of an image: float32 [H,W] or [H,W,channels]; anything else is refused, nothing is converted silently"""
    dims = 2 if channels is None else 3
    if not isinstance(t, torch.Tensor) or t.dim() != dims or (channels is not None and t.size(2) != channels) or 0 in t.shape:
        want = "(H,W)" if channels is None else f"(H,W,{channels})"
        raise RuntimeError(f"`{name}` must be a non-empty tensor of shape {want}" + (f", got {tuple(t.shape)}" if isinstance(t, torch.Tensor) else ""))
    if t.dtype != torch.float32:
        raise RuntimeError(f"`{name}` must be float32, got {str(t.dtype).replace('torch.', '')}")
    if shape is not None and tuple(t.shape[:2]) != tuple(shape):
        raise RuntimeError(f"`{name}` must be {shape[0]}x{shape[1]} like `depth`, got {t.shape[0]}x{t.shape[1]}")


def _block_coords(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.size(1) != 3:
        raise RuntimeError(f"`{name}` must be a tensor of shape (n,3)" + (f", got {tuple(t.shape)}" if isinstance(t, torch.Tensor) else ""))
    if t.dtype != torch.int32:
        raise RuntimeError(f"`{name}` must be int32, got {str(t.dtype).replace('torch.', '')}")


def _on_device(t, name, dev=None):
    """the tensor as the kernels address it, once its shape and type have passed: on the GPU (on `dev` when given), contiguous"""
    _C._require_gpu(t, name)
    if dev is not None and t.device != dev:
        raise RuntimeError(f"`{name}` must be on the grid's device {dev}, it is on {t.device}")
    return t.detach().contiguous()


def _camera16(intrinsic, matrix34):
    fx, fy, cx, cy = intrinsic[0, 0], intrinsic[1, 1], intrinsic[0, 2], intrinsic[1, 2]
    if fx == 0 or fy == 0:
        raise RuntimeError("`intrinsic` has a zero focal length")
    return (ctypes.c_float * 16)(*[float(v) for v in (fx, fy, cx, cy, *matrix34.reshape(-1))])


def _range_error(what):
    raise RuntimeError(f"{what}: a block coordinate is outside [-2^20, 2^20), the range of the grid's 21-bit-per-axis keys -- "
                       "check the pose, depth_scale and voxel_size")


@torch.no_grad()
def unique_block_coordinates(coords):
    """the distinct rows of `coords` (int32 [n,3] on the GPU) in ascending key order (z, then y, then x): the sort and compaction that
    compute_unique_block_coordinates ends with"""
    _block_coords(coords, "coords")
    c = _on_device(coords, "coords")
    dev, n = c.device, c.shape[0]
    nbytes = _lib().radegs_tsdf_unique_bytes(n)
    if n and nbytes == 0:
        gh.check(gh.ERR_TOO_LARGE, "unique_block_coordinates")
    ws = gh.workspace(nbytes, dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    _call("radegs_tsdf_unique_plan", dev, n, c, 0, None, ws, nbytes, counts)
    n_unique, _, bad = counts.tolist()          # the one host read
    if bad:
        _range_error("unique_block_coordinates")
    out = torch.empty((n_unique, 3), dtype=torch.int32, device=dev)
    _call("radegs_tsdf_unique_emit", dev, n, ws, n_unique, out)
    return out


class VoxelBlockGrid:
    """Open3D's VoxelBlockGrid as mesh_extract.py uses it (attributes tsdf, weight and optionally color; 16^3 blocks), on the GPU.
    `block_count` is the initial capacity: when a view needs more the storage doubles (allocate, copy) -- no block is ever dropped.
    The grid: `keys` int64 [n] ascending, `slots` int32 [n] into `tsdf` / `weight` [capacity,4096] and `color` [capacity,4096,3]."""

    def __init__(self, voxel_size=0.002, block_resolution=16, block_count=50000, with_color=True, device="cuda:0"):
        self.voxel_size = gh.positive(voxel_size, "voxel_size")
        if block_resolution != BLOCK_RESOLUTION:
            raise RuntimeError(f"`block_resolution` must be {BLOCK_RESOLUTION}: the kernels are written for 16^3 blocks, got {block_resolution}")
        if not isinstance(block_count, int) or isinstance(block_count, bool) or not 1 <= block_count <= MAX_BLOCKS:
            raise RuntimeError(f"`block_count` must be an integer in [1, {MAX_BLOCKS}]")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("tsdf (MI355X build): VoxelBlockGrid needs a GPU device -- this operator has no CPU implementation")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.with_color = bool(with_color)
        self.block_size = self.voxel_size * BLOCK_RESOLUTION
        self.n, self.capacity = 0, block_count
        self.keys = self.slots = self.tsdf = self.weight = self.color = None       # allocated by the first integrate()

    # ---------------------------------------------------------------- storage ----------------------------------------------------------------
    def _allocate(self, capacity):
        old = (self.tsdf, self.weight, self.color) if self.tsdf is not None else None
        self.capacity = capacity
        self.tsdf = torch.empty((capacity, 4096), dtype=torch.float32, device=self.device)
        self.weight = torch.empty((capacity, 4096), dtype=torch.float32, device=self.device)
        self.color = torch.empty((capacity, 4096, 3), dtype=torch.float32, device=self.device) if self.with_color else None
        if old is not None and self.n:
            self.tsdf[:self.n].copy_(old[0][:self.n])
            self.weight[:self.n].copy_(old[1][:self.n])
            if self.with_color:
                self.color[:self.n].copy_(old[2][:self.n])

    def _reserve(self, blocks):
        if blocks > MAX_BLOCKS:
            raise RuntimeError(f"VoxelBlockGrid: {blocks} blocks, more than the {MAX_BLOCKS} the extraction addresses -- use a larger voxel_size")
        capacity = self.capacity
        while capacity < blocks:
            capacity = min(2 * capacity, MAX_BLOCKS)
        if capacity != self.capacity or self.tsdf is None:
            self._allocate(capacity)

    def _params(self, depth_scale, depth_max, trunc_voxel_multiplier):
        return (gh.positive(depth_scale, "depth_scale"), gh.positive(depth_max, "depth_max"),
                self.voxel_size * gh.positive(trunc_voxel_multiplier, "trunc_voxel_multiplier"))

    def block_coordinates(self):
        """the grid's block coordinates, int32 [n,3] in key order"""
        if self.keys is None:
            return torch.empty((0, 3), dtype=torch.int32, device=self.device)
        k = self.keys
        mask = (1 << 21) - 1
        return torch.stack([(k & mask) - COORD_LIMIT, ((k >> 21) & mask) - COORD_LIMIT, ((k >> 42) & mask) - COORD_LIMIT], 1).to(torch.int32)

    # ------------------------------------------------------------------ touch ------------------------------------------------------------------
    @torch.no_grad()
    def compute_unique_block_coordinates(self, depth, intrinsic, extrinsic, depth_scale=1.0, depth_max=8.0, trunc_voxel_multiplier=8.0):
        """the blocks a depth map touches: int32 [n,3], ascending by key.  `depth` float32 [H,W] on the grid's device; `intrinsic` 3x3,
        `extrinsic` 4x4 world to camera (host; any array type, read as float64)."""
        K, E = _matrix(intrinsic, "intrinsic", (3, 3)), _matrix(extrinsic, "extrinsic", (4, 4))
        _image(depth, "depth")
        scale, dmax, trunc = self._params(depth_scale, depth_max, trunc_voxel_multiplier)
        d = _on_device(depth, "depth", self.device)
        try:
            pose = np.linalg.inv(E)                 # camera to world, in float64
        except np.linalg.LinAlgError:
            raise RuntimeError("`extrinsic` is singular") from None
        cam = _camera16(K, pose[:3])
        H, W = d.shape
        n = 4 * (H // 4) * (W // 4)
        nbytes = _lib().radegs_tsdf_unique_bytes(n)
        ws = gh.workspace(nbytes, self.device)
        counts = torch.zeros(3, dtype=torch.int64, device=self.device)
        _call("radegs_tsdf_touch", self.device, W, H, d, cam, scale, dmax, trunc, self.block_size, ws, nbytes, counts)
        n_unique, _, bad = counts.tolist()      # the one host read
        if bad:
            _range_error("compute_unique_block_coordinates")
        out = torch.empty((n_unique, 3), dtype=torch.int32, device=self.device)
        _call("radegs_tsdf_unique_emit", self.device, n, ws, n_unique, out)
        return out

    # ---------------------------------------------------------------- integrate ----------------------------------------------------------------
    @torch.no_grad()
    def integrate(self, block_coords, depth, color, intrinsic, extrinsic, depth_scale=1.0, depth_max=8.0, trunc_voxel_multiplier=8.0):
        """one view into the blocks of `block_coords` (int32 [n,3]; duplicates count once); blocks new to the grid are inserted first,
        zero-filled.  `color` float32 [H,W,3] in [0, 1], None iff the grid has no colour."""
        if (color is None) == self.with_color:
            raise RuntimeError("`color` must be given for a grid with_color=True and must be None for a grid with_color=False")
        K, E = _matrix(intrinsic, "intrinsic", (3, 3)), _matrix(extrinsic, "extrinsic", (4, 4))
        _block_coords(block_coords, "block_coords")
        _image(depth, "depth")
        if color is not None:
            _image(color, "color", shape=depth.shape, channels=3)
        scale, dmax, trunc = self._params(depth_scale, depth_max, trunc_voxel_multiplier)
        coords, d = _on_device(block_coords, "block_coords", self.device), _on_device(depth, "depth", self.device)
        c = None if color is None else _on_device(color, "color", self.device)
        m = E[:3].copy()
        m[:, :3] *= self.voxel_size                 # a voxel's integer coordinates go straight to the camera
        cam = _camera16(K, m)
        H, W = d.shape
        n = coords.shape[0]
        if n == 0:
            return
        nbytes = _lib().radegs_tsdf_unique_bytes(n)
        if nbytes == 0:
            gh.check(gh.ERR_TOO_LARGE, "integrate")
        ws = gh.workspace(nbytes, self.device)
        counts = torch.zeros(3, dtype=torch.int64, device=self.device)
        _call("radegs_tsdf_unique_plan", self.device, n, coords, self.n, self.keys, ws, nbytes, counts)
        n_unique, n_new, bad = counts.tolist()  # the one host read
        if bad:
            _range_error("integrate")
        self._reserve(self.n + n_new)
        keys = torch.empty(self.n + n_new, dtype=torch.int64, device=self.device)
        slots = torch.empty(self.n + n_new, dtype=torch.int32, device=self.device)
        active_slots = torch.empty(n_unique, dtype=torch.int32, device=self.device)
        active_coords = torch.empty((n_unique, 3), dtype=torch.int32, device=self.device)
        _call("radegs_tsdf_insert_apply", self.device, n, ws, self.n, self.keys, self.slots, n_unique, n_new, keys, slots, active_slots, active_coords)
        if n_new:                               # the new blocks' slots are one range of the storage
            self.tsdf[self.n:self.n + n_new].zero_()
            self.weight[self.n:self.n + n_new].zero_()
            if self.with_color:
                self.color[self.n:self.n + n_new].zero_()
        self.keys, self.slots, self.n = keys, slots, self.n + n_new
        _call("radegs_tsdf_integrate", self.device, n_unique, active_slots, active_coords, self.capacity, W, H, d, c, cam, scale, dmax, trunc,
              self.tsdf, self.weight, self.color)

    # ----------------------------------------------------------------- extract -----------------------------------------------------------------
    @torch.no_grad()
    def extract_triangle_mesh(self, weight_threshold=3.0):
        """marching cubes over the cells whose eight corners all have weight > weight_threshold: (vertices float32 [V,3], faces int64
        [F,3], colors float32 [V,3] or None), in the canonical order of include/radegs.h -- two runs give the same bits"""
        if not (isinstance(weight_threshold, (int, float)) and not isinstance(weight_threshold, bool) and not math.isnan(weight_threshold)):
            raise RuntimeError("`weight_threshold` must be a number")
        dev = self.device
        if self.n == 0:
            return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev),
                    torch.empty((0, 3), dtype=torch.float32, device=dev) if self.with_color else None)
        nbytes = _lib().radegs_tsdf_extract_bytes(self.n)
        ws = gh.workspace(nbytes, dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        _call("radegs_tsdf_extract_plan", dev, self.n, self.keys, self.slots, self.tsdf, self.weight, float(weight_threshold), ws, nbytes, counts)
        V, F = counts.tolist()                  # the one host read: the two sizes
        if V >= 2 ** 32 - 1 or F >= 2 ** 32 - 1:
            gh.check(gh.ERR_TOO_LARGE, "extract_triangle_mesh")
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int64, device=dev)
        colors = torch.empty((V, 3), dtype=torch.float32, device=dev) if self.with_color else None
        _call("radegs_tsdf_extract_emit", dev, self.n, self.keys, self.slots, self.tsdf, self.color, self.voxel_size, ws, V, F, vertices, faces, colors)
        return vertices, faces, colors


def _view_image(t, name, H, W):
    """a map of the renderer ([H,W], [1,H,W] or [C,H,W]: channel 0) as float32 [H,W]"""
    _C._require_gpu(t, name)
    t = t.detach()
    if t.dim() == 3:
        t = t[0]
    if tuple(t.shape) != (H, W):
        raise RuntimeError(f"`{name}` must be a ({H},{W}) map, got {tuple(t.shape)}")
    return t.float()


@torch.no_grad()
def fuse_views(views, render_fn, voxel_size=0.002, depth_max=8.0, alpha_thres=0.5, block_count=50000, depth_scale=1.0, trunc_voxel_multiplier=8.0,
               weight_threshold=3.0, device=None):
    """mesh_extract.py:51-105 without the file system.  Per view: `render_fn(view)` returns the renderer's dict -- `render` [3+,H,W] (the first
    three channels are the colour, clamped to [0, 1] here), `median_depth` and `mask` ([1,H,W] or [H,W]).  The depth is zeroed where the
    view's `gt_mask` < 0.5 (when it has one) and where mask < alpha_thres; intrinsics from FoVx / FoVy with the principal point at the
    centre, extrinsic = world_view_transform.T.  Touch, integrate, extract -- everything stays on the device.  Returns (vertices, faces,
    colors) as VoxelBlockGrid.extract_triangle_mesh does."""
    grid = None
    for view in views:
        out = render_fn(view)
        rgb = out["render"]
        _C._require_gpu(rgb, "render")
        if grid is None:
            grid = VoxelBlockGrid(voxel_size, BLOCK_RESOLUTION, block_count, True, rgb.device if device is None else device)
        W, H = int(view.image_width), int(view.image_height)
        if rgb.dim() != 3 or rgb.size(0) < 3 or tuple(rgb.shape[1:]) != (H, W):
            raise RuntimeError(f"`render` must be [3+,{H},{W}], got {tuple(rgb.shape)}")
        color = rgb[:3].detach().float().clamp(0.0, 1.0).permute(1, 2, 0).contiguous()
        depth = _view_image(out["median_depth"], "median_depth", H, W).clone()
        gt_mask = getattr(view, "gt_mask", None)
        if gt_mask is not None:
            depth[_view_image(gt_mask, "gt_mask", H, W) < 0.5] = 0
        depth[_view_image(out["mask"], "mask", H, W) < alpha_thres] = 0
        K = np.array([[W / (2 * math.tan(view.FoVx / 2)), 0, W / 2], [0, H / (2 * math.tan(view.FoVy / 2)), H / 2], [0, 0, 1]], np.float64)
        E = np.asarray(view.world_view_transform.detach().cpu().numpy(), np.float64).T
        blocks = grid.compute_unique_block_coordinates(depth, K, E, depth_scale, depth_max, trunc_voxel_multiplier)
        grid.integrate(blocks, depth, color, K, E, depth_scale, depth_max, trunc_voxel_multiplier)
    if grid is None:
        raise RuntimeError("fuse_views: no views")
    return grid.extract_triangle_mesh(weight_threshold)


def write_ply(path, vertices, faces, colors=None, normals=None):
    """binary little-endian PLY of a triangle mesh: float32 x y z per vertex, then float32 nx ny nz when `normals` ([V,3], e.g.
    mesh_clean.compute_vertex_normals) is given, then uchar red green blue when `colors` ([V,3] in [0, 1]) is given; `uchar 3, int32 x 3` per
    face.  Without `normals` the file is what it was before the keyword existed, byte for byte."""
    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    v = np.ascontiguousarray(host(vertices), dtype="<f4").reshape(-1, 3)
    f = host(faces).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise RuntimeError("write_ply: a face index is outside the vertices")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % v.shape[0]
    if normals is not None:
        n = np.ascontiguousarray(host(normals), dtype="<f4").reshape(-1, 3)
        if n.shape[0] != v.shape[0]:
            raise RuntimeError("write_ply: `normals` must have one row per vertex")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        c = host(colors).reshape(-1, 3)
        if c.shape[0] != v.shape[0]:
            raise RuntimeError("write_ply: `colors` must have one row per vertex")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % f.shape[0]
    vrec = np.empty(v.shape[0], dtype=fields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        vrec["nx"], vrec["ny"], vrec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if colors is not None:
        c8 = np.rint(np.clip(c.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
        vrec["red"], vrec["green"], vrec["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = f
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
