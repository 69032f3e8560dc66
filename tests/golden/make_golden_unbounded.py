"""Generates tests/golden/unbounded_*.npz from the REFERENCE's own GaussianExtractor.extract_mesh_unbounded (/root/reference,
utils/mesh_utils.py:162-270) run on the CPU.  Build container only.  The npz files hold data: inputs, the reference's results, and the
bookkeeping of the comparison -- none of the reference's text.

open3d, trimesh, skimage and mediapy are stubbed and `cuda` is routed to the CPU, as make_golden_scene_io.py does.  utils.mcube_utils is
replaced by a stand-in whose marching_cubes_with_contraction receives upstream's `sdf`, the box and `inv_contraction`, evaluates `sdf` on
the fixture's sample set and hands back an object whose vertices are the fixture's colouring points, so that upstream's colouring pass
runs over them.  Everything between -- scene normalisation, R, voxel_size, the contraction, the per-sample truncation, the per-view
projection, grid_sample and the running average -- is upstream's code.

Each fixture records two runs of that code: one as upstream runs it (float32), one fed with the same samples, maps and matrices converted
to float64.  `band` is the largest |float32 run - float64 run| over the samples that are kept; a sample is left out when, in float64,
some view has |px| or |py| within 1e-4 of 1, |z| < 1e-4, or |sdf + trunc| < 1e-4 trunc while in view: there the two runs may decide
differently, which is no rounding error.  A fixture that leaves out more than 1 % of its samples is refused."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import unbounded_restatement as ur  # noqa: E402

for name in ("open3d", "trimesh", "skimage", "skimage.measure", "mediapy", "cv2"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["open3d"].utility = types.SimpleNamespace(Vector3dVector=lambda a: a)
sys.path.insert(0, "/root/reference")
for fn in ("zeros", "ones", "empty", "full", "tensor", "rand", "randn"):   # device="cuda" -> CPU
    def _route(*a, __f=getattr(torch, fn), **k):
        if str(k.get("device", "")).startswith("cuda"):
            k.pop("device")
        return __f(*a, **k)
    setattr(torch, fn, _route)
torch.Tensor.cuda = lambda self, *a, **k: self
torch.cuda.empty_cache = lambda: None

captured = {}


class _Mesh:
    def __init__(self, vertices):
        self.vertices, self.vertex_colors = vertices, None

    @property
    def as_open3d(self):
        return self


def _marching_cubes_with_contraction(sdf, resolution=512, bounding_box_min=(-1.0, -1.0, -1.0), bounding_box_max=(1.0, 1.0, 1.0), return_mesh=False,
                                     level=0, simplify_mesh=True, inv_contraction=None, max_range=32.0):
    captured["R"] = float(bounding_box_max[0])
    assert tuple(bounding_box_min) == (-captured["R"],) * 3 and tuple(bounding_box_max) == (captured["R"],) * 3 and level == 0
    captured["tsdf"] = sdf(torch.from_numpy(captured["samples"](captured["R"]))).numpy()
    return _Mesh(captured["colour_points"])


stub = types.ModuleType("utils.mcube_utils")
stub.marching_cubes_with_contraction = _marching_cubes_with_contraction
import utils  # noqa: E402  (the reference's package)
sys.modules["utils.mcube_utils"] = stub
import utils.mesh_utils as mu  # noqa: E402


class _Cam:
    def __init__(self, world_view, full_proj):
        self.world_view_transform, self.full_proj_transform = world_view, full_proj


def run_reference(scene, samples_of_R, colour_points, resolution, dtype):
    """upstream's extract_mesh_unbounded over the scene; dtype float32: as upstream; float64: the same numbers fed as float64"""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32).astype(dtype))
    ex = mu.GaussianExtractor.__new__(mu.GaussianExtractor)
    ex.clean()
    # the world_view_transform stays float32 in both runs: center and radius are float64 host arithmetic over it either way
    ex.viewpoint_stack = [_Cam(torch.from_numpy(np.asarray(wv, np.float32)), t(full)) for wv, (full, _, _) in zip(scene["world_view"], scene["views"])]
    ex.depthmaps = [t(d)[None] for _, d, _ in scene["views"]]
    ex.rgbmaps = [t(c) for _, _, c in scene["views"]]
    ex.depth_normals = [torch.zeros((3,) + d.shape, dtype=t(d).dtype) for _, d, _ in scene["views"]]
    ex.gaussians = types.SimpleNamespace(get_xyz=torch.from_numpy(scene["xyz"]))
    captured["samples"] = lambda R: samples_of_R(R).astype(dtype)
    captured["colour_points"] = np.asarray(colour_points, np.float32)
    # upstream's colour accumulator is torch.zeros(...) of the default type, and index_put refuses float64 values for a float32 destination:
    # the float64 run makes float64 the default for its duration.  Upstream also converts the colouring points (and the centre) with
    # .float(), which a float64 matrix then refuses: in the float64 run .float() keeps float64 (the centre is stored rounded to float32
    # beforehand, so both runs use the same number)
    keep_float = torch.Tensor.float
    if dtype is np.float64:
        torch.set_default_dtype(torch.float64)
        torch.Tensor.float = lambda self, *a, **k: (keep_float(self).double() if self.numel() == 3 and self.dim() == 1 else self.double())
    try:
        mesh = ex.extract_mesh_unbounded(resolution=resolution)
    finally:
        torch.set_default_dtype(torch.float32)
        torch.Tensor.float = keep_float
    return captured["tsdf"].copy(), np.asarray(mesh.vertex_colors).copy(), captured["R"]


def left_out(x, trunc, scene):
    """float64, this file's own arithmetic: which world points x [M,3] sit on a decision of some view"""
    out = np.zeros(len(x), bool)
    for full, depth, _ in scene["views"]:
        m = np.asarray(full, np.float64)
        q = np.concatenate([x, np.ones((len(x), 1))], 1) @ m
        z = q[:, 3]
        with np.errstate(all="ignore"):
            px, py = q[:, 0] / z, q[:, 1] / z
            grid = torch.from_numpy(np.stack([px, py], -1))[None, None]
            d = torch.nn.functional.grid_sample(torch.from_numpy(np.asarray(depth, np.float64))[None, None], grid, mode="bilinear", padding_mode="border",
                                                align_corners=True).reshape(-1).numpy()
            inview = (np.abs(px) < 1) & (np.abs(py) < 1) & (z > 0)
            out |= (np.abs(np.abs(px) - 1) < 1e-4) | (np.abs(np.abs(py) - 1) < 1e-4) | (np.abs(z) < 1e-4)
            out |= inview & (np.abs((d - z) + trunc) < 1e-4 * trunc)
    return out


def make(name, scene, samples_of_R, colour_points, resolution):
    t32, c32, R = run_reference(scene, samples_of_R, colour_points, resolution, np.float32)
    # the float64 run normalises the cloud in float64 and arrives at an R of its own, a few 1e-8 away: both runs get the samples of the
    # float32 run's R, which is the R on record
    t64, c64, R64 = run_reference(scene, lambda _: samples_of_R(R), colour_points, resolution, np.float64)
    assert abs(R - R64) < 1e-6 and t32.dtype == np.float32 and t64.dtype == np.float64
    center, radius = ur.scene_normalisation(scene["world_view"])       # only to locate the decisions; the fixture's own are upstream's below
    voxel = radius * 2 / resolution
    c32f = center.astype(np.float32).astype(np.float64)
    y = samples_of_R(R).astype(np.float64)
    with np.errstate(all="ignore"):
        mag = np.linalg.norm(y, axis=-1)[:, None]
        x = np.where(mag < 1, y, (1 / (2 - mag)) * (y / mag)) * radius + c32f
        n = np.linalg.norm(x, axis=-1)
        trunc = np.where(n > 1, 5 * voxel / (2 - np.minimum(n, 1.9)), 5 * voxel)
    out_t = left_out(x, trunc, scene)
    out_c = left_out(np.asarray(colour_points, np.float64), np.full(len(colour_points), 5 * voxel), scene)
    share_t, share_c = float(out_t.mean()), float(out_c.mean())
    print(name, "left out: samples %.4f %%, colour points %.4f %%" % (100 * share_t, 100 * share_c))
    if share_t > 0.01 or share_c > 0.01:
        raise SystemExit(f"{name}: more than 1 % of the samples sit on a decision; fixture refused")
    same_nan = np.array_equal(np.isnan(t32), np.isnan(t64))
    assert same_nan, "the two runs disagree on where NaN is"
    keep = ~out_t & ~np.isnan(t64)
    band_t = float(np.abs(t32[keep].astype(np.float64) - t64[keep]).max())
    band_c = float(np.abs(c32[~out_c].astype(np.float64) - c64[~out_c].astype(np.float64)).max())
    print(name, "band tsdf %.3e colour %.3e" % (band_t, band_c), "R", R, "integrated", float((t64 != 1).mean()))
    # center, radius, voxel_size as upstream computes them: the same host arithmetic as mesh_utils.py:236-246 -- recorded from a third
    # place, upstream's focus_point_fn itself
    from utils.render_utils import focus_point_fn
    c2ws = np.array([np.linalg.inv(np.asarray(np.asarray(wv, np.float32).T)) for wv in scene["world_view"]])
    poses = c2ws[:, :3, :] @ np.diag([1, -1, -1, 1])
    ref_center = focus_point_fn(poses)
    ref_radius = np.linalg.norm(c2ws[:, :3, 3] - ref_center, axis=-1).min()
    data = dict(full_proj=np.array([v[0] for v in scene["views"]], np.float32), depth=np.array([v[1] for v in scene["views"]], np.float32),
                world_view=np.array(scene["world_view"], np.float32), xyz=scene["xyz"], samples=samples_of_R(R).astype(np.float32),
                colour_points=np.asarray(colour_points, np.float32), resolution=np.asarray(resolution), tsdf32=t32, tsdf64=t64, colour32=c32, colour64=c64,
                left_out=out_t, left_out_colour=out_c, band=np.asarray(band_t), band_colour=np.asarray(band_c), center=ref_center,
                radius=np.asarray(ref_radius), R=np.asarray(R), voxel_size=np.asarray(ref_radius * 2 / resolution))
    path = os.path.join(HERE, f"unbounded_{name}.npz")
    np.savez_compressed(path, **data)
    print(os.path.basename(path), os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


rng = np.random.default_rng(1717)
scene = ur.sphere_scene(pattern=True)
d = rng.standard_normal((1500, 3))
shell = (ur.SPHERE_CENTRE + (ur.SPHERE_RADIUS + rng.uniform(-0.05, 0.15, (1500, 1))) * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)

# the lattice of one crop over the whole cube, 24^3: everything inside the unit ball of the contracted space
make("sphere", scene, lambda R: ur.lattice_points(*[np.linspace(-R, R, 24).astype(np.float32)] * 3), shell, 32)

# samples all over the contracted cube, most of them beyond the unit ball, up to |y| = 1.95: world points up to 40 from the centre, beyond
# the far wall of the depth maps, and world norms on both sides of the 1.9 at which the truncation stops growing
wide = rng.uniform(-1.9, 1.9, (20000, 3)).astype(np.float32)
wide = wide[np.linalg.norm(wide.astype(np.float64), axis=1) < 1.95][:6000]
make("wide", scene, lambda R: wide, shell, 64)
