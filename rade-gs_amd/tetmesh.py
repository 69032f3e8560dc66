"""HIP-backed mesh extraction: the steps of the reference's mesh_extract_tetrahedra.py around
GaussianRasterizer.integrate -- marching tetrahedra (utils/tetmesh.py), GaussianModel.get_tetra_points, the per-view
accumulation of evaluage_cull_alpha, the bisection along every crossing edge and the final vertex / face filter.  GPU only:
upstream moves marching tetrahedra to the CPU to save memory; here it is a sort over the crossing edges on the device.
The Delaunay triangulation (`cells`) is an input of every function here; delaunay.triangulate, the step that makes it
(mesh_extract_tetrahedra.py:63), is passed on under its name."""
import functools

import numpy as np
import torch

import delaunay
import geom_host as gh
import unbounded_mesh
from diff_gaussian_rasterization import _C
from geom_host import i32, ll, sz, vp

_SIGNATURES = {
    "radegs_tetmesh_plan_bytes": (sz, [i32, ll]),
    "radegs_tetmesh_plan": (i32, [i32, ll, vp, vp, vp, sz, vp, vp]),
    "radegs_tetmesh_emit": (i32, [i32, ll, vp, vp, vp, vp, vp, ll, ll, vp, vp, vp, vp, vp, vp]),
    "radegs_tetra_points": (i32, [i32, vp, vp, vp, vp, vp, vp]),
    "radegs_cull_alpha_accumulate": (i32, [ll, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp]),
    "radegs_cull_alpha_finish": (i32, [ll, vp, vp, vp, vp]),
    "radegs_tetmesh_bisect": (i32, [ll, vp, vp, vp, vp, vp, vp, vp]),
    "radegs_tetmesh_filter_plan_bytes": (sz, [ll, ll]),
    "radegs_tetmesh_filter_plan": (i32, [ll, ll, vp, vp, vp, vp, sz, vp, vp]),
    "radegs_tetmesh_filter_apply": (i32, [ll, ll, vp, vp, vp, ll, ll, vp, vp, vp]),
    # delaunay.py binds its own table; it is merged here because the check that the signature tables of the host modules together cover every
    # exported symbol reads this module's table, not delaunay's
    **delaunay.SIGNATURES,
    # likewise unbounded_mesh.py, the other route from a trained model to a mesh
    **unbounded_mesh.SIGNATURES,
}
triangulate = delaunay.triangulate      # mesh_extract_tetrahedra.py:63, cpp.triangulate


def _lib():
    return gh.bind(_SIGNATURES)


_call = functools.partial(gh.call, _SIGNATURES)


def _f32(t, name, shape=None):
    """a float32 GPU tensor as the kernels address it: contiguous, optionally of a given shape (-1 = any)"""
    _C._require_gpu(t, name)
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    if shape is not None and (t.dim() != len(shape) or any(s != -1 and s != d for s, d in zip(shape, t.shape))):
        raise RuntimeError(f"`{name}` must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


# ------------------------------------------------------------ marching tetrahedra ------------------------------------------------------------
def _prepare_tets(tets, V):
    """[T,4] int32 contiguous on the GPU, its index range checked once (one host read)"""
    _C._require_gpu(tets, "tets")
    if tets.dim() != 2 or tets.size(1) != 4 or tets.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("`tets` must be an int32 or int64 tensor of shape (T,4)")
    if tets.numel():
        lo, hi = torch.aminmax(tets)
        lo, hi = int(lo), int(hi)
        if lo < 0 or hi >= V:
            raise RuntimeError(f"`tets` holds indices in [{lo}, {hi}], outside the {V} vertices")
    return tets.to(torch.int32).contiguous()


def _unbatched_marching_tetrahedra(vertices, tets32, sdf, scales):
    V, T, dev = vertices.shape[0], tets32.shape[0], vertices.device
    if V >= 2 ** 31:
        raise RuntimeError("marching_tetrahedra: more than 2^31 - 1 vertices")
    nbytes = _lib().radegs_tetmesh_plan_bytes(V, T)
    ws = gh.workspace(nbytes, dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    _call("radegs_tetmesh_plan", dev, V, T, tets32, sdf, ws, nbytes, counts)
    nv, nf = counts.tolist()          # the one host read: the two sizes
    end_points = torch.empty((nv, 2, 3), dtype=torch.float32, device=dev)
    end_sdf = torch.empty((nv, 2, 1), dtype=torch.float32, device=dev)
    end_scales = torch.empty((nv, 2, 1), dtype=torch.float32, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int64, device=dev)
    interp_v = torch.empty((nv, 2), dtype=torch.int64, device=dev)
    _call("radegs_tetmesh_emit", dev, V, T, tets32, sdf, vertices, scales, ws, nv, nf, end_points, end_sdf, end_scales, faces, interp_v)
    return (end_points, end_sdf), end_scales, faces, interp_v


@torch.no_grad()
def marching_tetrahedra(vertices, tets, sdf, scales):
    """Drop-in for utils.tetmesh.marching_tetrahedra with every tensor on the GPU: `vertices` (B,V,3), `tets` (T,4) int32 or int64,
    `sdf` (B,V), `scales` (B,V) or (B,V,1).  Returns upstream's zipped list
        [((end_points[NV,2,3], end_sdf[NV,2,1]), ...), (scales[NV,2,1], ...), (faces long[NF,3], ...), (interp_v long[NV,2], ...)]
    with one entry per batch element.  Vertices are the distinct crossing edges in ascending (min, max) order; faces are the
    one-triangle tets in tet order, then the two-triangle tets -- upstream's order for up to 32 Mi tets (above that upstream chunks
    and its face order becomes chunk by chunk; this stays the single-chunk order)."""
    for t, n in ((vertices, "vertices"), (tets, "tets"), (sdf, "sdf"), (scales, "scales")):
        _C._require_gpu(t, n)
    if vertices.dim() != 3 or vertices.size(2) != 3:
        raise RuntimeError("`vertices` must be (B,V,3)")
    B, V = vertices.shape[0], vertices.shape[1]
    tets32 = _prepare_tets(tets, V)
    outs = []
    for b in range(B):
        outs.append(_unbatched_marching_tetrahedra(_f32(vertices[b], "vertices", (V, 3)), tets32, _f32(sdf[b].reshape(-1), "sdf", (V,)),
                                                   _f32(scales[b].reshape(-1), "scales", (V,))))
    return list(zip(*outs))


# --------------------------------------------------------------- per-point steps ---------------------------------------------------------------
@torch.no_grad()
def tetra_points(xyz, scales3, rotation_raw):
    """radegs_tetra_points on explicit tensors: returns (points[9P,3], scale[9P,1])"""
    x = _f32(xyz, "xyz", (-1, 3))
    P = x.shape[0]
    s, q = _f32(scales3, "scales", (P, 3)), _f32(rotation_raw, "rotation", (P, 4))
    pts = torch.empty((9 * P, 3), dtype=torch.float32, device=x.device)
    sc = torch.empty((9 * P, 1), dtype=torch.float32, device=x.device)
    _call("radegs_tetra_points", x.device, P, x, s, q, pts, sc)
    return pts, sc


def get_tetra_points(model):
    """GaussianModel.get_tetra_points (scene/gaussian_model.py:400-429): the eight corners of every Gaussian's +-3 sigma box, then
    the centres, and 3 * the largest filtered scale per point.  Reads `get_xyz`, `get_scaling_with_3D_filter` and `_rotation`."""
    return tetra_points(model.get_xyz, model.get_scaling_with_3D_filter, model._rotation)


def _integrate_fields(res):
    """(mask[H,W], alpha_integrated[PN], point_coordinate[PN,2]) from gaussian_renderer.integrate's dict or from the tuple
    GaussianRasterizer.integrate returns (color[9,H,W] first: channel 7 is the rendered mask)"""
    if isinstance(res, dict):
        return res["render"][7], res["alpha_integrated"], res["point_coordinate"]
    return res[0][7], res[1], res[3]


class CullAlpha:
    """evaluage_cull_alpha (mesh_extract_tetrahedra.py:32-56) as one fused launch per view: add_view() after every integrate(),
    sdf() at the end.  `point_coordinate` is read, not rewritten in place as upstream does."""

    def __init__(self, num_points, device):
        self.n = int(num_points)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("tetmesh (MI355X build): CullAlpha needs a GPU device -- this operator has no CPU implementation")
        self.final_sdf = torch.ones(self.n, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(self.n, dtype=torch.int32, device=self.device)

    @torch.no_grad()
    def add_view(self, integrate_result, view, extra_mask=None):
        mask, alpha, coord = _integrate_fields(integrate_result)
        W, H = int(view.image_width), int(view.image_height)
        mask = _f32(mask, "rendered mask", (H, W))
        alpha, coord = _f32(alpha, "alpha_integrated", (self.n,)), _f32(coord, "point_coordinate", (self.n, 2))
        gt = getattr(view, "gt_mask", None)
        gt = None if gt is None else _f32(gt.reshape(H, W), "gt_mask", (H, W))
        extra = None if extra_mask is None else _f32(extra_mask.reshape(H, W), "extra_mask", (H, W))
        _call("radegs_cull_alpha_accumulate", self.device, self.n, alpha, coord, mask, gt, extra, W, H, self.final_sdf, self.weight)

    @torch.no_grad()
    def sdf(self):
        out = torch.empty(self.n, dtype=torch.float32, device=self.device)
        _call("radegs_cull_alpha_finish", self.device, self.n, self.final_sdf, self.weight, out)
        return out


@torch.no_grad()
def evaluate_cull_alpha(points, views, integrate_fn, masks=None):
    """evaluage_cull_alpha: `integrate_fn(points, view)` returns what gaussian_renderer.integrate (or GaussianRasterizer.integrate)
    returns for that view; `masks[i]`: an optional extra mask per view.  No empty_cache() per view."""
    _C._require_gpu(points, "points")
    acc = CullAlpha(points.shape[0], points.device)
    for i, view in enumerate(views):
        acc.add_view(integrate_fn(points, view), view, None if masks is None else masks[i])
    return acc.sdf()


@torch.no_grad()
def bisect_step(left_pts, right_pts, left_sdf, right_sdf, mid_sdf, mid_pts_out=None):
    """radegs_tetmesh_bisect: one step in place on contiguous float32 tensors; returns the next mid-points"""
    N = left_pts.shape[0]
    for t, n, shape in ((left_pts, "left_pts", (N, 3)), (right_pts, "right_pts", (N, 3)), (left_sdf, "left_sdf", (N,)), (right_sdf, "right_sdf", (N,))):
        _C._require_gpu(t, n)
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise RuntimeError(f"`{n}` must be a contiguous float32 GPU tensor of shape {shape} (it is updated in place)")
    mid = _f32(mid_sdf.reshape(-1), "mid_sdf", (N,))
    out = torch.empty_like(left_pts) if mid_pts_out is None else mid_pts_out
    _call("radegs_tetmesh_bisect", left_pts.device, N, left_pts, right_pts, left_sdf, right_sdf, mid, out)
    return out


@torch.no_grad()
def filter_mesh(end_points, end_scales, points, faces):
    """mesh_extract_tetrahedra.py:107-110: keeps vertex v when |end_points[v,0] - end_points[v,1]| <= end_scales[v,0] + end_scales[v,1],
    keeps the faces whose three vertices are kept and renumbers them.  Returns (vertices[N,3], faces long[M,3])."""
    ep = _f32(end_points, "end_points", (-1, 2, 3))
    NV = ep.shape[0]
    es, pts = _f32(end_scales.reshape(-1, 2), "end_scales", (NV, 2)), _f32(points, "points", (NV, 3))
    _C._require_gpu(faces, "faces")
    f = faces.to(torch.int64).contiguous()
    NF, dev = f.shape[0], ep.device
    nbytes = _lib().radegs_tetmesh_filter_plan_bytes(NV, NF)
    ws = gh.workspace(nbytes, dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    _call("radegs_tetmesh_filter_plan", dev, NV, NF, ep, es, f, ws, nbytes, counts)
    nv, nf = counts.tolist()          # the one host read
    out_v = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((nf, 3), dtype=torch.int64, device=dev)
    _call("radegs_tetmesh_filter_apply", dev, NV, NF, pts, f, ws, nv, nf, out_v, out_f)
    return out_v, out_f


@torch.no_grad()
def marching_tetrahedra_with_binary_search(points, points_scale, cells, evaluate_sdf, n_binary_steps=8):
    """The body of mesh_extract_tetrahedra.py's function of the same name, everything on the GPU.  `points` [V,3] / `points_scale` [V,1]
    from get_tetra_points, `cells` [T,4] the Delaunay tetrahedra of `points`, `evaluate_sdf(p[N,3]) -> sdf[N]` (normally
    evaluate_cull_alpha over all training views).  Returns (vertices float32[N,3], faces int64[M,3]) on the GPU."""
    sdf = evaluate_sdf(points)
    verts_list, scale_list, faces_list, _ = marching_tetrahedra(points[None], cells, sdf.reshape(1, -1), points_scale.reshape(1, -1))
    end_points, end_sdf = verts_list[0]
    end_scales, faces = scale_list[0], faces_list[0]
    left, right = end_points[:, 0, :].contiguous(), end_points[:, 1, :].contiguous()
    left_sdf, right_sdf = end_sdf[:, 0, 0].contiguous(), end_sdf[:, 1, 0].contiguous()
    mid = (left + right) / 2
    for _ in range(n_binary_steps):
        mid = bisect_step(left, right, left_sdf, right_sdf, evaluate_sdf(mid))
    return filter_mesh(end_points, end_scales, mid, faces)


def write_ply(path, vertices, faces):
    """binary little-endian PLY of a triangle mesh: float32 x y z per vertex, `uchar 3, int32 x 3` per face"""
    v = np.ascontiguousarray((vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)), dtype="<f4").reshape(-1, 3)
    f = (faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise RuntimeError("write_ply: a face index is outside the vertices")
    rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    rec["n"] = 3
    rec["v"] = f
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (v.shape[0], f.shape[0]))
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


def read_ply(path):
    """reads back what write_ply wrote: (vertices float32[N,3], faces int64[M,3])"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    if head[0] != "ply" or head[1] != "format binary_little_endian 1.0":
        raise RuntimeError("read_ply: not a binary little-endian PLY")
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in head if l.startswith("element face")][0].split()[-1])
    v = np.frombuffer(data, dtype="<f4", count=3 * nv, offset=end).reshape(nv, 3).copy()
    rec = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=nf, offset=end + 12 * nv)
    if nf and not (rec["n"] == 3).all():
        raise RuntimeError("read_ply: a face is not a triangle")
    return v, rec["v"].astype(np.int64)
