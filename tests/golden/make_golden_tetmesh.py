"""Generates tests/golden/tetmesh_delaunay.npz, tetmesh_small.npz, tetmesh_cull.npz and tetmesh_bisect.npz from the REFERENCE's own code
run on the CPU (/root/reference: utils/tetmesh.py, GaussianModel.get_tetra_points at scene/gaussian_model.py:400-429, and
mesh_extract_tetrahedra.py's evaluage_cull_alpha and marching_tetrahedra_with_binary_search).  Build container only.

The modules' unavailable imports are stubbed, `device="cuda"` factory calls and `.cuda()` are routed to the CPU, as
make_golden_densify.py does.  The reference's functions are CALLED, on recorded inputs:
  * `integrate` (a module global of mesh_extract_tetrahedra) is replaced by a function that hands out recorded alpha_integrated /
    point_coordinate / rendered mask per view; torch.where and grid_sample are wrapped to record what the function computes on the way
    (final_sdf and weight after every view, the sampled probabilities);
  * for the bisection, `evaluage_cull_alpha` is replaced by a function that hands out recorded sdf arrays (the first for the points, then
    one per step) and snapshots the end-point tensors it is called between (they were caught when the function called `.cuda()` on them);
  * `trimesh` is absent: `trimesh.creation.box` is a stand-in object carrying the +-0.5 corner array in binary-counting order (x most
    significant; believed to be trimesh's order, UNVERIFIED -- it only permutes the eight points of one Gaussian), and `trimesh.Trimesh`
    records the arrays and the two masks it is handed.  The filter's expected output is those masks applied as update_vertices followed
    by update_faces are documented to (kept vertices in order, faces renumbered).
  * `cells` come from scipy.spatial.Delaunay and are committed as int32 data.

Decisions that sit on a threshold (the 0.5 test of the sampled mask, distance <= scale) are ASSERTED to keep a margin, so that the tests
can demand exact equality from implementations whose arithmetic differs in the last bit.  On a failed assertion change the seed, never
the margin."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules.setdefault(name, m)
    return sys.modules[name]


class FakeTrimesh:
    last = None

    def __init__(self, vertices=None, faces=None, process=True):
        self.vertices, self.faces, self.vmask, self.fmask = np.array(vertices), np.array(faces), None, None
        FakeTrimesh.last = self

    def update_vertices(self, mask):
        self.vmask = np.array(mask)

    def update_faces(self, mask):
        self.fmask = np.array(mask)

    def export(self, path):
        pass


def fake_box():
    corners = np.array([[(1 if j & 4 else -1), (1 if j & 2 else -1), (1 if j & 1 else -1)] for j in range(8)], dtype=np.float64) * 0.5
    return types.SimpleNamespace(vertices=corners)


stub("plyfile", PlyData=None, PlyElement=None)
stub("simple_knn")
stub("simple_knn._C", distCUDA2=None)
stub("cv2")
stub("trimesh", creation=types.SimpleNamespace(box=fake_box), Trimesh=FakeTrimesh)
stub("tqdm", tqdm=lambda it, **k: it)
stub("gaussian_renderer", render=None, integrate=None, GaussianModel=None)
stub("arguments", ModelParams=None, PipelineParams=None, get_combined_args=None)
stub("tetranerf")
stub("tetranerf.utils")
stub("tetranerf.utils.extension", cpp=types.SimpleNamespace(triangulate=None))
sys.path.insert(0, REF)
pkg = types.ModuleType("scene")            # keep scene/__init__.py (dataset readers, PIL, ...) from running
pkg.__path__ = [os.path.join(REF, "scene")]
pkg.Scene = None
sys.modules["scene"] = pkg
from scene.gaussian_model import GaussianModel  # noqa: E402
import mesh_extract_tetrahedra as met  # noqa: E402
from utils.tetmesh import marching_tetrahedra  # noqa: E402

for fn in ("zeros", "ones", "empty", "full", "tensor", "rand", "randn"):   # device="cuda" -> CPU
    def _route(*a, __f=getattr(torch, fn), **k):
        if str(k.get("device", "")).startswith("cuda"):
            k.pop("device")
        return __f(*a, **k)
    setattr(torch, fn, _route)
CUDA_CALLS = []


def _cuda(self, *a, **k):
    CUDA_CALLS.append(self)
    return self


torch.Tensor.cuda = _cuda
torch.cuda.empty_cache = lambda: None


def save(name, **data):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    assert size < (1 << 20), (name, size)
    print(name, size, "bytes;", {k: tuple(np.shape(v)) for k, v in data.items()})


def run_marching(vertices, tets, sdf, scales):
    v, s, f, i = marching_tetrahedra(torch.from_numpy(vertices)[None], torch.from_numpy(tets).long(), torch.from_numpy(sdf)[None],
                                     torch.from_numpy(scales)[None])
    (ep, es), sc, faces, interp = v[0], s[0], f[0], i[0]
    return dict(end_points=ep.numpy(), end_sdf=es.numpy(), end_scales=sc.numpy(), faces=faces.numpy(), interp_v=interp.numpy())


def delaunay_fixture(seed):
    """(a) + (d): 300 Gaussians -> the reference's get_tetra_points -> 2 700 points, Delaunay cells, a noisy unit sphere"""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    P = 300
    gm = object.__new__(GaussianModel)
    gm.setup_functions()
    gm._xyz = torch.from_numpy((0.75 * rng.standard_normal((P, 3))).astype(np.float32))
    gm._scaling = torch.from_numpy((np.log(0.035) + 0.5 * rng.standard_normal((P, 3))).astype(np.float32))
    gm._rotation = torch.from_numpy(rng.standard_normal((P, 4)).astype(np.float32))
    gm.filter_3D = torch.from_numpy((0.01 + 0.01 * rng.random((P, 1))).astype(np.float32))
    scales3 = gm.get_scaling_with_3D_filter.numpy().copy()
    points, points_scale = gm.get_tetra_points()
    points, points_scale = points.numpy().copy(), points_scale.numpy().copy()
    assert points.shape == (9 * P, 3) and points_scale.shape == (9 * P, 1)
    cells = Delaunay(points.astype(np.float64)).simplices.astype(np.int32)
    sdf = (1.0 - np.linalg.norm(points, axis=1) + 0.05 * rng.standard_normal(9 * P)).astype(np.float32)
    near = np.argsort(np.abs(sdf))[:5]
    sdf[near] = 0.0                                        # exact zeros on the surface: occ = sdf > 0 puts them outside
    out = run_marching(points, cells, sdf, points_scale)
    assert out["interp_v"].shape[0] > 1000 and out["faces"].shape[0] > 2000
    crossing = int(((sdf > 0)[cells][:, [0, 0, 0, 1, 1, 2]] != (sdf > 0)[cells][:, [1, 2, 3, 2, 3, 3]]).sum())
    assert crossing > 2048, crossing                       # both sort passes and the scans run over more than one block
    save("tetmesh_delaunay.npz", xyz=gm._xyz.numpy(), scales3=scales3, rotation=gm._rotation.numpy(), points=points, points_scale=points_scale,
         cells=cells, sdf=sdf, crossing_instances=np.asarray(crossing), **out)
    return points, points_scale, cells, sdf, out


def small_fixture(seed):
    """(b) V = 50, T = 300 random tets (repeated corners included) and (c) the same with every sdf negative"""
    rng = np.random.default_rng(seed)
    V, T = 50, 300
    vertices = rng.standard_normal((V, 3)).astype(np.float32)
    tets = rng.integers(0, V, (T, 4)).astype(np.int32)
    sdf = rng.standard_normal(V).astype(np.float32)
    sdf[[3, 17, 40]] = 0.0
    scales = rng.random((V, 1)).astype(np.float32)
    out = run_marching(vertices, tets, sdf, scales)
    data = dict(vertices=vertices, tets=tets, sdf=sdf, scales=scales, **out)
    outside = -np.abs(sdf) - 1.0
    try:
        empty = run_marching(vertices, tets, outside.astype(np.float32), scales)
        empty_from = "reference"
    except Exception as e:                                 # the reference's torch.unique(dim=0) may refuse an empty tensor: the empty result by shape
        print("reference on the all-outside input:", type(e).__name__, e)
        empty = dict(end_points=np.zeros((0, 2, 3), np.float32), end_sdf=np.zeros((0, 2, 1), np.float32), end_scales=np.zeros((0, 2, 1), np.float32),
                     faces=np.zeros((0, 3), np.int64), interp_v=np.zeros((0, 2), np.int64))
        empty_from = "shapes"
    assert all(v.shape[0] == 0 for v in empty.values())
    data.update(sdf_outside=outside.astype(np.float32), empty_from=np.asarray(empty_from), **{"empty_" + k: v for k, v in empty.items()})
    save("tetmesh_small.npz", **data)


def cull_fixture(seed):
    """(e) two views (37x23 with gt_mask, 64x48 without), 5 000 points, a fifth of them outside the image; run twice: masks=None and with an
    extra mask per view"""
    rng = np.random.default_rng(seed)
    PN = 5000
    sizes = ((37, 23), (64, 48))
    views, rec = [], []
    for v, (W, H) in enumerate(sizes):
        yy, xx = np.mgrid[0:H, 0:W]
        field = np.sin(xx * 0.31 + v) * np.cos(yy * 0.27 - v) + 0.35
        mask = (1.0 / (1.0 + np.exp(-25.0 * field))).astype(np.float32)      # mostly saturated: few samples near 0.5
        gt = (rng.random((1, H, W)) < 0.85).astype(np.float32) if v == 0 else None
        extra = (rng.random((1, H, W)) < 0.9).astype(np.float32)
        coord = np.stack([rng.uniform(0, W - 1, PN), rng.uniform(0, H - 1, PN)], 1)
        out = rng.random(PN) < 0.2
        coord[out] = np.stack([rng.uniform(-0.6 * W, 1.6 * W, out.sum()), rng.uniform(-0.6 * H, 1.6 * H, out.sum())], 1)
        coord[:3] = [[-0.5, -0.5], [W - 0.5, H - 0.5], [-1e6, 1e6]]           # the image's corners in grid units, and far away
        alpha = rng.random(PN).astype(np.float32)
        render = np.zeros((9, H, W), np.float32)
        render[7] = mask
        rec.append(dict(alpha=alpha, coord=coord.astype(np.float32), mask=mask, render=render, gt=gt, extra=extra, W=W, H=H))
        views.append(types.SimpleNamespace(image_width=W, image_height=H, gt_mask=None if gt is None else torch.from_numpy(gt)))
    data = {}
    for tag, masks in (("", None), ("x_", [torch.from_numpy(r["extra"]) for r in rec])):
        state = dict(i=0, where=[], prob=[])

        def fake_integrate(points, view, *a, **k):
            r = rec[state["i"]]
            state["i"] += 1
            return dict(alpha_integrated=torch.from_numpy(r["alpha"].copy()), point_coordinate=torch.from_numpy(r["coord"].copy()),
                        render=torch.from_numpy(r["render"].copy()))
        real_where, real_gs = torch.where, torch.nn.functional.grid_sample

        def rec_where(*a, **k):
            out = real_where(*a, **k)
            state["where"].append(out.numpy().copy())
            return out

        def rec_gs(*a, **k):
            out = real_gs(*a, **k)
            state["prob"].append(out.numpy().reshape(-1).copy())
            return out
        met.integrate, torch.where, torch.nn.functional.grid_sample = fake_integrate, rec_where, rec_gs
        try:
            sdf = met.evaluage_cull_alpha(torch.zeros(PN, 3), views, masks, None, None, None, 0.0)
        finally:
            torch.where, torch.nn.functional.grid_sample = real_where, real_gs
        assert len(state["where"]) == 2 * len(views) + 1 and len(state["prob"]) == len(views)
        gap = min(float(np.abs(p - 0.5).min()) for p in state["prob"])
        print("cull-alpha", tag or "plain", "smallest |prob - 0.5|:", gap, "; valid per view:", [int((p > 0.5).sum()) for p in state["prob"]])
        assert gap > 1e-5, "a sampled probability within 1e-5 of 0.5: change the seed"
        for v in range(len(views)):
            data[f"{tag}final_sdf{v}"], data[f"{tag}weight{v}"] = state["where"][2 * v], state["where"][2 * v + 1]
            assert data[f"{tag}weight{v}"].dtype == np.int32
        data[f"{tag}sdf"] = sdf.numpy()
        assert np.array_equal(state["where"][-1], data[f"{tag}sdf"])
    for v, r in enumerate(rec):
        data.update({f"alpha{v}": r["alpha"], f"coord{v}": r["coord"], f"mask{v}": r["mask"], f"extra{v}": r["extra"], f"size{v}": np.asarray([r["W"], r["H"]])})
        if r["gt"] is not None:
            data[f"gt{v}"] = r["gt"]
    save("tetmesh_cull.npz", **data)


def bisect_fixture(seed, points, points_scale, cells, sdf, marched):
    """(f) the reference's marching_tetrahedra_with_binary_search on fixture (a) with recorded sdf arrays.  The point scales are (a)'s
    times a recorded per-point factor in [0.95, 1.05]: two corners of one Gaussian's box along its longest axis are exactly 2 * smax apart,
    which IS the sum of their scales, so with get_tetra_points' own scales the filter's comparison sits on a tie for every such edge (in the
    reference too: its decision there is rounding noise) and no margin could be asserted."""
    rng = np.random.default_rng(seed)
    points_scale = (points_scale * rng.uniform(0.95, 1.05, points_scale.shape)).astype(np.float32)
    NV, steps = marched["interp_v"].shape[0], 8
    mids = []
    for k in range(steps):
        m = (0.3 * rng.standard_normal(NV)).astype(np.float32)
        m[rng.integers(0, NV, 7)] = 0.0                   # exact zeros: the right end moves
        mids.append(m)
    seq = [sdf] + mids
    state = dict(i=0, snaps=[])
    del CUDA_CALLS[:]

    def snapshot():
        ep, es = CUDA_CALLS[0], CUDA_CALLS[1]             # end_points [NV,2,3], end_sdf [NV,2,1]: the function's own tensors, updated in place
        assert tuple(ep.shape) == (NV, 2, 3) and tuple(es.shape) == (NV, 2, 1)
        state["snaps"].append((ep.numpy().copy(), es.numpy().copy()))

    def fake_eval(pts, *a, **k):
        if state["i"] > 0:
            snapshot()                                    # the state the previous step left (before the first step: the initial end points)
        out = torch.from_numpy(seq[state["i"]].copy())
        state["i"] += 1
        return out
    met.evaluage_cull_alpha = fake_eval
    met.cpp.triangulate = lambda p: torch.from_numpy(cells)
    gaussians = types.SimpleNamespace(get_tetra_points=lambda: (torch.from_numpy(points.copy()), torch.from_numpy(points_scale.copy())))
    met.marching_tetrahedra_with_binary_search("/tmp", "test", 0, [], gaussians, None, None, 0.0)
    snapshot()
    mesh = FakeTrimesh.last
    assert state["i"] == steps + 1 and len(state["snaps"]) == steps + 1
    assert np.array_equal(state["snaps"][0][0], marched["end_points"]) and np.array_equal(state["snaps"][0][1], marched["end_sdf"])
    assert np.array_equal(mesh.faces, marched["faces"])
    # the margin of the filter's comparison
    end_scales = CUDA_CALLS[2].numpy().copy()
    assert np.array_equal(end_scales, points_scale[marched["interp_v"].reshape(-1)].reshape(-1, 2, 1))
    ep0, sc0 = marched["end_points"].astype(np.float64), end_scales.astype(np.float64)[:, :, 0]
    dist, scale = np.linalg.norm(ep0[:, 0] - ep0[:, 1], axis=1), sc0.sum(1)
    gap = float((np.abs(dist - scale) / scale).min())
    print("filter: smallest relative |distance - scale|:", gap, "; vertices kept", int(mesh.vmask.sum()), "of", NV, "; faces kept", int(mesh.fmask.sum()),
          "of", mesh.faces.shape[0])
    assert gap > 1e-5, "a distance within 1e-5 of its scale: change the seed"
    assert np.array_equal(mesh.vmask, dist <= scale) and 0 < mesh.vmask.sum() < NV and 0 < mesh.fmask.sum() < mesh.faces.shape[0]
    remap = np.cumsum(mesh.vmask) - 1
    data = dict(points_scale=points_scale, end_scales=end_scales, final_points=mesh.vertices.astype(np.float32), vertex_mask=mesh.vmask, face_mask=mesh.fmask,
                out_vertices=mesh.vertices.astype(np.float32)[mesh.vmask], out_faces=remap[mesh.faces[mesh.fmask]].astype(np.int64))
    for k in range(steps):
        data[f"mid_sdf{k}"] = mids[k]
        data[f"end_points{k}"], data[f"end_sdf{k}"] = state["snaps"][k + 1]
    save("tetmesh_bisect.npz", **data)


if __name__ == "__main__":
    a = delaunay_fixture(seed=11)
    small_fixture(seed=12)
    cull_fixture(seed=13)
    bisect_fixture(14, *a)
