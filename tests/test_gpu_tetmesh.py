"""GPU tier of mesh extraction: the HIP kernels and tetmesh.py against the fixtures the reference's own code wrote
(tests/golden/make_golden_tetmesh.py) and against tests/tetmesh_restatement.py at sizes the fixtures do not reach.  Exact: every output of
marching tetrahedra, the cull-alpha accumulation, every bisection step and the filter.  get_tetra_points' computed coordinates: 1e-5 abs /
1e-4 rel."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tetmesh_restatement as tr
from test_tetmesh_golden import MARCH_KEYS, check_marching, load, within_bar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def march(vertices, tets, sdf, scales):
    """tetmesh.marching_tetrahedra on one batch element -> the five outputs as numpy arrays, upstream's return structure checked on the way"""
    import tetmesh
    tets = tets if isinstance(tets, torch.Tensor) else dev(tets)
    out = tetmesh.marching_tetrahedra(dev(vertices)[None], tets, dev(sdf).reshape(1, -1), dev(scales).reshape(1, -1, 1))
    assert isinstance(out, list) and len(out) == 4 and all(isinstance(o, tuple) and len(o) == 1 for o in out)
    (ep, es), sc, faces, iv = out[0][0], out[1][0], out[2][0], out[3][0]
    assert faces.dtype == torch.int64 and iv.dtype == torch.int64 and ep.dtype == torch.float32
    return tuple(t.cpu().numpy() for t in (ep, es, sc, faces, iv))


@pytest.fixture(scope="module")
def delaunay():
    return load("tetmesh_delaunay.npz")


@pytest.fixture(scope="module")
def large():
    """V = 70 001 (17 bits: the sorts take a third digit), T = 300 000, and its restated result -- computed once, never modified"""
    case = tr.random_case(70001, 300000, seed=21)
    return case, tr.marching(*case)


def test_marching_delaunay_fixture(delaunay):
    fx = delaunay
    check_marching(march(fx["points"], fx["cells"], fx["sdf"], fx["points_scale"]), fx)


def test_marching_small_and_empty_fixtures():
    fx = load("tetmesh_small.npz")
    check_marching(march(fx["vertices"], fx["tets"], fx["sdf"], fx["scales"]), fx)
    check_marching(march(fx["vertices"], fx["tets"], fx["sdf_outside"], fx["scales"]), fx, "empty_")


def test_marching_against_the_restatement_at_three_digits(large):
    (v, t, s, sc), want = large
    got = march(v, t, s, sc)
    assert got[4].shape[0] > 100_000 and got[3].shape[0] > 100_000
    for g, w, key in zip(got, want, MARCH_KEYS):
        assert g.shape == w.shape and np.array_equal(g, w), key


def test_marching_input_variants(large):
    import tetmesh
    (v, t, s, sc), want = large
    n = 50_000
    want = tr.marching(v, t[:n], s, sc)
    t32 = dev(t[:n])
    wide = torch.zeros((n, 6), dtype=torch.int32, device=DEV)
    wide[:, 1:5] = t32
    view = wide[:, 1:5]                                            # row stride 6, not 16-byte aligned
    assert not view.is_contiguous()
    for tets in (t32, t32.long(), view, t32.long().t().contiguous().t()):
        got = march(v, tets, s, sc)
        for g, w, key in zip(got, want, MARCH_KEYS):
            assert np.array_equal(g, w), key
    empty = march(v, torch.zeros((0, 4), dtype=torch.int64, device=DEV), s, sc)                      # T = 0
    assert [e.shape for e in empty] == [(0, 2, 3), (0, 2, 1), (0, 2, 1), (0, 3), (0, 2)]
    for bad in (v.shape[0], -1):
        t_bad = t32.clone()
        t_bad[n // 2, 2] = bad
        with pytest.raises(RuntimeError, match="outside"):
            tetmesh.marching_tetrahedra(dev(v)[None], t_bad, dev(s)[None], dev(sc).reshape(1, -1))
    with pytest.raises(RuntimeError, match=r"\(T,4\)"):
        tetmesh.marching_tetrahedra(dev(v)[None], t32.float(), dev(s)[None], dev(sc).reshape(1, -1))


@pytest.mark.parametrize("tag", ["", "x_"], ids=["view_masks", "extra_masks"])
def test_cull_alpha_fixture(tag):
    import tetmesh
    fx = load("tetmesh_cull.npz")
    PN = fx["alpha0"].shape[0]
    acc = tetmesh.CullAlpha(PN, DEV)
    for v in range(2):
        W, H = (int(x) for x in fx[f"size{v}"])
        render = torch.zeros((9, H, W), device=DEV)
        render[7] = dev(fx[f"mask{v}"])
        coord = dev(fx[f"coord{v}"])
        res = dict(render=render, alpha_integrated=dev(fx[f"alpha{v}"]), point_coordinate=coord)
        view = SimpleNamespace(image_width=W, image_height=H, gt_mask=dev(fx[f"gt{v}"]) if f"gt{v}" in fx else None)
        acc.add_view(res, view, dev(fx[f"extra{v}"]) if tag else None)
        assert np.array_equal(coord.cpu().numpy(), fx[f"coord{v}"]), "point_coordinate was modified"
        assert np.array_equal(acc.final_sdf.cpu().numpy(), fx[f"{tag}final_sdf{v}"]), v
        assert acc.weight.dtype == torch.int32 and np.array_equal(acc.weight.cpu().numpy(), fx[f"{tag}weight{v}"]), v
    assert np.array_equal(acc.sdf().cpu().numpy(), fx[f"{tag}sdf"])
    if not tag:                                                    # the same through evaluate_cull_alpha and GaussianRasterizer.integrate's tuple
        views, results = [], []
        for v in range(2):
            W, H = (int(x) for x in fx[f"size{v}"])
            render = torch.zeros((9, H, W), device=DEV)
            render[7] = dev(fx[f"mask{v}"])
            views.append(SimpleNamespace(image_width=W, image_height=H, gt_mask=dev(fx[f"gt{v}"]) if f"gt{v}" in fx else None, index=v))
            results.append((render, dev(fx[f"alpha{v}"]), None, dev(fx[f"coord{v}"]), None, None))
        sdf = tetmesh.evaluate_cull_alpha(torch.zeros(PN, 3, device=DEV), views, lambda p, view: results[view.index])
        assert np.array_equal(sdf.cpu().numpy(), fx["sdf"])


def test_bisection_and_filter_fixture(delaunay):
    import tetmesh
    a, fx = delaunay, load("tetmesh_bisect.npz")
    ep = dev(a["end_points"])
    l, r = ep[:, 0].contiguous(), ep[:, 1].contiguous()
    ls, rs = dev(a["end_sdf"][:, 0, 0]), dev(a["end_sdf"][:, 1, 0])
    mid = (l + r) / 2
    for k in range(8):
        before = mid.clone()
        mid = tetmesh.bisect_step(l, r, ls, rs, dev(fx[f"mid_sdf{k}"]).reshape(-1, 1))
        for got, want in ((l, fx[f"end_points{k}"][:, 0]), (r, fx[f"end_points{k}"][:, 1]), (ls, fx[f"end_sdf{k}"][:, 0, 0]), (rs, fx[f"end_sdf{k}"][:, 1, 0])):
            assert np.array_equal(got.cpu().numpy(), want), k
        assert bool(((l == before).all(1) | (r == before).all(1)).all())   # the end that moved now IS the mid-point the step was evaluated at
        assert torch.equal(mid, (l + r) / 2)
    assert np.array_equal(mid.cpu().numpy(), fx["final_points"])
    v, f = tetmesh.filter_mesh(ep, dev(fx["end_scales"]), mid, dev(a["faces"]))
    assert f.dtype == torch.int64 and np.array_equal(v.cpu().numpy(), fx["out_vertices"]) and np.array_equal(f.cpu().numpy(), fx["out_faces"])
    # nothing kept / nothing to filter
    v0, f0 = tetmesh.filter_mesh(ep, torch.zeros_like(dev(fx["end_scales"])), mid, dev(a["faces"]))
    assert v0.shape == (0, 3) and f0.shape == (0, 3)
    v1, f1 = tetmesh.filter_mesh(ep[:0], dev(fx["end_scales"])[:0], mid[:0], dev(a["faces"])[:0])
    assert v1.shape == (0, 3) and f1.shape == (0, 3)


def test_filter_against_the_restatement_over_several_blocks(large):
    """NV + NF beyond one scan block, with the structural ties of box edges absent: random scales around the edge lengths"""
    import tetmesh
    _, (ep, _, _, faces, _) = large
    rng = np.random.default_rng(8)
    length = np.linalg.norm(ep[:, 0] - ep[:, 1], axis=1).astype(np.float32)
    scales = (length[:, None] * rng.uniform(0.3, 0.8, (ep.shape[0], 2))).astype(np.float32)
    pts = rng.standard_normal((ep.shape[0], 3)).astype(np.float32)
    want_v, want_f = tr.filter_mesh(ep, scales, pts, faces)
    assert 0 < want_v.shape[0] < ep.shape[0] and 0 < want_f.shape[0] < faces.shape[0]
    v, f = tetmesh.filter_mesh(dev(ep), dev(scales), dev(pts), dev(faces))
    assert np.array_equal(v.cpu().numpy(), want_v) and np.array_equal(f.cpu().numpy(), want_f)


def test_get_tetra_points_fixture(delaunay):
    import tetmesh
    fx = delaunay
    model = SimpleNamespace(get_xyz=dev(fx["xyz"]), get_scaling_with_3D_filter=dev(fx["scales3"]), _rotation=dev(fx["rotation"]))
    pts, sc = tetmesh.get_tetra_points(model)
    assert pts.shape == (2700, 3) and sc.shape == (2700, 1)
    pts, sc = pts.cpu().numpy(), sc.cpu().numpy()
    assert np.array_equal(sc, fx["points_scale"])
    assert np.array_equal(pts[2400:], fx["points"][2400:])
    assert within_bar(pts, fx["points"]), float(np.abs(pts - fx["points"]).max())
    p7, s7 = tetmesh.tetra_points(dev(fx["xyz"][:7]), dev(fx["scales3"][:7]), dev(fx["rotation"][:7]))
    want_p, want_s = tr.tetra_points(fx["xyz"][:7], fx["scales3"][:7], fx["rotation"][:7])
    assert within_bar(p7.cpu().numpy(), want_p) and np.array_equal(s7.cpu().numpy(), want_s)


def test_driver_with_an_analytic_sphere(delaunay):
    """sdf(p) = R - |p|: the bracket halves eight times and the vertex is its midpoint, so it lies within len * 2^-9 of the crossing along its
    edge, and |.| is 1-Lipschitz: | |v| - R | <= len * 2^-8 + 1e-6 (float32 arithmetic of the callback and the midpoints)"""
    import tetmesh
    fx = delaunay
    R = 1.0
    pts, sc, cells = dev(fx["points"]), dev(fx["points_scale"]), dev(fx["cells"])
    calls = []

    def sphere(p):
        calls.append(p.shape[0])
        return R - p.norm(dim=1)
    v, f = tetmesh.marching_tetrahedra_with_binary_search(pts, sc, cells, sphere)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and len(calls) == 9 and calls[0] == 2700
    (ep, _), esc, faces, _ = (o[0] for o in tetmesh.marching_tetrahedra(pts[None], cells, sphere(pts)[None], sc.reshape(1, -1)))
    ep, esc, faces = ep.cpu().numpy(), esc.cpu().numpy(), faces.cpu().numpy()
    keep = tr.keep_vertices(ep, esc)
    length = np.linalg.norm(ep[keep, 0].astype(np.float64) - ep[keep, 1], axis=1)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert v.shape[0] == keep.sum() > 100
    err = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - R)
    assert (err <= length * 2.0 ** -8 + 1e-6).all(), float((err - length * 2.0 ** -8).max())
    _, want_f = tr.apply_masks(ep[:, 0], faces, keep, keep[faces].all(axis=1))   # marching's faces after the filter's remap
    assert f.shape[0] > 100 and np.array_equal(f, want_f)


def test_end_to_end_through_integrate(delaunay, tmp_path):
    """structure only: 300 synthetic Gaussians, two 64x48 views, the committed cells as the topology over the 2 700 tetra points"""
    import tetmesh
    from diff_gaussian_rasterization import GaussianRasterizer
    from gpu_util import settings_for
    from synth_scene import jittered_view, make_scene, to_device
    s0 = make_scene(300, 64, 48, sh_degree=1, mu_px=6.0, seed=41, kernel_size=0.0, pose="random", require_coord=False, require_depth=True)
    scenes = [s0, jittered_view(s0, 5, angle_deg=8.0)]
    d = [to_device(s, DEV) for s in scenes]
    rasterizers = [GaussianRasterizer(settings_for(s, DEV)) for s in scenes]
    views = [SimpleNamespace(image_width=s.W, image_height=s.H, gt_mask=None, index=i) for i, s in enumerate(scenes)]
    model = SimpleNamespace(get_xyz=d[0].means3D, get_scaling_with_3D_filter=d[0].scales, _rotation=d[0].rotations)
    points, points_scale = tetmesh.get_tetra_points(model)
    assert points.shape == (2700, 3)
    cells = dev(delaunay["cells"])

    def integrate(p, view):
        g = d[view.index]
        return rasterizers[view.index].integrate(p.contiguous(), g.means3D, torch.zeros_like(g.means3D), g.opacities, shs=g.shs, scales=g.scales,
                                                 rotations=g.rotations)

    def evaluate(p):
        return tetmesh.evaluate_cull_alpha(p, views, integrate)
    sdf = evaluate(points)
    (ep, _), esc, faces, _ = (o[0] for o in tetmesh.marching_tetrahedra(points[None], cells, sdf[None], points_scale.reshape(1, -1)))
    v, f = tetmesh.marching_tetrahedra_with_binary_search(points, points_scale, cells, evaluate)
    print("end to end:", ep.shape[0], "crossing edges,", faces.shape[0], "faces ->", v.shape[0], "vertices,", f.shape[0], "faces after the filter")
    assert v.shape[1] == 3 and f.shape[1] == 3 and torch.isfinite(v).all()
    if f.numel():
        assert int(f.min()) >= 0 and int(f.max()) < v.shape[0]
    # Every vertex lies on its original edge segment.  A stored midpoint is rounded per component by at most half an ulp of the edge's largest
    # coordinate magnitude c, u/2 with u <= 2^-22 c; the midpoint of two points that are d off the line is at most d + sqrt(3) u / 2 off it, so
    # eight steps leave at most 8 * sqrt(3) / 2 * 2^-22 * c -- the distance to the SEGMENT, which also bounds how far past an end it may lie.
    keep = torch.from_numpy(tr.keep_vertices(ep.cpu().numpy(), esc.cpu().numpy())).to(DEV)
    l, r = ep[keep, 0].double(), ep[keep, 1].double()
    assert v.shape[0] == int(keep.sum())
    e = r - l
    t = (((v.double() - l) * e).sum(1) / (e * e).sum(1).clamp_min(1e-300)).clamp(0.0, 1.0)
    off = (v.double() - (l + t[:, None] * e)).norm(dim=1)
    cmax = torch.maximum(l.abs().amax(1), r.abs().amax(1))
    assert bool((off <= 8 * 3 ** 0.5 / 2 * 2.0 ** -22 * cmax).all()), float((off / cmax.clamp_min(1e-30)).max())
    path = str(tmp_path / "recon.ply")
    tetmesh.write_ply(path, v, f)
    v2, f2 = tetmesh.read_ply(path)
    assert np.array_equal(v2, v.cpu().numpy()) and np.array_equal(f2, f.cpu().numpy())

