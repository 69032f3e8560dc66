"""gaussian_model.GaussianModel and gaussian_render.render / integrate on the GPU, on tests/golden/scene_colmap (six 53 x 37 views, 40 points):
the model Scene builds is model_io's, render() is the direct rasterizer call fed with the eager composition bit for bit (and within
1e-5 / 1e-4 of it through the fused activations), integrate() is the direct integrate call, a PLY round trip reproduces the image, and one
optimisation step moves all six parameters."""
import math
import os
import shutil
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RENDER_KEYS = {"render": 3, "mask": 1, "expected_coord": 3, "median_coord": 3, "expected_depth": 1, "median_depth": 1, "normal": 3}


def close(a, b):
    a, b = a.detach().cpu().numpy().astype(np.float64), b.detach().cpu().numpy().astype(np.float64)
    return bool(np.all(np.abs(a - b) <= 1e-5 + 1e-4 * np.abs(b)))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def dataset(source, out):
    return types.SimpleNamespace(source_path=source, model_path=out, images="images", eval=False, white_background=False, resolution=1,
                                 data_device="cuda", sh_degree=3, kernel_size=0.1, disable_filter3D=False, use_coord_map=False,
                                 use_decoupled_appearance=False)


PIPE = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    import scene_io
    from gaussian_model import GaussianModel
    root = tmp_path_factory.mktemp("gaussian_model")
    source = shutil.copytree(os.path.join(GOLDEN, "scene_colmap"), str(root / "scene_colmap"))
    args = dataset(source, str(root / "model"))
    torch.manual_seed(0)
    gaussians = GaussianModel(3)
    scene = scene_io.Scene(args, gaussians)
    gaussians.compute_3D_filter(scene.getTrainCameras())
    with torch.no_grad():                                   # away from the initial state: anisotropic, rotated, coloured in every SH band
        g = torch.Generator(device="cpu").manual_seed(4)
        P = gaussians.get_xyz.shape[0]
        gaussians._features_rest += 0.1 * torch.randn((P, 15, 3), generator=g).to(DEV)
        gaussians._rotation += 0.3 * torch.randn((P, 4), generator=g).to(DEV)
        gaussians._scaling += 0.3 * torch.randn((P, 3), generator=g).to(DEV) + 1.0
        gaussians._opacity += 2.0
    gaussians.active_sh_degree = 3
    return types.SimpleNamespace(args=args, gaussians=gaussians, scene=scene, root=root, bg=torch.zeros(3, device=DEV))


def rasterizer(cam, gaussians, bg, kernel_size, require_coord=True, require_depth=True):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    return GaussianRasterizer(GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        kernel_size=kernel_size, bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
        sh_degree=gaussians.active_sh_degree, campos=cam.camera_center, prefiltered=False, require_depth=require_depth, require_coord=require_coord,
        debug=False))


def test_scene_builds_the_model_model_io_builds(built):
    import model_io as mio
    g = built.gaussians
    fresh_args = dataset(built.args.source_path, str(built.root / "model_again"))
    import scene_io
    from gaussian_model import GaussianModel
    fresh = GaussianModel(3)
    scene = scene_io.Scene(fresh_args, fresh)
    cloud = mio.fetch_ply(os.path.join(fresh_args.model_path, "input.ply"), device=DEV)
    st = mio.init_from_points(cloud.points.contiguous(), cloud.colors.contiguous(), 3)
    assert fresh.get_xyz.shape == (40, 3)
    for attr, want in zip(mio._PARAMS, st[:6]):
        got = getattr(fresh, attr)
        assert isinstance(got, torch.nn.Parameter) and got.requires_grad and same(got.detach(), want), attr
    assert fresh.spatial_lr_scale == scene.cameras_extent and fresh.active_sh_degree == 0 and fresh.max_sh_degree == 3
    assert tuple(fresh.max_radii2D.shape) == (40,) and not fresh.max_radii2D.any()
    assert tuple(g.filter_3D.shape) == (40, 1) and bool((g.filter_3D > 0).all())
    assert fresh._appearance_embeddings.shape == (2048, 64) and fresh._appearance_embeddings.is_cuda
    assert next(fresh.appearance_network.parameters()).is_cuda


@pytest.mark.parametrize("coord,depth", [(True, True), (False, True), (True, False), (False, False)])
def test_render_is_the_direct_rasterizer_call(built, coord, depth):
    import gaussian_model_ops as gmo
    from gaussian_render import render
    g, cam = built.gaussians, built.scene.getTrainCameras()[1]
    H, W, P = cam.image_height, cam.image_width, g.get_xyz.shape[0]
    with torch.no_grad():
        eager = render(cam, g, PIPE, built.bg, 0.1, require_coord=coord, require_depth=depth, fused=False)
        fused = render(cam, g, PIPE, built.bg, 0.1, require_coord=coord, require_depth=depth, fused=True)
        scales, opacity = gmo.scaling_n_opacity_with_3D_filter(g._scaling, g._opacity, g.filter_3D)
        direct = rasterizer(cam, g, built.bg, 0.1, coord, depth)(
            means3D=g._xyz, means2D=torch.zeros_like(g._xyz), shs=torch.cat((g._features_dc, g._features_rest), dim=1), colors_precomp=None,
            opacities=opacity, scales=scales, rotations=torch.nn.functional.normalize(g._rotation), cov3D_precomp=None)
    d_image, d_radii, d_ecoord, d_mcoord, d_edepth, d_mdepth, d_alpha, d_normal = direct
    want = {"render": d_image, "mask": d_alpha, "expected_coord": d_ecoord, "median_coord": d_mcoord, "expected_depth": d_edepth,
            "median_depth": d_mdepth, "normal": d_normal}
    for out in (eager, fused):
        assert set(out) == set(RENDER_KEYS) | {"viewspace_points", "visibility_filter", "radii"} and len(out) == 10
        for k, c in RENDER_KEYS.items():
            assert tuple(out[k].shape) == (c, H, W) and out[k].dtype == torch.float32, k
        assert tuple(out["viewspace_points"].shape) == (P, 3) and tuple(out["radii"].shape) == (P,) and out["radii"].dtype == torch.int32
        assert out["visibility_filter"].dtype == torch.bool and torch.equal(out["visibility_filter"], out["radii"] > 0)
    assert bool(eager["visibility_filter"].any()) and float(eager["render"].max()) > 0.05      # the view does see the cloud
    for k in RENDER_KEYS:
        assert same(eager[k], want[k]), k
        assert close(fused[k], want[k]), k
    assert torch.equal(eager["radii"], d_radii) and torch.equal(fused["radii"], d_radii)


def test_default_follows_the_module_switch(built, monkeypatch):
    import gaussian_model
    g = built.gaussians
    with torch.no_grad():
        for flag in (False, True):
            monkeypatch.setattr(gaussian_model, "FUSED_ACTIVATIONS", flag)
            assert all(same(a, b) for a, b in zip(g.activations(), g.activations(fused=flag)))
        a, b = g.activations(fused=True), g.activations(fused=False)
    assert same(a[0], b[0]) and same(a[2], b[2]) and same(a[3], b[3]) and close(a[1], b[1])


@pytest.mark.parametrize("branch", ["default", "cov3D_python", "SHs_python", "override_color"])
def test_integrate_is_the_direct_integrate_call(built, branch):
    from gaussian_render import eval_sh, integrate
    g, cam = built.gaussians, built.scene.getTrainCameras()[2]
    pipe = types.SimpleNamespace(convert_SHs_python=branch == "SHs_python", compute_cov3D_python=branch == "cov3D_python", debug=False)
    gen = torch.Generator(device="cpu").manual_seed(8)
    points = (g.get_xyz.detach()[torch.randint(0, 40, (300,), generator=gen).to(DEV)] + 0.05 * torch.randn((300, 3), generator=gen).to(DEV)).contiguous()
    override = torch.rand((40, 3), generator=gen).to(DEV) if branch == "override_color" else None
    with torch.no_grad():
        out = integrate(points, cam, g, pipe, built.bg, 0.1, override_color=override)
        scales, opacity = g.get_scaling_n_opacity_with_3D_filter
        kw = dict(shs=g.get_features, colors_precomp=None, scales=scales, rotations=g.get_rotation, cov3D_precomp=None)
        if branch == "cov3D_python":
            kw.update(scales=None, rotations=None, cov3D_precomp=g.get_covariance(1.0))
        elif branch == "SHs_python":
            d = g.get_xyz - cam.camera_center[None]
            kw.update(shs=None, colors_precomp=torch.clamp_min(eval_sh(3, g.get_features.transpose(1, 2), d / d.norm(dim=1, keepdim=True)) + 0.5, 0.0))
        elif branch == "override_color":
            kw.update(shs=None, colors_precomp=override)
        direct = rasterizer(cam, g, built.bg, 0.1).integrate(points3D=points, means3D=g.get_xyz, means2D=torch.zeros_like(g.get_xyz), opacities=opacity,
                                                             view2gaussian_precomp=None, **kw)
    keys = ("render", "alpha_integrated", "color_integrated", "point_coordinate", "point_sdf", "radii")
    assert set(out) == set(keys) | {"visibility_filter"} and len(out) == 7
    for k, want in zip(keys, direct):
        assert same(out[k], want), k
    assert torch.equal(out["visibility_filter"], out["radii"] > 0) and bool(out["visibility_filter"].any())
    assert tuple(out["render"].shape) == (9, cam.image_height, cam.image_width) and tuple(out["alpha_integrated"].shape) == (300,)
    if branch == "SHs_python":                               # the torch SH evaluation against the rasterizer's own
        ref = integrate(points, cam, g, PIPE, built.bg, 0.1)
        assert torch.allclose(out["render"][:3], ref["render"][:3], atol=2e-5) and torch.allclose(out["alpha_integrated"], ref["alpha_integrated"], atol=1e-6)


def test_ply_round_trip_reproduces_the_image(built):
    from gaussian_model import GaussianModel
    from gaussian_render import render
    g, cam = built.gaussians, built.scene.getTrainCameras()[0]
    path = str(built.root / "round_trip" / "point_cloud.ply")
    g.save_ply(path)
    again = GaussianModel(3)
    again.load_ply(path)
    assert again.active_sh_degree == 3
    for attr in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "filter_3D"):
        assert same(getattr(again, attr).detach(), getattr(g, attr).detach()), attr
    with torch.no_grad():
        for fused in (False, True):
            a, b = render(cam, g, PIPE, built.bg, 0.1, fused=fused), render(cam, again, PIPE, built.bg, 0.1, fused=fused)
            assert all(same(a[k], b[k]) for k in RENDER_KEYS)


@pytest.mark.parametrize("fused", [False, True])
def test_one_optimisation_step_moves_all_six_parameters(built, fused):
    import loss_utils
    from argparse import ArgumentParser

    import train_args
    from gaussian_model import GaussianModel
    from gaussian_render import render
    src, cam = built.gaussians, built.scene.getTrainCameras()[1]
    g = GaussianModel(3)
    for attr in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        setattr(g, attr, torch.nn.Parameter(getattr(src, attr).detach().clone()))
    g.filter_3D, g.active_sh_degree, g.spatial_lr_scale = src.filter_3D.clone(), 3, src.spatial_lr_scale
    g.max_radii2D = torch.zeros(40, device=DEV)
    parser = ArgumentParser()
    opt = train_args.OptimizationParams(parser).extract(parser.parse_args([]))
    g.training_setup(opt)
    g.update_learning_rate(1)
    before = {a: getattr(g, a).detach().clone() for a in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")}
    pkg = render(cam, g, PIPE, built.bg, 0.1, fused=fused)
    loss = loss_utils.photometric_loss(pkg["render"], cam.original_image.cuda(), opt.lambda_dssim)
    loss.backward()
    assert pkg["viewspace_points"].grad is not None
    g.add_densification_stats(pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"])
    assert float(g.denom.sum()) == float(pkg["visibility_filter"].sum()) and float(g.max_radii2D.max()) == float(pkg["radii"].max())
    g.optimizer.step()
    g.optimizer.zero_grad(set_to_none=True)
    for a, old in before.items():
        new = getattr(g, a).detach()
        assert bool(torch.isfinite(new).all()) and not torch.equal(new, old), a
