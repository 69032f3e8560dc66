"""render / integrate / render_sets: upstream's gaussian_renderer/__init__.py:19-195 and render.py:37-49 on this project's
rasterizer and model.  `pc` is a gaussian_model.GaussianModel (or anything with its properties), cameras are scene_io.Camera or anything
with the same attributes (FoVx, FoVy, image_height, image_width, world_view_transform, full_proj_transform, camera_center).

render() reads the model through `pc.activations(fused)`: one HIP launch for the four per-Gaussian inputs, or the eager composition;
`fused=None` is the model's default (gaussian_model.FUSED_ACTIVATIONS)."""
import math
import sys

import torch

from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

# real spherical harmonics, degrees 0-3, in the rasterizer's order and signs
_C0 = 0.28209479177387814
_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
       -0.5900435899266435)


def eval_sh(deg, sh, dirs):
    """sh [P,3,M] coefficients and unit directions [P,3] -> colours [P,3] (before the + 0.5), degrees 0 to 3"""
    if not 0 <= deg <= 3:
        raise NotImplementedError("eval_sh: degrees 0 to 3")
    if sh.shape[-1] < (deg + 1) ** 2:
        raise RuntimeError(f"eval_sh: degree {deg} needs {(deg + 1) ** 2} coefficients, got {sh.shape[-1]}")
    x, y, z = dirs[:, 0:1], dirs[:, 1:2], dirs[:, 2:3]
    basis = [torch.full_like(x, _C0)]
    if deg > 0:
        basis += [-_C1 * y, _C1 * z, -_C1 * x]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        basis += [_C2[0] * xy, _C2[1] * yz, _C2[2] * (2.0 * zz - xx - yy), _C2[3] * xz, _C2[4] * (xx - yy)]
    if deg > 2:
        basis += [_C3[0] * y * (3 * xx - yy), _C3[1] * xy * z, _C3[2] * y * (4 * zz - xx - yy), _C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                  _C3[4] * x * (4 * zz - xx - yy), _C3[5] * z * (xx - yy), _C3[6] * x * (xx - 3 * yy)]
    b = torch.cat(basis, dim=1)                              # [P, (deg+1)^2]
    return (sh[..., :b.shape[1]] * b[:, None, :]).sum(-1)


def _settings(viewpoint_camera, pc, pipe, bg_color, kernel_size, scaling_modifier, require_coord, require_depth):
    return GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), kernel_size=kernel_size, bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform, projmatrix=viewpoint_camera.full_proj_transform,
        sh_degree=pc.active_sh_degree, campos=viewpoint_camera.camera_center, prefiltered=False, require_coord=require_coord,
        require_depth=require_depth, debug=pipe.debug)


def _screenspace_points(pc):
    """the zero tensor whose gradient is the 2D means' (densification reads it after backward)"""
    pts = torch.zeros_like(pc.get_xyz, dtype=pc.get_xyz.dtype, requires_grad=True) + 0
    try:
        pts.retain_grad()
    except Exception:
        pass
    return pts


def _refuse_for_pose(pipe):
    """The pose gradient is formed from the cotangents of means3D, rotations and shs (pose_opt.tap).  A precomputed covariance or colour
    depends on the pose along a path that does not pass through those three, so its part of the gradient would be missing."""
    for flag, what in (("compute_cov3D_python", "the covariance is precomputed (cov3D_precomp): its rotation with the camera does not pass through "
                                                 "`rotations`"),
                       ("convert_SHs_python", "the colours are precomputed (colors_precomp / override_color): their view direction does not pass "
                                              "through `shs`")):
        if getattr(pipe, flag, False):
            raise RuntimeError(f"render(pose=...): pipe.{flag} is set and {what}; the pose gradient would be incomplete")


def render(viewpoint_camera, pc, pipe, bg_color, kernel_size, scaling_modifier=1.0, require_coord=True, require_depth=True, fused=None, pose=None):
    """Upstream's ten keys: render, mask, expected_coord, median_coord, expected_depth, median_depth, viewspace_points, visibility_filter,
    radii, normal.  `bg_color` must be on the GPU.  `pose`: a pose_opt.CameraPoses that holds this camera -- its delta receives the
    gradient of the camera's pose in the backward; None: every line executes as it did before the argument existed."""
    if pose is not None:
        _refuse_for_pose(pipe)
    rasterizer = GaussianRasterizer(raster_settings=_settings(viewpoint_camera, pc, pipe, bg_color, kernel_size, scaling_modifier, require_coord,
                                                              require_depth))
    means2D = _screenspace_points(pc)
    shs, rotations, scales, opacity = pc.activations(fused)
    means3D = pc.get_xyz
    if pose is not None:
        import pose_opt
        means3D, rotations, shs = pose_opt.tap(means3D, rotations, shs, pose.delta(viewpoint_camera.uid), viewpoint_camera, pc.active_sh_degree)
    image, radii, expected_coord, median_coord, expected_depth, median_depth, alpha, normal = rasterizer(
        means3D=means3D, means2D=means2D, shs=shs, colors_precomp=None, opacities=opacity, scales=scales, rotations=rotations,
        cov3D_precomp=None)
    return {"render": image, "mask": alpha, "expected_coord": expected_coord, "median_coord": median_coord, "expected_depth": expected_depth,
            "median_depth": median_depth, "viewspace_points": means2D, "visibility_filter": radii > 0, "radii": radii, "normal": normal}


def integrate(points3D, viewpoint_camera, pc, pipe, bg_color, kernel_size, scaling_modifier=1.0, override_color=None):
    """Upstream's seven keys: render, alpha_integrated, color_integrated, point_coordinate, point_sdf, visibility_filter, radii; the
    compute_cov3D_python and convert_SHs_python branches in plain torch."""
    rasterizer = GaussianRasterizer(raster_settings=_settings(viewpoint_camera, pc, pipe, bg_color, kernel_size, scaling_modifier, True, True))
    means2D = _screenspace_points(pc)
    scales, opacity = pc.get_scaling_n_opacity_with_3D_filter
    rotations = cov3D_precomp = None
    if pipe.compute_cov3D_python:
        scales, cov3D_precomp = None, pc.get_covariance(scaling_modifier)
    else:
        rotations = pc.get_rotation
    shs = colors_precomp = None
    if override_color is not None:
        colors_precomp = override_color
    elif pipe.convert_SHs_python:
        features = pc.get_features
        shs_view = features.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
        dir_pp = pc.get_xyz - viewpoint_camera.camera_center.repeat(features.shape[0], 1)
        colors_precomp = torch.clamp_min(eval_sh(pc.active_sh_degree, shs_view, dir_pp / dir_pp.norm(dim=1, keepdim=True)) + 0.5, 0.0)
    else:
        shs = pc.get_features
    image, alpha_integrated, color_integrated, point_coordinate, point_sdf, radii = rasterizer.integrate(
        points3D=points3D, means3D=pc.get_xyz, means2D=means2D, shs=shs, colors_precomp=colors_precomp, opacities=opacity, scales=scales,
        rotations=rotations, cov3D_precomp=cov3D_precomp, view2gaussian_precomp=None)
    return {"render": image, "alpha_integrated": alpha_integrated, "color_integrated": color_integrated, "point_coordinate": point_coordinate,
            "point_sdf": point_sdf, "visibility_filter": radii > 0, "radii": radii}


def render_sets(dataset, iteration, pipeline, skip_train, skip_test):
    """render.py:37-49: loads <model_path>/point_cloud/iteration_<iteration> (-1: the newest) and writes the renders and ground truths of
    the train and test cameras through image_eval.render_set"""
    import image_eval
    from gaussian_model import GaussianModel
    from scene_io import Scene
    with torch.no_grad():
        gaussians = GaussianModel(dataset.sh_degree)
        scene = Scene(dataset, gaussians, load_iteration=iteration, shuffle=False)
        background = torch.tensor([1, 1, 1] if dataset.white_background else [0, 0, 0], dtype=torch.float32, device="cuda")
        kernel_size = dataset.kernel_size

        def render_fn(view):
            return render(view, gaussians, pipeline, background, kernel_size)["render"]
        if not skip_train:
            image_eval.render_set(dataset.model_path, "train", scene.loaded_iter, scene.getTrainCameras(), render_fn)
        if not skip_test:
            image_eval.render_set(dataset.model_path, "test", scene.loaded_iter, scene.getTestCameras(), render_fn)


def main(argv=None):
    """python rade-gs_amd/gaussian_render.py -m OUT [--iteration N] [--skip_train] [--skip_test] [--quiet]"""
    from argparse import ArgumentParser

    import train_args
    parser = ArgumentParser(description="Testing script parameters")
    model = train_args.ModelParams(parser, sentinel=True)
    pipeline = train_args.PipelineParams(parser)
    parser.add_argument("--iteration", default=-1, type=int)
    parser.add_argument("--skip_train", action="store_true")
    parser.add_argument("--skip_test", action="store_true")
    parser.add_argument("--quiet", action="store_true")
    args = train_args.get_combined_args(parser, argv)
    print("Rendering " + args.model_path)
    render_sets(model.extract(args), args.iteration, pipeline.extract(args), args.skip_train, args.skip_test)


def install():
    """Registers this module as `gaussian_renderer`, so that upstream's `from gaussian_renderer import render, integrate` resolves to it.
    Opt-in: nothing calls it."""
    sys.modules["gaussian_renderer"] = sys.modules[__name__]
    return sys.modules[__name__]


if __name__ == "__main__":
    main()
