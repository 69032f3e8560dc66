"""The training loop: upstream's train.py:61-214 statement for statement on this project's ops -- scene_io.Scene,
gaussian_model.GaussianModel, gaussian_render.render, loss_utils, graphics_utils.normal_consistency_loss, the fused densification and
Adam -- with checkpoints, the evaluation report and upstream's command line.

    python rade-gs_amd/trainer.py -s DATA -m OUT [--iterations N] [--start_checkpoint OUT/chkpntN.pth] ...

Omitted: the network viewer (`--ip`, `--port` are accepted and ignored), TensorBoard and tqdm.  The report upstream sends to TensorBoard
is printed and appended to <model_path>/training_report.json."""
import json
import os
import random
import sys
import uuid
from argparse import ArgumentParser, Namespace
from random import randint

import numpy as np
import torch


def prepare_output_and_logger(args):
    """makes <model_path> (./output/<10 characters> when none is given) and writes `cfg_args`: str(Namespace(**vars(args))), the file
    train_args.get_combined_args reads back"""
    if not args.model_path:
        unique_str = os.getenv("OAR_JOB_ID") or str(uuid.uuid4())
        args.model_path = os.path.join("./output/", unique_str[0:10])
    print("Output folder: {}".format(args.model_path))
    os.makedirs(args.model_path, exist_ok=True)
    with open(os.path.join(args.model_path, "cfg_args"), "w") as cfg_log_f:
        cfg_log_f.write(str(Namespace(**vars(args))))


def psnr(img1, img2):
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


@torch.no_grad()
def training_report(iteration, Ll1, loss, normal_loss, testing_iterations, scene, render_fn, render_args):
    """At `testing_iterations`: mean L1 and PSNR over the test cameras and over upstream's five training cameras (indices 5, 10, ..., 25
    modulo their number), printed, written to chkpnt<iteration>.txt for the test set as upstream does, and appended to
    <model_path>/training_report.json.  Returns the record, or None at other iterations."""
    import loss_utils
    if iteration not in testing_iterations:
        return None
    torch.cuda.empty_cache()
    train = scene.getTrainCameras()
    configs = ({"name": "test", "cameras": scene.getTestCameras()},
               {"name": "train", "cameras": [train[idx % len(train)] for idx in range(5, 30, 5)] if train else []})
    record = {"iteration": iteration, "l1_loss": float(Ll1), "total_loss": float(loss), "normal_loss": float(normal_loss),
              "total_points": int(scene.gaussians.get_xyz.shape[0])}
    for config in configs:
        if not config["cameras"]:
            continue
        l1_test, psnr_test = 0.0, 0.0
        for viewpoint in config["cameras"]:
            image = torch.clamp(render_fn(viewpoint, scene.gaussians, *render_args)["render"], 0.0, 1.0)
            gt_image = torch.clamp(viewpoint.original_image.cuda(), 0.0, 1.0)
            l1_test += loss_utils.l1_loss(image, gt_image).mean().double()
            psnr_test += psnr(image, gt_image).mean().double()
        psnr_test /= len(config["cameras"])
        l1_test /= len(config["cameras"])
        line = "\n[ITER {}] Evaluating {}: L1 {} PSNR {}".format(iteration, config["name"], l1_test, psnr_test)
        print(line)
        if config["name"] == "test":
            with open(scene.model_path + "/chkpnt" + str(iteration) + ".txt", "w") as file_object:
                print(line, file=file_object)
        record[config["name"]] = {"l1": float(l1_test), "psnr": float(psnr_test), "views": len(config["cameras"])}
    path = os.path.join(scene.model_path, "training_report.json")
    history = []
    if os.path.exists(path):
        with open(path) as f:
            history = json.load(f)
    history.append(record)
    with open(path, "w") as f:
        json.dump(history, f, indent=1)
    torch.cuda.empty_cache()
    return record


def write_refined_cameras(scene, cameras):
    """<model_path>/cameras_refined.json, beside upstream's cameras.json and with its keys, from the cameras' host-side R / T"""
    from scene_io import fov2focal
    records = []
    for id, cam in enumerate(cameras):
        Rt = np.zeros((4, 4))
        Rt[:3, :3], Rt[:3, 3], Rt[3, 3] = np.asarray(cam.R).transpose(), cam.T, 1.0
        C2W = np.linalg.inv(Rt)
        records.append({"id": id, "img_name": cam.image_name, "width": int(cam.image_width), "height": int(cam.image_height), "position": C2W[:3, 3].tolist(),
                        "rotation": [x.tolist() for x in C2W[:3, :3]], "fy": fov2focal(cam.FoVy, cam.image_height), "fx": fov2focal(cam.FoVx, cam.image_width)})
    with open(os.path.join(scene.model_path, "cameras_refined.json"), "w") as f:
        json.dump(records, f)


def training(dataset, opt, pipe, testing_iterations, saving_iterations, checkpoint_iterations, checkpoint, debug_from, view_sampler=None, pose_args=None):
    """train.py:61-214.  view_sampler(iteration, n_train) -> index into the training cameras replaces upstream's pop from a shuffled stack
    (which draws from Python's `random`) when given.  pose_args (optimize_poses, pose_lr_translation, pose_lr_rotation, pose_from_iter):
    refine the training cameras' poses along with the Gaussians (pose_opt.py); None or optimize_poses off: the loop is upstream's.
    Returns {"iteration": the last one run, "losses": [loss per iteration], "report": [training_report's records], "gaussians", "scene",
    "poses": the CameraPoses or None}."""
    import graphics_utils
    import loss_utils
    from gaussian_model import GaussianModel
    from gaussian_render import render
    from scene_io import Scene
    first_iter = 0
    prepare_output_and_logger(dataset)
    gaussians = GaussianModel(dataset.sh_degree)
    scene = Scene(dataset, gaussians)
    gaussians.training_setup(opt)
    poses = None
    if pose_args is not None and pose_args.optimize_poses:
        import pose_opt
        from diff_gaussian_rasterization import _C
        poses = pose_opt.CameraPoses(scene.getTrainCameras(), pose_args.pose_lr_translation, pose_args.pose_lr_rotation)
        if dataset.kernel_size > 0 and not _C.OPACITY_GRAD_INTENDED:
            # the pose gradient is linear in what the backward returns and inherits the reference's argument slip, which a kernel_size above
            # zero makes large: this run takes the intended derivative
            _C.OPACITY_GRAD_INTENDED = True
            print("--optimize_poses with kernel_size > 0: switching the backward to opacity_grad_intended")
    if checkpoint:
        loaded = torch.load(checkpoint, weights_only=False)
        (model_params, first_iter) = loaded[0], loaded[1]
        gaussians.restore(model_params, opt)
        if poses is not None and len(loaded) > 2:
            poses.load_state_dict(loaded[2])
    bg_color = [1, 1, 1] if dataset.white_background else [0, 0, 0]
    background = torch.tensor(bg_color, dtype=torch.float32, device="cuda")
    kernel_size = dataset.kernel_size

    trainCameras = scene.getTrainCameras().copy()
    if dataset.disable_filter3D:
        gaussians.reset_3D_filter()
    else:
        gaussians.compute_3D_filter(cameras=trainCameras)

    viewpoint_stack = None
    require_depth = not dataset.use_coord_map
    require_coord = dataset.use_coord_map
    losses, report = [], []
    iteration = first_iter
    first_iter += 1
    for iteration in range(first_iter, opt.iterations + 1):
        gaussians.update_learning_rate(iteration)

        # every 1000 iterations one more SH degree, up to the maximum
        if iteration % 1000 == 0:
            gaussians.oneupSHdegree()

        if view_sampler is not None:
            viewpoint_cam = trainCameras[int(view_sampler(iteration, len(trainCameras)))]
        else:
            if not viewpoint_stack:
                viewpoint_stack = scene.getTrainCameras().copy()
            viewpoint_cam = viewpoint_stack.pop(randint(0, len(viewpoint_stack) - 1))

        if (iteration - 1) == debug_from:
            pipe.debug = True

        reg_kick_on = iteration >= opt.regularization_from_iter
        pose_on = poses is not None and iteration >= pose_args.pose_from_iter
        if pose_on:
            render_pkg = render(viewpoint_cam, gaussians, pipe, background, kernel_size, require_coord=require_coord and reg_kick_on,
                                require_depth=require_depth and reg_kick_on, pose=poses)
        else:
            render_pkg = render(viewpoint_cam, gaussians, pipe, background, kernel_size, require_coord=require_coord and reg_kick_on,
                                require_depth=require_depth and reg_kick_on)
        rendered_image, viewspace_point_tensor, visibility_filter, radii = (render_pkg["render"], render_pkg["viewspace_points"],
                                                                            render_pkg["visibility_filter"], render_pkg["radii"])
        gt_image = viewpoint_cam.original_image.cuda()

        if dataset.use_decoupled_appearance:
            Ll1_render = loss_utils.l1_loss_appearance(rendered_image, gt_image, gaussians, viewpoint_cam.uid)
            rgb_loss = (1.0 - opt.lambda_dssim) * Ll1_render + opt.lambda_dssim * (1.0 - loss_utils.ssim(rendered_image, gt_image))
        else:
            # (1 - lambda) * l1 + lambda * (1 - ssim) and the L1 term on its own from one launch
            rgb_loss, Ll1_render, _ = loss_utils._Photometric.apply(rendered_image, gt_image, opt.lambda_dssim)

        if reg_kick_on:
            lambda_depth_normal = opt.lambda_depth_normal
            if require_depth:
                depth_normal_loss = graphics_utils.normal_consistency_loss(viewpoint_cam, render_pkg["normal"], render_pkg["expected_depth"],
                                                                           render_pkg["median_depth"], 0.6)
            else:
                depth_normal_loss = graphics_utils.normal_consistency_loss(viewpoint_cam, render_pkg["normal"], render_pkg["expected_coord"],
                                                                           render_pkg["median_coord"], 0.6, points=True)
        else:
            lambda_depth_normal = 0
            depth_normal_loss = torch.tensor([0], dtype=torch.float32, device="cuda")

        loss = rgb_loss + depth_normal_loss * lambda_depth_normal
        loss.backward()

        with torch.no_grad():
            losses.append(float(loss.item()))
            if iteration % 10 == 0:
                print(f"[ITER {iteration}] loss {losses[-1]:.4f} loss_normal {float(depth_normal_loss.item()):.4f} points {gaussians.get_xyz.shape[0]}")

            rec = training_report(iteration, Ll1_render, loss, depth_normal_loss, testing_iterations, scene, render, (pipe, background, kernel_size))
            if rec is not None:
                report.append(rec)
            if iteration in saving_iterations:
                print("\n[ITER {}] Saving Gaussians".format(iteration))
                scene.save(iteration)
                if poses is not None:
                    poses.sync()
                    write_refined_cameras(scene, poses.cameras)

            # densification
            if iteration < opt.densify_until_iter:
                # the statistics and `max_radii2D = max(max_radii2D, radii)` on the visible rows in one launch
                gaussians.add_densification_stats(viewspace_point_tensor, visibility_filter, radii)

                if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                    size_threshold = 20 if iteration > opt.opacity_reset_interval else None
                    gaussians.densify_and_prune(opt.densify_grad_threshold, 0.05, scene.cameras_extent, size_threshold)
                    if dataset.disable_filter3D:
                        gaussians.reset_3D_filter()
                    else:
                        if poses is not None:
                            poses.sync()
                        gaussians.compute_3D_filter(cameras=trainCameras)

                if iteration % opt.opacity_reset_interval == 0 or (dataset.white_background and iteration == opt.densify_from_iter):
                    gaussians.reset_opacity()

            if iteration % 100 == 0 and iteration > opt.densify_until_iter and not dataset.disable_filter3D:
                if iteration < opt.iterations - 100:     # not at the end of training
                    if poses is not None:
                        poses.sync()
                    gaussians.compute_3D_filter(cameras=trainCameras)

            if iteration < opt.iterations:
                gaussians.optimizer.step()
                gaussians.optimizer.zero_grad(set_to_none=True)
                if pose_on:
                    poses.step(viewpoint_cam.uid)

            if iteration in checkpoint_iterations:
                print("\n[ITER {}] Saving Checkpoint".format(iteration))
                if poses is not None:
                    poses.sync()
                    torch.save((gaussians.capture(), iteration, poses.state_dict()), scene.model_path + "/chkpnt" + str(iteration) + ".pth")
                else:
                    torch.save((gaussians.capture(), iteration), scene.model_path + "/chkpnt" + str(iteration) + ".pth")
    if poses is not None:
        poses.sync()
        write_refined_cameras(scene, poses.cameras)
    return {"iteration": iteration, "losses": losses, "report": report, "gaussians": gaussians, "scene": scene, "poses": poses}


class _Quiet:
    """stdout that drops everything (`--quiet`)"""

    def write(self, x):
        return len(x)

    def flush(self):
        pass


def safe_state(silent):
    """seeds Python's, NumPy's and torch's generators with 0 and selects cuda:0, as upstream's safe_state; `silent` drops stdout"""
    if silent:
        sys.stdout = _Quiet()
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    torch.cuda.set_device(torch.device("cuda:0"))


def main(argv=None, view_sampler=None):
    """upstream's command line; returns training()'s record"""
    import train_args
    parser = ArgumentParser(description="Training script parameters")
    lp = train_args.ModelParams(parser)
    op = train_args.OptimizationParams(parser)
    pp = train_args.PipelineParams(parser)
    parser.add_argument("--ip", type=str, default="127.0.0.1")       # the network viewer is not built: accepted, ignored
    parser.add_argument("--port", type=int, default=6009)
    parser.add_argument("--debug_from", type=int, default=-1)
    parser.add_argument("--detect_anomaly", action="store_true", default=False)
    parser.add_argument("--test_iterations", nargs="+", type=int, default=[7_000, 30_000])
    parser.add_argument("--save_iterations", nargs="+", type=int, default=[7_000, 30_000])
    parser.add_argument("--quiet", action="store_true")
    parser.add_argument("--checkpoint_iterations", nargs="+", type=int, default=[15000])
    parser.add_argument("--start_checkpoint", type=str, default=None)
    # camera pose refinement (pose_opt.py), off by default; the trainer's own flags, not upstream's
    parser.add_argument("--optimize_poses", action="store_true", default=False)
    parser.add_argument("--pose_lr_translation", type=float, default=1e-4)
    parser.add_argument("--pose_lr_rotation", type=float, default=1e-4)
    parser.add_argument("--pose_from_iter", type=int, default=0)
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    args.save_iterations.append(args.iterations)
    print("Optimizing " + args.model_path)
    stdout = sys.stdout
    safe_state(args.quiet)
    try:
        with torch.autograd.set_detect_anomaly(args.detect_anomaly):
            out = training(lp.extract(args), op.extract(args), pp.extract(args), args.test_iterations, args.save_iterations,
                           args.checkpoint_iterations, args.start_checkpoint, args.debug_from, view_sampler=view_sampler, pose_args=args)
    finally:
        sys.stdout = stdout
    print("\nTraining complete.")
    return out


if __name__ == "__main__":
    main()
