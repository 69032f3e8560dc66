"""Measures camera pose refinement (csrc/radegs_pose.hip, pose_opt.py) on the GPU at C2 scale (1 M Gaussians, 1920 x 1080, SH degree 3), in ONE
process:

  (i)   radegs_pose_gradient alone on the cotangents of a real backward, for a trained-scene-shaped visibility (config C2H: clustered
        Gaussians, a share of them outside the view) and with every Gaussian counted as visible (every DC cotangent made non-zero);
  (ii)  radegs_pose_step alone;
  (iii) the full training iteration of scripts/gpu_trainer_bench.py (fused activations) with and without pose=, interleaved, next to the
        iteration the parent commit recorded in profiles/trainer_bench.json.

    python scripts/gpu_pose_bench.py [--steps 100] [--rounds 7] [--out profiles/pose_bench.json]

Times are device events around windows that end in a synchronise; every shape is warmed up first; medians over the rounds with the smallest
and largest next to them.  Reported, not thresholded.  No GPU, no number: the script fails without one."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rade-gs_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_pose_bench.py measures on the GPU and there is none")
    import graphics_utils as gu
    import loss_utils as lu
    import pose_opt
    import train_args
    from gaussian_render import render
    from gpu_trainer_bench import build, summary, timed
    from synth_scene import projection_matrix
    dev = torch.device("cuda:0")
    pipe = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    parser = argparse.ArgumentParser()
    opt = train_args.OptimizationParams(parser).extract(parser.parse_args([]))
    res = {"steps_per_window": args.steps, "device": torch.cuda.get_device_name(0)}

    def camera_for(s, cam):
        cam.uid, cam.R, cam.T = 0, np.eye(3), np.zeros(3)
        cam.projection_matrix = torch.from_numpy(np.ascontiguousarray(projection_matrix(0.01, 100.0, cam.FoVx, cam.FoVy).T, dtype=np.float32)).to(dev)
        cam.world_view_transform, cam.full_proj_transform, cam.camera_center = (t.clone().contiguous() for t in (s.viewmatrix, s.projmatrix, s.campos))
        return cam

    # ---- (i) the gradient kernel on the cotangents of a real backward ---------------------------------------------------------------------
    s, g, cam = build("C2H", dev)
    cam = camera_for(s, cam)
    g.training_setup(opt)
    poses = pose_opt.CameraPoses([cam])
    pose_opt.KEEP_LAST = True
    pkg = render(cam, g, pipe, s.bg, s.kernel_size, require_coord=False, require_depth=True, pose=poses)
    (pkg["render"].square().mean() + pkg["expected_depth"].mean()).backward()
    pose_opt.KEEP_LAST = False
    saw = pose_opt.LAST
    P = saw["means3D"].shape[0]
    live = int((saw["dL_dsh"][:, 0, :] != 0).any(1).sum())
    every = saw["dL_dsh"].clone()
    every[:, 0, :] = torch.where(every[:, 0, :] == 0, torch.full_like(every[:, 0, :], 1e-3), every[:, 0, :])

    def kernel(dsh):
        return lambda: pose_opt.pose_gradient(saw["means3D"], saw["rotations"], saw["shs"], 3, cam.camera_center, cam.world_view_transform,
                                              saw["dL_dmeans3D"], saw["dL_drotations"], dsh)
    res["gradient_kernel"] = {"P": P, "sh_degree": 3, "rows_with_a_DC_cotangent": live,
                              "note": "per call of pose_opt.pose_gradient back to back: both launches and the wrapper's two allocations, device events"}
    for name, fn, nlive in (("trained_scene_visibility", kernel(saw["dL_dsh"]), live), ("all_visible", kernel(every), P)):
        timed(fn, 10)
        r = summary([timed(fn, 5 * args.steps) for _ in range(args.rounds)])
        r["bytes"] = 68 * P + 192 * nlive
        r["GBps_of_needed_bytes"] = r["bytes"] / (r["median_ms"] * 1e-3) / 1e9
        res["gradient_kernel"][name] = r
    # ---- (ii) the step ------------------------------------------------------------------------------------------------------------------------
    grad = poses.grad(0).clone()

    def step():
        poses.delta(0).grad = grad
        poses.step(0)
    timed(step, 10)
    res["pose_step"] = summary([timed(step, 5 * args.steps) for _ in range(args.rounds)])
    res["pose_step"]["note"] = "one launch plus the Python around it (a fresh delta tensor per call)"
    del s, g, cam, poses, saw, every
    torch.cuda.empty_cache()
    # ---- (iii) the training iteration -----------------------------------------------------------------------------------------------------------
    s, g, cam = build("C2", dev)
    cam = camera_for(s, cam)
    g.training_setup(opt)
    poses = pose_opt.CameraPoses([cam], 1e-6, 1e-6)
    with torch.no_grad():
        target = render(cam, g, pipe, s.bg, s.kernel_size, require_coord=False, require_depth=True, fused=False)["render"].clone()
        for p in (g._features_dc, g._opacity, g._scaling):
            p.add_(0.1 * torch.randn_like(p))

    def iteration(with_pose):
        def run():
            pkg = render(cam, g, pipe, s.bg, s.kernel_size, require_coord=False, require_depth=True, pose=poses if with_pose else None)
            loss = lu.photometric_loss(pkg["render"], target, opt.lambda_dssim) + opt.lambda_depth_normal * gu.normal_consistency_loss(
                cam, pkg["normal"], pkg["expected_depth"], pkg["median_depth"], 0.6)
            loss.backward()
            g.optimizer.step()
            g.optimizer.zero_grad(set_to_none=True)
            if with_pose:
                poses.step(0)
        return run
    fns = {"without_pose": iteration(False), "with_pose": iteration(True)}
    for fn in fns.values():
        timed(fn, 3)
    samples = {k: [] for k in fns}
    for r in range(args.rounds):
        for mode in (("without_pose", "with_pose") if r % 2 == 0 else ("with_pose", "without_pose")):
            samples[mode].append(timed(fns[mode], args.steps))
    res["iteration"] = {m: summary(v) for m, v in samples.items()}
    res["iteration"]["config"] = "C2"
    res["iteration"]["with_over_without"] = res["iteration"]["with_pose"]["median_ms"] / res["iteration"]["without_pose"]["median_ms"]
    parent = os.path.join(ROOT, "profiles", "trainer_bench.json")
    if os.path.exists(parent):
        with open(parent) as f:
            res["iteration"]["parent_commit_fused_median_ms"] = json.load(f)["iteration"]["fused"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
