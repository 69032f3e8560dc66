"""Measures the fused model activations (csrc/radegs_activate.hip) against the eager composition, on the GPU, at C2 scale (1 M Gaussians,
1920 x 1080, SH degree 3, depth + normal regulariser), in ONE process with the two settings interleaved:

  (i)  the full training iteration through gaussian_model.GaussianModel + gaussian_render.render -- activations, rasterizer, photometric and
       normal-consistency loss, backward, fused Adam -- with fused against eager activations;
  (ii) the two activation calls alone (forward + backward with all four cotangents) against the sum of torch.cat, F.normalize and
       radegs_filter3d_* with their autograd, with the bytes the algorithm has to move and the GB/s that makes.

    python scripts/gpu_trainer_bench.py [--config C2] [--steps 100] [--rounds 7] [--out profiles/trainer_bench.json]

Times are device events around windows that end in a synchronise; every shape is warmed up first; the figure reported per setting is the
median over the rounds, with the smallest and largest next to it.  No GPU, no number: the script fails without one."""
import argparse
import json
import math
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rade-gs_amd"))


def build(config, dev):
    import torch

    from gaussian_model import GaussianModel
    from synth_scene import make_config, to_device
    s = to_device(make_config(config), dev)
    P = s.means3D.shape[0]
    g = GaussianModel(s.sh_degree, device=dev)
    gen = torch.Generator(device="cpu").manual_seed(0)
    raw = dict(_xyz=s.means3D, _features_dc=s.shs[:, :1], _features_rest=s.shs[:, 1:], _opacity=torch.logit(s.opacities.clamp(1e-4, 1 - 1e-4)),
               _scaling=torch.log(s.scales), _rotation=s.rotations * (0.5 + 1.5 * torch.rand((P, 1), generator=gen).to(dev)))
    for k, v in raw.items():
        setattr(g, k, torch.nn.Parameter(v.contiguous().clone()))
    g.filter_3D = torch.full((P, 1), 0.002, device=dev)
    g.active_sh_degree, g.spatial_lr_scale, g.max_radii2D = s.sh_degree, 1.0, torch.zeros(P, device=dev)
    cam = types.SimpleNamespace(FoVx=2 * math.atan(s.tanfovx), FoVy=2 * math.atan(s.tanfovy), image_width=s.W, image_height=s.H,
                                world_view_transform=s.viewmatrix, full_proj_transform=s.projmatrix, camera_center=s.campos)
    return s, g, cam


def timed(fn, steps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def summary(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "rounds": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainer_bench.json"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("gpu_trainer_bench.py measures on the GPU and there is none")
    import gaussian_model_ops as gmo
    import graphics_utils as gu
    import loss_utils as lu
    import train_args
    from gaussian_render import render
    dev = torch.device("cuda:0")
    s, g, cam = build(args.config, dev)
    P, K = g.get_xyz.shape[0], g._features_rest.shape[1]
    parser = argparse.ArgumentParser()
    opt = train_args.OptimizationParams(parser).extract(parser.parse_args([]))
    g.training_setup(opt)
    pipe = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    with torch.no_grad():
        target = render(cam, g, pipe, s.bg, s.kernel_size, require_coord=False, require_depth=True, fused=False)["render"].clone()
        for p in (g._features_dc, g._opacity, g._scaling):      # away from the optimum: every gradient is live
            p.add_(0.1 * torch.randn_like(p))

    def iteration(fused):
        def run():
            pkg = render(cam, g, pipe, s.bg, s.kernel_size, require_coord=False, require_depth=True, fused=fused)
            loss = lu.photometric_loss(pkg["render"], target, opt.lambda_dssim) + opt.lambda_depth_normal * gu.normal_consistency_loss(
                cam, pkg["normal"], pkg["expected_depth"], pkg["median_depth"], 0.6)
            loss.backward()
            g.optimizer.step()
            g.optimizer.zero_grad(set_to_none=True)
        return run

    cot = [torch.randn((P, K + 1, 3), device=dev), torch.randn((P, 4), device=dev), torch.randn((P, 3), device=dev), torch.randn((P, 1), device=dev)]
    leaves = [g._features_dc, g._features_rest, g._rotation, g._scaling, g._opacity]

    def activations(fused):
        def run():
            if fused:
                outs = gmo.model_activations(*leaves, g.filter_3D)
            else:
                scales, opacity = gmo.scaling_n_opacity_with_3D_filter(g._scaling, g._opacity, g.filter_3D)
                outs = (torch.cat((g._features_dc, g._features_rest), dim=1), F.normalize(g._rotation), scales, opacity)
            torch.autograd.backward(outs, cot)
            for p in leaves:
                p.grad = None
        return run

    res = {"config": args.config, "P": P, "K": K, "width": s.W, "height": s.H, "steps_per_window": args.steps, "device": torch.cuda.get_device_name(0)}
    for name, make, steps in (("iteration", iteration, args.steps), ("activations", activations, 5 * args.steps)):
        fns = {"eager": make(False), "fused": make(True)}
        for fn in fns.values():                               # warm-up: code objects, the allocator's blocks, the binning capacity
            timed(fn, 3)
        samples = {"eager": [], "fused": []}
        for r in range(args.rounds):
            for mode in (("eager", "fused") if r % 2 == 0 else ("fused", "eager")):
                samples[mode].append(timed(fns[mode], steps))
        res[name] = {m: summary(v) for m, v in samples.items()}
        res[name]["fused_over_eager"] = res[name]["fused"]["median_ms"] / res[name]["eager"]["median_ms"]
    # the bytes the activations have to move, forward + backward, per Gaussian: every input read once, every output written once
    fwd = 4 * (3 + 3 * K + 4 + 3 + 1 + 1) + 4 * (3 * (K + 1) + 4 + 3 + 1)
    bwd = 4 * (4 + 3 + 1 + 1) + 4 * (3 * (K + 1) + 4 + 3 + 1) + 4 * (3 + 3 * K + 4 + 3 + 1)
    res["activations"]["bytes_per_gaussian"] = {"forward": fwd, "backward": bwd}
    for m in ("eager", "fused"):
        res["activations"][m]["GBps_of_needed_bytes"] = (fwd + bwd) * P / (res["activations"][m]["median_ms"] * 1e-3) / 1e9
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
