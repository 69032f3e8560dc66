"""Worker of tests/test_gpu_deterministic.py::test_training_loop_is_reproducible: the optimisation loop of tests/test_gpu_train_loop.py
(3D-filter activations -> rasterizer -> normal-consistency + L1/SSIM loss -> backward -> Adam; 3000 Gaussians, 192 x 128) for a number of
iterations, then ONE line `DIGEST <sha256>` over every parameter and both Adam moments.  Run as a fresh process so that the history of
forward calls (binning speculation, which blend formulation a view gets) is the same every time; the switch comes from the environment
(RADEGS_DETERMINISTIC).

    python tests/deterministic_train_worker.py [iterations]
"""
import hashlib
import math
import os
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rade-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

View = namedtuple("View", "image_width image_height FoVx FoVy")


def main(iters):
    import torch

    import fused_adam
    import gaussian_model_ops as gmo
    import graphics_utils as gu
    import loss_utils as lu
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from synth_scene import make_scene, to_device
    dev = torch.device("cuda:0")
    s = to_device(make_scene(3000, 192, 128, sh_degree=1, mu_px=4.0, seed=90, kernel_size=0.1, require_coord=False, require_depth=True,
                             filter3d=False), dev)
    view = View(s.W, s.H, 2 * math.atan(s.tanfovx), 2 * math.atan(s.tanfovy))
    rs = GaussianRasterizationSettings(image_height=s.H, image_width=s.W, tanfovx=s.tanfovx, tanfovy=s.tanfovy, kernel_size=s.kernel_size,
                                       bg=s.bg, scale_modifier=1.0, viewmatrix=s.viewmatrix, projmatrix=s.projmatrix, sh_degree=s.sh_degree,
                                       campos=s.campos, prefiltered=False, require_depth=True, require_coord=False, debug=False)
    rast = GaussianRasterizer(rs)
    filter_3D = torch.full((s.means3D.shape[0], 1), 0.002, device=dev)

    def render(xyz, f, op_raw, sc_raw, rot):
        scales, opacity = gmo.scaling_n_opacity_with_3D_filter(sc_raw, op_raw, filter_3D)
        return rast(means3D=xyz, means2D=torch.zeros_like(xyz, requires_grad=True), shs=f, colors_precomp=None, opacities=opacity,
                    scales=scales, rotations=torch.nn.functional.normalize(rot), cov3D_precomp=None)

    gt = dict(xyz=s.means3D, f=s.shs[:, :4].contiguous(), op=torch.logit(s.opacities.clamp(1e-4, 1 - 1e-4)), sc=torch.log(s.scales), rot=s.rotations)
    with torch.no_grad():
        target = render(gt["xyz"], gt["f"], gt["op"], gt["sc"], gt["rot"])[0]
    g = torch.Generator(device="cpu").manual_seed(0)
    P = s.means3D.shape[0]
    params = dict(xyz=(gt["xyz"] + 0.01 * torch.randn(P, 3, generator=g).to(dev)), f=(gt["f"] + 0.3 * torch.randn(P, 4, 3, generator=g).to(dev)),
                  op=(gt["op"] + 0.5 * torch.randn(P, 1, generator=g).to(dev)), sc=(gt["sc"] + 0.2 * torch.randn(P, 3, generator=g).to(dev)),
                  rot=gt["rot"].clone())
    params = {k: torch.nn.Parameter(v.contiguous()) for k, v in params.items()}
    lrs = dict(xyz=1e-4, f=5e-3, op=2e-2, sc=5e-3, rot=1e-3)
    opt = fused_adam.Adam([{"params": [params[k]], "lr": lrs[k], "name": k} for k in params], lr=0.0, eps=1e-15)
    for _ in range(iters):
        out = render(params["xyz"], params["f"], params["op"], params["sc"], params["rot"])
        image, depth, mdepth, normal = out[0], out[4], out[5], out[7]
        loss = lu.photometric_loss(image, target, 0.2) + 0.05 * gu.normal_consistency_loss(view, normal, depth, mdepth, 0.6)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    torch.cuda.synchronize(dev)
    h = hashlib.sha256()
    for k in sorted(params):
        p = params[k]
        assert bool(torch.isfinite(p).all()), k
        for t in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]):
            h.update(t.contiguous().cpu().numpy().tobytes())
    print("DIGEST", h.hexdigest(), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 15)
