"""A small consistent dataset for the trainer's GPU tests, written from this project's own pieces: a ground-truth model from
synth_scene.make_scene (about 2000 Gaussians, SH degree 1), rendered by the rasterizer from six jittered cameras at 96 x 64 and saved as PNG,
and a COLMAP *text* model (cameras.txt, images.txt, points3D.txt) with about 300 of the centres as points -- scene_io's reader takes the
.txt files when there is no .bin pair.  Also the worker of the resume test:

    python tests/trainer_dataset.py DATA OUT ITERATIONS [--checkpoint_iterations N] [--start_checkpoint FILE]

runs trainer.main with the fixed view order and the compressed schedule below and prints ONE line `DIGEST <sha256>` over the six
parameters and both Adam moments, as tests/deterministic_train_worker.py forms it."""
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rade-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H, VIEWS, POINTS = 96, 64, 6, 300
PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
# the schedule compressed into the first 15 iterations: densification at 6 and 12, the opacity reset at 13
SCHEDULE = ["--densify_from_iter", "3", "--densification_interval", "6", "--densify_until_iter", "15", "--opacity_reset_interval", "13",
            "--densify_grad_threshold", "0.00002", "--opacity_lr", "0.1"]


def view_sampler(iteration, n):
    """a fixed order that visits every view"""
    return (5 * iteration + 1) % n


def rotmat2qvec(R):
    """COLMAP's (w, x, y, z) of a rotation matrix"""
    import numpy as np
    w = math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 1e-6:
        return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    raise ValueError("a half-turn: not among the jittered views")


def write(path, device="cuda:0"):
    """writes <path>/images/view_*.png and <path>/sparse/0/*.txt; returns the folder"""
    import numpy as np
    import torch

    import image_eval
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from synth_scene import jittered_view, make_scene, to_device
    base = make_scene(2000, W, H, sh_degree=1, mu_px=3.0, seed=314, kernel_size=0.1, require_coord=False, require_depth=False, filter3d=False)
    os.makedirs(os.path.join(path, "images"), exist_ok=True)
    os.makedirs(os.path.join(path, "sparse", "0"), exist_ok=True)
    focal = W / (2 * base.tanfovx)
    with open(os.path.join(path, "sparse", "0", "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        f.write(f"1 PINHOLE {W} {H} {focal!r} {focal!r} {W / 2} {H / 2}\n")
    lines = []
    for v in range(VIEWS):
        s = jittered_view(base, v, angle_deg=6.0, shift=0.6)
        w2c = s.viewmatrix.double().numpy().T
        q, t = rotmat2qvec(w2c[:3, :3]), w2c[:3, 3]
        lines.append(f"{v + 1} {' '.join(repr(float(x)) for x in q)} {' '.join(repr(float(x)) for x in t)} 1 view_{v}.png\n\n")
        d = to_device(s, device)
        rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=s.tanfovx, tanfovy=s.tanfovy, kernel_size=s.kernel_size, bg=d.bg,
                                           scale_modifier=1.0, viewmatrix=d.viewmatrix, projmatrix=d.projmatrix, sh_degree=1, campos=d.campos,
                                           prefiltered=False, require_depth=False, require_coord=False, debug=False)
        with torch.no_grad():
            image = GaussianRasterizer(rs)(means3D=d.means3D, means2D=torch.zeros_like(d.means3D), shs=d.shs[:, :4].contiguous(), colors_precomp=None,
                                           opacities=d.opacities, scales=d.scales, rotations=d.rotations, cov3D_precomp=None)[0]
        image_eval.save_png(image.clamp(0.0, 1.0), os.path.join(path, "images", f"view_{v}.png"))
    with open(os.path.join(path, "sparse", "0", "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        f.writelines(lines)
    xyz = base.means3D.double().numpy()
    front = np.flatnonzero(xyz[:, 2] > 1.0)                 # the base camera is the identity: z is the depth
    pick = front[np.random.default_rng(5).permutation(len(front))[:POINTS]]
    rgb = np.clip(0.5 + 0.28209479177387814 * base.shs[:, 0].double().numpy(), 0.0, 1.0)
    with open(os.path.join(path, "sparse", "0", "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for k, i in enumerate(pick):
            r, g, b = (int(round(255 * c)) for c in rgb[i])
            f.write(f"{k + 1} {float(xyz[i, 0])!r} {float(xyz[i, 1])!r} {float(xyz[i, 2])!r} {r} {g} {b} 0.5\n")
    return path


def digest(gaussians):
    import torch
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for a in sorted(PARAMS):
        p = getattr(gaussians, a)
        assert bool(torch.isfinite(p).all()), a
        st = gaussians.optimizer.state[p]
        for t in (p.detach(), st["exp_avg"], st["exp_avg_sq"]):
            h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def main(argv):
    import trainer
    data, out, iterations = argv[0], argv[1], argv[2]
    args = ["-s", data, "-m", out, "--iterations", iterations, "--sh_degree", "1", "--kernel_size", "0.1", "--disable_filter3D", "--regularization_from_iter",
            "8", "--test_iterations", "-1", "--save_iterations", "-1"] + SCHEDULE + list(argv[3:])
    if "--checkpoint_iterations" not in args:
        args += ["--checkpoint_iterations", "-1"]
    res = trainer.main(args, view_sampler=view_sampler)
    print("ROWS", res["gaussians"].get_xyz.shape[0], "ITERATION", res["iteration"], flush=True)
    print("DIGEST", digest(res["gaussians"]), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
