"""trainer.training / trainer.main on the GPU, on a dataset the test writes itself (tests/trainer_dataset.py: a synthetic ground truth rendered
from six cameras at 96 x 64, a COLMAP text model with 300 points).

(a) 60 iterations with the schedule compressed so that two densifications and an opacity reset fall inside leave upstream's artefacts, a
    model of another size, a lower mean L1 over the training views, finite parameters.
(b) With the eager activations, the deterministic backward and a fixed view order the trainer's parameters after 30 iterations equal, bit
    for bit, those of an arbiter loop written here from the ops the project had before the trainer (as tests/test_gpu_train_loop.py wires
    them).  With the fused activations the final mean training L1 stays within a band of the arbiter's: four times the difference the
    arbiter loop itself shows between its deterministic and its atomic backward (its own order noise), printed.  The band is ONE sample
    of that noise, so it varies from run to run.  Measured on the MI355X: in this test, |fused - arbiter| = 9.9e-9 against a band of
    4 x 6.2e-9; in a process of its own, |fused - arbiter| = 0 (9.3e-10 with the L1 summed in float64) and eight atomic runs gave
    |atomic - deterministic| = 3.7e-9, 1.2e-8, 0, 1.5e-8, 1.2e-8, 1.4e-8, 6.2e-10, 1.2e-8 -- all of it at the resolution of a
    float32 mean near 0.069 (7.5e-9 per view), and two of the eight samples would have made a band below 9.9e-9.  The check can
    therefore miss by chance; when it does, the printed figures say which side moved.
(c) Resume: three fresh processes, one after the other, each under its own time limit.  40 iterations straight; 21 iterations with a
    checkpoint at 20; 20 more from that checkpoint.  (Upstream's loop takes no optimizer step in its LAST iteration, so a run of exactly 20
    iterations would checkpoint a state the straight run never passes through: the second run goes one iteration further and its
    checkpoint is the state after the step of iteration 20.)  The digest over the parameters and both Adam moments is the same for the
    straight and the resumed run.  disable_filter3D: upstream does not checkpoint filter_3D and recomputes it from the resumed positions,
    so with the filter on the two differ by design."""
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import trainer_dataset as td

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return td.write(str(tmp_path_factory.mktemp("trainer") / "data"), DEV)


def raster(cam, sh_degree, bg, kernel_size, require_depth):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    return GaussianRasterizer(GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        kernel_size=kernel_size, bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
        sh_degree=sh_degree, campos=cam.camera_center, prefiltered=False, require_depth=require_depth, require_coord=False, debug=False))


def eager_render(m, cam, bg, kernel_size, require_depth):
    """the pre-step and the rasterizer as tests/test_gpu_train_loop.py wires them; `m` has the six raw parameters and filter_3D"""
    import gaussian_model_ops as gmo
    scales, opacity = gmo.scaling_n_opacity_with_3D_filter(m._scaling, m._opacity, m.filter_3D)
    means2D = torch.zeros_like(m._xyz, requires_grad=True) + 0
    return raster(cam, m.active_sh_degree, bg, kernel_size, require_depth)(
        means3D=m._xyz, means2D=means2D, shs=torch.cat((m._features_dc, m._features_rest), dim=1), colors_precomp=None, opacities=opacity,
        scales=scales, rotations=torch.nn.functional.normalize(m._rotation), cov3D_precomp=None)


@torch.no_grad()
def mean_train_l1(m, cams, kernel_size=0.1):
    bg = torch.zeros(3, device=DEV)
    return float(np.mean([float((eager_render(m, c, bg, kernel_size, False)[0] - c.original_image.cuda()).abs().mean()) for c in cams]))


def dataset_args(data, out):
    return types.SimpleNamespace(source_path=data, model_path=out, images="images", eval=False, white_background=False, resolution=-1, data_device="cuda")


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------
def test_main_trains_and_leaves_upstreams_artefacts(data, tmp_path, capsys):
    import model_io
    import scene_io
    import trainer
    from gaussian_model import GaussianModel
    # the state training starts from, made the way training() makes it
    start = GaussianModel(1)
    scene = scene_io.Scene(dataset_args(data, str(tmp_path / "start")), start)
    cams = scene.getTrainCameras()
    start.compute_3D_filter(cams)
    before, rows_before = mean_train_l1(start, cams), start.get_xyz.shape[0]
    assert len(cams) == td.VIEWS and rows_before == td.POINTS and (cams[0].image_width, cams[0].image_height) == (td.W, td.H)
    out = str(tmp_path / "out")
    res = trainer.main(["-s", data, "-m", out, "--iterations", "60", "--sh_degree", "1", "--kernel_size", "0.1", "--regularization_from_iter", "30",
                        "--test_iterations", "30", "60", "--save_iterations", "60", "--checkpoint_iterations", "60"] + td.SCHEDULE,
                       view_sampler=td.view_sampler)
    g = res["gaussians"]
    assert res["iteration"] == 60 and len(res["losses"]) == 60 and all(math.isfinite(x) for x in res["losses"])
    for name in ("cfg_args", "cameras.json", "input.ply", "chkpnt60.pth", "training_report.json", "point_cloud/iteration_60/point_cloud.ply"):
        assert os.path.exists(os.path.join(out, name)), name
    loaded = model_io.load_ply(os.path.join(out, "point_cloud/iteration_60/point_cloud.ply"), max_sh_degree=1, device=DEV)
    rows_after = loaded.xyz.shape[0]
    assert rows_after == g.get_xyz.shape[0] and rows_after != rows_before
    assert torch.equal(loaded.xyz, g.get_xyz.detach()) and torch.equal(loaded.filter_3D, g.filter_3D)
    report = json.load(open(os.path.join(out, "training_report.json")))
    assert [r["iteration"] for r in report] == [30, 60] and report == res["report"]
    assert all(r["train"]["views"] == 5 and math.isfinite(r["train"]["psnr"]) and "test" not in r for r in report)
    params, it = torch.load(os.path.join(out, "chkpnt60.pth"), weights_only=False)
    assert it == 60 and len(params) == 14 and torch.equal(params[1], g._xyz)
    import train_args
    cfg = train_args.read_cfg_args(open(os.path.join(out, "cfg_args")).read())
    assert cfg.sh_degree == 1 and cfg.source_path == os.path.abspath(data) and cfg.kernel_size == 0.1
    after = mean_train_l1(g, cams)
    with capsys.disabled():
        print(f"\ntrainer: rows {rows_before} -> {rows_after}; mean training L1 {before:.5f} -> {after:.5f}; loss {res['losses'][0]:.4f} -> {res['losses'][-1]:.4f}")
    assert after < before
    for a in td.PARAMS:
        assert bool(torch.isfinite(getattr(g, a)).all()), a
    assert g.active_sh_degree == 0 and g.optimizer is not None


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
ITERS, REG_FROM, LAMBDA_DSSIM, LAMBDA_NORMAL, KERNEL = 30, 10, 0.2, 0.05, 0.1


def arbiter(data, out, iterations):
    """train.py's iteration on the ops the project had before the trainer: scene_io.Scene on a bare object, compute_3D_filter,
    scaling_n_opacity_with_3D_filter + torch.cat + F.normalize, the rasterizer, photometric_loss, normal_consistency_loss, fused Adam.
    Same data, same order, no densification (the default schedule starts it at 500)."""
    import fused_adam
    import gaussian_model_ops as gmo
    import graphics_utils as gu
    import loss_utils as lu
    import scene_io
    m = types.SimpleNamespace(max_sh_degree=1, active_sh_degree=0)
    scene = scene_io.Scene(dataset_args(data, out), m)
    cams = scene.getTrainCameras()
    m.filter_3D = gmo.compute_3D_filter(m._xyz, cams)
    extent = scene.cameras_extent
    lrs = (("_xyz", 0.00016 * extent), ("_features_dc", 0.0025), ("_features_rest", 0.0025 / 20.0), ("_opacity", 0.05), ("_scaling", 0.005), ("_rotation", 0.001))
    opt = fused_adam.Adam([{"params": [getattr(m, a)], "lr": lr, "name": a} for a, lr in lrs], lr=0.0, eps=1e-15)
    bg = torch.tensor([0, 0, 0], dtype=torch.float32, device=DEV)
    lr_init, lr_final = 0.00016 * extent, 0.0000016 * extent
    for it in range(1, iterations + 1):
        t = np.clip(it / 30_000, 0, 1)
        opt.param_groups[0]["lr"] = 1.0 * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)
        cam = cams[td.view_sampler(it, len(cams))]
        reg = it >= REG_FROM
        res = eager_render(m, cam, bg, KERNEL, reg)
        image, depth, mdepth, normal = res[0], res[4], res[5], res[7]
        rgb = lu.photometric_loss(image, cam.original_image.cuda(), LAMBDA_DSSIM)
        if reg:
            loss = rgb + gu.normal_consistency_loss(cam, normal, depth, mdepth, 0.6) * LAMBDA_NORMAL
        else:
            loss = rgb + torch.tensor([0], dtype=torch.float32, device=DEV) * 0
        loss.backward()
        if it < iterations:
            opt.step()
            opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    return m, cams


def run_trainer(data, out, fused, monkeypatch):
    import gaussian_model
    import trainer
    monkeypatch.setattr(gaussian_model, "FUSED_ACTIVATIONS", fused)
    res = trainer.main(["-s", data, "-m", out, "--iterations", str(ITERS), "--sh_degree", "1", "--kernel_size", str(KERNEL), "--regularization_from_iter",
                        str(REG_FROM), "--test_iterations", "-1", "--save_iterations", "-1", "--checkpoint_iterations", "-1"], view_sampler=td.view_sampler)
    torch.cuda.synchronize()
    return res["gaussians"]


def test_trainer_equals_the_arbiter_loop_and_the_fused_run_stays_in_its_noise(data, tmp_path, monkeypatch, capsys):
    import diff_gaussian_rasterization._C as C
    monkeypatch.setenv("RADEGS_STREAMS", "0")
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    C.reload_env()
    ref, cams = arbiter(data, str(tmp_path / "arbiter"), ITERS)
    eager = run_trainer(data, str(tmp_path / "eager"), False, monkeypatch)
    assert eager.get_xyz.shape[0] == td.POINTS
    for a in td.PARAMS:
        got, want = getattr(eager, a).detach(), getattr(ref, a).detach()
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), a
        if a != "_features_rest":                            # (the active SH degree is 0 for the first 1000 iterations: zero gradient, no step)
            assert not torch.equal(want, getattr(arbiter_start(data, tmp_path), a).detach()), a   # and they did move
    assert torch.equal(eager.filter_3D, ref.filter_3D)
    fused = run_trainer(data, str(tmp_path / "fused"), True, monkeypatch)
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "0")
    C.reload_env()
    atomic, _ = arbiter(data, str(tmp_path / "arbiter_atomic"), ITERS)
    l1_ref, l1_atomic, l1_fused = mean_train_l1(ref, cams), mean_train_l1(atomic, cams), mean_train_l1(fused, cams)
    band = 4.0 * abs(l1_ref - l1_atomic)
    with capsys.disabled():
        print(f"\nmean training L1 after {ITERS} iterations: arbiter {l1_ref:.9f} (atomic backward {l1_atomic:.9f}), trainer with fused activations "
              f"{l1_fused:.9f}; |fused - arbiter| = {abs(l1_fused - l1_ref):.3e}, band = 4 x {abs(l1_ref - l1_atomic):.3e} = {band:.3e}")
    assert abs(l1_fused - l1_ref) <= band


_START = {}


def arbiter_start(data, tmp_path):
    if "m" not in _START:
        import scene_io
        m = types.SimpleNamespace(max_sh_degree=1, active_sh_degree=0)
        scene_io.Scene(dataset_args(data, str(tmp_path / "start")), m)
        _START["m"] = m
    return _START["m"]


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
def test_resumed_run_equals_the_straight_run(data, tmp_path):
    worker = os.path.join(ROOT, "tests", "trainer_dataset.py")
    env = dict(os.environ, RADEGS_DETERMINISTIC="1", RADEGS_STREAMS="0")
    straight, first, second = str(tmp_path / "straight"), str(tmp_path / "first"), str(tmp_path / "second")
    runs = (("straight", [data, straight, "40"]),
            ("first half", [data, first, "21", "--checkpoint_iterations", "20"]),
            ("second half", [data, second, "40", "--start_checkpoint", os.path.join(first, "chkpnt20.pth")]))
    seen = {}
    for name, argv in runs:                                  # one after the other; a failure ends the sequence
        r = subprocess.run([sys.executable, worker] + argv, env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"
        lines = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l.startswith(("DIGEST ", "ROWS "))}
        assert set(lines) == {"DIGEST", "ROWS"}, r.stdout[-2000:]
        seen[name] = (lines["DIGEST"][0], int(lines["ROWS"][0]), int(lines["ROWS"][2]))
    assert seen["straight"][2] == 40 and seen["first half"][2] == 21 and seen["second half"][2] == 40
    assert seen["straight"][1] != td.POINTS                  # the densification did happen, in the first half
    assert seen["second half"][1] == seen["straight"][1]
    assert seen["second half"][0] == seen["straight"][0], seen
    assert seen["first half"][0] != seen["straight"][0]
