"""trainer.py with --optimize_poses on the GPU, on the dataset of the trainer's own tests (tests/trainer_dataset.py).

(a) Resume: three fresh processes (tests/pose_trainer_worker.py), one after the other, each under its own time limit, with the deterministic
    backward.  40 iterations straight; 21 iterations with a checkpoint at 20; 20 more from that checkpoint (as tests/test_gpu_trainer.py (c):
    upstream takes no step in its last iteration, so the first half runs one iteration further than its checkpoint).  The losses, the poses
    (masters, pose Adam state, step counts, the cameras' tensors, host-side R / T) and the Gaussians (parameters and both Adam moments) of
    the resumed run equal the straight run's bit for bit; the poses did move; kernel_size 0.1 made the run announce the intended derivative.
(b) Off by default: without the flag training() returns no poses, writes upstream's two-entry checkpoint and no cameras_refined.json, and a
    run with the flag on whose --pose_from_iter lies beyond the end -- the tap is never inserted -- has the same losses and parameters bit for
    bit (kernel_size 0, where the flag does not change the derivative)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import trainer_dataset as td

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return td.write(str(tmp_path_factory.mktemp("pose_trainer") / "data"), DEV)


def test_resumed_pose_run_equals_the_straight_run(data, tmp_path):
    worker = os.path.join(ROOT, "tests", "pose_trainer_worker.py")
    env = dict(os.environ, RADEGS_DETERMINISTIC="1", RADEGS_STREAMS="0")
    straight, first, second = str(tmp_path / "straight"), str(tmp_path / "first"), str(tmp_path / "second")
    runs = (("straight", [data, straight, "40"]),
            ("first half", [data, first, "21", "--checkpoint_iterations", "20"]),
            ("second half", [data, second, "40", "--start_checkpoint", os.path.join(first, "chkpnt20.pth")]))
    seen = {}
    for name, argv in runs:                                  # one after the other; a failure ends the sequence
        r = subprocess.run([sys.executable, worker] + argv, env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"
        assert "switching the backward to opacity_grad_intended" in r.stdout, name
        lines = {l.split()[0]: l.split(None, 2)[1:] for l in r.stdout.splitlines() if l.startswith(("DIGEST ", "ROWS ", "POSES ", "LOSSES "))}
        assert set(lines) == {"DIGEST", "ROWS", "POSES", "LOSSES"}, r.stdout[-2000:]
        seen[name] = {"digest": lines["DIGEST"][0], "rows": int(lines["ROWS"][0]), "poses": lines["POSES"][0], "steps": [int(s) for s in lines["POSES"][1].split()],
                      "losses": json.loads(lines["LOSSES"][1])}
    s, f, h = seen["straight"], seen["first half"], seen["second half"]
    assert len(s["losses"]) == 40 and len(f["losses"]) == 21 and len(h["losses"]) == 20
    assert f["losses"][:20] == s["losses"][:20] and h["losses"] == s["losses"][20:]
    assert sum(s["steps"]) == 39 - 2 and min(s["steps"]) >= 5     # iterations 3 .. 39 stepped a pose; every camera was visited
    assert h["steps"] == s["steps"] and h["poses"] == s["poses"] and f["poses"] != s["poses"]
    assert h["rows"] == s["rows"] and h["digest"] == s["digest"] and f["digest"] != s["digest"]
    refined = json.load(open(os.path.join(straight, "cameras_refined.json")))
    original = json.load(open(os.path.join(straight, "cameras.json")))
    assert len(refined) == len(original) == td.VIEWS
    by_name = {o["img_name"]: o for o in original}              # (the training cameras are shuffled, cameras.json is not)
    moved = [max(abs(a - b) for a, b in zip(r["position"], by_name[r["img_name"]]["position"])) for r in refined]
    assert all(0 < m < 0.05 for m in moved), moved            # a few steps of 1e-4: moved, and not far


def run(data, out, extra):
    import trainer
    res = trainer.main(["-s", data, "-m", out, "--iterations", "12", "--sh_degree", "1", "--kernel_size", "0.0", "--disable_filter3D", "--regularization_from_iter",
                        "6", "--test_iterations", "-1", "--save_iterations", "-1", "--checkpoint_iterations", "10"] + extra, view_sampler=td.view_sampler)
    torch.cuda.synchronize()
    return res


def test_pose_refinement_is_off_by_default(data, tmp_path, monkeypatch):
    import diff_gaussian_rasterization._C as C
    monkeypatch.setenv("RADEGS_STREAMS", "0")
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    C.reload_env()
    plain = run(data, str(tmp_path / "plain"), [])
    assert plain["poses"] is None and not os.path.exists(str(tmp_path / "plain" / "cameras_refined.json"))
    assert len(torch.load(str(tmp_path / "plain" / "chkpnt10.pth"), weights_only=False)) == 2
    idle = run(data, str(tmp_path / "idle"), ["--optimize_poses", "--pose_from_iter", "1000"])
    assert idle["poses"] is not None and idle["poses"].steps == [0] * td.VIEWS and os.path.exists(str(tmp_path / "idle" / "cameras_refined.json"))
    assert len(torch.load(str(tmp_path / "idle" / "chkpnt10.pth"), weights_only=False)) == 3
    assert plain["losses"] == idle["losses"] and len(plain["losses"]) == 12
    for a in td.PARAMS:
        assert torch.equal(getattr(plain["gaussians"], a).detach().view(torch.int32), getattr(idle["gaussians"], a).detach().view(torch.int32)), a
