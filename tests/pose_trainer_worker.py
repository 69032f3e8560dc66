"""Worker of tests/test_gpu_pose_trainer.py: one trainer run with --optimize_poses in a process of its own.

    python tests/pose_trainer_worker.py DATA OUT ITERATIONS [trainer flags ...]

tests/trainer_dataset.py's run (its fixed view order and compressed schedule) plus the pose flags; prints `ROWS n ITERATION k`, `DIGEST` over
the six parameters and both Adam moments as that file forms it, `POSES` = sha256 over the float64 masters, the pose Adam state, the step
counts and every camera's three tensors, and `LOSSES` = sha256 over the losses' float64 bytes with the list itself as JSON."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "rade-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pose_digest(poses):
    import torch
    torch.cuda.synchronize()
    h = hashlib.sha256()
    state = poses.state_dict()
    for k in ("master", "exp_avg", "exp_avg_sq", "world_view_transform", "full_proj_transform", "camera_center"):
        h.update(state[k].contiguous().cpu().numpy().tobytes())
    h.update(np.asarray(state["steps"], np.int64).tobytes())
    for cam in poses.cameras:
        h.update(np.asarray(cam.R, np.float64).tobytes() + np.asarray(cam.T, np.float64).tobytes())
    return h.hexdigest()


def main(argv):
    import trainer
    import trainer_dataset as td
    data, out, iterations = argv[0], argv[1], argv[2]
    args = ["-s", data, "-m", out, "--iterations", iterations, "--sh_degree", "1", "--kernel_size", "0.1", "--disable_filter3D", "--regularization_from_iter",
            "8", "--test_iterations", "-1", "--save_iterations", "-1", "--optimize_poses", "--pose_lr_translation", "1e-4", "--pose_lr_rotation", "1e-4",
            "--pose_from_iter", "3"] + td.SCHEDULE + list(argv[3:])
    if "--checkpoint_iterations" not in args:
        args += ["--checkpoint_iterations", "-1"]
    res = trainer.main(args, view_sampler=td.view_sampler)
    print("ROWS", res["gaussians"].get_xyz.shape[0], "ITERATION", res["iteration"], flush=True)
    print("DIGEST", td.digest(res["gaussians"]), flush=True)
    print("POSES", pose_digest(res["poses"]), " ".join(str(s) for s in res["poses"].steps), flush=True)
    print("LOSSES", hashlib.sha256(np.asarray(res["losses"], np.float64).tobytes()).hexdigest(), json.dumps(res["losses"]), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
