"""Generates the evalio_* fixtures of tests/golden.  Build container only (needs the reference's sources).

The small input files are written first (a .log of a dozen poses, a mapping file, a _trans.txt, a .npy stack of 3x4 poses, three
pos_XXX.txt projection matrices); evalio_reference.npz then records what the reference's own NumPy code returns for them -- RUN, not copied:
  * eval_tnt/trajectory_io.read_trajectory, eval_tnt/registration.read_mapping and gen_sparse_trajectory, imported with `open3d` stubbed as
    an empty module;
  * read_trajectory / get_traj of eval_tnt/cull_mesh.py (.log and .npy branches) and best_fit_transform with the scale lines of
    evaluate_dtu_mesh.py: both modules import packages that are not installed (trimesh, pyrender, cv2), so the functions are compiled from
    their file lines and executed.
cv2.decomposeProjectionMatrix cannot be run here: the projection matrices are built from known camera centres, and those are recorded."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_mesheval import save  # noqa: E402


def rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 2] *= -1
    return q


def lines_of(path, first, last):
    """the source lines first..last (1-based, inclusive) of a reference file, dedented as they stand"""
    with open(path) as f:
        return "".join(f.read().splitlines(keepends=True)[first - 1:last])


def write_inputs(seed):
    rng = np.random.default_rng(seed)
    poses = np.tile(np.eye(4), (12, 1, 1))
    for k in range(12):
        poses[k, :3, :3] = rotation(rng)
        poses[k, :3, 3] = rng.uniform(-4, 4, 3)
    with open(os.path.join(HERE, "evalio_traj.log"), "w") as f:          # write_trajectory's layout; tabs and runs of blanks among the separators
        for k, p in enumerate(poses):
            f.write(f"{k} {k} {k + 1}\n")
            for r, row in enumerate(p):
                sep = "\t" if (k + r) % 3 == 0 else "  " if (k + r) % 3 == 1 else " "
                f.write(sep.join("{0:.12f}".format(v) for v in row) + "\n")
    with open(os.path.join(HERE, "evalio_mapping.txt"), "w") as f:
        f.write("5\n12\n")
        for a, b in enumerate([1, 4, 7, 9, 12]):
            f.write(f"{a} {b}\n")
    trans = np.eye(4)
    trans[:3, :3], trans[:3, 3] = 1.3 * rotation(rng), rng.uniform(-1, 1, 3)
    np.savetxt(os.path.join(HERE, "evalio_trans.txt"), trans)
    np.save(os.path.join(HERE, "evalio_traj34.npy"), poses[:5, :3, :] + 0.1)      # float64 3x4 poses: rounded to float32 and padded
    os.makedirs(os.path.join(HERE, "evalio_dtu"), exist_ok=True)
    centres = rng.uniform(-300, 300, (3, 3)) + np.array([0.0, 0.0, -600.0])
    K = np.array([[2892.33, 0.0, 823.205], [0.0, 2883.18, 619.071], [0.0, 0.0, 1.0]])
    for i, c in enumerate(centres):
        R = rotation(rng)
        P = K @ np.concatenate([R, -(R @ c)[:, None]], 1)
        np.savetxt(os.path.join(HERE, "evalio_dtu", f"pos_{i + 1:03d}.txt"), P, fmt="%.6f")
    return centres


def reference_outputs():
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))
    sys.path.insert(0, os.path.join(REF, "eval_tnt"))
    import registration
    import trajectory_io
    log, mapping_file = os.path.join(HERE, "evalio_traj.log"), os.path.join(HERE, "evalio_mapping.txt")
    traj = trajectory_io.read_trajectory(log)
    poses = np.array([p.pose for p in traj])
    meta = np.array([list(p.metadata) for p in traj], np.int64)
    n_sampled, n_total, mapping = registration.read_mapping(mapping_file)
    sparse = np.array([p.pose for p in registration.gen_sparse_trajectory(mapping, traj)])

    ns = dict(np=np, torch=torch, print=lambda *a, **k: None)
    src = lines_of(os.path.join(REF, "eval_tnt", "cull_mesh.py"), 321, 382)
    assert src.startswith("def read_trajectory(filename):") and "def get_traj(traj_path):" in src and src.rstrip().endswith("return traj_to_register")
    exec(src, ns)
    get_log = np.stack([t.numpy() for t in ns["get_traj"](log)])
    get_npy = np.stack([t.numpy() for t in ns["get_traj"](os.path.join(HERE, "evalio_traj34.npy"))])
    assert get_log.dtype == np.float32 and get_npy.shape == (5, 4, 4)

    dtu = os.path.join(REF, "evaluate_dtu_mesh.py")
    fit = lines_of(dtu, 16, 57)
    assert fit.startswith("def best_fit_transform(A, B):") and fit.rstrip().endswith("return T, R, t")
    scale = "".join(line.lstrip() for line in lines_of(dtu, 160, 164).splitlines(keepends=True))
    assert scale.startswith("scale_points = ") and "best_fit_transform(points, gt_points)" in scale
    rng = np.random.default_rng(7)
    gt_points = rng.uniform(-300, 300, (9, 3)).astype(np.float32)
    R0 = rotation(rng)
    points = (((gt_points - gt_points.mean(0)) @ R0.T) / 350.0 + rng.normal(0, 1e-3, (9, 3)) + [0.1, -0.2, 0.3]).astype(np.float32)
    ns2 = dict(np=np, points=points.copy(), gt_points=gt_points.copy())
    exec(fit + "\n" + scale, ns2)
    T_fit = ns2["best_fit_transform"](points.astype(np.float64), gt_points.astype(np.float64))[0]      # and once on float64 inputs
    return dict(log_poses=poses, log_meta=meta, n_sampled=np.asarray(n_sampled), n_total=np.asarray(n_total), mapping=mapping, sparse=sparse,
                get_traj_log=get_log, get_traj_npy=get_npy, fit_points=points, fit_gt_points=gt_points,
                fit_scale_points=np.asarray(ns2["scale_points"]), fit_scale_gt_points=np.asarray(ns2["scale_gt_points"]), fit_r=ns2["r"], fit_t=ns2["t"],
                fit_T64=T_fit)


if __name__ == "__main__":
    centres = write_inputs(seed=18)
    save("evalio_reference.npz", dtu_centres=centres, **reference_outputs())
