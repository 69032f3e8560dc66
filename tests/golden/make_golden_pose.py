"""Writes tests/golden/pose_*.npz, the fixtures of the pose-gradient tests, from this project's oracle alone.

    python tests/golden/make_golden_pose.py

Four scenes of P = 300 at 64 x 48, SH degree 3, a random pose, one per require_coord / require_depth mode (kernel_size 0.1 in two), with the
INTENDED derivative (oracle.set_opacity_slip(0)), as the gradient tests of the suite run.  Each file holds the float32 inputs and the output
cotangents, the per-Gaussian gradients of the float64 and of the float32 oracle on those inputs, g_xi and g_tau that tests/pose_restatement.py
forms from either, and `band_tau`: for the translation and the rotation triple of g_tau, the Euclidean deviation of the float32 oracle's pose
gradient from the float64 one, maximum over the four scenes, times 4 -- the reference's own float32 arithmetic is the noise a float32
implementation is allowed."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "rade-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SCENES = [("plain", 21, False, False, 0.0), ("depth", 22, False, True, 0.0), ("coord", 23, True, False, 0.1), ("both", 24, True, True, 0.1)]
P, W, H = 300, 64, 48


def main():
    import pose_restatement as pr
    from oracle import oracle as orc
    from synth_scene import make_scene, projection_matrix, upstream_grads
    from util import oracle_for
    orc.build()
    orc.set_opacity_slip(0)
    records = []
    for name, seed, coord, depth, ks in SCENES:
        s = make_scene(P, W, H, sh_degree=3, mu_px=3.0, seed=seed, kernel_size=ks, require_coord=coord, require_depth=depth, pose="random",
                       bg=(0.3, 0.1, 0.7))
        g = upstream_grads(s, seed)
        rec = {k: getattr(s, k).numpy() for k in ("means3D", "opacities", "scales", "rotations", "shs", "viewmatrix", "projmatrix", "campos", "bg")}
        rec["proj"] = np.float32(projection_matrix(0.01, 100.0, 2 * math.atan(s.tanfovx), 2 * math.atan(s.tanfovy)).T)
        rec.update(tanfovx=np.float64(s.tanfovx), tanfovy=np.float64(s.tanfovy), W=np.int32(W), H=np.int32(H), sh_degree=np.int32(3),
                   kernel_size=np.float64(ks), require_coord=np.bool_(coord), require_depth=np.bool_(depth))
        rec.update({"cot_" + k: v.numpy() for k, v in g.items()})
        for tag, precision in (("64", 64), ("32", 32)):
            o = oracle_for(s, precision=precision, nthreads=1)
            o.forward()
            o.backward(g["color"], g["coord"], g["mcoord"], g["depth"], g["mdepth"], g["alpha"], g["normal"])
            gr = o.grads()
            o.close()
            gm, gq, gs = gr["dL_dmeans3D"].reshape(P, 3), gr["dL_drotations"].reshape(P, 4), gr["dL_dsh"].reshape(P, 16, 3)
            gxi, gtau = pr.pose_gradient(rec["means3D"], rec["rotations"], rec["shs"], 3, rec["campos"], rec["viewmatrix"], gm, gq, gs)
            rec.update({"dL_dmeans3D_" + tag: gm, "dL_drotations_" + tag: gq, "dL_dsh_" + tag: gs, "g_xi_" + tag: gxi, "g_tau_" + tag: gtau})
        records.append((name, rec))
    dev = np.array([[np.linalg.norm((r["g_tau_32"] - r["g_tau_64"])[:3]), np.linalg.norm((r["g_tau_32"] - r["g_tau_64"])[3:])] for _, r in records])
    band = 4.0 * dev.max(0)
    for (name, rec), d in zip(records, dev):
        rec["band_tau"] = band
        np.savez_compressed(os.path.join(HERE, f"pose_{name}.npz"), **rec)
        n = rec["g_tau_64"]
        print(f"pose_{name}.npz: |g_tau| translation {np.linalg.norm(n[:3]):.4e} rotation {np.linalg.norm(n[3:]):.4e}; float32 oracle off by "
              f"{d[0]:.3e} / {d[1]:.3e}; band {band[0]:.3e} / {band[1]:.3e}")


if __name__ == "__main__":
    main()
