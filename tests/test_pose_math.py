"""The mathematics of camera pose refinement on the CPU, before anything is built on it.

(a) tests/pose_restatement.py's pose gradient -- the rigid-motion functional of the per-Gaussian gradients plus the SH direction correction --
    against central finite differences of the float64 oracle under a perturbed camera, in tests/test_oracle_fd.py's setup (P = 16, 24 x 24, SH
    degree 3, the four flag modes, a random pose, every output cotangent on, h = 1e-6, that file's criterion).  Both parametrisations: the
    world-frame twist xi (w2c Exp(xi)) and the camera-frame twist tau (Exp(tau) w2c), whose change of frame is checked by differences of the
    LEFT-perturbed pose, not by algebra.  A component whose perturbation changes a discrete decision is skipped; at least 20 of the 24 per
    parametrisation must remain.  Without the SH term the check fails (so the term is exercised).
(b) the retraction: orthonormal to 1e-14 after 1000 random steps; series and Rodrigues branches agree at the switch.
(c) the committed fixtures tests/golden/pose_*.npz still say what tests/golden/make_golden_pose.py computes from them."""
import glob
import math
import os

import numpy as np
import pytest
import torch

import pose_restatement as pr
from synth_scene import make_scene, projection_matrix, upstream_grads
from util import oracle_for

MODES = [(1, False, False, 0.0), (2, False, True, 0.0), (3, True, False, 0.1), (4, True, True, 0.1)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _run(scene, cam, g, grads=False):
    vm, pm, cp = cam
    s = scene._replace(viewmatrix=torch.from_numpy(vm), projmatrix=torch.from_numpy(pm), campos=torch.from_numpy(cp))
    o = oracle_for(s, precision=64, nthreads=1)
    o.forward()
    out = o.outputs()
    L = 0.0
    for k, i in (("color", 0), ("coord", 2), ("mcoord", 3), ("depth", 4), ("mdepth", 5), ("alpha", 6), ("normal", 7)):
        L += float((g[k].numpy().astype(np.float64) * out[i]).sum())
    gr = None
    if grads:
        o.backward(g["color"], g["coord"], g["mcoord"], g["depth"], g["mdepth"], g["alpha"], g["normal"])
        gr = o.grads()
    nc = np.concatenate([o.get("n_contrib").astype(np.int64), o.get("point_list").astype(np.int64), o.get("radii").astype(np.int64),
                         np.array([o.stat_blended()], dtype=np.int64)])
    o.close()
    return L, gr, nc


def _setup(seed, coord, depth, ks):
    s = make_scene(16, 24, 24, sh_degree=3, mu_px=3.0, seed=seed, kernel_size=ks, require_coord=coord, require_depth=depth, pose="random",
                   bg=(0.3, 0.1, 0.7))
    s = s._replace(**{k: getattr(s, k).double() for k in ("means3D", "opacities", "scales", "rotations", "shs")})
    proj_t = projection_matrix(0.01, 100.0, 2 * math.atan(s.tanfovx), 2 * math.atan(s.tanfovy)).T
    vm = s.viewmatrix.double().numpy()
    return s, proj_t, vm, upstream_grads(s, seed)


def _analytic(s, base, gr, sh_term=True):
    P = s.means3D.shape[0]
    return pr.pose_gradient(s.means3D.numpy(), s.rotations.numpy(), s.shs.numpy(), s.sh_degree, base[2], base[0], gr["dL_dmeans3D"].reshape(P, 3),
                            gr["dL_drotations"].reshape(P, 4), gr["dL_dsh"].reshape(P, -1, 3), sh_term=sh_term)


_RESULTS = {}


def _fd_table(mode):
    """{side: [(fd, analytic) or None per component]} and the analytic gradients without the SH term; computed once per mode"""
    if mode not in _RESULTS:
        s, proj_t, vm, g = _setup(*mode)
        base = pr.perturbed_camera(vm, proj_t, np.zeros(6), "right")
        _, gr, nc0 = _run(s, base, g, True)
        ana = dict(zip(("right", "left"), _analytic(s, base, gr)))
        bare = dict(zip(("right", "left"), _analytic(s, base, gr, sh_term=False)))
        h, table = 1e-6, {}
        for side in ("right", "left"):
            rows = []
            for k in range(6):
                e = np.zeros(6)
                e[k] = h
                Lp, _, ncp = _run(s, pr.perturbed_camera(vm, proj_t, e, side), g)
                Lm, _, ncm = _run(s, pr.perturbed_camera(vm, proj_t, -e, side), g)
                same = ncp.shape == nc0.shape and ncm.shape == nc0.shape and np.array_equal(ncp, nc0) and np.array_equal(ncm, nc0)
                rows.append(((Lp - Lm) / (2 * h), ana[side][k]) if same else None)
            table[side] = rows
        _RESULTS[mode] = (table, bare)
    return _RESULTS[mode]


@pytest.mark.parametrize("side", ["right", "left"])
def test_pose_gradient_matches_finite_differences_of_the_perturbed_camera(side, capsys):
    kept = 0
    for mode in MODES:
        table, _ = _fd_table(mode)
        for k, row in enumerate(table[side]):
            if row is None:
                continue                     # the perturbation crossed a thresholded decision: not differentiable there
            fd, ana = row
            with capsys.disabled():
                print(f"\npose fd {side} mode {mode} component {k}: fd {fd:+.9e} analytic {ana:+.9e} diff {abs(fd - ana):.2e}", end="")
            assert abs(fd - ana) <= 2e-3 * (abs(fd) + abs(ana)) + 2e-7, (side, mode, k, fd, ana)
            kept += 1
    assert kept >= 20, kept


def test_the_sh_correction_term_is_needed():
    """degree 3 and a camera that rotates: without -d x c the rotation components miss the differences"""
    missed = 0
    for mode in MODES:
        table, bare = _fd_table(mode)
        for k in (3, 4, 5):
            row = table["right"][k]
            if row is not None and not abs(row[0] - bare["right"][k]) <= 2e-3 * (abs(row[0]) + abs(bare["right"][k])) + 2e-7:
                missed += 1
    assert missed >= 6, missed


def _rotation_defect(M):
    return np.abs(M[:3, :3].T @ M[:3, :3] - np.eye(3)).max()


def test_retraction_stays_orthonormal_over_1000_steps():
    rng = np.random.default_rng(7)
    M = np.eye(4)
    M[:3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    M[:3, 3] = rng.standard_normal(3)
    worst = 0.0
    for _ in range(1000):
        M = pr.retract(np.concatenate([rng.standard_normal(3) * 1e-2, rng.standard_normal(3) * 10.0 ** rng.uniform(-6, -1)]), M)
        worst = max(worst, _rotation_defect(M))
    assert worst <= 1e-14, worst
    assert abs(np.linalg.det(M[:3, :3]) - 1.0) <= 1e-13 and np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0])


def test_retraction_of_a_float32_pose_becomes_orthonormal():
    """a master that starts from a float32 matrix (1e-7 from a rotation) is a rotation to 1e-13 after the first step"""
    rng = np.random.default_rng(8)
    M = np.eye(4)
    M[:3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0].astype(np.float32)
    assert _rotation_defect(M) > 1e-9
    assert _rotation_defect(pr.retract(np.array([0.0, 0.0, 0.0, 1e-4, -2e-4, 3e-4]), M)) <= 1e-13


def test_series_and_rodrigues_branches_agree_at_the_switch():
    rng = np.random.default_rng(9)
    M = np.eye(4)
    M[:3, :3] = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    M[:3, 3] = rng.standard_normal(3)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    for th in (pr.SERIES_BELOW * (1 - 1e-9), pr.SERIES_BELOW, pr.SERIES_BELOW * (1 + 1e-9)):
        tau = np.concatenate([rng.standard_normal(3), axis * th])
        th2 = float(np.dot(tau[3:], tau[3:]))
        series = pr.retract(tau, M, coefficients=(1.0, 0.5, 1.0 / 6.0))
        rodrigues = pr.retract(tau, M, coefficients=(np.sin(np.sqrt(th2)) / np.sqrt(th2), 2.0 * np.sin(0.5 * np.sqrt(th2)) ** 2 / th2,
                                                     (np.sqrt(th2) - np.sin(np.sqrt(th2))) / (th2 * np.sqrt(th2))))
        # the coefficient of K2 differs by O(1) in C only where theta - sin(theta) has lost every bit; K2 rho is 1e-16 there
        assert np.abs(series - rodrigues).max() <= 4 * 2.0 ** -52 * np.abs(series).max(), th
    # and Exp is the matrix exponential: against the power series at an ordinary angle
    tau = np.array([0.3, -0.2, 0.5, 0.4, -0.7, 0.2])
    X = np.zeros((4, 4))
    X[:3, :3] = [[0, -tau[5], tau[4]], [tau[5], 0, -tau[3]], [-tau[4], tau[3], 0]]
    X[:3, 3] = tau[:3]
    S, term = np.eye(4), np.eye(4)
    for n in range(1, 30):
        term = term @ X / n
        S = S + term
    assert np.abs(pr.se3_exp(tau) - S).max() <= 1e-14


def test_camera_tensors_are_the_cameras_own():
    """view, view @ proj and the centre as scene/cameras.py forms them, to float32 rounding"""
    s = make_scene(4, 24, 24, seed=3, pose="random")
    proj_t = np.float32(projection_matrix(0.01, 100.0, 2 * math.atan(s.tanfovx), 2 * math.atan(s.tanfovy)).T)
    view, full, center = pr.camera_tensors(s.viewmatrix.double().numpy().T, proj_t)
    assert np.array_equal(view, s.viewmatrix.numpy())
    assert np.allclose(full, s.projmatrix.numpy(), rtol=1e-6, atol=1e-7) and np.allclose(center, s.campos.numpy(), rtol=1e-6, atol=1e-6)


def test_golden_pose_fixtures_say_what_their_maker_computes():
    files = sorted(glob.glob(os.path.join(GOLDEN, "pose_*.npz")))
    assert len(files) == 4, files
    bands = set()
    for f in files:
        z = np.load(f)
        for tag in ("64", "32"):
            gxi, gtau = pr.pose_gradient(z["means3D"], z["rotations"], z["shs"], int(z["sh_degree"]), z["campos"], z["viewmatrix"],
                                         z["dL_dmeans3D_" + tag], z["dL_drotations_" + tag], z["dL_dsh_" + tag])
            assert np.array_equal(gxi, z["g_xi_" + tag]) and np.array_equal(gtau, z["g_tau_" + tag]), (f, tag)
        dev = z["g_tau_32"] - z["g_tau_64"]
        assert np.all(np.array([np.linalg.norm(dev[:3]), np.linalg.norm(dev[3:])]) * 4 <= z["band_tau"]), f
        bands.add(tuple(z["band_tau"].tolist()))
    assert len(bands) == 1      # one band, the maximum over the four
