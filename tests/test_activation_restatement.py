"""tests/activation_restatement.py against the reference's own values (tests/golden/activations_sh*.npz, written by
make_golden_trainer.py from the reference's GaussianModel properties and torch autograd): `shs` exact, everything else inside the
project's 1e-5 abs + 1e-4 rel.  The restatement's rotation chain sums its squares as ((x0^2 + x1^2) + x2^2) + x3^2 and torch's norm in
another order: under 1e-6 relative forward; the fixture keeps norms in [0.5, 2] and cotangents O(1), where the backward's cancellation
does not amplify that.  Degenerate rows carry no reference claim: stated branch and finite values only."""
import os

import numpy as np
import pytest

import activation_restatement as ar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def close(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= 1e-5 + 1e-4 * np.abs(b.astype(np.float64))


@pytest.fixture(scope="module", params=[0, 1, 2, 3])
def golden(request):
    return dict(np.load(os.path.join(GOLDEN, f"activations_sh{request.param}.npz")))


def test_fixture_is_what_the_tests_assume(golden):
    g = golden
    P, K = g["features_dc"].shape[0], g["features_rest"].shape[1]
    assert P == 257 and K == (int(g["sh_degree"]) + 1) ** 2 - 1
    n = np.linalg.norm(g["rotation"].astype(np.float64), axis=1)
    assert n.min() >= 0.5 - 1e-6 and n.max() <= 2.0 + 1e-6
    assert (g["filter_3D"] == 0).any() and (g["filter_3D"] > 0).any()
    for k in ("g_shs", "g_rotations", "g_scales", "g_opacity"):
        assert 0.5 < np.abs(g[k]).mean() < 2.0


def test_forward_against_the_reference(golden):
    g = golden
    shs, rot, scales, opacity = ar.forward(g["features_dc"], g["features_rest"], g["rotation"], g["scaling"], g["opacity"], g["filter_3D"])
    assert shs.dtype == np.float32 and np.array_equal(shs.view(np.uint32), g["out_shs"].view(np.uint32))
    assert close(rot, g["out_rotations"]).all()
    rel = np.abs(rot.astype(np.float64) - g["out_rotations"]) / np.maximum(np.abs(g["out_rotations"].astype(np.float64)), 1e-3)
    assert rel.max() < 1e-6, rel.max()
    assert close(scales, g["out_scales"]).all()
    assert close(opacity, g["out_opacity"]).all()


def test_backward_against_the_reference(golden):
    g = golden
    K = g["features_rest"].shape[1]
    g_dc, g_rest, g_rot, g_sc, g_op = ar.backward(g["rotation"], g["scaling"], g["opacity"], g["filter_3D"], g["g_shs"], g["g_rotations"], g["g_scales"],
                                                  g["g_opacity"], K)
    assert np.array_equal(g_dc, g["grad_features_dc"]) and np.array_equal(g_rest, g["grad_features_rest"])
    assert close(g_rot, g["grad_rotation"]).all(), np.abs(g_rot - g["grad_rotation"]).max()
    assert close(g_sc, g["grad_scaling"]).all(), np.abs(g_sc - g["grad_scaling"]).max()
    assert close(g_op, g["grad_opacity"]).all(), np.abs(g_op - g["grad_opacity"]).max()


def test_absent_cotangents_are_zero(golden):
    g = golden
    K = g["features_rest"].shape[1]
    full = ar.backward(g["rotation"], g["scaling"], g["opacity"], g["filter_3D"], g["g_shs"], g["g_rotations"], g["g_scales"], g["g_opacity"], K)
    none = ar.backward(g["rotation"], g["scaling"], g["opacity"], g["filter_3D"], None, None, None, None, K)
    assert all((a == 0).all() and a.shape == b.shape for a, b in zip(none, full))
    only_op = ar.backward(g["rotation"], g["scaling"], g["opacity"], g["filter_3D"], None, None, None, g["g_opacity"], K)
    assert np.array_equal(only_op[4], full[4]) and (only_op[2] == 0).all() and (only_op[3] != 0).any()


def test_degenerate_rotations_take_the_stated_branch():
    x = ar.degenerate_rotations()
    live = ar.rotation_branch(x)
    #        zero   3e-13  ~3e-13  unit  unit  denormal  den+1  1e-12  below  above  NaN    inf   1e20  signed zeros
    want = [False, False, False, True, True, False, True, True, False, True, False, True, True, False]
    assert live.tolist() == want
    y = ar.normalize_forward(x)
    g = np.tile(np.array([[0.5, -1.0, 2.0, 0.25]], dtype=np.float32), (len(x), 1))
    gx = ar.normalize_backward(x, g)
    finite_rows = np.isfinite(x).all(axis=1)
    assert np.isfinite(y[finite_rows]).all() and np.isfinite(gx[finite_rows]).all()
    dead = ~live & finite_rows
    assert np.array_equal(gx[dead], g[dead] / np.float32(1e-12))          # the clamp is active: d is a constant
    assert np.array_equal(y[dead], x[dead] / np.float32(1e-12))
    assert np.array_equal(y[3], x[3]) and np.array_equal(y[4], x[4])        # norm exactly 1: the row itself
    assert np.array_equal(gx[3], np.array([0.0, -1.0, 2.0, 0.25], dtype=np.float32))   # g - y (g.y): the radial part goes
    # filter_3D = 0: scales = exp(raw) up to the rounding of sqrt(s^2), the opacity factor exactly 1
    sc = np.array([[-3.0, 0.5, 1.25]], dtype=np.float32)
    scales, op = ar.scale_opacity_forward(sc, np.array([[0.3]], np.float32), np.zeros((1, 1), np.float32))
    assert np.allclose(scales, np.exp(sc), rtol=3e-7, atol=0) and op[0, 0] == np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-0.3)))
