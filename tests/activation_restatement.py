"""NumPy float32 restatement of the model activations (csrc/radegs_activate.hip, csrc/rg_activate.h; include/radegs.h, "Model activations"),
forward and backward, one rounding per operation in the order the header states.  The rotation chain uses IEEE products, sums, square
roots and quotients only, which NumPy and the device round alike: the kernel is held to it bit for bit.  Scales and opacity go through
exp, which differs by an ulp between libraries: the kernel's bits for those are held to radegs_filter3d's, and this file to the band."""
import numpy as np

F = np.float32
EPS = F(1e-12)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def quat_norm(x):
    """sqrtf(((x0^2 + x1^2) + x2^2) + x3^2)"""
    x = _f(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        n2 = ((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]) + x[:, 3] * x[:, 3]
        return np.sqrt(n2)


def normalize_forward(x):
    x = _f(x)
    d = np.fmax(quat_norm(x), EPS)                     # fmaxf: a NaN norm gives the eps
    with np.errstate(all="ignore"):
        return x / d[:, None]


def normalize_backward(x, g):
    """n >= 1e-12f: (g - y ((g0 y0 + g1 y1) + g2 y2) + g3 y3) / n with y = x / n; otherwise (NaN norms included) g / 1e-12f"""
    x, g = _f(x), _f(g)
    n = quat_norm(x)
    with np.errstate(all="ignore"):
        live = n >= EPS
        nn = np.where(live, n, F(1.0))[:, None]
        y = x / nn
        s = ((g[:, 0] * y[:, 0] + g[:, 1] * y[:, 1]) + g[:, 2] * y[:, 2]) + g[:, 3] * y[:, 3]
        out = (g - y * s[:, None]) / nn
        return np.where(live[:, None], out, g / EPS).astype(np.float32)


def rotation_branch(x):
    """per row: True where the backward takes the live branch (n >= 1e-12f)"""
    return quat_norm(x) >= EPS


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return F(1.0) / (F(1.0) + np.exp(-_f(x)))


def scale_opacity_forward(scaling_raw, opacity_raw, filter_3D):
    sc, f = _f(scaling_raw), _f(filter_3D)[:, 0]
    with np.errstate(all="ignore"):
        f2 = f * f
        s = np.exp(sc)
        s2 = s * s
        a2 = s2 + f2[:, None]
        det1 = ((F(1.0) * s2[:, 0]) * s2[:, 1]) * s2[:, 2]
        det2 = ((F(1.0) * a2[:, 0]) * a2[:, 1]) * a2[:, 2]
        opacity = _sigmoid(opacity_raw)[:, 0] * np.sqrt(det1 / det2)
        return np.sqrt(a2), opacity[:, None]


def scale_opacity_backward(scaling_raw, opacity_raw, filter_3D, g_scales, g_opacity):
    """g_scales / g_opacity None = zero cotangent"""
    sc, f = _f(scaling_raw), _f(filter_3D)[:, 0]
    P = sc.shape[0]
    gs = np.zeros((P, 3), np.float32) if g_scales is None else _f(g_scales)
    go = np.zeros(P, np.float32) if g_opacity is None else _f(g_opacity)[:, 0]
    with np.errstate(all="ignore"):
        f2 = f * f
        s = np.exp(sc)
        s2 = s * s
        a2 = s2 + f2[:, None]
        det1 = ((F(1.0) * s2[:, 0]) * s2[:, 1]) * s2[:, 2]
        det2 = ((F(1.0) * a2[:, 0]) * a2[:, 1]) * a2[:, 2]
        coef = np.sqrt(det1 / det2)
        sg = _sigmoid(opacity_raw)[:, 0]
        g_op = go * coef * sg * (F(1.0) - sg)
        gc = go * sg * coef
        g_sc = gs * s2 / np.sqrt(a2) + (gc * f2)[:, None] / a2
        return g_sc.astype(np.float32), g_op[:, None].astype(np.float32)


def forward(f_dc, f_rest, rotation_raw, scaling_raw, opacity_raw, filter_3D):
    """(shs, rotations, scales, opacity)"""
    shs = np.concatenate([_f(f_dc), _f(f_rest).reshape(len(f_dc), -1, 3)], axis=1)
    scales, opacity = scale_opacity_forward(scaling_raw, opacity_raw, filter_3D)
    return shs, normalize_forward(rotation_raw), scales, opacity


def backward(rotation_raw, scaling_raw, opacity_raw, filter_3D, g_shs, g_rotations, g_scales, g_opacity, K):
    """(g_f_dc, g_f_rest, g_rotation_raw, g_scaling_raw, g_opacity_raw); a None cotangent is zero"""
    P = len(rotation_raw)
    g_shs = np.zeros((P, K + 1, 3), np.float32) if g_shs is None else _f(g_shs)
    g_rot = np.zeros((P, 4), np.float32) if g_rotations is None else normalize_backward(rotation_raw, g_rotations)
    g_sc, g_op = scale_opacity_backward(scaling_raw, opacity_raw, filter_3D, g_scales, g_opacity)
    return g_shs[:, :1].copy(), g_shs[:, 1:].copy(), g_rot, g_sc, g_op


def degenerate_rotations():
    """the rows no reference speaks for: zero quaternion, norm below 1e-12, norm exactly 1, denormal components, a norm on the threshold's
    two sides, a NaN, an infinite component"""
    den = np.float32(1e-42)
    return np.array([[0, 0, 0, 0], [3e-13, 0, 0, 0], [1e-13, -2e-13, 1e-13, 2e-13], [1, 0, 0, 0], [0, 0.6, 0, 0.8], [den, den, 0, -den],
                     [den, 0, 0, 1], [1e-12, 0, 0, 0], [9.9999e-13, 0, 0, 0], [1.0001e-12, 0, 0, 0], [np.nan, 1, 0, 0], [np.inf, 1, 0, 0],
                     [1e20, 1e20, 0, 0], [-0.0, 0.0, -0.0, 0.0]], dtype=np.float32)
