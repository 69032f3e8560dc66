"""NumPy float64 restatement of csrc/rg_pose.h (camera pose refinement): the per-Gaussian row of the SE(3) pose gradient, its
fixed-order sum, the change to the camera frame, and the pose step.  Every expression is written as the header writes it -- same association,
one rounding per operation -- so that the kernel can be held to it bit for bit (NumPy's element-wise float64 operations round once and never
fuse).  sin is the one exception: the device's and the host's differ in the last bits, which the step test's tolerance allows for."""
import numpy as np

from mesheval_restatement import fixed_order_sum

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)
SERIES_BELOW = 1e-8


def sh_basis_gradient(deg, x, y, z):
    """{k: (d basis_k / dx, dy, dz)} at the unit directions, k = 1 .. (deg + 1)^2 - 1"""
    o = np.zeros_like(x)
    w = {1: (o, o - C1, o), 2: (o, o, o + C1), 3: (o - C1, o, o)}
    if deg < 2:
        return w
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    w[4] = (C2[0] * y, C2[0] * x, o)
    w[5] = (o, C2[1] * z, C2[1] * y)
    w[6] = (C2[2] * (-2.0 * x), C2[2] * (-2.0 * y), C2[2] * (4.0 * z))
    w[7] = (C2[3] * z, o, C2[3] * x)
    w[8] = (C2[4] * (2.0 * x), C2[4] * (-2.0 * y), o)
    if deg < 3:
        return w
    w[9] = (C3[0] * (6.0 * xy), C3[0] * (3.0 * (xx - yy)), o)
    w[10] = (C3[1] * yz, C3[1] * xz, C3[1] * xy)
    w[11] = (C3[2] * (-2.0 * xy), C3[2] * ((4.0 * zz - xx) - 3.0 * yy), C3[2] * (8.0 * yz))
    w[12] = (C3[3] * (-6.0 * xz), C3[3] * (-6.0 * yz), C3[3] * (3.0 * ((2.0 * zz - xx) - yy)))
    w[13] = (C3[4] * ((4.0 * zz - 3.0 * xx) - yy), C3[4] * (-2.0 * xy), C3[4] * (8.0 * xz))
    w[14] = (C3[5] * (2.0 * xz), C3[5] * (-2.0 * yz), C3[5] * (xx - yy))
    w[15] = (C3[6] * (3.0 * (xx - yy)), C3[6] * (-6.0 * xy), o)
    return w


def sh_direction_cotangent(deg, sh, d, dRGB):
    """c = J^T dRGB for the rows given: sh [n, M, 3], d [n, 3] unnormalised, dRGB [n, 3]"""
    d0, d1, d2 = d[:, 0], d[:, 1], d[:, 2]
    n2 = (d0 * d0 + d1 * d1) + d2 * d2
    ln = np.sqrt(n2)
    w = sh_basis_gradient(deg, d0 / ln, d1 / ln, d2 / ln)
    dd = [np.zeros_like(n2) for _ in range(3)]
    for ch in range(3):
        s = [np.zeros_like(n2) for _ in range(3)]
        for k in range(1, (deg + 1) ** 2):
            v = sh[:, k, ch]
            for a in range(3):
                s[a] = s[a] + w[k][a] * v
        for a in range(3):
            dd[a] = dd[a] + s[a] * dRGB[:, ch]
    inv = 1.0 / np.sqrt(n2 * n2 * n2)
    c0 = (((n2 - d0 * d0) * dd[0] - d1 * d0 * dd[1]) - d2 * d0 * dd[2]) * inv
    c1 = ((-d0 * d1 * dd[0] + (n2 - d1 * d1) * dd[1]) - d2 * d1 * dd[2]) * inv
    c2 = ((-d0 * d2 * dd[0] - d1 * d2 * dd[1]) + (n2 - d2 * d2) * dd[2]) * inv
    return np.stack([c0, c1, c2], 1)


def rows(means3D, rotations, shs, sh_degree, campos, dL_dmeans3D, dL_drotations, dL_dsh, sh_term=True):
    """[P, 6]: every Gaussian's contribution to (dL/drho, dL/dtheta).  The inputs are widened to float64 as they are (float32 inputs: exactly).
    sh_term=False leaves out the SH correction (what a caller that forgot it would compute)."""
    f = lambda a: np.asarray(a).astype(np.float64)
    m, q, g, gq, sh, dsh = f(means3D), f(rotations), f(dL_dmeans3D), f(dL_drotations), f(shs), f(dL_dsh)
    cam = f(campos)
    mx, my, mz, gx, gy, gz = m[:, 0], m[:, 1], m[:, 2], g[:, 0], g[:, 1], g[:, 2]
    w, vx, vy, vz, gw, hx, hy, hz = q[:, 0], q[:, 1], q[:, 2], q[:, 3], gq[:, 0], gq[:, 1], gq[:, 2], gq[:, 3]
    ax, ay, az = my * gz - mz * gy, mz * gx - mx * gz, mx * gy - my * gx
    bx = (w * hx - gw * vx) + (vy * hz - vz * hy)
    by = (w * hy - gw * vy) + (vz * hx - vx * hz)
    bz = (w * hz - gw * vz) + (vx * hy - vy * hx)
    tx, ty, tz = ax + 0.5 * bx, ay + 0.5 * by, az + 0.5 * bz
    dsh0 = dsh[:, 0, :]
    live = np.flatnonzero((dsh0 != 0).any(1)) if (sh_degree > 0 and sh_term) else np.zeros(0, np.int64)
    if live.size:
        d = np.stack([mx[live] - cam[0], my[live] - cam[1], mz[live] - cam[2]], 1)
        c = sh_direction_cotangent(sh_degree, sh[live], d, dsh0[live] / C0)
        tx, ty, tz = tx.copy(), ty.copy(), tz.copy()
        tx[live] = tx[live] - (d[:, 1] * c[:, 2] - d[:, 2] * c[:, 1])
        ty[live] = ty[live] - (d[:, 2] * c[:, 0] - d[:, 0] * c[:, 2])
        tz[live] = tz[live] - (d[:, 0] * c[:, 1] - d[:, 1] * c[:, 0])
    return np.stack([gx, gy, gz, tx, ty, tz], 1)


def to_camera_frame(viewmatrix, gxi):
    """g_tau of g_xi: w2c = (R, t) = viewmatrix^T"""
    vm = np.asarray(viewmatrix).astype(np.float64).reshape(4, 4)
    out, r = np.zeros(6), np.zeros(3)
    for i in range(3):
        R0, R1, R2 = vm[0, i], vm[1, i], vm[2, i]
        out[i] = (R0 * gxi[0] + R1 * gxi[1]) + R2 * gxi[2]
        r[i] = (R0 * gxi[3] + R1 * gxi[4]) + R2 * gxi[5]
    t0, t1, t2 = vm[3, 0], vm[3, 1], vm[3, 2]
    out[3] = r[0] + (t1 * out[2] - t2 * out[1])
    out[4] = r[1] + (t2 * out[0] - t0 * out[2])
    out[5] = r[2] + (t0 * out[1] - t1 * out[0])
    return out


def pose_gradient(means3D, rotations, shs, sh_degree, campos, viewmatrix, dL_dmeans3D, dL_drotations, dL_dsh, sh_term=True):
    """(g_xi [6], g_tau [6]) as radegs_pose_gradient leaves them"""
    r = rows(means3D, rotations, shs, sh_degree, campos, dL_dmeans3D, dL_drotations, dL_dsh, sh_term)
    gxi = fixed_order_sum(r, 6) if r.shape[0] else np.zeros(6)
    return gxi, to_camera_frame(viewmatrix, gxi)


def adam_delta(g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-15):
    """radegs_pose_step's Adam on float32 arrays: returns (delta, m, v), all float32"""
    f = np.float32
    g, m, v = np.asarray(g, f), np.asarray(m, f), np.asarray(v, f)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    step_size, bc2_sqrt = (np.asarray(lr, np.float64) / bc1).astype(f), f(np.sqrt(bc2))
    omb1, b2, omb2 = f(1.0 - beta1), f(beta2), f(1.0 - beta2)
    m = m + omb1 * (g - m)
    v = v * b2 + omb2 * (g * g)
    denom = np.sqrt(v) / bc2_sqrt + f(eps)
    return f(0) - step_size * (m / denom), m, v


def exp_coefficients(th2):
    th = np.sqrt(th2)
    if th < SERIES_BELOW:
        return 1.0, 0.5, 1.0 / 6.0
    sn, sh = np.sin(th), np.sin(0.5 * th)
    return sn / th, 2.0 * sh * sh / th2, (th - sn) / (th2 * th)


def retract(tau, master, coefficients=None):
    """Exp(tau) master, then the Newton step towards the nearest rotation: the new [4,4] float64 master"""
    tau = np.asarray(tau, np.float64)
    M = np.asarray(master, np.float64).reshape(4, 4)
    t0, t1, t2 = tau[3], tau[4], tau[5]
    A, B, C = coefficients or exp_coefficients((t0 * t0 + t1 * t1) + t2 * t2)
    K = np.array([0.0, -t2, t1, t2, 0.0, -t0, -t1, t0, 0.0])
    K2 = np.array([-(t1 * t1 + t2 * t2), t0 * t1, t0 * t2, t0 * t1, -(t0 * t0 + t2 * t2), t1 * t2, t0 * t2, t1 * t2, -(t0 * t0 + t1 * t1)])
    I = np.eye(3).reshape(9)
    E, V = ((I + A * K) + B * K2).reshape(3, 3), ((I + B * K) + C * K2).reshape(3, 3)
    R, t = np.zeros((3, 3)), np.zeros(3)
    for i in range(3):
        for j in range(3):
            R[i, j] = (E[i, 0] * M[0, j] + E[i, 1] * M[1, j]) + E[i, 2] * M[2, j]
        et = (E[i, 0] * M[0, 3] + E[i, 1] * M[1, 3]) + E[i, 2] * M[2, 3]
        vr = (V[i, 0] * tau[0] + V[i, 1] * tau[1]) + V[i, 2] * tau[2]
        t[i] = et + vr
    H = np.zeros((3, 3))
    for i in range(3):
        for j in range(i, 3):
            s = (R[0, i] * R[0, j] + R[1, i] * R[1, j]) + R[2, i] * R[2, j]
            H[i, j] = H[j, i] = 0.5 * ((3.0 if i == j else 0.0) - s)
    out = M.copy()
    for i in range(3):
        for j in range(3):
            out[i, j] = (R[i, 0] * H[0, j] + R[i, 1] * H[1, j]) + R[i, 2] * H[2, j]
        out[i, 3] = t[i]
    return out


def camera_tensors(master, proj):
    """(world_view_transform [4,4], full_proj_transform [4,4], camera_center [3]) in float32 from the float64 master and the float32 projection
    matrix (stored transposed)"""
    M = np.asarray(master, np.float64).reshape(4, 4)
    p = np.asarray(proj).astype(np.float64).reshape(4, 4)
    view = M.T
    full = np.zeros((4, 4))
    for r in range(4):
        for c in range(4):
            full[r, c] = (((view[r, 0] * p[0, c]) + view[r, 1] * p[1, c]) + view[r, 2] * p[2, c]) + view[r, 3] * p[3, c]
    center = np.array([0.0 - ((M[0, j] * M[0, 3] + M[1, j] * M[1, 3]) + M[2, j] * M[2, 3]) for j in range(3)])
    return view.astype(np.float32), full.astype(np.float32), center.astype(np.float32)


def pose_step(master, grad6, m, v, step, lr_translation, lr_rotation, proj, beta1=0.9, beta2=0.999, eps=1e-15):
    """radegs_pose_step: returns (master, m, v, view, full, center)"""
    lr = np.array([lr_translation] * 3 + [lr_rotation] * 3)
    delta, m, v = adam_delta(np.asarray(grad6, np.float64).astype(np.float32), m, v, step, lr, beta1, beta2, eps)
    master = retract(delta.astype(np.float64), master)
    return (master, m, v) + camera_tensors(master, proj)


# ---- the twists themselves, for the finite-difference checks ---------------------------------------------------------------------------------
def se3_exp(tau):
    """[4,4] Exp of a twist (rho, theta), the same coefficients as retract"""
    return retract(tau, np.eye(4))


def perturbed_camera(viewmatrix, proj_t, twist, side):
    """(viewmatrix, projmatrix, campos) in float64 of w2c Exp(twist) (side = "right", the world-frame xi) or Exp(twist) w2c ("left", the
    camera-frame tau); viewmatrix and proj_t are stored transposed"""
    w2c = np.asarray(viewmatrix, np.float64).reshape(4, 4).T
    E = se3_exp(twist)
    w2c = w2c @ E if side == "right" else E @ w2c
    vm = w2c.T.copy()
    return vm, vm @ np.asarray(proj_t, np.float64), -w2c[:3, :3].T @ w2c[:3, 3]
