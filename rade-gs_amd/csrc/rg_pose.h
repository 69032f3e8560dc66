// rg_pose.h -- camera pose refinement: the per-Gaussian row of the SE(3) pose gradient, the change of frame of the summed
// gradient, and the pose step (Adam on the six-vector, retraction on the float64 master, the three float32 camera tensors).  Host + device,
// fp64 throughout, -ffp-contract=off: every expression below is evaluated as written, left to right, one rounding per operation, IEEE divide
// and sqrt.  tests/pose_restatement.py restates the same expressions in NumPy; radegs_pose.hip is held to it bit for bit.
//
// Conventions (the project's): viewmatrix is the world-to-camera matrix stored transposed (row-major vm[4 r + c] = w2c[c][r]); quaternions
// are (w, x, y, z).  World-frame twist xi = (rho, theta): w2c(xi) = w2c [[Exp(theta), rho], [0, 1]].  Moving the camera like that is moving
// every Gaussian by m -> Exp(theta) m + rho, q -> (1, theta / 2) q, except that the SH colour keeps reading the unrotated direction: the
// last term takes that rotation back out.  At xi = 0
//   dL/drho   = sum_i g_i
//   dL/dtheta = sum_i [ m_i x g_i + 1/2 (w_i gv_i - gw_i v_i + v_i x gv_i) - d_i x c_i ],  d_i = m_i - campos,  c_i = J_i^T (dL/dsh[i,0,:] / C0)
// with J_i the derivative of the SH colour with respect to the unnormalised direction d_i (through the normalisation).
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define RG_POSE_HD __host__ __device__ inline
#else
#define RG_POSE_HD inline
#endif

namespace rgpose {

constexpr double kC0 = 0.28209479177387814;
constexpr double kC1 = 0.4886025119029199;
constexpr double kC2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396};
constexpr double kC3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
                           1.445305721320277, -0.5900435899266435};
constexpr double kSeriesBelow = 1e-8;   // |theta| under which Exp takes its series coefficients

// d(basis_k)/d(x, y, z) at the unit direction (x, y, z), k = 1 .. (deg + 1)^2 - 1, in the rasterizer's order and signs.  w[3 k + a].
RG_POSE_HD void sh_basis_gradient(int deg, double x, double y, double z, double* w) {
  w[3] = 0.0; w[4] = -kC1; w[5] = 0.0;
  w[6] = 0.0; w[7] = 0.0; w[8] = kC1;
  w[9] = -kC1; w[10] = 0.0; w[11] = 0.0;
  if (deg < 2) return;
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
  w[12] = kC2[0] * y; w[13] = kC2[0] * x; w[14] = 0.0;
  w[15] = 0.0; w[16] = kC2[1] * z; w[17] = kC2[1] * y;
  w[18] = kC2[2] * (-2.0 * x); w[19] = kC2[2] * (-2.0 * y); w[20] = kC2[2] * (4.0 * z);
  w[21] = kC2[3] * z; w[22] = 0.0; w[23] = kC2[3] * x;
  w[24] = kC2[4] * (2.0 * x); w[25] = kC2[4] * (-2.0 * y); w[26] = 0.0;
  if (deg < 3) return;
  w[27] = kC3[0] * (6.0 * xy); w[28] = kC3[0] * (3.0 * (xx - yy)); w[29] = 0.0;
  w[30] = kC3[1] * yz; w[31] = kC3[1] * xz; w[32] = kC3[1] * xy;
  w[33] = kC3[2] * (-2.0 * xy); w[34] = kC3[2] * ((4.0 * zz - xx) - 3.0 * yy); w[35] = kC3[2] * (8.0 * yz);
  w[36] = kC3[3] * (-6.0 * xz); w[37] = kC3[3] * (-6.0 * yz); w[38] = kC3[3] * (3.0 * ((2.0 * zz - xx) - yy));
  w[39] = kC3[4] * ((4.0 * zz - 3.0 * xx) - yy); w[40] = kC3[4] * (-2.0 * xy); w[41] = kC3[4] * (8.0 * xz);
  w[42] = kC3[5] * (2.0 * xz); w[43] = kC3[5] * (-2.0 * yz); w[44] = kC3[5] * (xx - yy);
  w[45] = kC3[6] * (3.0 * (xx - yy)); w[46] = kC3[6] * (-6.0 * xy); w[47] = 0.0;
}

// c = J^T dRGB of one Gaussian: d = m - campos (unnormalised), sh [M,3] float32 rows of which (deg + 1)^2 are read, deg >= 1.
//   u = d / sqrt((dx dx + dy dy) + dz dz);  ddir_a = sum_ch (sum_k w[k][a] sh[k][ch]) dRGB_ch, k ascending from 1 starting at 0.0, ch ascending
//   starting at 0.0;  c = dnormvdv(d, ddir) as the rasterizer's backward forms it.
template <int deg>
RG_POSE_HD void sh_direction_cotangent_of(const float* sh, const double d[3], const double dRGB[3], double c[3]) {
  const double n2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  const double len = sqrt(n2);
  const double x = d[0] / len, y = d[1] / len, z = d[2] / len;
  double w[48];
  sh_basis_gradient(deg, x, y, z, w);
  constexpr int M = (deg + 1) * (deg + 1);
  double ddir[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 1; k < M; k++) {
      const double v = (double)sh[3 * k + ch];
      s0 = s0 + w[3 * k] * v;
      s1 = s1 + w[3 * k + 1] * v;
      s2 = s2 + w[3 * k + 2] * v;
    }
    ddir[0] = ddir[0] + s0 * dRGB[ch];
    ddir[1] = ddir[1] + s1 * dRGB[ch];
    ddir[2] = ddir[2] + s2 * dRGB[ch];
  }
  const double inv = 1.0 / sqrt(n2 * n2 * n2);
  c[0] = (((n2 - d[0] * d[0]) * ddir[0] - d[1] * d[0] * ddir[1]) - d[2] * d[0] * ddir[2]) * inv;
  c[1] = ((-d[0] * d[1] * ddir[0] + (n2 - d[1] * d[1]) * ddir[1]) - d[2] * d[1] * ddir[2]) * inv;
  c[2] = ((-d[0] * d[2] * ddir[0] - d[1] * d[2] * ddir[1]) + (n2 - d[2] * d[2]) * ddir[2]) * inv;
}

// (the degree is a template argument so that the table above stays in registers on the device; the arithmetic does not depend on it)
RG_POSE_HD void sh_direction_cotangent(int deg, const float* sh, const double d[3], const double dRGB[3], double c[3]) {
  if (deg == 1) sh_direction_cotangent_of<1>(sh, d, dRGB, c);
  else if (deg == 2) sh_direction_cotangent_of<2>(sh, d, dRGB, c);
  else sh_direction_cotangent_of<3>(sh, d, dRGB, c);
}

// One Gaussian's contribution to (dL/drho, dL/dtheta).  m [3], q [4], g = dL/dmeans3D [3], gq = dL/drotations [4], dsh0 = dL/dsh[i,0,:] [3],
// sh = the Gaussian's SH row: read only when deg > 0 and dsh0 is not all zero (it may be null otherwise).
RG_POSE_HD void row(const float* m, const float* q, const float* g, const float* gq, const float* dsh0, const float* sh, int deg,
                    const float* campos, double out[6]) {
  const double mx = m[0], my = m[1], mz = m[2], gx = g[0], gy = g[1], gz = g[2];
  const double w = q[0], vx = q[1], vy = q[2], vz = q[3], gw = gq[0], hx = gq[1], hy = gq[2], hz = gq[3];
  out[0] = gx; out[1] = gy; out[2] = gz;
  const double ax = my * gz - mz * gy, ay = mz * gx - mx * gz, az = mx * gy - my * gx;
  const double bx = (w * hx - gw * vx) + (vy * hz - vz * hy);
  const double by = (w * hy - gw * vy) + (vz * hx - vx * hz);
  const double bz = (w * hz - gw * vz) + (vx * hy - vy * hx);
  double tx = ax + 0.5 * bx, ty = ay + 0.5 * by, tz = az + 0.5 * bz;
  if (deg > 0 && (dsh0[0] != 0.f || dsh0[1] != 0.f || dsh0[2] != 0.f)) {
    const double d[3] = {mx - (double)campos[0], my - (double)campos[1], mz - (double)campos[2]};
    const double dRGB[3] = {(double)dsh0[0] / kC0, (double)dsh0[1] / kC0, (double)dsh0[2] / kC0};
    double c[3];
    sh_direction_cotangent(deg, sh, d, dRGB, c);
    tx = tx - (d[1] * c[2] - d[2] * c[1]);
    ty = ty - (d[2] * c[0] - d[0] * c[2]);
    tz = tz - (d[0] * c[1] - d[1] * c[0]);
  }
  out[3] = tx; out[4] = ty; out[5] = tz;
}

// The summed world-frame gradient in the camera frame: Exp(tau) w2c = w2c Exp(xi), w2c = (R, t) read from the float32 viewmatrix.
//   g_tau_rho = R g_rho;  g_tau_theta = R g_theta + t x g_tau_rho;  rows as (R_i0 a_0 + R_i1 a_1) + R_i2 a_2.
RG_POSE_HD void to_camera_frame(const float* viewmatrix, const double gxi[6], double gtau[6]) {
  double r[3];
  for (int i = 0; i < 3; i++) {
    const double R0 = viewmatrix[i], R1 = viewmatrix[4 + i], R2 = viewmatrix[8 + i];
    gtau[i] = (R0 * gxi[0] + R1 * gxi[1]) + R2 * gxi[2];
    r[i] = (R0 * gxi[3] + R1 * gxi[4]) + R2 * gxi[5];
  }
  const double t0 = viewmatrix[12], t1 = viewmatrix[13], t2 = viewmatrix[14];
  gtau[3] = r[0] + (t1 * gtau[2] - t2 * gtau[1]);
  gtau[4] = r[1] + (t2 * gtau[0] - t0 * gtau[2]);
  gtau[5] = r[2] + (t0 * gtau[1] - t1 * gtau[0]);
}

// Adam on one component, as radegs_adam.hip's adam1 with the parameter starting from 0: returns the step -step_size (m / denom).
RG_POSE_HD float adam_delta(float g, float& m, float& v, float omb1, float b2, float omb2, float eps, float step_size, float bc2_sqrt) {
  m = m + omb1 * (g - m);
  v = v * b2 + omb2 * (g * g);
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  return 0.f - step_size * (m / denom);
}

// master <- Exp(tau) master.  master: the float64 w2c, row-major [4,4] (NOT transposed), last row (0, 0, 0, 1) left alone.  tau = (rho, theta).
//   th2 = (t0 t0 + t1 t1) + t2 t2, th = sqrt(th2).  th < kSeriesBelow: A = 1, B = 1/2, C = 1/6; else A = sin(th) / th,
//   B = 2 s s / th2 with s = sin(th / 2), C = (th - sin(th)) / (th2 th).  K = [theta]x, K2 = K K written out;
//   E = I + A K + B K2, V = I + B K + C K2;  R' = E R and t' = (E t) + (V rho), rows as (a0 b0 + a1 b1) + a2 b2.
//   Then one Newton step towards the nearest rotation, so that rounding does not accumulate over thousands of steps:
//   S = R'^T R' (symmetric, upper triangle computed), R'' = R' (3 I - S) / 2.
RG_POSE_HD void retract(const double tau[6], double* master) {
  const double t0 = tau[3], t1 = tau[4], t2 = tau[5];
  const double th2 = (t0 * t0 + t1 * t1) + t2 * t2;
  const double th = sqrt(th2);
  double A, B, C;
  if (th < kSeriesBelow) {
    A = 1.0; B = 0.5; C = 1.0 / 6.0;
  } else {
    const double sn = sin(th), sh = sin(0.5 * th);
    A = sn / th;
    B = 2.0 * sh * sh / th2;
    C = (th - sn) / (th2 * th);
  }
  const double K[9] = {0.0, -t2, t1, t2, 0.0, -t0, -t1, t0, 0.0};
  const double K2[9] = {-(t1 * t1 + t2 * t2), t0 * t1, t0 * t2, t0 * t1, -(t0 * t0 + t2 * t2), t1 * t2, t0 * t2, t1 * t2, -(t0 * t0 + t1 * t1)};
  double E[9], V[9];
  for (int i = 0; i < 9; i++) {
    const double I = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
    E[i] = (I + A * K[i]) + B * K2[i];
    V[i] = (I + B * K[i]) + C * K2[i];
  }
  double R[9], t[3];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) R[3 * i + j] = (E[3 * i] * master[j] + E[3 * i + 1] * master[4 + j]) + E[3 * i + 2] * master[8 + j];
    const double et = (E[3 * i] * master[3] + E[3 * i + 1] * master[7]) + E[3 * i + 2] * master[11];
    const double vr = (V[3 * i] * tau[0] + V[3 * i + 1] * tau[1]) + V[3 * i + 2] * tau[2];
    t[i] = et + vr;
  }
  double H[9];   // (3 I - R^T R) / 2
  for (int i = 0; i < 3; i++)
    for (int j = i; j < 3; j++) {
      const double s = (R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j];
      H[3 * i + j] = H[3 * j + i] = 0.5 * ((i == j ? 3.0 : 0.0) - s);
    }
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) master[4 * i + j] = (R[3 * i] * H[j] + R[3 * i + 1] * H[3 + j]) + R[3 * i + 2] * H[6 + j];
    master[4 * i + 3] = t[i];
  }
}

// The three float32 tensors the rasterizer reads, from the float64 master and the camera's float32 projection matrix (stored transposed,
// like the view matrix): view[4 r + c] = w2c[c][r]; full = view proj in float64, ((v0 p0 + v1 p1) + v2 p2) + v3 p3, rounded once;
// centre_j = 0 - ((R_0j t_0 + R_1j t_1) + R_2j t_2).  `e` selects the element: 0-15 view, 16-31 full, 32-34 centre.
RG_POSE_HD float camera_element(const double* master, const float* proj, int e) {
  if (e < 16) return (float)master[4 * (e & 3) + (e >> 2)];
  if (e < 32) {
    const int r = (e - 16) >> 2, c = (e - 16) & 3;
    const double v0 = master[r], v1 = master[4 + r], v2 = master[8 + r], v3 = master[12 + r];
    return (float)((((v0 * (double)proj[c]) + v1 * (double)proj[4 + c]) + v2 * (double)proj[8 + c]) + v3 * (double)proj[12 + c]);
  }
  const int j = e - 32;
  return (float)(0.0 - ((master[j] * master[3] + master[4 + j] * master[7]) + master[8 + j] * master[11]));
}

}  // namespace rgpose
