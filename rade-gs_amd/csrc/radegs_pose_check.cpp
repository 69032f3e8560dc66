// radegs_pose_check.cpp -- test-only stand-alone program (tests/test_pose_hostcheck.py builds it together with radegs_pose.hip, host code under
// -fsanitize=address,undefined, and runs it on the CPU): the argument checks of radegs_pose_gradient / radegs_pose_step, which refuse before
// the first HIP call, and rg_pose.h's row term, step and camera elements on heap arrays of exactly the documented sizes, so that a read or
// write past any of them is caught.  Never linked into the product, never run on a GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/radegs.h"
#include "rg_pose.h"

static int failures = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);               \
      failures++;                                                         \
    }                                                                     \
  } while (0)

// the SH colour of one channel at the direction d (unnormalised), written independently of rg_pose.h's derivative table
static double sh_colour(int deg, const float* sh, int ch, const double d[3]) {
  using namespace rgpose;
  const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const double x = d[0] / len, y = d[1] / len, z = d[2] / len, xx = x * x, yy = y * y, zz = z * z;
  double b[16] = {kC0, -kC1 * y, kC1 * z, -kC1 * x, kC2[0] * x * y, kC2[1] * y * z, kC2[2] * (2 * zz - xx - yy), kC2[3] * x * z, kC2[4] * (xx - yy),
                  kC3[0] * y * (3 * xx - yy), kC3[1] * x * y * z, kC3[2] * y * (4 * zz - xx - yy), kC3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                  kC3[4] * x * (4 * zz - xx - yy), kC3[5] * z * (xx - yy), kC3[6] * x * (xx - 3 * yy)};
  double c = 0;
  for (int k = 0; k < (deg + 1) * (deg + 1); k++) c += b[k] * sh[3 * k + ch];
  return c;
}

static void check_arguments() {
  EXPECT(radegs_pose_gradient_bytes(0) == 48 && radegs_pose_gradient_bytes(1) == 48 && radegs_pose_gradient_bytes(256) == 48);
  EXPECT(radegs_pose_gradient_bytes(257) == 96 && radegs_pose_gradient_bytes(262144) == 1024 * 48 && radegs_pose_gradient_bytes(262145) == 1024 * 48);
  EXPECT(radegs_pose_gradient_bytes(1000000000000LL) == 1024 * 48 && radegs_pose_gradient_bytes(-5) == 48);
  float f[48] = {0};
  double w[6], o[12];
  // every refusal comes before the first HIP call: these "device" pointers are host memory that must not be touched
  EXPECT(radegs_pose_gradient(-1, 16, 3, f, f, f, f, f, f, f, f, w, 48, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_gradient(1, 16, 4, f, f, f, f, f, f, f, f, w, 48, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_gradient(1, 16, -1, f, f, f, f, f, f, f, f, w, 48, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_gradient(1, 15, 3, f, f, f, f, f, f, f, f, w, 48, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_gradient(1, 17, 3, f, f, f, f, f, f, f, f, w, 48, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_gradient(1, 0, 0, f, f, f, f, f, f, f, f, w, 48, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_gradient(1, 16, 3, f, f, f, f, f, f, f, f, w, 47, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_gradient(257, 16, 3, f, f, f, f, f, f, f, f, w, 95, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_gradient(1, 16, 3, f, f, f, f, f, f, f, f, nullptr, 48, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_gradient(1, 16, 3, f, f, f, f, f, f, f, f, w, 48, nullptr, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_gradient(0, 16, 3, nullptr, nullptr, nullptr, nullptr, f, nullptr, nullptr, nullptr, w, 48, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_gradient(0, 16, 3, nullptr, nullptr, nullptr, f, nullptr, nullptr, nullptr, nullptr, w, 48, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  const float* p[8] = {f, f, f, f, f, f, f, f};
  for (int k = 0; k < 8; k++) {
    if (k == 3 || k == 4) continue;   // campos, viewmatrix: above
    const float* q[8];
    for (int j = 0; j < 8; j++) q[j] = j == k ? nullptr : p[j];
    EXPECT(radegs_pose_gradient(1, 16, 3, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], w, 48, o, nullptr) == RADEGS_ERR_INVALID_ARG);
  }
  double m[16];
  const double nan = std::numeric_limits<double>::quiet_NaN();
  EXPECT(radegs_pose_step(nullptr, w, f, f, 1, 1e-3, 1e-3, 0.9, 0.999, 1e-15, f, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, nullptr, f, f, 1, 1e-3, 1e-3, 0.9, 0.999, 1e-15, f, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, nullptr, f, 1, 1e-3, 1e-3, 0.9, 0.999, 1e-15, f, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, nullptr, 1, 1e-3, 1e-3, 0.9, 0.999, 1e-15, f, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, f, 1, 1e-3, 1e-3, 0.9, 0.999, 1e-15, nullptr, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, f, 1, 1e-3, 1e-3, 0.9, 0.999, 1e-15, f, nullptr, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, f, 1, 1e-3, 1e-3, 0.9, 0.999, 1e-15, f, f, nullptr, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, f, 1, 1e-3, 1e-3, 0.9, 0.999, 1e-15, f, f, f, nullptr, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, f, 0, 1e-3, 1e-3, 0.9, 0.999, 1e-15, f, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, f, nan, 1e-3, 1e-3, 0.9, 0.999, 1e-15, f, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, f, 1, -1e-3, 1e-3, 0.9, 0.999, 1e-15, f, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, f, 1, 1e-3, nan, 0.9, 0.999, 1e-15, f, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, f, 1, 1e-3, 1e-3, 1.0, 0.999, 1e-15, f, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, f, 1, 1e-3, 1e-3, 0.9, -0.1, 1e-15, f, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
  EXPECT(radegs_pose_step(m, w, f, f, 1, 1e-3, 1e-3, 0.9, 0.999, -1.0, f, f, f, f, nullptr) == RADEGS_ERR_INVALID_ARG);
}

static void check_row() {
  // arrays of exactly the sizes the row may read
  std::vector<float> m = {1.f, 2.f, 3.f}, q = {1.f, 0.f, 0.f, 0.f}, g = {0.5f, -1.f, 2.f}, gq = {9.f, 0.25f, -0.5f, 0.75f}, campos = {0.5f, -0.25f, -4.f};
  std::vector<float> dsh0 = {0.f, 0.f, 0.f};
  double out[6];
  rgpose::row(m.data(), q.data(), g.data(), gq.data(), dsh0.data(), nullptr, 3, campos.data(), out);   // zero DC cotangent: the SH row is not read
  EXPECT(out[0] == 0.5 && out[1] == -1.0 && out[2] == 2.0);
  EXPECT(out[3] == 7.0 + 0.125 && out[4] == -0.5 - 0.25 && out[5] == -2.0 + 0.375);
  dsh0 = {0.3f, -0.2f, 0.1f};
  double flat[6];
  rgpose::row(m.data(), q.data(), g.data(), gq.data(), dsh0.data(), nullptr, 0, campos.data(), flat);   // degree 0: no view dependence, not read either
  EXPECT(flat[3] == out[3] && flat[4] == out[4] && flat[5] == out[5]);
  for (int deg = 1; deg <= 3; deg++) {
    const int M = (deg + 1) * (deg + 1);
    std::vector<float> sh(3 * M);                    // exactly (deg + 1)^2 rows
    for (int i = 0; i < 3 * M; i++) sh[i] = 0.1f * (float)((i * 37) % 11 - 5);
    const double d[3] = {1.0 - 0.5, 2.0 + 0.25, 3.0 + 4.0};
    const double dRGB[3] = {0.3f / rgpose::kC0, -0.2f / rgpose::kC0, 0.1f / rgpose::kC0};
    double c[3];
    rgpose::sh_direction_cotangent(deg, sh.data(), d, dRGB, c);
    EXPECT(std::fabs(d[0] * c[0] + d[1] * c[1] + d[2] * c[2]) < 1e-13);   // the colour does not change along the ray
    for (int a = 0; a < 3; a++) {                    // c = d(sum_ch dRGB_ch colour_ch) / dd, by central differences
      const double h = 1e-5;
      double dp[3] = {d[0], d[1], d[2]}, dm[3] = {d[0], d[1], d[2]}, fd = 0;
      dp[a] += h; dm[a] -= h;
      for (int ch = 0; ch < 3; ch++) fd += dRGB[ch] * (sh_colour(deg, sh.data(), ch, dp) - sh_colour(deg, sh.data(), ch, dm)) / (2 * h);
      EXPECT(std::fabs(fd - c[a]) < 1e-8 * (1 + std::fabs(c[a])));
    }
    double with[6];
    rgpose::row(m.data(), q.data(), g.data(), gq.data(), dsh0.data(), sh.data(), deg, campos.data(), with);
    EXPECT(with[3] == out[3] - (d[1] * c[2] - d[2] * c[1]) && with[4] == out[4] - (d[2] * c[0] - d[0] * c[2]) && with[5] == out[5] - (d[0] * c[1] - d[1] * c[0]));
    EXPECT(with[3] != out[3]);
  }
  std::vector<float> vm = {0.f, 0.f, 1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 1.f, 2.f, 3.f, 1.f};   // R = a cyclic permutation, t = (1, 2, 3)
  const double gxi[6] = {1, 2, 3, 4, 5, 6};
  double gtau[6];
  rgpose::to_camera_frame(vm.data(), gxi, gtau);
  EXPECT(gtau[0] == 2 && gtau[1] == 3 && gtau[2] == 1);                       // R g_rho
  EXPECT(gtau[3] == 5 + (2 * 1 - 3 * 3) && gtau[4] == 6 + (3 * 2 - 1 * 1) && gtau[5] == 4 + (1 * 3 - 2 * 2));
}

static void check_step() {
  float mo = 0.f, vo = 0.f;
  const float d = rgpose::adam_delta(2.f, mo, vo, 0.1f, 0.999f, 0.001f, 1e-15f, (float)(1e-3 / 0.1), (float)std::sqrt(0.001));
  EXPECT(std::fabs(d + 1e-3f) < 1e-8f && std::fabs(mo - 0.2f) < 1e-7f && std::fabs(vo - 0.004f) < 1e-8f);   // the first Adam step is -lr sign(g)
  std::vector<double> master = {1, 0, 0, 0.5, 0, 1, 0, -1.0, 0, 0, 1, 2.0, 0, 0, 0, 1};
  unsigned long long s = 88172645463325252ULL;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0 - 0.5; };
  double worst = 0;
  for (int it = 0; it < 1000; it++) {
    const double scale = it % 3 == 0 ? 1e-9 : (it % 3 == 1 ? 1e-3 : 0.7);     // the series branch, a training-sized step, a large one
    const double tau[6] = {0.02 * rnd(), 0.02 * rnd(), 0.02 * rnd(), scale * rnd(), scale * rnd(), scale * rnd()};
    rgpose::retract(tau, master.data());
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double dot = 0;
        for (int k = 0; k < 3; k++) dot += master[4 * k + i] * master[4 * k + j];
        worst = std::fmax(worst, std::fabs(dot - (i == j ? 1.0 : 0.0)));
      }
  }
  EXPECT(worst <= 1e-14);
  EXPECT(master[12] == 0 && master[13] == 0 && master[14] == 0 && master[15] == 1);
  const double zero[6] = {0, 0, 0, 0, 0, 0};
  std::vector<double> id = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  rgpose::retract(zero, id.data());
  for (int i = 0; i < 16; i++) EXPECT(id[i] == (i % 5 == 0 ? 1.0 : 0.0));     // a step of zero leaves the identity alone
  std::vector<float> proj = {1.7f, 0, 0, 0, 0, 2.5f, 0, 0, 0, 0, 1.0001f, 1.f, 0, 0, -0.010001f, 0};
  std::vector<double> w2c = {0, 1, 0, 1.0, 0, 0, 1, 2.0, 1, 0, 0, 3.0, 0, 0, 0, 1};
  float e[35];
  for (int k = 0; k < 35; k++) e[k] = rgpose::camera_element(w2c.data(), proj.data(), k);
  EXPECT(e[1] == 0.f && e[2] == 1.f && e[4] == 1.f && e[12] == 1.f && e[13] == 2.f && e[14] == 3.f && e[15] == 1.f && e[3] == 0.f);
  EXPECT(e[16 + 2] == 1.0001f && e[16 + 3] == 1.f);                           // row 0 of view = (0, 0, 1, 0): picks proj's row 2
  EXPECT(e[16 + 12] == 1.7f && e[16 + 13] == 5.f && e[16 + 14] == (float)(3.0 * (double)1.0001f + (double)-0.010001f) && e[16 + 15] == 3.f);
  EXPECT(e[32] == -3.f && e[33] == -1.f && e[34] == -2.f);                    // -R^T t
}

int main() {
  check_arguments();
  check_row();
  check_step();
  if (failures) {
    std::printf("radegs_pose_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("radegs_pose_check: ok\n");
  return 0;
}
