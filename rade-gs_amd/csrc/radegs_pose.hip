// radegs_pose.hip -- camera pose refinement (include/radegs.h, "Camera pose refinement").
//   radegs_pose_gradient: the SE(3) pose gradient as a fixed linear functional of the gradients the rasterizer's backward already returns.
//     One lane per Gaussian forms rg_pose.h's row in fp64 from the fp32 inputs; the rows go through rg_reduce.h's fixed-order sum (up to
//     kSumBlocks blocks leave 6 partials each, one block adds them), whose last thread also moves the sum into the camera frame.  No atomics,
//     nothing read back: two calls give the same bits.  Traffic: 68 B per Gaussian (means, rotations and three cotangent rows), plus the
//     (deg + 1)^2 x 12 B SH row where the DC cotangent is not zero, i.e. for the Gaussians the view contributed to.
//   radegs_pose_step: Adam on one camera's six-vector, the retraction on its fp64 master and the three fp32 tensors the rasterizer reads,
//     one block of 64 lanes, stream-ordered.
#include <hip/hip_runtime.h>

#include "../../include/radegs.h"
#include "rg_pose.h"
#include "rg_reduce.h"

namespace rgpose {

struct RowArgs {
  long long P;
  int M, deg;
  const float *means, *rots, *shs, *campos, *dmeans, *drots, *dsh;
};

__global__ void __launch_bounds__(256) rows_kernel(const RowArgs a, double* __restrict__ partial) {
  __shared__ double sh[6 * 256];
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const long long stride = (long long)gridDim.x * 256;
  const long long row_floats = 3LL * a.M;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.P; i += stride) {
    double r[6];
    row(a.means + 3 * i, a.rots + 4 * i, a.dmeans + 3 * i, a.drots + 4 * i, a.dsh + row_floats * i, a.shs + row_floats * i, a.deg, a.campos, r);
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] += r[k];
  }
  rg::block_sum<6>(v, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 6; k++) partial[6 * blockIdx.x + k] = v[k];
  }
}

__global__ void __launch_bounds__(256) finish_kernel(const double* __restrict__ partial, int nblocks, const float* __restrict__ viewmatrix,
                                                     double* __restrict__ out12) {
  __shared__ double sh[6 * 256];
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  rg::add_partials<6>(partial, nblocks, v);
  rg::block_sum<6>(v, sh);
  if (threadIdx.x == 0) {
    double t[6];
    to_camera_frame(viewmatrix, v, t);
    for (int k = 0; k < 6; k++) { out12[k] = v[k]; out12[6 + k] = t[k]; }
  }
}

struct StepArgs {
  double* master;
  const double* grad6;
  float *exp_avg, *exp_avg_sq;
  const float* proj;
  float *view, *full, *center;
  float step_size_t, step_size_r, bc2_sqrt, omb1, beta2, omb2, eps;
};

__global__ void __launch_bounds__(64) step_kernel(const StepArgs a) {
  __shared__ double tau[6];
  __shared__ double m[16];
  const int t = threadIdx.x;
  if (t < 6) {
    float mo = a.exp_avg[t], vo = a.exp_avg_sq[t];
    tau[t] = (double)adam_delta((float)a.grad6[t], mo, vo, a.omb1, a.beta2, a.omb2, a.eps, t < 3 ? a.step_size_t : a.step_size_r, a.bc2_sqrt);
    a.exp_avg[t] = mo; a.exp_avg_sq[t] = vo;
  }
  if (t < 16) m[t] = a.master[t];
  __syncthreads();
  if (t == 0) retract(tau, m);
  __syncthreads();
  if (t < 12) a.master[t] = m[t];
  if (t < 16) a.view[t] = camera_element(m, a.proj, t);
  else if (t < 32) a.full[t - 16] = camera_element(m, a.proj, t);
  else if (t < 35) a.center[t - 32] = camera_element(m, a.proj, t);
}

}  // namespace rgpose

extern "C" size_t radegs_pose_gradient_bytes(long long P) {
  const int nb = rg::sum_blocks(P < 0 ? 0 : P);
  return (size_t)(nb < 1 ? 1 : nb) * 6 * sizeof(double);
}

extern "C" int radegs_pose_gradient(long long P, int M, int sh_degree, const float* means3D, const float* rotations, const float* shs,
                                    const float* campos, const float* viewmatrix, const float* dL_dmeans3D, const float* dL_drotations,
                                    const float* dL_dsh, void* workspace, size_t workspace_bytes, double* out12, void* stream) {
  if (P < 0 || sh_degree < 0 || sh_degree > 3 || M < (sh_degree + 1) * (sh_degree + 1) || M > 16 || !campos || !viewmatrix || !workspace ||
      !out12 || workspace_bytes < radegs_pose_gradient_bytes(P))
    return RADEGS_ERR_INVALID_ARG;
  if (P > 0 && (!means3D || !rotations || !shs || !dL_dmeans3D || !dL_drotations || !dL_dsh)) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = rg::sum_blocks(P);
  double* partial = static_cast<double*>(workspace);
  if (nb > 0) {
    const rgpose::RowArgs a{P, M, sh_degree, means3D, rotations, shs, campos, dL_dmeans3D, dL_drotations, dL_dsh};
    hipLaunchKernelGGL(rgpose::rows_kernel, dim3(nb), dim3(256), 0, s, a, partial);
  }
  hipLaunchKernelGGL(rgpose::finish_kernel, dim3(1), dim3(256), 0, s, partial, nb, viewmatrix, out12);
  return hipGetLastError() == hipSuccess ? 0 : RADEGS_ERR_HIP;
}

extern "C" int radegs_pose_step(double* master, const double* grad6, float* exp_avg, float* exp_avg_sq, double step, double lr_translation,
                                double lr_rotation, double beta1, double beta2, double eps, const float* proj, float* world_view_transform,
                                float* full_proj_transform, float* camera_center, void* stream) {
  if (!master || !grad6 || !exp_avg || !exp_avg_sq || !proj || !world_view_transform || !full_proj_transform || !camera_center) return RADEGS_ERR_INVALID_ARG;
  if (!(step >= 1.0) || !(lr_translation >= 0.0) || !(lr_rotation >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
    return RADEGS_ERR_INVALID_ARG;
  // bias corrections in double on the host, like radegs_adam_step
  const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
  const rgpose::StepArgs a{master, grad6, exp_avg, exp_avg_sq, proj, world_view_transform, full_proj_transform, camera_center,
                           (float)(lr_translation / bc1), (float)(lr_rotation / bc1), (float)sqrt(bc2), (float)(1.0 - beta1), (float)beta2,
                           (float)(1.0 - beta2), (float)eps};
  hipLaunchKernelGGL(rgpose::step_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? 0 : RADEGS_ERR_HIP;
}
