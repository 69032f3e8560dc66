// rg_activate.h -- the per-Gaussian arithmetic of the model's activations, one routine per chain.
//
// Scales and opacity restate radegs_filter3d.hip's two kernels expression for expression: the unit that includes this
// header is built with that unit's -ffp-contract=on, which contracts within one source expression only, so the same
// expressions give the same bits (tests/test_gpu_model_activations.py holds the two units to each other).
//
// The rotation chain is F.normalize(x, dim=1, eps=1e-12) as a stated float32 chain, one rounding per operation: every
// product and sum is an __fmul_rn / __fadd_rn / __fsub_rn call, which no contraction flag fuses.
//   forward   n2 = ((x0^2 + x1^2) + x2^2) + x3^2;  n = sqrtf(n2);  d = fmaxf(n, 1e-12f);  y = x / d
//   backward  n >= 1e-12f:  s = ((g0 y0 + g1 y1) + g2 y2) + g3 y3;  g_x = (g - y s) / d
//             otherwise  :  g_x = g / 1e-12f          (the clamp is active: d is a constant)
#pragma once
#include <hip/hip_runtime.h>

namespace rga {

constexpr float kNormEps = 1e-12f;

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// row i of get_scaling_n_opacity_with_3D_filter
__device__ __forceinline__ void scale_opacity_fwd(size_t i, const float* __restrict__ scaling_raw, const float* __restrict__ opacity_raw,
                                                  const float* __restrict__ filter_3D, float* __restrict__ scales_out,
                                                  float* __restrict__ opacity_out) {
  const float f = filter_3D[i], f2 = f * f;
  float det1 = 1.0f, det2 = 1.0f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float s = expf(scaling_raw[3 * i + k]);
    const float s2 = s * s, a2 = s2 + f2;
    det1 *= s2; det2 *= a2;
    scales_out[3 * i + k] = sqrtf(a2);
  }
  opacity_out[i] = sigmoidf(opacity_raw[i]) * sqrtf(det1 / det2);
}

// its backward; g_scales / g_opacity may be NULL (= zero cotangent)
__device__ __forceinline__ void scale_opacity_bwd(size_t i, const float* __restrict__ scaling_raw, const float* __restrict__ opacity_raw,
                                                  const float* __restrict__ filter_3D, const float* __restrict__ g_scales,
                                                  const float* __restrict__ g_opacity, float* __restrict__ g_scaling_raw,
                                                  float* __restrict__ g_opacity_raw) {
  const float f = filter_3D[i], f2 = f * f;
  float s2[3], a2[3], det1 = 1.0f, det2 = 1.0f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float s = expf(scaling_raw[3 * i + k]);
    s2[k] = s * s; a2[k] = s2[k] + f2;
    det1 *= s2[k]; det2 *= a2[k];
  }
  const float coef = sqrtf(det1 / det2);
  const float sg = sigmoidf(opacity_raw[i]);
  const float go = g_opacity ? g_opacity[i] : 0.0f;
  g_opacity_raw[i] = go * coef * sg * (1.0f - sg);
  const float gc = go * sg * coef;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float gs = g_scales ? g_scales[3 * i + k] : 0.0f;
    g_scaling_raw[3 * i + k] = gs * s2[k] / sqrtf(a2[k]) + gc * f2 / a2[k];
  }
}

__device__ __forceinline__ float quat_norm(const float4 x) {
  const float n2 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x.x, x.x), __fmul_rn(x.y, x.y)), __fmul_rn(x.z, x.z)), __fmul_rn(x.w, x.w));
  return sqrtf(n2);
}

__device__ __forceinline__ float4 normalize_fwd(const float4 x) {
  const float d = fmaxf(quat_norm(x), kNormEps);
  return make_float4(x.x / d, x.y / d, x.z / d, x.w / d);
}

__device__ __forceinline__ float4 normalize_bwd(const float4 x, const float4 g) {
  const float n = quat_norm(x);
  if (!(n >= kNormEps)) return make_float4(g.x / kNormEps, g.y / kNormEps, g.z / kNormEps, g.w / kNormEps);
  const float4 y = make_float4(x.x / n, x.y / n, x.z / n, x.w / n);
  const float s = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(g.x, y.x), __fmul_rn(g.y, y.y)), __fmul_rn(g.z, y.z)), __fmul_rn(g.w, y.w));
  return make_float4(__fsub_rn(g.x, __fmul_rn(y.x, s)) / n, __fsub_rn(g.y, __fmul_rn(y.y, s)) / n, __fsub_rn(g.z, __fmul_rn(y.z, s)) / n,
                     __fsub_rn(g.w, __fmul_rn(y.w, s)) / n);
}

}  // namespace rga
