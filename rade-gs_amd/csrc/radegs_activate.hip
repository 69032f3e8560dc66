// radegs_activate.hip -- the model's pre-step: raw parameters in, the rasterizer's four per-Gaussian inputs out,
//     shs       = torch.cat((_features_dc, _features_rest), dim=1)        GaussianModel.get_features
//     rotations = F.normalize(_rotation)                                  GaussianModel.get_rotation
//     scales, opacity = get_scaling_n_opacity_with_3D_filter              (radegs_filter3d.hip's arithmetic, rg_activate.h)
// and back: the cotangents of those four become the gradients of the five parameters.  One launch per direction; include/radegs.h,
// "Model activations", is the specification.  Built with -ffp-contract=on like radegs_filter3d (build.py: UNIT_FLAGS).
//
// A workgroup takes a tile of 64 Gaussians.  The SH rows are a copy whose difficulty is layout: a joined row is 12 (K+1) bytes, an f_dc
// row 12 and an f_rest row 12 K, so a row of one side never starts on a 16-byte boundary of the other -- but a tile of 64 rows is
// contiguous and 256-byte aligned on every side.  As in radegs_modelio.hip's pack kernel the tile goes through an LDS image of the JOINED
// rows: forward reads the two sources with consecutive lanes on consecutive dwords and stores the image as it lies in whole 16-byte
// stores; backward loads the image in 16-byte loads and gathers each 16-byte store of the two slices from it.  Lanes 0-63 of the
// workgroup do the tile's scales and opacity, lanes 64-127 its rotations (one 16-byte load and store per row), before the barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_activate.h"

namespace rga {

constexpr int kTile = 64;        // rows per workgroup; 64 * 12 (K+1) bytes <= 61 440 for K <= RADEGS_MODELIO_MAX_REST
constexpr int kThreads = 256;

// the tile's n * w contiguous floats at `s` -> columns [col, col + w) of the image's rows (W floats each)
__device__ __forceinline__ void stage(float* tile, int W, int col, const float* __restrict__ s, int n, int w) {
  for (int i = threadIdx.x; i < n * w; i += kThreads) {
    const int r = i / w;
    tile[r * W + col + (i - r * w)] = s[i];
  }
}

// columns [col, col + w) of the image's rows -> the tile's n * w contiguous floats at `o` (16-byte aligned), whole 16-byte stores
__device__ __forceinline__ void unstage(const float* tile, int W, int col, float* __restrict__ o, int n, int w) {
  const int total = n * w, quads = total >> 2;
  for (int q = threadIdx.x; q < quads; q += kThreads) {
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = 4 * q + j, r = i / w;
      e[j] = tile[r * W + col + (i - r * w)];
    }
    reinterpret_cast<float4*>(o)[q] = make_float4(e[0], e[1], e[2], e[3]);
  }
  for (int i = 4 * quads + threadIdx.x; i < total; i += kThreads) {      // the last tile's odd floats
    const int r = i / w;
    o[i] = tile[r * W + col + (i - r * w)];
  }
}

__device__ __forceinline__ void fill_zero(float* __restrict__ o, int total) {
  const int quads = total >> 2;
  for (int q = threadIdx.x; q < quads; q += kThreads) reinterpret_cast<float4*>(o)[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int i = 4 * quads + threadIdx.x; i < total; i += kThreads) o[i] = 0.0f;
}

__global__ void __launch_bounds__(kThreads) activate_fwd_kernel(int P, int K, const float* __restrict__ f_dc, const float* __restrict__ f_rest,
                                                                const float* __restrict__ rotation_raw, const float* __restrict__ scaling_raw,
                                                                const float* __restrict__ opacity_raw, const float* __restrict__ filter_3D,
                                                                float* __restrict__ shs, float* __restrict__ rotations,
                                                                float* __restrict__ scales, float* __restrict__ opacity) {
  extern __shared__ __align__(16) float tile[];
  const size_t row0 = (size_t)blockIdx.x * kTile;
  const int n = min(kTile, (int)((size_t)P - row0));
  const int w = 3 * K, W = w + 3;
  stage(tile, W, 0, f_dc + row0 * 3, n, 3);
  if (K > 0) stage(tile, W, 3, f_rest + row0 * w, n, w);
  const int t = threadIdx.x;
  if (t < n) {
    scale_opacity_fwd(row0 + t, scaling_raw, opacity_raw, filter_3D, scales, opacity);
  } else if (t >= kTile && t - kTile < n) {
    const size_t i = row0 + (t - kTile);
    reinterpret_cast<float4*>(rotations)[i] = normalize_fwd(reinterpret_cast<const float4*>(rotation_raw)[i]);
  }
  __syncthreads();
  float* o = shs + row0 * W;                             // 64 W floats = 256 W bytes per tile: 16-byte stores stay aligned
  const int total = n * W, quads = total >> 2;
  for (int i = threadIdx.x; i < quads; i += kThreads) reinterpret_cast<float4*>(o)[i] = reinterpret_cast<const float4*>(tile)[i];
  for (int i = 4 * quads + threadIdx.x; i < total; i += kThreads) o[i] = tile[i];
}

__global__ void __launch_bounds__(kThreads) activate_bwd_kernel(int P, int K, const float* __restrict__ rotation_raw, const float* __restrict__ scaling_raw,
                                                                const float* __restrict__ opacity_raw, const float* __restrict__ filter_3D,
                                                                const float* __restrict__ g_shs, const float* __restrict__ g_rotations,
                                                                const float* __restrict__ g_scales, const float* __restrict__ g_opacity,
                                                                float* __restrict__ g_f_dc, float* __restrict__ g_f_rest,
                                                                float* __restrict__ g_rotation_raw, float* __restrict__ g_scaling_raw,
                                                                float* __restrict__ g_opacity_raw) {
  extern __shared__ __align__(16) float tile[];
  const size_t row0 = (size_t)blockIdx.x * kTile;
  const int n = min(kTile, (int)((size_t)P - row0));
  const int w = 3 * K, W = w + 3;
  if (g_shs) {
    const float* s = g_shs + row0 * W;
    const int total = n * W, quads = total >> 2;
    for (int i = threadIdx.x; i < quads; i += kThreads) reinterpret_cast<float4*>(tile)[i] = reinterpret_cast<const float4*>(s)[i];
    for (int i = 4 * quads + threadIdx.x; i < total; i += kThreads) tile[i] = s[i];
  }
  const int t = threadIdx.x;
  if (t < n) {
    scale_opacity_bwd(row0 + t, scaling_raw, opacity_raw, filter_3D, g_scales, g_opacity, g_scaling_raw, g_opacity_raw);
  } else if (t >= kTile && t - kTile < n) {
    const size_t i = row0 + (t - kTile);
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // no cotangent: exactly zero, whatever the quaternion
    if (g_rotations) g = normalize_bwd(reinterpret_cast<const float4*>(rotation_raw)[i], reinterpret_cast<const float4*>(g_rotations)[i]);
    reinterpret_cast<float4*>(g_rotation_raw)[i] = g;
  }
  if (!g_shs) {                                          // uniform over the grid: no barrier is skipped by part of a workgroup
    fill_zero(g_f_dc + row0 * 3, n * 3);
    if (K > 0) fill_zero(g_f_rest + row0 * w, n * w);
    return;
  }
  __syncthreads();
  unstage(tile, W, 0, g_f_dc + row0 * 3, n, 3);
  if (K > 0) unstage(tile, W, 3, g_f_rest + row0 * w, n, w);
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace rga

extern "C" {

int radegs_model_activate_forward(int P, int K, const float* f_dc, const float* f_rest, const float* rotation_raw, const float* scaling_raw,
                                  const float* opacity_raw, const float* filter_3D, float* shs, float* rotations, float* scales, float* opacity,
                                  void* stream) {
  if (P < 0 || K < 0 || K > RADEGS_MODELIO_MAX_REST) return RADEGS_ERR_INVALID_ARG;
  if (P == 0) return 0;
  if ((K == 0) != (f_rest == nullptr)) return RADEGS_ERR_INVALID_ARG;
  if (!f_dc || !rotation_raw || !scaling_raw || !opacity_raw || !filter_3D || !shs || !rotations || !scales || !opacity) return RADEGS_ERR_INVALID_ARG;
  if (rga::misaligned(f_dc) || rga::misaligned(f_rest) || rga::misaligned(rotation_raw) || rga::misaligned(shs) || rga::misaligned(rotations))
    return RADEGS_ERR_INVALID_ARG;
  const unsigned tiles = (unsigned)(((long long)P + rga::kTile - 1) / rga::kTile);
  hipLaunchKernelGGL(rga::activate_fwd_kernel, dim3(tiles), dim3(rga::kThreads), (size_t)rga::kTile * 3 * (K + 1) * sizeof(float),
                     static_cast<hipStream_t>(stream), P, K, f_dc, f_rest, rotation_raw, scaling_raw, opacity_raw, filter_3D, shs, rotations, scales,
                     opacity);
  return hipGetLastError() == hipSuccess ? 0 : RADEGS_ERR_HIP;
}

int radegs_model_activate_backward(int P, int K, const float* rotation_raw, const float* scaling_raw, const float* opacity_raw, const float* filter_3D,
                                   const float* g_shs, const float* g_rotations, const float* g_scales, const float* g_opacity, float* g_f_dc,
                                   float* g_f_rest, float* g_rotation_raw, float* g_scaling_raw, float* g_opacity_raw, void* stream) {
  if (P < 0 || K < 0 || K > RADEGS_MODELIO_MAX_REST) return RADEGS_ERR_INVALID_ARG;
  if (P == 0) return 0;
  if ((K == 0) != (g_f_rest == nullptr)) return RADEGS_ERR_INVALID_ARG;
  if (!rotation_raw || !scaling_raw || !opacity_raw || !filter_3D || !g_f_dc || !g_rotation_raw || !g_scaling_raw || !g_opacity_raw)
    return RADEGS_ERR_INVALID_ARG;
  if (rga::misaligned(rotation_raw) || rga::misaligned(g_shs) || rga::misaligned(g_rotations) || rga::misaligned(g_f_dc) || rga::misaligned(g_f_rest) ||
      rga::misaligned(g_rotation_raw))
    return RADEGS_ERR_INVALID_ARG;
  const unsigned tiles = (unsigned)(((long long)P + rga::kTile - 1) / rga::kTile);
  hipLaunchKernelGGL(rga::activate_bwd_kernel, dim3(tiles), dim3(rga::kThreads), (size_t)rga::kTile * 3 * (K + 1) * sizeof(float),
                     static_cast<hipStream_t>(stream), P, K, rotation_raw, scaling_raw, opacity_raw, filter_3D, g_shs, g_rotations, g_scales,
                     g_opacity, g_f_dc, g_f_rest, g_rotation_raw, g_scaling_raw, g_opacity_raw);
  return hipGetLastError() == hipSuccess ? 0 : RADEGS_ERR_HIP;
}

}  // extern "C"
