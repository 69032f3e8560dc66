// radegs_blend_check.hip -- test-only C entry points over the DEVICE build of csrc/rg_blend.h: the arithmetic that decides on the GPU which
// (entry, block) pairs the sub-tile entry streams drop -- ellipse_* with the approximate sqrt / rcp intrinsics, skip_threshold with the device's
// logf, exp_spec / exp_spec_floor / splat_power -- one trivial kernel per entry point that calls the header functions, nothing more.  Built with
// the product's flags into libradegs_blend_check.so (build.py), next to libradegs_sort_check.so; never part of libradegs_hip.so.  Loaded with
// ctypes by tests/test_gpu_stream_lists.py.  Plain device pointers and a stream; every call returns the hipError_t as an int; nothing synchronises.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rg_blend.h"

namespace {

constexpr int kThreads = 256;
inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

__global__ void __launch_bounds__(kThreads) block_masks_kernel(int n, const float* rec, float tx0, float ty0, uint32_t* mask) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float* r = rec + 6 * (size_t)i;
  mask[i] = rg::ellipse_block_mask(r[0], r[1], r[2], r[3], r[4], r[5], tx0, ty0);
}

// one workgroup per splat; every output position recovers its tile from its row-major number the way the emission does
__global__ void __launch_bounds__(kThreads) block_masks_rect_kernel(int n, const float* rec, const int* rect, const uint32_t* off, uint32_t* mask,
                                                                    uint32_t* tile_xy) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const float* r = rec + 6 * (size_t)i;
  const int x0 = rect[4 * i], y0 = rect[4 * i + 1], x1 = rect[4 * i + 2], y1 = rect[4 * i + 3];
  const int w = x1 - x0;
  const uint32_t total = (uint32_t)(w * (y1 - y0));
  const rg::EllipseSetup e = rg::ellipse_setup_rect(r[0], r[1], r[2], r[3], r[4], r[5], x0, y0, x1, y1);
  for (uint32_t local = threadIdx.x; local < total; local += kThreads) {
    RG_RECT_TILE_OF(local, w, tx, ty)
    mask[off[i] + local] = rg::ellipse_rect_tile_mask(e, r[0], r[1], x0, y0, tx, (int)ty);
    tile_xy[off[i] + local] = ((uint32_t)tx & 0xFFFFu) | (ty << 16);
  }
}

__global__ void __launch_bounds__(kThreads) exp_spec_bits_kernel(uint32_t first_bits, uint32_t count, uint32_t stride, uint32_t* out_spec,
                                                                 uint32_t* out_floor) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= count) return;
  const float x = __uint_as_float(first_bits + i * stride);
  out_spec[i] = __float_as_uint(rg::exp_spec(x));
  out_floor[i] = __float_as_uint(rg::exp_spec_floor(x));
}

__global__ void __launch_bounds__(kThreads) skip_thresholds_kernel(int n, const float* op, float* thr) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) thr[i] = rg::skip_threshold(op[i]);
}

__global__ void __launch_bounds__(kThreads) splat_powers_kernel(int n, const float* cx, const float* cy, const float* cz, const float* dx,
                                                                const float* dy, float* out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) out[i] = rg::splat_power((cx[i] * dx[i]) * dx[i], cy[i] * dx[i], cz[i], dy[i]);
}

// Brute-force truth: bit b is set when some pixel centre of block b of the 16x16 tile at (ox, oy) passes the forward blend loop's own test
// (power <= 0 and min(0.99, op exp_spec(power)) >= 1/255), evaluated as the kernels evaluate it.  rec: records of `stride` floats whose words
// 0..5 are mx, my, cx, cy, cz, op (a splat_a record: stride 16); pair i uses record gid[i] (record i when gid is null).
__global__ void __launch_bounds__(kThreads) truth_masks_kernel(int n, const float* rec, int stride, const uint32_t* gid, const float* ox,
                                                               const float* oy, uint32_t* out) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float* r = rec + (size_t)stride * (gid ? gid[i] : (uint32_t)i);
  const float mx = r[0], my = r[1], cx = r[2], cy = r[3], cz = r[4], op = r[5];
  uint32_t truth = 0u;
  for (int b = 0; b < 8; b++) {
    bool any = false;
    for (int py = 0; py < 4; py++)
      for (int px = 0; px < 8; px++) {
        const float dx = mx - (ox[i] + (float)((b & 1) * 8 + px)), dy = my - (oy[i] + (float)((b >> 1) * 4 + py));
        const float power = rg::splat_power((cx * dx) * dx, cy * dx, cz, dy);
        const float alpha = fminf(0.99f, op * rg::exp_spec(power));
        if (!(power > 0.0f) && !(alpha < 1.0f / 255.0f)) any = true;
      }
    if (any) truth |= 1u << b;
  }
  out[i] = truth;
}

}  // namespace

extern "C" {

int blendcheck_block_masks(int n, const float* rec, float tx0, float ty0, uint32_t* mask, void* stream) {
  if (n > 0) hipLaunchKernelGGL(block_masks_kernel, grid_for((size_t)n), dim3(kThreads), 0, (hipStream_t)stream, n, rec, tx0, ty0, mask);
  return (int)hipGetLastError();
}

// rect: [n][4] = x0, y0, x1, y1 in tiles; off: [n] first output position of each splat (exclusive prefix of its tile counts); mask / tile_xy: one
// word per (splat, tile), rows outer; tile_xy = tx | ty << 16, the tile (relative to the rectangle's origin) the kernel recovered for that position
int blendcheck_block_masks_rect(int n, const float* rec, const int* rect, const uint32_t* off, uint32_t* mask, uint32_t* tile_xy, void* stream) {
  if (n > 0) hipLaunchKernelGGL(block_masks_rect_kernel, dim3((unsigned)n), dim3(kThreads), 0, (hipStream_t)stream, n, rec, rect, off, mask, tile_xy);
  return (int)hipGetLastError();
}

int blendcheck_exp_spec_bits(uint32_t first_bits, uint32_t count, uint32_t stride, uint32_t* out_spec, uint32_t* out_floor, void* stream) {
  if (count > 0) hipLaunchKernelGGL(exp_spec_bits_kernel, grid_for(count), dim3(kThreads), 0, (hipStream_t)stream, first_bits, count, stride, out_spec, out_floor);
  return (int)hipGetLastError();
}

int blendcheck_skip_thresholds(int n, const float* op, float* thr, void* stream) {
  if (n > 0) hipLaunchKernelGGL(skip_thresholds_kernel, grid_for((size_t)n), dim3(kThreads), 0, (hipStream_t)stream, n, op, thr);
  return (int)hipGetLastError();
}

int blendcheck_splat_powers(int n, const float* cx, const float* cy, const float* cz, const float* dx, const float* dy, float* out, void* stream) {
  if (n > 0) hipLaunchKernelGGL(splat_powers_kernel, grid_for((size_t)n), dim3(kThreads), 0, (hipStream_t)stream, n, cx, cy, cz, dx, dy, out);
  return (int)hipGetLastError();
}

int blendcheck_truth_masks(int n, const float* rec, int stride, const uint32_t* gid, const float* ox, const float* oy, uint32_t* out, void* stream) {
  if (n > 0) hipLaunchKernelGGL(truth_masks_kernel, grid_for((size_t)n), dim3(kThreads), 0, (hipStream_t)stream, n, rec, stride, gid, ox, oy, out);
  return (int)hipGetLastError();
}

}  // extern "C"
