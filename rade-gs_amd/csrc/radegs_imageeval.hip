// radegs_imageeval.hip -- image-quality evaluation (include/radegs.h, "Image evaluation"): the 8-bit round trip of a saved
// render, the squared-difference sum behind PSNR, and LPIPS-VGG: thirteen 3x3 convolutions on the f32-input MFMA plus one tap kernel that
// forms a layer's LPIPS term and the 2x2 max pool in the same pass.  Built with the library's -ffp-contract=off: every fused multiply-add
// in here is either spelled fmaf() or is the MFMA, which is a k-ordered fmaf chain, so a convolution output is the chain of rg_conv_chain.h
// bit for bit.  Sums that cross threads go through rg_reduce.h's fixed-order tree; there is no float atomic in this file.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rg_conv_chain.h"
#include "rg_reduce.h"
#include "rg_workspace.h"

namespace rgie {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// ------------------------------------------------------------- conv3x3 + bias + ReLU, MFMA -------------------------------------------------------------
// Implicit GEMM, M = pixels, N = Cout, K = 9 Cin.  A block of 4 waves owns a 16x16 patch of output pixels of one image and 64 output
// channels; wave w owns rows 4w .. 4w+3 of the patch (two 32-pixel M tiles of 2 rows x 16 columns) and both 32-channel N tiles: four
// 32x32 accumulators, each started at the bias.  Per chunk of 16 input channels the block stages the 18x18 input patch (one-pixel halo,
// zeros outside the image) channel-major in LDS and the chunk's 9 x 16 x 64 weights, then walks tap by tap, two channels per
// v_mfma_f32_32x32x2_f32 (lane l feeds k = l >> 5): per output element the products arrive in the order of rgconv::term.
// LDS: 16 x 352 + 144 x 64 floats = 59 392 B.  kPlane = 352 puts the two k halves of an A read 32 banks apart; the B rows of odd k are
// rotated by 32 channels for the same reason.
constexpr int kCK = rgconv::kChunk;
constexpr int kTile = 16, kPW = kTile + 2, kPatch = kPW * kPW, kPlane = 352, kBN = 64;
constexpr int kWChunk = 9 * kCK * kBN;   // floats of one (Cout tile, chunk) block of the packed weights

__global__ __launch_bounds__(256) void conv3x3_mfma_kernel(int H, int W, int Cin, int Cout, int tilesX, int tilesY, const float* __restrict__ x,
                                                           const float* __restrict__ wp, const float* __restrict__ bias, float* __restrict__ y) {
  __shared__ float s_patch[kCK * kPlane];
  __shared__ float s_w[kWChunk];
  const int per_image = tilesX * tilesY;
  const int n = blockIdx.x / per_image, r = blockIdx.x - n * per_image, ty = r / tilesX, tx = r - ty * tilesX;
  const int cot = blockIdx.y, y0 = ty * kTile, x0 = tx * kTile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lk = lane >> 5;
  const size_t img = (size_t)n * H * W;

  f32x16 acc[2][2];
#pragma unroll
  for (int nt = 0; nt < 2; nt++) {
    const float b = bias[cot * kBN + nt * 32 + li];
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[mt][nt][e] = b;
  }
  // lane's A element: pixel li of M tile mt is row 4 wave + 2 mt + (li >> 4), column li & 15 of the patch; its k half picks the channel
  const int a_base = lk * kPlane + (wave * 4 + (li >> 4)) * kPW + (li & 15);
  const int b_col0 = (li + 32 * lk) & 63, b_col1 = (32 + li + 32 * lk) & 63;

  const int chunks = Cin / kCK;
  for (int c = 0; c < chunks; c++) {
    __syncthreads();   // the previous chunk's reads are done
    for (int i = threadIdx.x; i < kPatch * 4; i += 256) {
      const int p = i >> 2, q = i & 3, py = p / kPW, px = p - py * kPW, gy = y0 + py - 1, gx = x0 + px - 1;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const float4*>(x + (img + (size_t)gy * W + gx) * Cin + c * kCK + q * 4);
      float* d = s_patch + (q * 4) * kPlane + p;
      d[0] = v.x;
      d[kPlane] = v.y;
      d[2 * kPlane] = v.z;
      d[3 * kPlane] = v.w;
    }
    const float4* src = reinterpret_cast<const float4*>(wp + ((size_t)cot * chunks + c) * kWChunk);
    for (int i = threadIdx.x; i < kWChunk / 4; i += 256) {
      const int k = i >> 4, c4 = (i & 15) * 4;
      *reinterpret_cast<float4*>(s_w + k * kBN + ((c4 + 32 * (k & 1)) & 63)) = src[i];
    }
    __syncthreads();
    for (int tap = 0; tap < 9; tap++) {
      const int ky = tap / 3, kx = tap - ky * 3;
      const float* pa = s_patch + a_base + ky * kPW + kx;
      const float* pb = s_w + (tap * kCK + lk) * kBN;
#pragma unroll
      for (int kk = 0; kk < kCK / 2; kk++) {
        const float a0 = pa[2 * kk * kPlane], a1 = pa[2 * kk * kPlane + 2 * kPW];
        const float b0 = pb[2 * kk * kBN + b_col0], b1 = pb[2 * kk * kBN + b_col1];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
  }
  // C/D map of the 32x32 forms: column (channel) = lane & 31, row (pixel of the M tile) = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int mt = 0; mt < 2; mt++)
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const int m = (e & 3) + 8 * (e >> 2) + 4 * lk, gy = y0 + wave * 4 + mt * 2 + (m >> 4), gx = x0 + (m & 15);
      if (gy < H && gx < W) {
        float* o = y + (img + (size_t)gy * W + gx) * Cout + cot * kBN + li;
        o[0] = fmaxf(acc[mt][0][e], 0.f);
        o[32] = fmaxf(acc[mt][1][e], 0.f);
      }
    }
}

// ------------------------------------------------------- first layer: z-score + conv3x3 + bias + ReLU, VALU -------------------------------------------------------
// Cin = 3, K = 27: the same chain (one chunk of 3 channels: tap by tap, channels ascending) on the vector pipe.  The image is planar
// [N,3,H,W]; (x - mean) / std is applied as a pixel is loaded and a pixel outside the image is 0 AFTER normalisation.  A thread owns one
// pixel and 16 consecutive output channels of the block's 64.
__global__ __launch_bounds__(256) void conv3x3_first_kernel(long long pixels, int H, int W, int Cout, const float* __restrict__ image, float m0, float m1,
                                                            float m2, float s0, float s1, float s2, const float* __restrict__ wp,
                                                            const float* __restrict__ bias, float* __restrict__ y) {
  __shared__ float s_w[27 * kBN];
  __shared__ float s_b[kBN];
  const int cot = blockIdx.y;
  for (int i = threadIdx.x; i < 27 * kBN; i += 256) s_w[i] = wp[(size_t)(i >> 6) * Cout + cot * kBN + (i & 63)];
  if (threadIdx.x < kBN) s_b[threadIdx.x] = bias[cot * kBN + threadIdx.x];
  __syncthreads();
  const long long pix = (long long)blockIdx.x * 64 + (threadIdx.x >> 2);
  if (pix >= pixels) return;
  const long long hw = (long long)H * W;
  const long long n = pix / hw, rem = pix - n * hw;
  const int oy = (int)(rem / W), ox = (int)(rem - (long long)oy * W);
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
  float v[27];
#pragma unroll
  for (int tap = 0; tap < 9; tap++) {
    const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
    const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
    for (int ci = 0; ci < 3; ci++) v[tap * 3 + ci] = in ? (image[(n * 3 + ci) * hw + (long long)iy * W + ix] - mean[ci]) / stdv[ci] : 0.f;
  }
  const int cg = (threadIdx.x & 3) * 16;
  float out[16];
#pragma unroll
  for (int j = 0; j < 16; j++) {
    float acc = s_b[cg + j];
#pragma unroll
    for (int k = 0; k < 27; k++) acc = fmaf(v[k], s_w[k * kBN + cg + j], acc);
    out[j] = fmaxf(acc, 0.f);
  }
  float4* o = reinterpret_cast<float4*>(y + (size_t)pix * Cout + cot * kBN + cg);
#pragma unroll
  for (int j = 0; j < 4; j++) o[j] = make_float4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
}

// ------------------------------------------------------------------- LPIPS tap + 2x2 max pool -------------------------------------------------------------------
// One wave per 2x2 quad of full-resolution pixels (the quads of the last row / column of an odd size hold 2 or 1 pixels).  Lane l holds
// channels l, l + 64, ... of both images.  Per pixel: the two squared norms (per lane ascending j, then the xor butterfly 32, 16, .. 1, whose
// result is the same on every lane), n = sqrt(.) + 1e-10, and d = sum_c lin_c (fx_c / nx - fy_c / ny)^2 summed the same way; a pixel of
// zeros gives 0 / 1e-10 = 0.  The quad's d (pixels in row-major order, as doubles) goes to quad[q]; the running maxima are the pooled
// map, written only for a complete quad (floor on odd sizes).  The feature map is read once.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int J>
__global__ __launch_bounds__(256) void tap_kernel(int H, int W, const float* __restrict__ feat, const float* __restrict__ lin, float* __restrict__ pooled,
                                                  double* __restrict__ quad) {
  constexpr int C = 64 * J;
  const int lane = threadIdx.x & 63, QW = (W + 1) / 2, QH = (H + 1) / 2, PH = H / 2, PW = W / 2;
  const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= (long long)QW * QH) return;   // whole waves leave; no barrier below
  const int qy = (int)(q / QW), qx = (int)(q - (long long)qy * QW);
  const size_t image = (size_t)H * W * C;
  float l[J], mx[J], my[J];
#pragma unroll
  for (int j = 0; j < J; j++) l[j] = lin[j * 64 + lane];
  double s = 0.0;
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int py = 2 * qy + (p >> 1), px = 2 * qx + (p & 1);
    if (py >= H || px >= W) continue;
    const float* fx = feat + ((size_t)py * W + px) * C + lane;
    const float* fy = fx + image;
    float vx[J], vy[J], sx = 0.f, sy = 0.f;
#pragma unroll
    for (int j = 0; j < J; j++) {
      vx[j] = fx[j * 64];
      vy[j] = fy[j * 64];
      sx += vx[j] * vx[j];
      sy += vy[j] * vy[j];
      mx[j] = p == 0 ? vx[j] : fmaxf(mx[j], vx[j]);
      my[j] = p == 0 ? vy[j] : fmaxf(my[j], vy[j]);
    }
    const float nx = sqrtf(wave_sum(sx)) + 1e-10f, ny = sqrtf(wave_sum(sy)) + 1e-10f;
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < J; j++) {
      const float t = vx[j] / nx - vy[j] / ny;
      d += l[j] * (t * t);
    }
    s += (double)wave_sum(d);
  }
  if (lane == 0) quad[q] = s;
  if (pooled && 2 * qy + 1 < H && 2 * qx + 1 < W) {
    float* ox = pooled + ((size_t)qy * PW + qx) * C + lane;
    float* oy = ox + (size_t)PH * PW * C;
#pragma unroll
    for (int j = 0; j < J; j++) {
      ox[j * 64] = mx[j];
      oy[j * 64] = my[j];
    }
  }
}

// ------------------------------------------------------------------ the fixed-order sums ------------------------------------------------------------------
__global__ __launch_bounds__(256) void sum_partial_kernel(long long n, const double* __restrict__ v, double* __restrict__ partial) {
  __shared__ double sh[256];
  double a[1] = {0.0};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) a[0] += v[i];
  rg::block_sum<1>(a, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = a[0];
}

// each term is the reference's own float32 (a - b)^2; only the adding is wider
__global__ __launch_bounds__(256) void ssd_partial_kernel(long long n, const float* __restrict__ x, const float* __restrict__ y, double* __restrict__ partial) {
  __shared__ double sh[256];
  double a[1] = {0.0};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float d = x[i] - y[i];
    a[0] += (double)(d * d);
  }
  rg::block_sum<1>(a, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = a[0];
}

__global__ __launch_bounds__(256) void sum_final_kernel(int nblocks, const double* __restrict__ partial, double divisor, double* __restrict__ out) {
  __shared__ double sh[256];
  double a[1] = {0.0};
  rg::add_partials<1>(partial, nblocks, a);
  rg::block_sum<1>(a, sh);
  if (threadIdx.x == 0) out[0] = a[0] / divisor;
}

// ------------------------------------------------------------------------ 8-bit round trip ------------------------------------------------------------------------
// u8 = trunc(clamp(x * 255 + 0.5, 0, 255)), two roundings as the reference's mul().add_() has; NaN reads as 0.  x' = u8 / 255, IEEE divide.
__global__ __launch_bounds__(256) void quantize_kernel(long long hw, const float* __restrict__ image, unsigned char* __restrict__ u8, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float t = image[c * hw + i] * 255.0f;
    t = t + 0.5f;
    t = !(t >= 0.f) ? 0.f : (t > 255.f ? 255.f : t);
    const unsigned char b = (unsigned char)(int)t;
    if (u8) u8[i * 3 + c] = b;
    if (out) out[c * hw + i] = (float)b / 255.0f;
  }
}

struct TapWorkspace {
  double* quad;
  double* partial;
  size_t bytes;
};

TapWorkspace tap_layout(void* base, int H, int W) {
  rg::Carver c(base);
  TapWorkspace w;
  w.quad = c.take<double>((size_t)((H + 1) / 2) * ((W + 1) / 2));
  w.partial = c.take<double>(rg::kSumBlocks);
  w.bytes = c.off;
  return w;
}

struct SsdWorkspace {
  double* partial;
  size_t bytes;
};

SsdWorkspace ssd_layout(void* base) {
  rg::Carver c(base);
  SsdWorkspace w;
  w.partial = c.take<double>(rg::kSumBlocks);
  w.bytes = c.off;
  return w;
}

constexpr long long kMaxSide = 1 << 15;   // H, W: pixel and quad counts stay far inside 32-bit grids

inline bool conv_shape_ok(int N, int H, int W) { return N >= 1 && H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide && (long long)N * H * W <= (1ll << 31) - 64; }

}  // namespace rgie

extern "C" {

int radegs_imageeval_conv3x3(int N, int H, int W, int Cin, int Cout, const float* x, const float* packed_weight, const float* bias, float* y, void* stream) {
  if (!rgie::conv_shape_ok(N, H, W) || Cin < rgie::kCK || Cin % rgie::kCK || Cout < rgie::kBN || Cout % rgie::kBN) return RADEGS_ERR_INVALID_ARG;
  if (!x || !packed_weight || !bias || !y || !rg::aligned16(x) || !rg::aligned16(packed_weight)) return RADEGS_ERR_INVALID_ARG;
  const int tilesX = (W + rgie::kTile - 1) / rgie::kTile, tilesY = (H + rgie::kTile - 1) / rgie::kTile;
  hipLaunchKernelGGL(rgie::conv3x3_mfma_kernel, dim3((unsigned)(N * tilesX * tilesY), (unsigned)(Cout / rgie::kBN)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     H, W, Cin, Cout, tilesX, tilesY, x, packed_weight, bias, y);
  return rg::launch_status();
}

int radegs_imageeval_conv3x3_first(int N, int H, int W, int Cout, const float* image, const float* mean3, const float* std3, const float* packed_weight,
                                   const float* bias, float* y, void* stream) {
  if (!rgie::conv_shape_ok(N, H, W) || Cout < rgie::kBN || Cout % rgie::kBN) return RADEGS_ERR_INVALID_ARG;
  if (!image || !mean3 || !std3 || !packed_weight || !bias || !y || !rg::aligned16(y)) return RADEGS_ERR_INVALID_ARG;
  const long long pixels = (long long)N * H * W;
  hipLaunchKernelGGL(rgie::conv3x3_first_kernel, dim3((unsigned)((pixels + 63) / 64), (unsigned)(Cout / rgie::kBN)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     pixels, H, W, Cout, image, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], packed_weight, bias, y);
  return rg::launch_status();
}

size_t radegs_imageeval_tap_bytes(int H, int W) {
  if (H < 1 || W < 1 || H > rgie::kMaxSide || W > rgie::kMaxSide) return 0;
  return rgie::tap_layout(nullptr, H, W).bytes;
}

int radegs_imageeval_tap(int H, int W, int C, const float* feat, const float* lin, float* pooled, void* workspace, size_t workspace_bytes, double* out,
                         void* stream) {
  if (H < 1 || W < 1 || H > rgie::kMaxSide || W > rgie::kMaxSide || (C != 64 && C != 128 && C != 256 && C != 512)) return RADEGS_ERR_INVALID_ARG;
  if (!feat || !lin || !out || !workspace || !rg::aligned16(workspace) || workspace_bytes < radegs_imageeval_tap_bytes(H, W)) return RADEGS_ERR_INVALID_ARG;
  if (pooled && (H < 2 || W < 2)) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const rgie::TapWorkspace w = rgie::tap_layout(workspace, H, W);
  const long long quads = (long long)((H + 1) / 2) * ((W + 1) / 2);
  const dim3 grid((unsigned)((quads + 3) / 4)), block(256);
  switch (C) {
    case 64: hipLaunchKernelGGL(rgie::tap_kernel<1>, grid, block, 0, s, H, W, feat, lin, pooled, w.quad); break;
    case 128: hipLaunchKernelGGL(rgie::tap_kernel<2>, grid, block, 0, s, H, W, feat, lin, pooled, w.quad); break;
    case 256: hipLaunchKernelGGL(rgie::tap_kernel<4>, grid, block, 0, s, H, W, feat, lin, pooled, w.quad); break;
    default: hipLaunchKernelGGL(rgie::tap_kernel<8>, grid, block, 0, s, H, W, feat, lin, pooled, w.quad); break;
  }
  const int nb = rg::sum_blocks(quads);
  hipLaunchKernelGGL(rgie::sum_partial_kernel, dim3(nb), dim3(256), 0, s, quads, w.quad, w.partial);
  hipLaunchKernelGGL(rgie::sum_final_kernel, dim3(1), dim3(256), 0, s, nb, w.partial, (double)H * (double)W, out);
  return rg::launch_status();
}

int radegs_imageeval_quantize(int H, int W, const float* image, unsigned char* u8, float* out, void* stream) {
  if (H < 1 || W < 1 || H > rgie::kMaxSide || W > rgie::kMaxSide || !image || (!u8 && !out)) return RADEGS_ERR_INVALID_ARG;
  const long long hw = (long long)H * W;
  hipLaunchKernelGGL(rgie::quantize_kernel, dim3(rg::blocks_of((size_t)hw)), dim3(256), 0, static_cast<hipStream_t>(stream), hw, image, u8, out);
  return rg::launch_status();
}

size_t radegs_imageeval_ssd_bytes(void) { return rgie::ssd_layout(nullptr).bytes; }

int radegs_imageeval_ssd(long long n, const float* a, const float* b, void* workspace, size_t workspace_bytes, double* out, void* stream) {
  if (n < 1 || !a || !b || !out || !workspace || !rg::aligned16(workspace) || workspace_bytes < radegs_imageeval_ssd_bytes()) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const rgie::SsdWorkspace w = rgie::ssd_layout(workspace);
  const int nb = rg::sum_blocks(n);
  hipLaunchKernelGGL(rgie::ssd_partial_kernel, dim3(nb), dim3(256), 0, s, n, a, b, w.partial);
  hipLaunchKernelGGL(rgie::sum_final_kernel, dim3(1), dim3(256), 0, s, nb, w.partial, 1.0, out);
  return rg::launch_status();
}

}  // extern "C"
