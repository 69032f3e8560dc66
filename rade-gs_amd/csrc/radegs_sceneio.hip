// radegs_sceneio.hip -- a decoded photograph on its way to a training camera: what utils/camera_utils.py loadCam,
// utils/general_utils.py PILtoTorch, scene/dataset_readers.py:270-276 and scene/cameras.py:59-68 do per image on one host thread.
// Four kernels: A the horizontal pass of Pillow's 8-bit antialiased bicubic resize, B its vertical pass fused with the / 255 table and
// the turn to planar float32, C the Blender RGBA composite, D the edge map.  A, B and C are integer / table work and reproduce the
// host's bytes; include/radegs.h, "Scene ingestion", is the specification and tests/scene_io_restatement.py restates it in NumPy.
// The coefficient tables come from the host (rade-gs_amd/scene_io.py, float64): no kernel here computes a filter weight.
// Built with build.py's default FLAGS (-ffp-contract=off): kernel C's float64 products round once each, as NumPy's do.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rg_workspace.h"

namespace rgsio {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRound = 1 << (RADEGS_SCENEIO_PRECISION_BITS - 1);

__device__ __forceinline__ int clip8(int v) { return min(max(v >> RADEGS_SCENEIO_PRECISION_BITS, 0), 255); }   // >> of an int is arithmetic

// ---- A: horizontal pass ---------------------------------------------------------------------------------------------------------
// A workgroup takes 64 consecutive output pixels of kWaves consecutive rows, one wave per row.  The source bytes those pixels read
// are one span per row, bounds[x0].xmin .. bounds[x1 - 1].xmin + n (xmin and xmin + n do not decrease along a table); the span is
// staged in LDS at the row's own phase within a dword: the bytes before the first whole dword and after the last one are moved one
// by one, the dwords between as dwords, so no load touches a byte outside [first, last) of the row.  Then lane l owns pixel x0 + l:
// its coefficients are column x0 + l of the transposed table [ksize, out] (consecutive lanes, consecutive ints).
template <int C>
__global__ void __launch_bounds__(kThreads) horizontal_kernel(int rows, int row_first, int W, int Wout, int ksize, int max_span, int lds_row_words,
                                                              const uint8_t* __restrict__ src, const int* __restrict__ bounds,
                                                              const int* __restrict__ kkT, uint8_t* __restrict__ dst) {
  extern __shared__ __align__(16) uint32_t lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = blockIdx.x * 64, x1 = min(x0 + 64, Wout);
  const int r = blockIdx.y * kWaves + wave;                 // row of the output; row_first + r of the source
  const int span0 = bounds[2 * x0], span1 = bounds[2 * (x1 - 1)] + bounds[2 * (x1 - 1) + 1];     // source pixels [span0, span1), within [0, W]
  uint32_t* row = lds + wave * lds_row_words;
  if (span1 - span0 > max_span) return;                     // workgroup-uniform; the host's max_span sized the LDS rows
  const bool live = r < rows;                               // wave-uniform
  long long base = 0, a0 = 0;
  uint8_t* row8 = reinterpret_cast<uint8_t*>(row);
  if (live) {
    base = ((long long)(row_first + r) * W) * C;                                    // the row's first byte in src
    const long long b0 = base + (long long)span0 * C, b1 = base + (long long)span1 * C;
    a0 = b0 & ~3LL;                                          // LDS byte i holds source byte a0 + i
    const long long body0 = min((b0 + 3) & ~3LL, b1), body1 = max(b1 & ~3LL, body0);
    for (long long b = b0 + lane; b < body0; b += 64) row8[b - a0] = src[b];                       // head: at most 3 bytes
    const uint32_t* src32 = reinterpret_cast<const uint32_t*>(src);                               // src is 4-byte aligned (checked)
    for (long long q = (body0 >> 2) + lane; q < (body1 >> 2); q += 64) row[q - (a0 >> 2)] = src32[q];
    for (long long b = body1 + lane; b < b1; b += 64) row8[b - a0] = src[b];                       // tail: at most 3 bytes
  }
  __syncthreads();
  if (live) {
    const int xx = x0 + lane;
    if (xx < x1) {
      const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
      int acc[C];
#pragma unroll
      for (int c = 0; c < C; c++) acc[c] = kRound;
      const uint8_t* p = row8 + ((base + (long long)xmin * C) - a0);
      for (int k = 0; k < n; k++) {
        const int w = kkT[(long long)k * Wout + xx];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] += (int)p[k * C + c] * w;
      }
      uint8_t* o = dst + ((long long)r * Wout + xx) * C;
#pragma unroll
      for (int c = 0; c < C; c++) o[c] = (uint8_t)clip8(acc[c]);
    }
  }
}

// ---- B: vertical pass and finish ---------------------------------------------------------------------------------------------------
// A lane owns an output pixel of row yy (blockIdx.y): the taps' rows ymin .. ymin + n and their coefficients kk[yy][.] are the same
// for the whole wave (scalar loads), and a wave reads 64 C consecutive bytes of each tap row.  kk == nullptr: the axis keeps its
// size, the byte is taken as it is.  The byte goes to out_u8 [Hout, W, C] (resize_u8) and / or through lut[256] to the planes:
// channel c < 3 to image + c Hout W, channel 3 (and nothing else) to mask; every float store of a wave is 256 consecutive bytes.
template <int C>
__global__ void __launch_bounds__(kThreads) vertical_kernel(int rows_in, int row_first, int W, int Hout, int ksize, const uint8_t* __restrict__ mid,
                                                            const int* __restrict__ bounds, const int* __restrict__ kk,
                                                            const float* __restrict__ lut, uint8_t* __restrict__ out_u8,
                                                            float* __restrict__ image, float* __restrict__ mask) {
  const int x = blockIdx.x * kThreads + threadIdx.x, yy = blockIdx.y;
  if (x >= W) return;
  int v[C];
  if (kk) {
    const int ymin = bounds[2 * yy] - row_first, n = bounds[2 * yy + 1];        // rows of mid: [ymin, ymin + n)
    if (ymin < 0 || n < 0 || ymin + n > rows_in) return;                          // wave-uniform; a table that leaves mid reads and writes nothing
    const int* w = kk + (long long)yy * ksize;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = kRound;
    for (int k = 0; k < n; k++) {
      const uint8_t* p = mid + ((long long)(ymin + k) * W + x) * C;
      const int wk = w[k];
#pragma unroll
      for (int c = 0; c < C; c++) acc[c] += (int)p[c] * wk;
    }
#pragma unroll
    for (int c = 0; c < C; c++) v[c] = clip8(acc[c]);
  } else {
    const uint8_t* p = mid + ((long long)(yy - row_first) * W + x) * C;
#pragma unroll
    for (int c = 0; c < C; c++) v[c] = p[c];
  }
  const long long pix = (long long)yy * W + x, plane = (long long)Hout * W;
  if (out_u8) {
#pragma unroll
    for (int c = 0; c < C; c++) out_u8[pix * C + c] = (uint8_t)v[c];
  }
  if (image) {
#pragma unroll
    for (int c = 0; c < C && c < 3; c++) image[c * plane + pix] = lut[v[c]];
    if (C == 4) mask[pix] = lut[v[C - 1]];
  }
}

// ---- C: Blender composite (dataset_readers.py:270-276) ---------------------------------------------------------------------------
// float64, one rounding per operation: a = A / 255.0, v = (c / 255.0) a + bg (1 - a), byte = trunc(v 255.0) & 0xFF (NumPy's cast of a
// float64 to np.byte on the hosts upstream runs on).  A thread takes four pixels: one 16-byte load, three dword stores; the last
// pixels of an image whose count is no multiple of four are stored byte by byte.
__device__ __forceinline__ uint32_t composite1(uint32_t rgba, double bg) {
  const double a = (double)(rgba >> 24) / 255.0, rest = bg * (1.0 - a);
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double v = ((double)((rgba >> (8 * c)) & 255u) / 255.0) * a + rest;
    out |= ((uint32_t)(int)(v * 255.0) & 255u) << (8 * c);
  }
  return out;
}

__global__ void __launch_bounds__(kThreads) composite_kernel(long long N, const uint32_t* __restrict__ rgba, double bg, uint8_t* __restrict__ rgb) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x, p0 = 4 * g;
  if (p0 >= N) return;
  if (p0 + 4 <= N) {
    const uint4 in = reinterpret_cast<const uint4*>(rgba)[g];
    const uint32_t a = composite1(in.x, bg), b = composite1(in.y, bg), c = composite1(in.z, bg), d = composite1(in.w, bg);
    uint32_t* o = reinterpret_cast<uint32_t*>(rgb) + 3 * g;
    o[0] = a | (b << 24);
    o[1] = (b >> 8) | (c << 16);
    o[2] = (c >> 16) | (d << 8);
  } else {
    for (long long p = p0; p < N; p++) {
      const uint32_t v = composite1(rgba[p], bg);
      rgb[3 * p] = (uint8_t)v; rgb[3 * p + 1] = (uint8_t)(v >> 8); rgb[3 * p + 2] = (uint8_t)(v >> 16);
    }
  }
}

// ---- D: edge map (cameras.py:59-68) ------------------------------------------------------------------------------------------------
// A workgroup takes a tile of kEdgeW x kEdgeH pixels and stages it with a one-pixel halo, every channel, in LDS: each image row is
// read from memory once per tile column.  Interior pixel: for each of left, right, top, bottom the mean over the channels of
// |centre - neighbour|, the largest of the four, exp(-.), in float64 and rounded to float32 once (upstream's float32 chain carries
// about one more unit of 2^-24; the kernel runs once per image at load time); the image's one-pixel border is 0.
constexpr int kEdgeW = 64, kEdgeH = 16, kEdgePitch = kEdgeW + 2;

__global__ void __launch_bounds__(kThreads) edge_kernel(int Cn, int H, int W, const float* __restrict__ image, float* __restrict__ edge) {
  __shared__ float tile[3 * (kEdgeH + 2) * kEdgePitch];
  const int x0 = blockIdx.x * kEdgeW, y0 = blockIdx.y * kEdgeH;
  const long long plane = (long long)H * W;
  for (int i = threadIdx.x; i < Cn * (kEdgeH + 2) * kEdgePitch; i += kThreads) {
    const int c = i / ((kEdgeH + 2) * kEdgePitch), rem = i - c * (kEdgeH + 2) * kEdgePitch, ty = rem / kEdgePitch, tx = rem - ty * kEdgePitch;
    const int x = x0 + tx - 1, y = y0 + ty - 1;
    tile[i] = (x >= 0 && x < W && y >= 0 && y < H) ? image[c * plane + (long long)y * W + x] : 0.0f;
  }
  __syncthreads();
  const int tx = threadIdx.x & 63, x = x0 + tx;
  if (x >= W) return;
  for (int ty = threadIdx.x >> 6; ty < kEdgeH; ty += kWaves) {
    const int y = y0 + ty;
    if (y >= H) break;
    float out = 0.0f;
    if (x > 0 && x < W - 1 && y > 0 && y < H - 1) {
      double l = 0.0, r = 0.0, t = 0.0, b = 0.0;          // float64: the differences are exact, the result is rounded once
      for (int c = 0; c < Cn; c++) {
        const float* p = tile + (c * (kEdgeH + 2) + ty + 1) * kEdgePitch + tx + 1;
        const double v = p[0];
        l += fabs(v - (double)p[-1]); r += fabs(v - (double)p[1]); t += fabs(v - (double)p[-kEdgePitch]); b += fabs(v - (double)p[kEdgePitch]);
      }
      const double n = (double)Cn;
      out = (float)exp(-fmax(fmax(l / n, r / n), fmax(t / n, b / n)));
    }
    edge[(long long)y * W + x] = out;
  }
}

inline bool misaligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

template <int C>
int resize_c(int H, int W, int Hout, int Wout, const uint8_t* src, const RadegsSceneioTable* th, const RadegsSceneioTable* tv, int row_first, int rows_mid,
             uint8_t* mid, const float* lut, uint8_t* out_u8, float* image, float* mask, hipStream_t stream) {
  const uint8_t* vin = src;
  if (th) {
    const int lds_row_words = (th->max_span * C + 3) / 4 + 2;          // the span's bytes at any phase within a dword
    const size_t lds = (size_t)kWaves * lds_row_words * 4;
    if (lds > 64 * 1024) return RADEGS_ERR_TOO_LARGE;
    hipLaunchKernelGGL(horizontal_kernel<C>, dim3((Wout + 63) / 64, (rows_mid + kWaves - 1) / kWaves), dim3(kThreads), lds, stream, rows_mid, row_first, W,
                       Wout, th->ksize, th->max_span, lds_row_words, src, th->bounds, th->kk, mid);
    if (hipGetLastError() != hipSuccess) return RADEGS_ERR_HIP;
    vin = mid;
  } else {
    row_first = 0;                                                       // the vertical pass reads the source itself
    rows_mid = H;
  }
  hipLaunchKernelGGL(vertical_kernel<C>, dim3((Wout + kThreads - 1) / kThreads, Hout), dim3(kThreads), 0, stream, rows_mid, row_first, Wout, Hout,
                     tv ? tv->ksize : 0, vin, tv ? tv->bounds : nullptr, tv ? tv->kk : nullptr, lut, out_u8, image, mask);
  return rg::launch_status();
}

}  // namespace rgsio

extern "C" {

int radegs_sceneio_resize(int H, int W, int C, int Hout, int Wout, const unsigned char* src, const RadegsSceneioTable* horizontal,
                          const RadegsSceneioTable* vertical, int row_first, int rows_mid, unsigned char* mid, const float* lut,
                          unsigned char* out_u8, float* image, float* mask, void* stream) {
  if (H < 1 || W < 1 || Hout < 1 || Wout < 1 || (C != 1 && C != 3 && C != 4) || Hout > 65535) return RADEGS_ERR_INVALID_ARG;
  if ((long long)H * W * C > 0x7fffffffLL || (long long)Hout * Wout * C > 0x7fffffffLL) return RADEGS_ERR_TOO_LARGE;
  if (!src || rgsio::misaligned(src, 4) || (!out_u8 && !image) || (image && !lut) || (image && C == 4 && !mask)) return RADEGS_ERR_INVALID_ARG;
  if ((horizontal == nullptr) != (W == Wout) || (vertical == nullptr) != (H == Hout)) return RADEGS_ERR_INVALID_ARG;
  if (horizontal) {
    const RadegsSceneioTable* t = horizontal;
    if (!t->bounds || !t->kk || t->in_size != W || t->out_size != Wout || t->ksize < 1 || t->max_span < 1 || t->max_span > W || !mid)
      return RADEGS_ERR_INVALID_ARG;
    if (row_first < 0 || rows_mid < 1 || row_first + rows_mid > H || (rows_mid + 3) / 4 > 65535) return RADEGS_ERR_INVALID_ARG;
    if (!vertical && (row_first != 0 || rows_mid != H)) return RADEGS_ERR_INVALID_ARG;
  }
  if (vertical) {
    const RadegsSceneioTable* t = vertical;
    if (!t->bounds || !t->kk || t->in_size != H || t->out_size != Hout || t->ksize < 1) return RADEGS_ERR_INVALID_ARG;
    if (horizontal && (t->first != row_first || t->last != row_first + rows_mid)) return RADEGS_ERR_INVALID_ARG;   // mid holds what the table reads
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (C == 1) return rgsio::resize_c<1>(H, W, Hout, Wout, src, horizontal, vertical, row_first, rows_mid, mid, lut, out_u8, image, mask, s);
  if (C == 3) return rgsio::resize_c<3>(H, W, Hout, Wout, src, horizontal, vertical, row_first, rows_mid, mid, lut, out_u8, image, mask, s);
  return rgsio::resize_c<4>(H, W, Hout, Wout, src, horizontal, vertical, row_first, rows_mid, mid, lut, out_u8, image, mask, s);
}

int radegs_sceneio_composite(long long N, const unsigned char* rgba, int white_background, unsigned char* rgb, void* stream) {
  if (N < 0) return RADEGS_ERR_INVALID_ARG;
  if (N == 0) return 0;
  if (!rgba || !rgb || rgsio::misaligned(rgba, 16) || rgsio::misaligned(rgb, 4)) return RADEGS_ERR_INVALID_ARG;
  const long long blocks = ((N + 3) / 4 + rgsio::kThreads - 1) / rgsio::kThreads;
  if (blocks > 0x7fffffffLL) return RADEGS_ERR_TOO_LARGE;
  hipLaunchKernelGGL(rgsio::composite_kernel, dim3((unsigned)blocks), dim3(rgsio::kThreads), 0, static_cast<hipStream_t>(stream), N,
                     reinterpret_cast<const uint32_t*>(rgba), white_background ? 1.0 : 0.0, rgb);
  return rg::launch_status();
}

int radegs_sceneio_edge(int C, int H, int W, const float* image, float* edge, void* stream) {
  if ((C != 1 && C != 3) || H < 1 || W < 1 || !image || !edge) return RADEGS_ERR_INVALID_ARG;
  if ((H + rgsio::kEdgeH - 1) / rgsio::kEdgeH > 65535) return RADEGS_ERR_TOO_LARGE;
  hipLaunchKernelGGL(rgsio::edge_kernel, dim3((W + rgsio::kEdgeW - 1) / rgsio::kEdgeW, (H + rgsio::kEdgeH - 1) / rgsio::kEdgeH), dim3(rgsio::kThreads), 0,
                     static_cast<hipStream_t>(stream), C, H, W, image, edge);
  return rg::launch_status();
}

}  // extern "C"
