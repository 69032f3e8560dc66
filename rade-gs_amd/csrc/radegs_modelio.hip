// radegs_modelio.hip -- the Gaussian model's state on its way to and from a file: the record buffer of
// GaussianModel.save_ply / load_ply (scene/gaussian_model.py:379-397, 515-559), reset_opacity (495-513) and the part of
// create_from_pcd after the kNN step (301-328).  Four streaming kernels, each one pass, no atomics, every loop bound a
// launch argument; include/radegs.h, "Model state", is the specification.  Built without fast-math and with
// -ffp-contract=off (build.py's default FLAGS): divisions and square roots are IEEE, every product rounds once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radegs.h"

namespace rgio {

constexpr int kTile = 64;        // rows per workgroup: 64 S bytes is a multiple of 4 for every record size S
constexpr int kThreads = 256;

// ---- pack: the seven tensors -> [rows, C] float32 records in file order -------------------------------------------------
// A tile's share of every source is contiguous (64 w floats from row0 w), so each is read with consecutive lanes on
// consecutive dwords and written to its columns of an LDS image of the output tile; f_rest's [K,3] -> [3,K] turn is that
// write address.  The image is then stored as it lies: 64 C floats, contiguous and 256-byte aligned in the output.
__device__ __forceinline__ void stage(float* tile, int C, int col, const float* __restrict__ src, long long row0, int n, int w) {
  const float* s = src + row0 * w;
  for (int i = threadIdx.x; i < n * w; i += kThreads) tile[(i / w) * C + col + i % w] = s[i];
}

__global__ void __launch_bounds__(kThreads) pack_kernel(long long row_begin, long long row_end, int K, int C, const float* __restrict__ xyz,
                                                        const float* __restrict__ f_dc, const float* __restrict__ f_rest,
                                                        const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                        const float* __restrict__ rotation, const float* __restrict__ filter_3D,
                                                        float* __restrict__ out) {
  extern __shared__ __align__(16) float tile[];
  const long long row0 = row_begin + (long long)blockIdx.x * kTile;
  const int n = (int)min((long long)kTile, row_end - row0);
  const int w = 3 * K, c_op = 9 + w;
  stage(tile, C, 0, xyz, row0, n, 3);
  for (int i = threadIdx.x; i < n * 3; i += kThreads) tile[(i / 3) * C + 3 + i % 3] = 0.0f;      // nx ny nz
  stage(tile, C, 6, f_dc, row0, n, 3);
  {
    const float* s = f_rest + row0 * w;
    for (int i = threadIdx.x; i < n * w; i += kThreads) {
      const int r = i / w, e = i - r * w, k = e / 3, c = e - 3 * k;
      tile[r * C + 9 + c * K + k] = s[i];                                                         // f_rest_{c K + k} = rest[k][c]
    }
  }
  stage(tile, C, c_op, opacity, row0, n, 1);
  stage(tile, C, c_op + 1, scaling, row0, n, 3);
  stage(tile, C, c_op + 4, rotation, row0, n, 4);
  if (filter_3D) stage(tile, C, c_op + 8, filter_3D, row0, n, 1);
  __syncthreads();
  float* o = out + (row0 - row_begin) * C;              // kTile C floats = 256 C bytes per tile: 16-byte stores stay aligned
  const int total = n * C, quads = total >> 2;
  for (int i = threadIdx.x; i < quads; i += kThreads) reinterpret_cast<float4*>(o)[i] = reinterpret_cast<const float4*>(tile)[i];
  for (int i = 4 * quads + threadIdx.x; i < total; i += kThreads) o[i] = tile[i];                // the last tile's odd floats
}

// ---- unpack: P records of S bytes -> float32 values at their final places -------------------------------------------------
struct Column { float* dst; long long dst_stride; int dst_elem; int src_offset; int src_type; int scale; };     // = RadegsModelioColumn
static_assert(sizeof(Column) == sizeof(RadegsModelioColumn) && sizeof(Column) == 32, "descriptor layout");

__device__ __forceinline__ uint32_t bytes4(const uint32_t* lds, int a) {       // the 4 bytes at byte address a, any alignment
  const int q = a >> 2;
  const uint64_t two = ((uint64_t)lds[q + 1] << 32) | lds[q];
  return (uint32_t)(two >> (8 * (a & 3)));
}

__global__ void __launch_bounds__(kThreads) unpack_kernel(long long P, int S, const uint32_t* __restrict__ records, int D, int log2_lanes,
                                                          const Column* __restrict__ columns) {
  extern __shared__ __align__(16) uint32_t lds[];
  const long long row0 = (long long)blockIdx.x * kTile;
  const int n = (int)min((long long)kTile, P - row0);
  const int words = (n * S + 3) >> 2;                    // the tile starts on a dword: 64 S is a multiple of 4
  Column* cols = reinterpret_cast<Column*>(lds);
  uint32_t* img = lds + 8 * D;
  {
    const uint32_t* c32 = reinterpret_cast<const uint32_t*>(columns);
    for (int i = threadIdx.x; i < 8 * D; i += kThreads) lds[i] = c32[i];
    const uint32_t* src = records + (row0 * S >> 2);
    for (int i = threadIdx.x; i < words; i += kThreads) img[i] = src[i];
    if (threadIdx.x < 3) img[words + threadIdx.x] = 0;   // bytes4's second word and the third of an f8 at the tile's end
  }
  __syncthreads();
  // a wave takes 64 >> log2_lanes rows at a time, 1 << log2_lanes lanes per row, lanes along the descriptors: the host
  // orders them by destination, so consecutive lanes store to consecutive floats
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lanes = 1 << log2_lanes, rows_per_wave = 64 >> log2_lanes;
  for (int rb = wave * rows_per_wave; rb < n; rb += (kThreads / 64) * rows_per_wave) {
    const int r = rb + (lane >> log2_lanes);
    if (r >= n) continue;
    for (int d = lane & (lanes - 1); d < D; d += lanes) {
      const Column c = cols[d];
      const int size = (unsigned)c.src_type < 8u ? (0x84442211u >> (4 * c.src_type)) & 15 : 0;
      if (size == 0 || c.src_offset < 0 || c.src_offset + size > S) continue;      // a descriptor outside the record reads nothing
      const int a = r * S + c.src_offset;
      const uint32_t lo = bytes4(img, a);
      float* dst = c.dst + (row0 + r) * c.dst_stride + c.dst_elem;
      if (c.src_type == RADEGS_MODELIO_F4 && !c.scale) { *dst = __uint_as_float(lo); continue; }     // the bits as they are, NaN payloads too
      double v;
      switch (c.src_type) {
        case RADEGS_MODELIO_I1: v = (double)(int8_t)lo; break;
        case RADEGS_MODELIO_U1: v = (double)(uint8_t)lo; break;
        case RADEGS_MODELIO_I2: v = (double)(int16_t)lo; break;
        case RADEGS_MODELIO_U2: v = (double)(uint16_t)lo; break;
        case RADEGS_MODELIO_I4: v = (double)(int32_t)lo; break;
        case RADEGS_MODELIO_U4: v = (double)lo; break;
        case RADEGS_MODELIO_F4: v = (double)__uint_as_float(lo); break;
        default: v = __longlong_as_double((long long)(((uint64_t)bytes4(img, a + 4) << 32) | lo)); break;   // F8
      }
      if (c.scale) v = v / 255.0;
      *dst = (float)v;                                   // round to nearest even, once
    }
  }
}

// ---- reset_opacity (gaussian_model.py:495-513), upstream's operations in upstream's order ---------------------------------
__global__ void __launch_bounds__(kThreads) reset_opacity_kernel(long long P, const float* __restrict__ opacity_raw, const float* __restrict__ scaling_raw,
                                                                 const float* __restrict__ filter_3D, float* __restrict__ out, float* __restrict__ zero_a,
                                                                 float* __restrict__ zero_b) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= P) return;
  const float f = filter_3D[i], f2 = f * f;
  const float s0 = expf(scaling_raw[3 * i]), s1 = expf(scaling_raw[3 * i + 1]), s2 = expf(scaling_raw[3 * i + 2]);
  const float q0 = s0 * s0, q1 = s1 * s1, q2 = s2 * s2;
  const float det1 = (q0 * q1) * q2, det2 = ((q0 + f2) * (q1 + f2)) * (q2 + f2);
  const float coef = sqrtf(det1 / det2);
  const float sig = 1.0f / (1.0f + expf(-opacity_raw[i]));
  const float cur = sig * coef;
  const float x = (cur != cur ? cur : fminf(cur, 0.01f)) / coef;           // torch.min passes a NaN on
  out[i] = logf(x / (1.0f - x));
  if (zero_a) zero_a[i] = 0.0f;
  if (zero_b) zero_b[i] = 0.0f;
}

// ---- create_from_pcd after the kNN step (gaussian_model.py:305-320) ----------------------------------------------------------
__global__ void __launch_bounds__(kThreads) init_kernel(long long P, int K, const float* __restrict__ colors, const float* __restrict__ dist2,
                                                        float opacity_value, float* __restrict__ f_dc, float* __restrict__ f_rest,
                                                        float* __restrict__ opacity, float* __restrict__ scaling, float* __restrict__ rotation) {
  const long long row0 = (long long)blockIdx.x * kThreads;
  const int n = (int)min((long long)kThreads, P - row0);
  for (int j = threadIdx.x; j < n * 3; j += kThreads) f_dc[row0 * 3 + j] = (colors[row0 * 3 + j] - 0.5f) / 0.28209479177387814f;
  {
    float* z = f_rest + row0 * 3 * K;                    // the block's rows are one contiguous stretch
    for (int j = threadIdx.x; j < n * 3 * K; j += kThreads) z[j] = 0.0f;
  }
  if ((int)threadIdx.x < n) {
    const long long i = row0 + threadIdx.x;
    const float s = logf(sqrtf(fmaxf(dist2[i], 0.0000001f)));
    opacity[i] = opacity_value;
    scaling[3 * i] = s; scaling[3 * i + 1] = s; scaling[3 * i + 2] = s;
    reinterpret_cast<float4*>(rotation)[i] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
  }
}

inline bool launched() { return hipGetLastError() == hipSuccess; }
inline bool misaligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace rgio

extern "C" {

int radegs_modelio_pack(long long P, long long row_begin, long long row_end, int K, const float* xyz, const float* f_dc, const float* f_rest,
                        const float* opacity, const float* scaling, const float* rotation, const float* filter_3D, float* out, void* stream) {
  if (P < 0 || row_begin < 0 || row_end < row_begin || row_end > P || K < 0 || K > RADEGS_MODELIO_MAX_REST) return RADEGS_ERR_INVALID_ARG;
  if (row_end == row_begin) return 0;
  if (!xyz || !f_dc || (K > 0 && !f_rest) || !opacity || !scaling || !rotation || !out || rgio::misaligned(out, 16)) return RADEGS_ERR_INVALID_ARG;
  const int C = 17 + 3 * K + (filter_3D ? 1 : 0);
  const long long tiles = (row_end - row_begin + rgio::kTile - 1) / rgio::kTile;
  if (tiles > 0x7fffffffLL) return RADEGS_ERR_TOO_LARGE;
  hipLaunchKernelGGL(rgio::pack_kernel, dim3((unsigned)tiles), dim3(rgio::kThreads), (size_t)rgio::kTile * C * sizeof(float), static_cast<hipStream_t>(stream),
                     row_begin, row_end, K, C, xyz, f_dc, f_rest, opacity, scaling, rotation, filter_3D, out);
  return rgio::launched() ? 0 : RADEGS_ERR_HIP;
}

int radegs_modelio_unpack(long long P, int S, const void* records, int D, const RadegsModelioColumn* columns, void* stream) {
  if (P < 0 || S < 1 || S > RADEGS_MODELIO_MAX_RECORD || D < 0 || D > RADEGS_MODELIO_MAX_COLUMNS) return RADEGS_ERR_INVALID_ARG;
  if (P == 0 || D == 0) return 0;
  if (!records || !columns || rgio::misaligned(records, 4) || rgio::misaligned(columns, 16)) return RADEGS_ERR_INVALID_ARG;
  const long long tiles = (P + rgio::kTile - 1) / rgio::kTile;
  if (tiles > 0x7fffffffLL) return RADEGS_ERR_TOO_LARGE;
  int log2_lanes = 0;
  while (log2_lanes < 6 && (1 << log2_lanes) < D) log2_lanes++;
  const size_t lds = (size_t)D * sizeof(rgio::Column) + (size_t)rgio::kTile * S + 16;
  hipLaunchKernelGGL(rgio::unpack_kernel, dim3((unsigned)tiles), dim3(rgio::kThreads), lds, static_cast<hipStream_t>(stream), P, S,
                     static_cast<const uint32_t*>(records), D, log2_lanes, reinterpret_cast<const rgio::Column*>(columns));
  return rgio::launched() ? 0 : RADEGS_ERR_HIP;
}

int radegs_modelio_reset_opacity(long long P, const float* opacity_raw, const float* scaling_raw, const float* filter_3D, float* opacity_out,
                                 float* zero_a, float* zero_b, void* stream) {
  if (P < 0) return RADEGS_ERR_INVALID_ARG;
  if (P == 0) return 0;
  if (!opacity_raw || !scaling_raw || !filter_3D || !opacity_out) return RADEGS_ERR_INVALID_ARG;
  const long long blocks = (P + rgio::kThreads - 1) / rgio::kThreads;
  if (blocks > 0x7fffffffLL) return RADEGS_ERR_TOO_LARGE;
  hipLaunchKernelGGL(rgio::reset_opacity_kernel, dim3((unsigned)blocks), dim3(rgio::kThreads), 0, static_cast<hipStream_t>(stream), P, opacity_raw,
                     scaling_raw, filter_3D, opacity_out, zero_a, zero_b);
  return rgio::launched() ? 0 : RADEGS_ERR_HIP;
}

int radegs_modelio_init(long long P, int K, const float* colors, const float* dist2, float opacity_value, float* f_dc, float* f_rest, float* opacity,
                        float* scaling, float* rotation, void* stream) {
  if (P < 0 || K < 0 || K > RADEGS_MODELIO_MAX_REST) return RADEGS_ERR_INVALID_ARG;
  if (P == 0) return 0;
  if (!colors || !dist2 || !f_dc || (K > 0 && !f_rest) || !opacity || !scaling || !rotation || rgio::misaligned(rotation, 16)) return RADEGS_ERR_INVALID_ARG;
  const long long blocks = (P + rgio::kThreads - 1) / rgio::kThreads;
  if (blocks > 0x7fffffffLL) return RADEGS_ERR_TOO_LARGE;
  hipLaunchKernelGGL(rgio::init_kernel, dim3((unsigned)blocks), dim3(rgio::kThreads), 0, static_cast<hipStream_t>(stream), P, K, colors, dist2,
                     opacity_value, f_dc, f_rest, opacity, scaling, rotation);
  return rgio::launched() ? 0 : RADEGS_ERR_HIP;
}

}  // extern "C"
