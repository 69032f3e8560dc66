// radegs_appearance.hip -- the decoupled appearance loss: train.py:37-58 `L1_loss_appearance` with
// scene/appearance_network.py behind it.  The trunk (conv1, four pixel-shuffle blocks, <= half resolution) stays in torch; this unit is
// everything that touches full resolution:
//     down  = bilinear(crop(image), (H/32, W/32), align_corners)                     appearance_downsample_{fwd,bwd}_kernel
//     U     = bilinear x2 (F), align_corners           F [16,H/2,W/2]: the trunk's output
//     A     = relu(conv2(U))         3x3, 16 -> 16, zero padding at the crop border
//     M     = sigmoid(conv3(A))      3x3, 16 -> 3
//     loss  = mean |M * crop(image) - crop(gt)|                                      appearance_head_fwd_kernel
// and its gradients w.r.t. F, image, W2, b2, W3, b3                                  appearance_head_bwd_kernel + appearance_dfeat_kernel
//
// Layout for gfx950: a 1024-thread workgroup owns a 32x32 region of A, one thread per pixel with all 16 output channels in registers;
// the 34x34x16 region of U it needs is built in LDS straight from F (L2-resident), A goes to LDS, conv3 runs on the 30x30 interior.
// Nothing of full resolution is written by the forward.  Workgroups walk the tiles with a grid stride (one workgroup per CU: the two
// images take 140..151 KB of the 160 KB of LDS), so the per-workgroup partial sums are at most MAXB rows.
// The backward recomputes U, A and M per tile (28x28 owned pixels of the same 32x32 region), keeps dZ2 = d loss / d conv2's
// pre-activation in LDS over A, sums dW3 / dW2 with one (c_out, c_in) pair per thread and nine taps in registers, and writes dZ2 once:
// the one full-resolution tensor.  appearance_dfeat_kernel, organised by 16x16 tiles of F, turns it into dU (conv2 transposed, eight
// channels at a time in LDS) and gathers dF with the forward's own index expression (src_index below) -- no atomics anywhere, every
// sum in a fixed order, the last level in double.
// Weights: repacked once per call by appearance_pack_weights_kernel so that the 16 (or 3, or 8) values a thread needs next to each
// other ARE next to each other; every read of them has a wave-uniform address (scalar loads).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/radegs.h"
#include "rg_reduce.h"
#include "rg_workspace.h"

namespace rgap {

constexpr int NT = 1024;                       // threads per workgroup of the head kernels
constexpr int AT = 32, UT = AT + 2;            // side of the A region (one thread per pixel) and of the U region under it
constexpr int USTR = UT * UT + 2;              // channel strides in LDS: 1158 % 32 = 6 -> the 16 channels of one pixel on 16 banks
constexpr int ASTR = AT * AT + 8;
constexpr int FT = AT - 2;                     // forward: owned output pixels per tile side (conv3 needs A one pixel around)
constexpr int BT = AT - 4, ZT = AT - 2;        // backward: owned pixels per side; dZ3 is needed one pixel around them
constexpr int MAXB = 256;                      // workgroups of the head kernels = rows of partial sums (one per CU)
// the repacked weights (floats)
constexpr int P_W2F = 0;                       // [ci][k][co]    conv2 forward: 16 c_out of one (c_in, tap) contiguous
constexpr int P_B2 = P_W2F + 2304;
constexpr int P_W3F = P_B2 + 16;               // [ci][k][4]     conv3 forward: 3 c_out (+1 pad)
constexpr int P_B3 = P_W3F + 576;              // [4]
constexpr int P_W2B = P_B3 + 4;                // [co][k][ci]    conv2 transposed: 16 c_in of one (c_out, tap)
constexpr int P_W3B = P_W2B + 2304;            // [co][k][ci]    conv3 transposed
constexpr int P_END = P_W3B + 432;
constexpr int PACK_FLOATS = 5760;              // P_END = 5636 rounded up: 23 040 bytes, a multiple of 256
constexpr int NWG = 2304 + 16 + 432 + 3;       // dW2, db2, dW3, db3: one row of weight-gradient partials
// appearance_dfeat_kernel
constexpr int GF = 16;                         // F tile side
constexpr int RMAX = 38, ZW = RMAX + 2;        // at most 36 rows of U touch 17 rows of F (scale > 15/31); dZ2 one pixel around them
constexpr int ZSTR = ZW * ZW + 8;
constexpr int SLAB = 8;                        // channels of dU held at a time

struct Geo {
  int origH, origW, H, W, top, left, h, w;     // crop H x W at (top, left) of the image; F is h x w = H/2 x W/2
  float sy, sx;                                // (h-1)/(H-1), (w-1)/(W-1)
};

// torch's align_corners=True source index (UpSample.h: area_pixel_compute_source_index + guard_index_and_lambda), fp32
__device__ __forceinline__ void src_index(int dst, float scale, int in, int& i0, int& i1, float& l1) {
  const float src = scale * (float)dst;
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f);
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- repack -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) appearance_pack_weights_kernel(const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ W3,
                                                                     const float* __restrict__ b3, float* __restrict__ pack) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= PACK_FLOATS) return;
  float v = 0.0f;
  if (i < P_B2) { const int co = i & 15, k = (i >> 4) % 9, ci = (i >> 4) / 9; v = W2[(co * 16 + ci) * 9 + k]; }
  else if (i < P_W3F) v = b2[i - P_B2];
  else if (i < P_B3) { const int j = i - P_W3F, co = j & 3, k = (j >> 2) % 9, ci = (j >> 2) / 9; v = co < 3 ? W3[(co * 16 + ci) * 9 + k] : 0.0f; }
  else if (i < P_W2B) { const int co = i - P_B3; v = co < 3 ? b3[co] : 0.0f; }
  else if (i < P_W3B) { const int j = i - P_W2B, ci = j & 15, k = (j >> 4) % 9, co = (j >> 4) / 9; v = W2[(co * 16 + ci) * 9 + k]; }
  else if (i < P_END) { const int j = i - P_W3B, ci = j & 15, k = (j >> 4) % 9, co = (j >> 4) / 9; v = W3[(co * 16 + ci) * 9 + k]; }
  pack[i] = v;
}

// ---- the pieces the forward and the backward share --------------------------------------------------------------------------------
struct Tables { int i0[2][UT], i1[2][UT]; float l1[2][UT]; };     // [0]: rows, [1]: columns of the tile's U region; i0 < 0: outside the crop

__device__ __forceinline__ void fill_tables(Tables& t, const Geo& g, int uy0, int ux0, int tid) {
  if (tid < 2 * UT) {
    const int d = tid >= UT, j = tid - d * UT;
    const int p = (d ? ux0 : uy0) + j, n = d ? g.W : g.H;
    int i0 = -1, i1 = -1; float l1 = 0.0f;
    if (p >= 0 && p < n) src_index(p, d ? g.sx : g.sy, d ? g.w : g.h, i0, i1, l1);
    t.i0[d][j] = i0; t.i1[d][j] = i1; t.l1[d][j] = l1;
  }
}

// U on the tile's 34x34 region, zero outside the crop (conv2's padding).  One pixel per thread and pass, its 16 channels unrolled: the
// indices and weights are computed once and the 64 loads are independent of each other.
__device__ __forceinline__ void stage_u(float* __restrict__ sU, const Tables& t, const Geo& g, const float* __restrict__ F, int tid) {
  const size_t hw = (size_t)g.h * g.w;
  for (int r = tid; r < UT * UT; r += NT) {
    const int uy = r / UT, ux = r - uy * UT;
    const int y0 = t.i0[0][uy], x0 = t.i0[1][ux];
    const bool in = y0 >= 0 && x0 >= 0;
    const int y1 = t.i1[0][uy], x1 = t.i1[1][ux];
    const float ly = t.l1[0][uy], lx = t.l1[1][ux];
    const size_t o00 = in ? (size_t)y0 * g.w + x0 : 0, o01 = in ? (size_t)y0 * g.w + x1 : 0, o10 = in ? (size_t)y1 * g.w + x0 : 0, o11 = in ? (size_t)y1 * g.w + x1 : 0;
    float v[16];
#pragma unroll
    for (int ci = 0; ci < 16; ci++) {
      const float* f = F + ci * hw;
      const float v00 = f[o00], v01 = f[o01], v10 = f[o10], v11 = f[o11];
      v[ci] = (1.0f - ly) * ((1.0f - lx) * v00 + lx * v01) + ly * ((1.0f - lx) * v10 + lx * v11);
    }
#pragma unroll
    for (int ci = 0; ci < 16; ci++) sU[ci * USTR + r] = in ? v[ci] : 0.0f;
  }
}

// A = relu(conv2(U)) at the thread's pixel (ty, tx) of the A region, zero outside the crop (conv3's padding) -> LDS
__device__ __forceinline__ void conv2_relu(const float* __restrict__ sU, float* __restrict__ sA, const float* __restrict__ pack, int ty, int tx, bool inside) {
  float acc[16];
#pragma unroll
  for (int co = 0; co < 16; co++) acc[co] = pack[P_B2 + co];
  const float* u = sU + ty * UT + tx;
#pragma unroll 1
  for (int ci = 0; ci < 16; ci++) {
#pragma unroll
    for (int k = 0; k < 9; k++) {
      const float uv = u[ci * USTR + (k / 3) * UT + (k % 3)];
      const float* w = pack + P_W2F + (ci * 9 + k) * 16;
#pragma unroll
      for (int co = 0; co < 16; co++) acc[co] = fmaf(w[co], uv, acc[co]);
    }
  }
#pragma unroll
  for (int co = 0; co < 16; co++) sA[co * ASTR + ty * AT + tx] = inside ? fmaxf(acc[co], 0.0f) : 0.0f;
}

// M = sigmoid(conv3(A)) at (ty, tx), 1 <= ty, tx <= AT-2
__device__ __forceinline__ void conv3_sigmoid(const float* __restrict__ sA, const float* __restrict__ pack, int ty, int tx, float m[3]) {
  float z0 = pack[P_B3], z1 = pack[P_B3 + 1], z2 = pack[P_B3 + 2];
  const float* a = sA + (ty - 1) * AT + (tx - 1);
#pragma unroll 4
  for (int ci = 0; ci < 16; ci++) {
#pragma unroll
    for (int k = 0; k < 9; k++) {
      const float av = a[ci * ASTR + (k / 3) * AT + (k % 3)];
      const float* w = pack + P_W3F + (ci * 9 + k) * 4;
      z0 = fmaf(w[0], av, z0); z1 = fmaf(w[1], av, z1); z2 = fmaf(w[2], av, z2);
    }
  }
  m[0] = sigmoidf_(z0); m[1] = sigmoidf_(z1); m[2] = sigmoidf_(z2);
}

// dZ3 = d loss / d conv3's pre-activation at (ty, tx), 1 <= ty, tx <= AT-2, into LDS (zero outside the crop); with `dimage`, the product's
// gradient w.r.t. the image goes out for the pixels the tile owns.  sign(0) = 0, as torch's abs.
__device__ __forceinline__ void stage_dz3(const float* __restrict__ sA, float* __restrict__ sZ3, const float* __restrict__ pack, const Geo& g,
                                          const float* __restrict__ image, const float* __restrict__ gt, float gn, int y, int x, int ty, int tx, bool inside,
                                          bool owned, float* __restrict__ dimage) {
  if (ty >= 1 && ty <= AT - 2 && tx >= 1 && tx <= AT - 2) {
    const size_t plane = (size_t)g.origH * g.origW;
    float d3[3] = {0.0f, 0.0f, 0.0f};
    if (inside) {
      float m[3];
      conv3_sigmoid(sA, pack, ty, tx, m);
      const size_t ip = (size_t)(g.top + y) * g.origW + (g.left + x);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float cv = image[c * plane + ip];
        const float t = m[c] * cv - gt[c * plane + ip];
        const float dt = t > 0.0f ? gn : (t < 0.0f ? -gn : 0.0f);
        if (dimage && owned) dimage[c * plane + ip] = dt * m[c];
        d3[c] = (dt * cv) * (m[c] * (1.0f - m[c]));
      }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) sZ3[c * (ZT * ZT) + (ty - 1) * ZT + (tx - 1)] = d3[c];
  }
}

// gA = conv3 transposed at (ty, tx), 2 <= ty, tx <= AT-3: A(q) feeds conv3's output at q - (k - 1) through tap k
__device__ __forceinline__ void conv3_transposed(const float* __restrict__ sZ3, const float* __restrict__ pack, int ty, int tx, float ga[16]) {
#pragma unroll
  for (int ci = 0; ci < 16; ci++) ga[ci] = 0.0f;
#pragma unroll
  for (int co = 0; co < 3; co++) {
#pragma unroll
    for (int k = 0; k < 9; k++) {
      const float gz = sZ3[co * (ZT * ZT) + (ty - k / 3) * ZT + (tx - k % 3)];
      const float* w = pack + P_W3B + (co * 9 + k) * 16;
#pragma unroll
      for (int ci = 0; ci < 16; ci++) ga[ci] = fmaf(w[ci], gz, ga[ci]);
    }
  }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) appearance_head_fwd_kernel(const Geo g, const float* __restrict__ F, const float* __restrict__ image,
                                                                const float* __restrict__ gt, const float* __restrict__ pack, int tiles_x, int ntiles,
                                                                double* __restrict__ partial, float* __restrict__ transformed /* [3,H,W] or null */) {
  __shared__ float sU[16 * USTR];
  __shared__ float sA[16 * ASTR];
  __shared__ Tables tab;
  __shared__ float red[NT / 64];
  const int tid = threadIdx.x, ty = tid >> 5, tx = tid & 31;
  const size_t plane = (size_t)g.origH * g.origW, cplane = (size_t)g.H * g.W;
  float sum = 0.0f;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int by = tile / tiles_x, bx = tile - by * tiles_x;
    const int ay0 = by * FT - 1, ax0 = bx * FT - 1;                    // A region origin in crop coordinates; U region one before it
    fill_tables(tab, g, ay0 - 1, ax0 - 1, tid);
    __syncthreads();
    stage_u(sU, tab, g, F, tid);
    __syncthreads();
    const int y = ay0 + ty, x = ax0 + tx;
    const bool inside = y >= 0 && y < g.H && x >= 0 && x < g.W;
    conv2_relu(sU, sA, pack, ty, tx, inside);
    __syncthreads();
    if (inside && ty >= 1 && ty <= AT - 2 && tx >= 1 && tx <= AT - 2) {
      float m[3];
      conv3_sigmoid(sA, pack, ty, tx, m);
      const size_t ip = (size_t)(g.top + y) * g.origW + (g.left + x);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float t = m[c] * image[c * plane + ip];
        sum += fabsf(t - gt[c * plane + ip]);
        if (transformed) transformed[c * cplane + (size_t)y * g.W + x] = t;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < NT / 64; i++) s += (double)red[i];
    partial[blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(256) appearance_loss_final_kernel(const double* __restrict__ partial, int n, double inv_n, float* __restrict__ loss) {
  __shared__ double sh[256];
  double a[1] = {0.0};
  rg::add_partials(partial, n, a);
  rg::block_sum(a, sh);
  if (threadIdx.x == 0) loss[0] = (float)(a[0] * inv_n);
}

// ---- backward, by full-resolution tile: d image, dZ2, partial dW2 / db2 / dW3 / db3 -----------------------------------------------
__global__ void __launch_bounds__(NT) appearance_head_bwd_kernel(const Geo g, const float* __restrict__ F, const float* __restrict__ image,
                                                                const float* __restrict__ gt, const float* __restrict__ pack,
                                                                const float* __restrict__ gloss, int tiles_x, int ntiles,
                                                                float* __restrict__ dimage, float* __restrict__ gz2 /* [16,H,W] */,
                                                                float* __restrict__ wpartial /* [gridDim.x][NWG] */) {
  __shared__ float sU[16 * USTR];
  __shared__ float sA[16 * ASTR];        // A, then dZ2 on the owned pixels
  __shared__ float sZ3[3 * ZT * ZT];
  __shared__ Tables tab;
  const int tid = threadIdx.x, ty = tid >> 5, tx = tid & 31;
  const size_t plane = (size_t)g.origH * g.origW, cplane = (size_t)g.H * g.W;
  const float gn = gloss[0] / (float)(3 * cplane);
  // d image outside the crop
  for (size_t i = (size_t)blockIdx.x * NT + tid; i < 3 * plane; i += (size_t)gridDim.x * NT) {
    const size_t r = i % plane;
    const int y = (int)(r / g.origW) - g.top, x = (int)(r % g.origW) - g.left;
    if (y < 0 || y >= g.H || x < 0 || x >= g.W) dimage[i] = 0.0f;
  }
  // dW2: thread <-> (c_out, c_in) pair, four row bands of the tile; dW3: thread < 768 <-> (c_out, c_in) pair, 16 pixel groups
  const int p2 = tid & 255, co2 = p2 >> 4, ci2 = p2 & 15, band = tid >> 8;
  const int p3 = tid % 48, co3 = p3 >> 4, ci3 = p3 & 15, grp3 = tid / 48;
  float acc2[9], acc3[9], accb2 = 0.0f, accb3 = 0.0f;
#pragma unroll
  for (int k = 0; k < 9; k++) acc2[k] = acc3[k] = 0.0f;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int by = tile / tiles_x, bx = tile - by * tiles_x;
    const int ay0 = by * BT - 2, ax0 = bx * BT - 2;                    // owned pixels: A-region coordinates 2 .. AT-3
    fill_tables(tab, g, ay0 - 1, ax0 - 1, tid);
    __syncthreads();
    stage_u(sU, tab, g, F, tid);
    __syncthreads();
    const int y = ay0 + ty, x = ax0 + tx;
    const bool inside = y >= 0 && y < g.H && x >= 0 && x < g.W;
    const bool owned = inside && ty >= 2 && ty <= AT - 3 && tx >= 2 && tx <= AT - 3;
    conv2_relu(sU, sA, pack, ty, tx, inside);
    __syncthreads();
    // dZ3 on the owned pixels and one around them; d image on the owned ones
    stage_dz3(sA, sZ3, pack, g, image, gt, gn, y, x, ty, tx, inside, owned, dimage);
    __syncthreads();
    // dW3[co][ci][k] += dZ3[co](p) * A[ci](p + k - 1) over the owned pixels
    if (tid < 768) {
      for (int p = grp3; p < BT * BT; p += 16) {
        const int py = p / BT, px = p - py * BT;
        const float gz = sZ3[co3 * (ZT * ZT) + (py + 1) * ZT + (px + 1)];
        const float* a = sA + ci3 * ASTR + (py + 1) * AT + (px + 1);
#pragma unroll
        for (int k = 0; k < 9; k++) acc3[k] = fmaf(gz, a[(k / 3) * AT + (k % 3)], acc3[k]);
        accb3 += gz;
      }
    }
    // gA = conv3 transposed at the owned pixels (registers), then dZ2 = gA where A > 0
    float ga[16];
    if (owned) conv3_transposed(sZ3, pack, ty, tx, ga);
    __syncthreads();                                                   // dW3 has read A
    if (owned) {
#pragma unroll
      for (int ci = 0; ci < 16; ci++) {
        const int ia = ci * ASTR + ty * AT + tx;
        const float v = sA[ia] > 0.0f ? ga[ci] : 0.0f;
        sA[ia] = v;
        gz2[ci * cplane + (size_t)y * g.W + x] = v;
      }
    }                                                                  // an owned slot outside the crop holds A = 0 already: dW2 walks it
    __syncthreads();
    // dW2[co][ci][k] += dZ2[co](p) * U[ci](p + k - 1): seven rows per band, a sliding 3x3 window of U
    for (int r = band * 7; r < band * 7 + 7; r++) {
      const float* u = sU + ci2 * USTR + (r + 2) * UT + 2;            // owned pixel (r, c) = A (r+2, c+2) = centre U (r+3, c+3)
      const float* z = sA + co2 * ASTR + (r + 2) * AT + 2;
      float c0[3], c1[3], c2[3];
#pragma unroll
      for (int ky = 0; ky < 3; ky++) { c0[ky] = u[ky * UT]; c1[ky] = u[ky * UT + 1]; }
#pragma unroll 4
      for (int c = 0; c < BT; c++) {
        const float gz = z[c];
#pragma unroll
        for (int ky = 0; ky < 3; ky++) {
          c2[ky] = u[ky * UT + c + 2];
          acc2[ky * 3 + 0] = fmaf(gz, c0[ky], acc2[ky * 3 + 0]);
          acc2[ky * 3 + 1] = fmaf(gz, c1[ky], acc2[ky * 3 + 1]);
          acc2[ky * 3 + 2] = fmaf(gz, c2[ky], acc2[ky * 3 + 2]);
          c0[ky] = c1[ky]; c1[ky] = c2[ky];
        }
        accb2 += gz;
      }
    }
    __syncthreads();                                                   // the next tile overwrites U and A
  }
  // the workgroup's row of partials: bands / groups summed in a fixed order through LDS (U's space)
  float* red = sU;
  float* out = wpartial + (size_t)blockIdx.x * NWG;
#pragma unroll
  for (int k = 0; k < 9; k++) red[band * 2320 + p2 * 9 + k] = acc2[k];
  if (ci2 == 0) red[band * 2320 + 2304 + co2] = accb2;
  __syncthreads();
  for (int j = tid; j < 2320; j += NT) out[j] = ((red[j] + red[2320 + j]) + red[2 * 2320 + j]) + red[3 * 2320 + j];
  __syncthreads();
  if (tid < 768) {
#pragma unroll
    for (int k = 0; k < 9; k++) red[grp3 * 435 + p3 * 9 + k] = acc3[k];
    if (ci3 == 0) red[grp3 * 435 + 432 + co3] = accb3;
  }
  __syncthreads();
  if (tid < 435) {
    float s = 0.0f;
    for (int q = 0; q < 16; q++) s += red[q * 435 + tid];
    out[2320 + tid] = s;
  }
}

__global__ void __launch_bounds__(256) appearance_wgrad_final_kernel(const float* __restrict__ wpartial, int nb, float* __restrict__ dW2, float* __restrict__ db2,
                                                                    float* __restrict__ dW3, float* __restrict__ db3) {
  __shared__ double s[4][64];
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), seg = threadIdx.x >> 6;
  double a = 0.0;
  if (j < NWG) for (int b = seg; b < nb; b += 4) a += (double)wpartial[(size_t)b * NWG + j];
  s[seg][threadIdx.x & 63] = a;
  __syncthreads();
  if (seg == 0 && j < NWG) {
    const float v = (float)(((s[0][threadIdx.x] + s[1][threadIdx.x]) + s[2][threadIdx.x]) + s[3][threadIdx.x]);
    if (j < 2304) dW2[j] = v; else if (j < 2320) db2[j - 2304] = v; else if (j < 2752) dW3[j - 2320] = v; else db3[j - 2752] = v;
  }
}

// ---- backward, by tile of F: dU = conv2 transposed (dZ2), dF = the bilinear x2's transpose as a gather ------------------------------
struct FeatTables { int i0[2][RMAX], i1[2][RMAX], lo[2][GF], hi[2][GF], ext[2][2]; float l1[2][RMAX]; };

// Which rows (wave 0) and columns (wave 1) of U read the 16x16 tile of F at (fy0, fx0): the forward's expression over a 64-wide window
// that contains them all (i0(y) <= y/2 and i0(y) >= y/2 - 2, so they lie in [2 f0 - 2, 2 f0 + 35]).  Ends with the extent in t.ext
// ({first, count} per axis) after a barrier; the per-row tables are ready after the caller's next barrier.
// count <= RMAX always, so the min() below never drops a row: a row is hit iff i0(y) = floor(s y) lies in [f0 - 1, f0 + 15], 17 values,
// and an interval of length 17 holds at most floor(17 / s) + 1 multiples of s.  s = (h - 1) / (2 h - 1) >= 15/31 for h >= 16 (the entry
// points refuse a crop below 32, so h >= 16), hence 17 / s <= 35.2 and count <= 36 in exact arithmetic; the fp32 rounding of s and of
// s * y (2^-24 relative each) can move at most one more y across each end of the interval: 38 = RMAX.
__device__ __forceinline__ void dfeat_extent(FeatTables& t, const Geo& g, int fy0, int fx0, int tid) {
  static_assert(2 * GF + 8 <= 64, "one wave scans the window");
  if (tid < 128) {
    const int d = tid >> 6, f0 = d ? fx0 : fy0, base = max(0, 2 * f0 - 4), p = base + (tid & 63), n = d ? g.W : g.H, nin = d ? g.w : g.h;
    int i0 = -1, i1 = -1; float l1 = 0.0f;
    if (p < n) src_index(p, d ? g.sx : g.sy, nin, i0, i1, l1);
    const bool hit = p < n && i1 >= f0 && i0 < f0 + GF;
    const unsigned long long mask = __ballot(hit);
    if ((tid & 63) == 0) {
      const int first = mask ? __ffsll((long long)mask) - 1 : 0, last = mask ? 63 - __clzll((long long)mask) : -1;
      t.ext[d][0] = base + first;
      t.ext[d][1] = min(last - first + 1, RMAX);
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void dfeat_rows(FeatTables& t, const Geo& g, int tid) {
  if (tid < 2 * RMAX) {
    const int d = tid >= RMAX, j = tid - d * RMAX;
    int i0 = -1, i1 = -1; float l1 = 0.0f;
    if (j < t.ext[d][1]) src_index(t.ext[d][0] + j, d ? g.sx : g.sy, d ? g.w : g.h, i0, i1, l1);
    t.i0[d][j] = i0; t.i1[d][j] = i1; t.l1[d][j] = l1;
  }
}

// per row / column of the F tile: the range of U rows / columns that read it (after dfeat_rows and a barrier)
__device__ __forceinline__ void dfeat_ranges(FeatTables& t, int fy0, int fx0, int tid) {
  if (tid < 2 * GF) {
    const int d = tid >= GF, k = tid - d * GF, f = (d ? fx0 : fy0) + k, n = t.ext[d][1];
    int a = 1, b = 0;
    bool any = false;
    for (int j = 0; j < n; j++) {
      if (t.i0[d][j] == f || t.i1[d][j] == f) { if (!any) a = j; b = j; any = true; }
    }
    t.lo[d][k] = a; t.hi[d][k] = b;
  }
}

// dU on the extent from dZ2 in LDS (sZ: the extent and one pixel around it), SLAB channels at a time into sD, then dF of the tile.
// Starts with a barrier.
__device__ __forceinline__ void dfeat_collect(const FeatTables& t, const float* __restrict__ sZ, float* __restrict__ sD, const float* __restrict__ pack,
                                              const Geo& g, int fy0, int fx0, float* __restrict__ dF, int tid) {
  const int rh = t.ext[0][1], rw = t.ext[1][1], npix = rh * rw;
  for (int slab = 0; slab < 16 / SLAB; slab++) {
    __syncthreads();                               // tables and dZ2 ready / the previous slab's gather has read sD
    for (int p = tid; p < npix; p += NT) {
      const int ry = p / rw, rx = p - ry * rw;
      float acc[SLAB];
#pragma unroll
      for (int j = 0; j < SLAB; j++) acc[j] = 0.0f;
      const float* z = sZ + (ry + 2) * ZW + (rx + 2);                  // U(q) feeds conv2's output at q - (k - 1) through tap k
#pragma unroll 1
      for (int co = 0; co < 16; co++) {
#pragma unroll
        for (int k = 0; k < 9; k++) {
          const float gz = z[co * ZSTR - (k / 3) * ZW - (k % 3)];
          const float* w = pack + P_W2B + (co * 9 + k) * 16 + slab * SLAB;
#pragma unroll
          for (int j = 0; j < SLAB; j++) acc[j] = fmaf(w[j], gz, acc[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < SLAB; j++) sD[j * (RMAX * RMAX) + ry * RMAX + rx] = acc[j];
    }
    __syncthreads();
    for (int o = tid; o < SLAB * GF * GF; o += NT) {
      const int j = o / (GF * GF), r = o - j * (GF * GF), fy = r / GF, fx = r - fy * GF;
      const int gy = fy0 + fy, gx = fx0 + fx;
      float s = 0.0f;
      for (int ry = t.lo[0][fy]; ry <= t.hi[0][fy]; ry++) {
        const float ly = t.l1[0][ry];
        const float wy = (t.i0[0][ry] == gy ? 1.0f - ly : 0.0f) + (t.i1[0][ry] == gy ? ly : 0.0f);
        float row = 0.0f;
        for (int rx = t.lo[1][fx]; rx <= t.hi[1][fx]; rx++) {
          const float lx = t.l1[1][rx];
          const float wx = (t.i0[1][rx] == gx ? 1.0f - lx : 0.0f) + (t.i1[1][rx] == gx ? lx : 0.0f);
          row = fmaf(wx, sD[j * (RMAX * RMAX) + ry * RMAX + rx], row);
        }
        s = fmaf(wy, row, s);
      }
      dF[(size_t)(slab * SLAB + j) * g.h * g.w + (size_t)gy * g.w + gx] = s;
    }
  }
}

// dZ2 is read back from the one full-resolution tensor appearance_head_bwd_kernel wrote (recomputing it here from F was measured and
// lost: DESIGN 11 N8)
__global__ void __launch_bounds__(NT) appearance_dfeat_kernel(const Geo g, const float* __restrict__ gz2, const float* __restrict__ pack, float* __restrict__ dF) {
  __shared__ float sZ[16 * ZSTR];                  // dZ2 on the rows / columns of U that touch this tile of F, one pixel around them
  __shared__ float sD[SLAB * RMAX * RMAX];         // dU, eight channels at a time
  __shared__ FeatTables t;
  const int tid = threadIdx.x;
  const int fy0 = (int)blockIdx.y * GF, fx0 = (int)blockIdx.x * GF;
  const size_t cplane = (size_t)g.H * g.W;
  dfeat_extent(t, g, fy0, fx0, tid);
  const int y0 = t.ext[0][0], rh = t.ext[0][1], x0 = t.ext[1][0], rw = t.ext[1][1];
  dfeat_rows(t, g, tid);
  for (int r = tid; r < ZW * ZW; r += NT) {       // one pixel per thread and pass, 16 independent loads
    const int zy = r / ZW, zx = r - zy * ZW;
    const int y = y0 - 1 + zy, x = x0 - 1 + zx;
    const bool in = zy < rh + 2 && zx < rw + 2 && y >= 0 && y < g.H && x >= 0 && x < g.W;
    const size_t o = in ? (size_t)y * g.W + x : 0;
    float v[16];
#pragma unroll
    for (int co = 0; co < 16; co++) v[co] = gz2[co * cplane + o];
#pragma unroll
    for (int co = 0; co < 16; co++) sZ[co * ZSTR + r] = in ? v[co] : 0.0f;
  }
  __syncthreads();
  dfeat_ranges(t, fy0, fx0, tid);
  dfeat_collect(t, sZ, sD, pack, g, fy0, fx0, dF, tid);
}

// ---- the 32x down-sampling of the crop ---------------------------------------------------------------------------------------------
struct DGeo { int origH, origW, H, W, top, left, hd, wd; float sy, sx; };

__global__ void __launch_bounds__(256) appearance_downsample_fwd_kernel(const DGeo g, const float* __restrict__ image, float* __restrict__ down) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * g.hd * g.wd) return;
  const int c = i / (g.hd * g.wd), r = i - c * (g.hd * g.wd), oy = r / g.wd, ox = r - oy * g.wd;
  int y0, y1, x0, x1; float ly, lx;
  src_index(oy, g.sy, g.H, y0, y1, ly);
  src_index(ox, g.sx, g.W, x0, x1, lx);
  const float* p = image + (size_t)c * g.origH * g.origW + (size_t)g.top * g.origW + g.left;
  const float v00 = p[(size_t)y0 * g.origW + x0], v01 = p[(size_t)y0 * g.origW + x1], v10 = p[(size_t)y1 * g.origW + x0], v11 = p[(size_t)y1 * g.origW + x1];
  down[i] = (1.0f - ly) * ((1.0f - lx) * v00 + lx * v01) + ly * ((1.0f - lx) * v10 + lx * v11);
}

// gimage is zero on entry.  Footprints of different outputs are >= 32 pixels apart, so a pixel belongs to one thread; on the clamped
// last row / column (i1 == i0) the same thread adds twice, in order.
__global__ void __launch_bounds__(256) appearance_downsample_bwd_kernel(const DGeo g, const float* __restrict__ gdown, float* __restrict__ gimage) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * g.hd * g.wd) return;
  const int c = i / (g.hd * g.wd), r = i - c * (g.hd * g.wd), oy = r / g.wd, ox = r - oy * g.wd;
  int y0, y1, x0, x1; float ly, lx;
  src_index(oy, g.sy, g.H, y0, y1, ly);
  src_index(ox, g.sx, g.W, x0, x1, lx);
  float* p = gimage + (size_t)c * g.origH * g.origW + (size_t)g.top * g.origW + g.left;
  const float gv = gdown[i];
  p[(size_t)y0 * g.origW + x0] += (1.0f - ly) * (1.0f - lx) * gv;
  p[(size_t)y0 * g.origW + x1] += (1.0f - ly) * lx * gv;
  p[(size_t)y1 * g.origW + x0] += ly * (1.0f - lx) * gv;
  p[(size_t)y1 * g.origW + x1] += ly * lx * gv;
}

static float scale_of(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f; }

static bool crop_of(int origH, int origW, int& H, int& W, int& top, int& left) {
  if (origH < 32 || origW < 32 || origH > 32768 || origW > 32768) return false;
  H = origH / 32 * 32; W = origW / 32 * 32;
  top = origH / 2 - H / 2; left = origW / 2 - W / 2;
  return true;
}

static bool make_geo(int origH, int origW, int fh, int fw, Geo& g) {
  if (!crop_of(origH, origW, g.H, g.W, g.top, g.left)) return false;
  if (fh != g.H / 2 || fw != g.W / 2) return false;
  g.origH = origH; g.origW = origW; g.h = fh; g.w = fw;
  g.sy = scale_of(fh, g.H); g.sx = scale_of(fw, g.W);
  return true;
}

static bool make_dgeo(int origH, int origW, DGeo& g) {
  if (!crop_of(origH, origW, g.H, g.W, g.top, g.left)) return false;
  g.origH = origH; g.origW = origW; g.hd = g.H / 32; g.wd = g.W / 32;
  g.sy = scale_of(g.H, g.hd); g.sx = scale_of(g.W, g.wd);
  return true;
}

constexpr size_t PACK_BYTES = PACK_FLOATS * sizeof(float);
constexpr size_t FWD_BYTES = PACK_BYTES + MAXB * sizeof(double);
static size_t wpartial_bytes() { return rg::align256((size_t)MAXB * NWG * sizeof(float)); }

}  // namespace rgap

using namespace rgap;

extern "C" {

int radegs_appearance_downsample_forward(int orig_height, int orig_width, const float* image, float* down, void* stream_v) {
  DGeo g;
  if (!image || !down || !make_dgeo(orig_height, orig_width, g)) return RADEGS_ERR_INVALID_ARG;
  const int n = 3 * g.hd * g.wd;
  hipLaunchKernelGGL(appearance_downsample_fwd_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream_v), g, image, down);
  return hipGetLastError() == hipSuccess ? 0 : RADEGS_ERR_HIP;
}

int radegs_appearance_downsample_backward(int orig_height, int orig_width, const float* grad_down, float* grad_image, void* stream_v) {
  DGeo g;
  if (!grad_down || !grad_image || !make_dgeo(orig_height, orig_width, g)) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (hipMemsetAsync(grad_image, 0, (size_t)3 * orig_height * orig_width * sizeof(float), s) != hipSuccess) return RADEGS_ERR_HIP;
  const int n = 3 * g.hd * g.wd;
  hipLaunchKernelGGL(appearance_downsample_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, s, g, grad_down, grad_image);
  return hipGetLastError() == hipSuccess ? 0 : RADEGS_ERR_HIP;
}

size_t radegs_appearance_head_scratch_bytes(int orig_height, int orig_width, int backward) {
  int H, W, top, left;
  if (!crop_of(orig_height, orig_width, H, W, top, left)) return 0;
  if (!backward) return FWD_BYTES;
  return PACK_BYTES + wpartial_bytes() + (size_t)16 * H * W * sizeof(float);
}

int radegs_appearance_head_forward(int orig_height, int orig_width, int feat_height, int feat_width, const float* feat, const float* image, const float* gt,
                                   const float* W2, const float* b2, const float* W3, const float* b3, void* scratch, size_t scratch_bytes,
                                   float* loss, float* transformed, void* stream_v) {
  Geo g;
  if (!feat || !image || !gt || !W2 || !b2 || !W3 || !b3 || !scratch || !loss || !make_geo(orig_height, orig_width, feat_height, feat_width, g))
    return RADEGS_ERR_INVALID_ARG;
  if (scratch_bytes < FWD_BYTES || ((uintptr_t)scratch & 15)) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  float* pack = static_cast<float*>(scratch);
  double* partial = reinterpret_cast<double*>(static_cast<char*>(scratch) + PACK_BYTES);
  const int tiles_x = (g.W + FT - 1) / FT, ntiles = tiles_x * ((g.H + FT - 1) / FT), nb = ntiles < MAXB ? ntiles : MAXB;
  hipLaunchKernelGGL(appearance_pack_weights_kernel, dim3((PACK_FLOATS + 255) / 256), dim3(256), 0, s, W2, b2, W3, b3, pack);
  hipLaunchKernelGGL(appearance_head_fwd_kernel, dim3(nb), dim3(NT), 0, s, g, feat, image, gt, pack, tiles_x, ntiles, partial, transformed);
  hipLaunchKernelGGL(appearance_loss_final_kernel, dim3(1), dim3(256), 0, s, partial, nb, 1.0 / (3.0 * g.H * g.W), loss);
  return hipGetLastError() == hipSuccess ? 0 : RADEGS_ERR_HIP;
}

int radegs_appearance_head_backward(int orig_height, int orig_width, int feat_height, int feat_width, const float* feat, const float* image, const float* gt,
                                    const float* W2, const float* b2, const float* W3, const float* b3, const float* grad_loss, void* scratch,
                                    size_t scratch_bytes, float* grad_feat, float* grad_image, float* grad_W2, float* grad_b2, float* grad_W3,
                                    float* grad_b3, void* stream_v) {
  Geo g;
  if (!feat || !image || !gt || !W2 || !b2 || !W3 || !b3 || !grad_loss || !scratch || !grad_feat || !grad_image || !grad_W2 || !grad_b2 || !grad_W3 ||
      !grad_b3 || !make_geo(orig_height, orig_width, feat_height, feat_width, g))
    return RADEGS_ERR_INVALID_ARG;
  if (scratch_bytes < radegs_appearance_head_scratch_bytes(orig_height, orig_width, 1) || ((uintptr_t)scratch & 15)) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  float* pack = static_cast<float*>(scratch);
  float* wpartial = reinterpret_cast<float*>(static_cast<char*>(scratch) + PACK_BYTES);
  float* gz2 = reinterpret_cast<float*>(static_cast<char*>(scratch) + PACK_BYTES + wpartial_bytes());
  const int tiles_x = (g.W + BT - 1) / BT, ntiles = tiles_x * ((g.H + BT - 1) / BT), nb = ntiles < MAXB ? ntiles : MAXB;
  hipLaunchKernelGGL(appearance_pack_weights_kernel, dim3((PACK_FLOATS + 255) / 256), dim3(256), 0, s, W2, b2, W3, b3, pack);
  hipLaunchKernelGGL(appearance_head_bwd_kernel, dim3(nb), dim3(NT), 0, s, g, feat, image, gt, pack, grad_loss, tiles_x, ntiles, grad_image, gz2, wpartial);
  hipLaunchKernelGGL(appearance_wgrad_final_kernel, dim3((NWG + 63) / 64), dim3(256), 0, s, wpartial, nb, grad_W2, grad_b2, grad_W3, grad_b3);
  hipLaunchKernelGGL(appearance_dfeat_kernel, dim3(g.w / GF, g.h / GF), dim3(NT), 0, s, g, gz2, pack, grad_feat);
  return hipGetLastError() == hipSuccess ? 0 : RADEGS_ERR_HIP;
}

}  // extern "C"
