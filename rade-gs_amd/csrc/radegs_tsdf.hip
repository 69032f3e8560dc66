// radegs_tsdf.hip -- TSDF fusion: the step between the renderer's median depth maps and recon.ply on the reference's DTU
// route, mesh_extract.py:51-105, which upstream hands to Open3D's VoxelBlockGrid on the CPU.
//     compute_unique_block_coordinates     touch_keys_kernel (the key as two words) -> rg::radix_sort_order_2xu32 (with the joined
//                                          key) -> first_kernel -> scans -> unique_emit_kernel
//     integrate                            coords_keys_kernel -> the same sort, first_kernel against the grid -> insert_old /
//                                          insert_new_kernel (the merged key array), fuse_view_kernel
//     extract_triangle_mesh                extract_count_kernel -> scans over the blocks -> extract_vertices_kernel, extract_faces_kernel
//
// The specification is include/radegs.h, "TSDF fusion"; tests/tsdf_restatement.py restates it in NumPy float32 and the kernels are held to
// that bit for bit.  -ffp-contract=off: one rounding per operation, products before sums, as numpy evaluates them.
//
// The grid.  A block is 16^3 voxels; its coordinate floor(world / block_size) per axis is packed into a 63-bit key (21 bits per axis, bias
// 2^20, z highest).  The grid is the ascending key array plus, per key, a slot into dense storage [capacity][4096] (voxel (z * 16 + y) * 16 + x);
// a block is found by rg::lower_bound, as radegs_mesheval.hip finds a cell.  A new block takes the next free slot, so a view's new blocks are one
// contiguous range of the storage (the caller zero-fills it) and no block ever moves.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_mc_tables.h"
#include "rg_prims.h"
#include "rg_workspace.h"

namespace rgts {

using rg::blocks_of;
constexpr unsigned long long kNoKey = ~0ull;   // a sample that touches nothing; sorts last (real keys have 63 bits)
constexpr int kBias = 1 << 20;
constexpr int kVox = 4096;
constexpr int kPad = 18, kPad3 = 18 * 18 * 18;      // a block's corners with one layer of its neighbours on every side
constexpr int kCells = 17, kCells3 = 17 * 17 * 17;  // the cells whose lowest corner is at -1 .. 15 per axis

struct Camera {
  float fx, fy, cx, cy;
  float m[12];   // rows of a 3x4 matrix: camera to world (touch), or world to camera with the rotation times voxel_size (integrate)
};

__device__ __forceinline__ unsigned long long pack_key(int bx, int by, int bz) {
  return ((unsigned long long)(bz + kBias) << 42) | ((unsigned long long)(by + kBias) << 21) | (unsigned long long)(bx + kBias);
}
__device__ __forceinline__ void unpack_key(unsigned long long key, int& bx, int& by, int& bz) {
  bx = (int)(key & 0x1FFFFFull) - kBias;
  by = (int)((key >> 21) & 0x1FFFFFull) - kBias;
  bz = (int)((key >> 42) & 0x1FFFFFull) - kBias;
}
__device__ __forceinline__ bool in_range(int c) { return c >= -kBias && c < kBias; }

// position of the block at (bx, by, bz) in the key array, -1 when absent (or outside the key range)
__device__ __forceinline__ int find_block(const unsigned long long* __restrict__ keys, uint32_t n, int bx, int by, int bz) {
  if (!in_range(bx) || !in_range(by) || !in_range(bz)) return -1;
  const unsigned long long key = pack_key(bx, by, bz);
  const uint32_t p = rg::lower_bound(keys, n, key);
  return (p < n && keys[p] == key) ? (int)p : -1;
}

// ------------------------------------------------------------------------- touch -------------------------------------------------------------------------
// One thread per sampled pixel (4i, 4j): four points along its ray between d - trunc and d + trunc, each one key.  A coordinate outside the
// 21 bits raises the flag and yields no key: it never wraps.  The key leaves as its two words, lo[] and hi[], which is what the sort takes.
__global__ void __launch_bounds__(256) touch_keys_kernel(int W, int H, const float* __restrict__ depth, Camera c, float depth_scale, float depth_max,
                                                         float trunc, float block_size, uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, uint32_t* __restrict__ flag) {
  const int w4 = W / 4, h4 = H / 4;
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= (long long)w4 * h4) return;
  const int x = 4 * (int)(s % w4), y = 4 * (int)(s / w4);
  const float d = depth[(size_t)y * W + x] / depth_scale;
  const bool ok = d > 0.0f && d < depth_max;
  const float xn = ((float)x - c.cx) / c.fx, yn = ((float)y - c.cy) / c.fy;
  const float tmin = fmaxf(d - trunc, 0.0f), tmax = fminf(d + trunc, depth_max);
  const float step = (tmax - tmin) / 3.0f;
  for (int k = 0; k < 4; k++) {
    unsigned long long key = kNoKey;
    if (ok) {
      const float t = tmin + (float)k * step;
      const float px = xn * t, py = yn * t;
      float b[3];
      bool fits = true;
#pragma unroll
      for (int r = 0; r < 3; r++) {
        b[r] = floorf((((c.m[4 * r] * px + c.m[4 * r + 1] * py) + c.m[4 * r + 2] * t) + c.m[4 * r + 3]) / block_size);
        fits = fits && b[r] >= (float)-kBias && b[r] < (float)kBias;   // false for NaN
      }
      if (fits) key = pack_key((int)b[0], (int)b[1], (int)b[2]);
      else *flag = 1u;
    }
    lo[4 * s + k] = (uint32_t)key;
    hi[4 * s + k] = (uint32_t)(key >> 32);
  }
}

__global__ void __launch_bounds__(256) coords_keys_kernel(uint32_t n, const int* __restrict__ coords, uint32_t* __restrict__ lo,
                                                          uint32_t* __restrict__ hi, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int bx = coords[3 * (size_t)i], by = coords[3 * (size_t)i + 1], bz = coords[3 * (size_t)i + 2];
  const bool fits = in_range(bx) && in_range(by) && in_range(bz);
  const unsigned long long key = fits ? pack_key(bx, by, bz) : kNoKey;
  lo[i] = (uint32_t)key;
  hi[i] = (uint32_t)(key >> 32);
  if (!fits) *flag = 1u;
}

// ------------------------------------------------------------------- sort, unique, insert -------------------------------------------------------------------
// first[j]: sorted[j] is a real key and differs from its predecessor.  Against the grid: pos[j] = how many grid keys are smaller,
// fresh[j] = first and not in the grid.
__global__ void __launch_bounds__(256) first_kernel(uint32_t n, const unsigned long long* __restrict__ sorted, uint32_t ngrid,
                                                    const unsigned long long* __restrict__ grid_keys, uint32_t* __restrict__ first,
                                                    uint32_t* __restrict__ fresh, uint32_t* __restrict__ pos) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const unsigned long long key = sorted[j];
  const bool f = key != kNoKey && (j == 0 || sorted[j - 1] != key);
  uint32_t p = 0;
  bool found = false;
  if (f && ngrid) {
    p = rg::lower_bound(grid_keys, ngrid, key);
    found = p < ngrid && grid_keys[p] == key;
  }
  first[j] = f;
  fresh[j] = f && !found;
  pos[j] = p;
}

__global__ void counts_kernel(uint32_t n, const uint32_t* __restrict__ first_incl, const uint32_t* __restrict__ fresh_incl,
                              const uint32_t* __restrict__ flag, long long* __restrict__ counts3) {
  counts3[0] = first_incl[n - 1];
  counts3[1] = fresh_incl[n - 1];
  counts3[2] = *flag;
}

__global__ void __launch_bounds__(256) unique_emit_kernel(uint32_t n, const unsigned long long* __restrict__ sorted, const uint32_t* __restrict__ first,
                                                          const uint32_t* __restrict__ first_incl, uint32_t n_unique, int* __restrict__ coords) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n || !first[j]) return;
  const uint32_t a = first_incl[j] - 1u;
  if (a >= n_unique) return;
  int bx, by, bz;
  unpack_key(sorted[j], bx, by, bz);
  coords[3 * (size_t)a] = bx;
  coords[3 * (size_t)a + 1] = by;
  coords[3 * (size_t)a + 2] = bz;
}

// The merged key array.  An old key moves up by the number of fresh keys below it; a fresh key of rank r stands after the pos old keys
// below it and the r fresh ones, and takes slot ngrid + r.
__global__ void __launch_bounds__(256) insert_old_kernel(uint32_t ngrid, const unsigned long long* __restrict__ grid_keys, const int* __restrict__ grid_slots,
                                                         uint32_t n, const unsigned long long* __restrict__ sorted, const uint32_t* __restrict__ fresh_incl,
                                                         uint32_t total, unsigned long long* __restrict__ new_keys, int* __restrict__ new_slots) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= ngrid) return;
  const unsigned long long key = grid_keys[i];
  const uint32_t p = n ? rg::lower_bound(sorted, n, key) : 0u;
  const uint32_t at = i + (p ? fresh_incl[p - 1] : 0u);
  if (at >= total) return;
  new_keys[at] = key;
  new_slots[at] = grid_slots[i];
}
__global__ void __launch_bounds__(256) insert_new_kernel(uint32_t n, const unsigned long long* __restrict__ sorted, const uint32_t* __restrict__ first,
                                                         const uint32_t* __restrict__ fresh, const uint32_t* __restrict__ pos,
                                                         const uint32_t* __restrict__ first_incl, const uint32_t* __restrict__ fresh_incl, uint32_t ngrid,
                                                         const int* __restrict__ grid_slots, uint32_t n_unique, uint32_t total,
                                                         unsigned long long* __restrict__ new_keys, int* __restrict__ new_slots,
                                                         int* __restrict__ active_slots, int* __restrict__ active_coords) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n || !first[j]) return;
  const unsigned long long key = sorted[j];
  int slot;
  if (fresh[j]) {
    const uint32_t r = fresh_incl[j] - 1u, at = pos[j] + r;
    slot = (int)(ngrid + r);
    if (at < total) {
      new_keys[at] = key;
      new_slots[at] = slot;
    }
  } else {
    slot = grid_slots[pos[j]];
  }
  const uint32_t a = first_incl[j] - 1u;
  if (a >= n_unique) return;
  int bx, by, bz;
  unpack_key(key, bx, by, bz);
  active_slots[a] = slot;
  active_coords[3 * (size_t)a] = bx;
  active_coords[3 * (size_t)a + 1] = by;
  active_coords[3 * (size_t)a + 2] = bz;
}

struct UniqueView {
  unsigned long long* sorted;
  uint32_t *lo, *hi, *hi_sorted, *perm, *first, *fresh, *pos, *first_incl, *fresh_incl, *flag;   // first, fresh, pos: the sort's scratch before
  void* temp;
  size_t temp_bytes, bytes;
};
static UniqueView unique_carve(long long N, void* base) {
  const size_t n = (size_t)N, ts = rg::sort_temp_bytes(n), tc = rg::scan_temp_bytes(n);
  rg::Carver c(base);
  UniqueView v;
  v.temp_bytes = ts > tc ? ts : tc;
  v.sorted = c.take<unsigned long long>(n);
  for (uint32_t** a : {&v.lo, &v.hi, &v.hi_sorted, &v.perm, &v.first, &v.fresh, &v.pos, &v.first_incl, &v.fresh_incl}) *a = c.take<uint32_t>(n);
  v.flag = c.take<uint32_t>(1);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

// the key words lo, hi [n] (and the flag) are in the workspace: sort them, mark the first occurrences, look them up in the grid, scan,
// leave the counts
static int unique_run(uint32_t n, const UniqueView& w, uint32_t ngrid, const unsigned long long* grid_keys, long long* counts3, hipStream_t s) {
  const unsigned nb = blocks_of(n);
  if (rg::radix_sort_order_2xu32(w.temp, w.temp_bytes, w.lo, w.hi, w.hi_sorted, w.perm, w.first, w.fresh, w.pos, n, 32, 32, s, nullptr, w.sorted) !=
      hipSuccess)
    return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(first_kernel, dim3(nb), dim3(256), 0, s, n, w.sorted, ngrid, grid_keys, w.first, w.fresh, w.pos);
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, w.first, nullptr, w.first_incl, n, s) != hipSuccess) return RADEGS_ERR_HIP;
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, w.fresh, nullptr, w.fresh_incl, n, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(counts_kernel, dim3(1), dim3(1), 0, s, n, w.first_incl, w.fresh_incl, w.flag, counts3);
  return rg::launch_status();
}

// ------------------------------------------------------------------------ integrate ------------------------------------------------------------------------
// One workgroup per listed block, thread = (x, y), 16 steps along z: every access to the block's storage is a full 1 KiB line per wave.
template <bool kColor>
__global__ void __launch_bounds__(256) fuse_view_kernel(const int* __restrict__ active_slots, const int* __restrict__ active_coords, uint32_t capacity,
                                                        int W, int H, const float* __restrict__ depth, const float* __restrict__ color, Camera c,
                                                        float depth_scale, float depth_max, float trunc, float* __restrict__ tsdf,
                                                        float* __restrict__ weight, float* __restrict__ block_color) {
  const int slot = active_slots[blockIdx.x];
  if (slot < 0 || (uint32_t)slot >= capacity) return;
  const int x = threadIdx.x & 15, y = threadIdx.x >> 4;
  const float Xx = (float)(16 * active_coords[3 * (size_t)blockIdx.x] + x), Xy = (float)(16 * active_coords[3 * (size_t)blockIdx.x + 1] + y);
  const int z0 = 16 * active_coords[3 * (size_t)blockIdx.x + 2];
  const size_t base = (size_t)slot * kVox + threadIdx.x;
  for (int z = 0; z < 16; z++) {
    const float Xz = (float)(z0 + z);
    const float px = ((c.m[0] * Xx + c.m[1] * Xy) + c.m[2] * Xz) + c.m[3];
    const float py = ((c.m[4] * Xx + c.m[5] * Xy) + c.m[6] * Xz) + c.m[7];
    const float pz = ((c.m[8] * Xx + c.m[9] * Xy) + c.m[10] * Xz) + c.m[11];
    if (!(pz > 0.0f)) continue;
    const float u = (c.fx * px) / pz + c.cx, v = (c.fy * py) / pz + c.cy;
    const float ui = roundf(u), vi = roundf(v);
    if (!(ui >= 0.0f && ui < (float)W && vi >= 0.0f && vi < (float)H)) continue;
    const size_t pix = (size_t)(int)vi * W + (int)ui;
    const float d = depth[pix] / depth_scale, sdf = d - pz;
    if (!(d > 0.0f) || d > depth_max || sdf < -trunc) continue;
    const float s = (sdf < trunc ? sdf : trunc) / trunc;
    const size_t i = base + (size_t)z * 256;
    const float w = weight[i], inv = 1.0f / (w + 1.0f);
    tsdf[i] = (w * tsdf[i] + s) * inv;
    if (kColor) {
#pragma unroll
      for (int k = 0; k < 3; k++) block_color[3 * i + k] = (w * block_color[3 * i + k] + color[3 * pix + k]) * inv;
    }
    weight[i] = w + 1.0f;
  }
}

// ----------------------------------------------------------------------- extraction -----------------------------------------------------------------------
__device__ __forceinline__ int pad_index(int x, int y, int z) { return ((z + 1) * kPad + (y + 1)) * kPad + (x + 1); }      // x, y, z in -1 .. 16
__device__ __forceinline__ int cell_index(int x, int y, int z) { return ((z + 1) * kCells + (y + 1)) * kCells + (x + 1); }  // x, y, z in -1 .. 15
__device__ __forceinline__ int scan_index(int i) { return i + (i >> 4); }   // 16 consecutive counts per thread, one bank apart between threads

// cnt [4096 + 256] (at scan_index): packed counts in, their exclusive prefix sums in voxel order out.  part [256].
__device__ __forceinline__ void block_scan(uint32_t* cnt, uint32_t* part) {
  const int t = threadIdx.x;
  uint32_t sum = 0;
  for (int k = 0; k < 16; k++) {
    const int i = scan_index(16 * t + k);
    const uint32_t c = cnt[i];
    cnt[i] = sum;
    sum += c;
  }
  part[t] = sum;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const uint32_t v = t >= off ? part[t - off] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  const uint32_t before = part[t] - sum;
  for (int k = 0; k < 16; k++) cnt[scan_index(16 * t + k)] += before;
  __syncthreads();
}

// Per voxel: which of its three owned edges carry a vertex (bits 0-2) and how many triangles its cell yields (bits 3-5); per block the
// two sums.  The block's corners and one layer of its 26 neighbours are staged as two bits each: valid (weight > threshold), negative.
__global__ void __launch_bounds__(256) extract_count_kernel(uint32_t n, const unsigned long long* __restrict__ keys, const int* __restrict__ slots,
                                                            const float* __restrict__ tsdf, const float* __restrict__ weight, float threshold,
                                                            uint8_t* __restrict__ info, uint32_t* __restrict__ block_nv, uint32_t* __restrict__ block_nt,
                                                            unsigned long long* __restrict__ totals) {
  __shared__ int nb[27];
  __shared__ uint8_t st[kPad3];
  __shared__ uint8_t cell_ok[kCells3];
  __shared__ uint32_t sums[2];
  const uint32_t b = blockIdx.x;
  int bx, by, bz;
  unpack_key(keys[b], bx, by, bz);
  if (threadIdx.x < 27) {
    const int j = find_block(keys, n, bx + (int)(threadIdx.x % 3) - 1, by + (int)((threadIdx.x / 3) % 3) - 1, bz + (int)(threadIdx.x / 9) - 1);
    nb[threadIdx.x] = j < 0 ? -1 : slots[j];
  }
  if (threadIdx.x < 2) sums[threadIdx.x] = 0u;
  __syncthreads();
  for (int i = threadIdx.x; i < kPad3; i += 256) {
    const int lx = i % kPad - 1, ly = (i / kPad) % kPad - 1, lz = i / (kPad * kPad) - 1;
    const int which = (lx < 0 ? 0 : (lx > 15 ? 2 : 1)) + 3 * (ly < 0 ? 0 : (ly > 15 ? 2 : 1)) + 9 * (lz < 0 ? 0 : (lz > 15 ? 2 : 1));
    const int slot = nb[which];
    uint8_t s = 0;
    if (slot >= 0) {
      const size_t v = (size_t)slot * kVox + (((lz & 15) * 16 + (ly & 15)) * 16 + (lx & 15));
      s = (uint8_t)((weight[v] > threshold ? 1 : 0) | (tsdf[v] < 0.0f ? 2 : 0));
    }
    st[i] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kCells3; i += 256) {
    const int cx = i % kCells - 1, cy = (i / kCells) % kCells - 1, cz = i / (kCells * kCells) - 1;
    uint8_t ok = 1;
#pragma unroll
    for (int k = 0; k < 8; k++) ok &= st[pad_index(cx + (k & 1), cy + ((k >> 1) & 1), cz + (k >> 2))] & 1;
    cell_ok[i] = ok;
  }
  __syncthreads();
  const int x = threadIdx.x & 15, y = threadIdx.x >> 4;
  uint32_t nv = 0, nt = 0;
  for (int z = 0; z < 16; z++) {
    const int o = st[pad_index(x, y, z)];
    uint32_t mask = 0;
    // edge along +x: the four cells at (x, y - {0,1}, z - {0,1}); likewise for the others
    if (((o ^ st[pad_index(x + 1, y, z)]) & 2) &&
        (cell_ok[cell_index(x, y, z)] | cell_ok[cell_index(x, y - 1, z)] | cell_ok[cell_index(x, y, z - 1)] | cell_ok[cell_index(x, y - 1, z - 1)]))
      mask |= 1u;
    if (((o ^ st[pad_index(x, y + 1, z)]) & 2) &&
        (cell_ok[cell_index(x, y, z)] | cell_ok[cell_index(x - 1, y, z)] | cell_ok[cell_index(x, y, z - 1)] | cell_ok[cell_index(x - 1, y, z - 1)]))
      mask |= 2u;
    if (((o ^ st[pad_index(x, y, z + 1)]) & 2) &&
        (cell_ok[cell_index(x, y, z)] | cell_ok[cell_index(x - 1, y, z)] | cell_ok[cell_index(x, y - 1, z)] | cell_ok[cell_index(x - 1, y - 1, z)]))
      mask |= 4u;
    uint32_t tris = 0;
    if (cell_ok[cell_index(x, y, z)]) {
      int cs = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) cs |= ((st[pad_index(x + (k & 1), y + ((k >> 1) & 1), z + (k >> 2))] >> 1) & 1) << k;
      tris = kMcNumTris[cs];
    }
    info[(size_t)b * kVox + z * 256 + threadIdx.x] = (uint8_t)(mask | (tris << 3));
    nv += __popc(mask);
    nt += tris;
  }
  if (nv) atomicAdd(&sums[0], nv);
  if (nt) atomicAdd(&sums[1], nt);
  __syncthreads();
  if (threadIdx.x == 0) {
    block_nv[b] = sums[0];
    block_nt[b] = sums[1];
    if (sums[0]) atomicAdd(&totals[0], (unsigned long long)sums[0]);
    if (sums[1]) atomicAdd(&totals[1], (unsigned long long)sums[1]);
  }
}

__global__ void extract_counts_kernel(const unsigned long long* __restrict__ totals, long long* __restrict__ counts2) {
  counts2[0] = (long long)totals[0];
  counts2[1] = (long long)totals[1];
}

// tsdf (and colour) of the voxel at local (x, y, z), one coordinate of which may be 16: the neighbour's first layer
struct Corner {
  int block;      // position in the key array, -1: absent
  size_t voxel;   // slot * 4096 + voxel index
};

// The vertices in (block, voxel, axis) order, and per voxel the number of its first vertex.
template <bool kColor>
__global__ void __launch_bounds__(256) extract_vertices_kernel(uint32_t n, const unsigned long long* __restrict__ keys, const int* __restrict__ slots,
                                                               const float* __restrict__ tsdf, const float* __restrict__ block_color, float voxel_size,
                                                               const uint8_t* __restrict__ info, const uint32_t* __restrict__ nv_incl,
                                                               uint32_t* __restrict__ vbase, uint32_t V, float* __restrict__ vertices,
                                                               float* __restrict__ colors) {
  __shared__ int nb[3];
  __shared__ uint32_t cnt[kVox + 256];
  __shared__ uint32_t part[256];
  const uint32_t b = blockIdx.x;
  int bc[3];
  unpack_key(keys[b], bc[0], bc[1], bc[2]);
  if (threadIdx.x < 3) {
    const int j = find_block(keys, n, bc[0] + (threadIdx.x == 0), bc[1] + (threadIdx.x == 1), bc[2] + (threadIdx.x == 2));
    nb[threadIdx.x] = j < 0 ? -1 : slots[j];
  }
  for (int i = threadIdx.x; i < kVox; i += 256) cnt[scan_index(i)] = __popc(info[(size_t)b * kVox + i] & 7u);
  __syncthreads();
  block_scan(cnt, part);
  const uint32_t first = b ? nv_incl[b - 1] : 0u;
  const int own = slots[b];
  const int l[3] = {(int)(threadIdx.x & 15), (int)(threadIdx.x >> 4), 0};
  for (int z = 0; z < 16; z++) {
    const int v = z * 256 + threadIdx.x;
    const uint32_t mask = info[(size_t)b * kVox + v] & 7u;
    uint32_t id = first + cnt[scan_index(v)];
    vbase[(size_t)b * kVox + v] = id;
    if (!mask) continue;
    const size_t o = (size_t)own * kVox + v;
    const float t_o = tsdf[o];
    const int X[3] = {16 * bc[0] + l[0], 16 * bc[1] + l[1], 16 * bc[2] + z};
    for (int a = 0; a < 3; a++) {
      if (!(mask >> a & 1u)) continue;
      const int loc = a == 2 ? z : l[a];
      const int stride = a == 0 ? 1 : (a == 1 ? 16 : 256);
      const int slot = loc == 15 ? nb[a] : own;
      if (slot < 0 || id >= V) { id++; continue; }   // cannot happen for a marked edge: its far corner belongs to a valid cell
      const size_t e = loc == 15 ? (size_t)slot * kVox + (v - 15 * stride) : o + stride;
      const float t_e = tsdf[e];
      const float ratio = (0.0f - t_o) / (t_e - t_o);
#pragma unroll
      for (int k = 0; k < 3; k++) vertices[3 * (size_t)id + k] = voxel_size * ((float)X[k] + (k == a ? ratio : 0.0f));
      if (kColor) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const float c_o = block_color[3 * o + k], c_e = block_color[3 * e + k];
          colors[3 * (size_t)id + k] = c_o + ratio * (c_e - c_o);
        }
      }
      id++;
    }
  }
}

// The faces in (block, voxel, table) order: the case of each cell from its eight corners, each triangle corner the vertex of an owned
// edge of the voxel at the cell's offset kMcEdgeInfo names.
__global__ void __launch_bounds__(256) extract_faces_kernel(uint32_t n, const unsigned long long* __restrict__ keys, const int* __restrict__ slots,
                                                            const float* __restrict__ tsdf, const uint8_t* __restrict__ info,
                                                            const uint32_t* __restrict__ nt_incl, const uint32_t* __restrict__ vbase, uint32_t F,
                                                            long long* __restrict__ faces) {
  __shared__ int nb_block[8], nb_slot[8];
  __shared__ uint32_t cnt[kVox + 256];
  __shared__ uint32_t part[256];
  const uint32_t b = blockIdx.x;
  int bx, by, bz;
  unpack_key(keys[b], bx, by, bz);
  if (threadIdx.x < 8) {
    const int j = find_block(keys, n, bx + (int)(threadIdx.x & 1), by + (int)((threadIdx.x >> 1) & 1), bz + (int)(threadIdx.x >> 2));
    nb_block[threadIdx.x] = j;
    nb_slot[threadIdx.x] = j < 0 ? -1 : slots[j];
  }
  for (int i = threadIdx.x; i < kVox; i += 256) cnt[scan_index(i)] = (info[(size_t)b * kVox + i] >> 3) & 7u;
  __syncthreads();
  block_scan(cnt, part);
  const uint32_t first = b ? nt_incl[b - 1] : 0u;
  const int x = threadIdx.x & 15, y = threadIdx.x >> 4;
  for (int z = 0; z < 16; z++) {
    const int v = z * 256 + threadIdx.x;
    const uint32_t tris = (info[(size_t)b * kVox + v] >> 3) & 7u;
    if (!tris) continue;
    int cs = 0;
    bool whole = true;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int cx = x + (k & 1), cy = y + ((k >> 1) & 1), cz = z + (k >> 2);
      const int slot = nb_slot[(cx >> 4) | ((cy >> 4) << 1) | ((cz >> 4) << 2)];
      if (slot < 0) { whole = false; continue; }
      cs |= (tsdf[(size_t)slot * kVox + (((cz & 15) * 16 + (cy & 15)) * 16 + (cx & 15))] < 0.0f ? 1 : 0) << k;
    }
    if (!whole) continue;   // cannot happen: the count pass saw all eight corners
    uint32_t fid = first + cnt[scan_index(v)];
    for (uint32_t t = 0; t < tris && t < RG_MC_MAX_TRIS; t++, fid++) {
      if (fid >= F) break;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const int e = kMcTriTable[cs][3 * t + k];
        long long id = -1;
        if (e >= 0) {
          const int ox = x + kMcEdgeInfo[e][0], oy = y + kMcEdgeInfo[e][1], oz = z + kMcEdgeInfo[e][2], axis = kMcEdgeInfo[e][3];
          const int j = nb_block[(ox >> 4) | ((oy >> 4) << 1) | ((oz >> 4) << 2)];
          if (j >= 0) {
            const size_t ov = (size_t)j * kVox + (((oz & 15) * 16 + (oy & 15)) * 16 + (ox & 15));
            id = (long long)vbase[ov] + __popc(info[ov] & ((1u << axis) - 1u));
          }
        }
        faces[3 * (size_t)fid + k] = id;
      }
    }
  }
}

struct ExtractView {
  uint8_t* info;
  uint32_t *vbase, *block_nv, *block_nt, *nv_incl, *nt_incl;
  unsigned long long* totals;
  void* temp;
  size_t temp_bytes, bytes;
};
static ExtractView extract_carve(long long N, void* base) {
  const size_t n = (size_t)N;
  rg::Carver c(base);
  ExtractView v;
  v.temp_bytes = rg::scan_temp_bytes(n);
  v.info = c.take<uint8_t>(n * kVox);
  v.vbase = c.take<uint32_t>(n * kVox);
  for (uint32_t** a : {&v.block_nv, &v.block_nt, &v.nv_incl, &v.nt_incl}) *a = c.take<uint32_t>(n);
  v.totals = c.take<unsigned long long>(2);
  v.temp = c.take<char>(v.temp_bytes);
  v.bytes = c.off;
  return v;
}

static bool camera_ok(const float* cam16) {
  if (!cam16) return false;
  for (int k = 0; k < 16; k++)
    if (!isfinite(cam16[k])) return false;
  return cam16[0] != 0.0f && cam16[1] != 0.0f;
}
static Camera camera_of(const float* cam16) {
  Camera c;
  c.fx = cam16[0];
  c.fy = cam16[1];
  c.cx = cam16[2];
  c.cy = cam16[3];
  for (int k = 0; k < 12; k++) c.m[k] = cam16[4 + k];
  return c;
}
static bool positive(float v) { return v > 0.0f && isfinite(v); }

}  // namespace rgts

extern "C" {

size_t radegs_tsdf_unique_bytes(long long n) {
  if (n <= 0 || (unsigned long long)n >= rg::kMaxItems) return 0;
  return rgts::unique_carve(n, nullptr).bytes;
}

int radegs_tsdf_touch(int W, int H, const float* depth, const float* cam16, float depth_scale, float depth_max, float sdf_trunc, float block_size,
                      void* workspace, size_t workspace_bytes, long long* counts3, void* stream_v) {
  if (W < 1 || H < 1 || !counts3 || !rgts::camera_ok(cam16) || !rgts::positive(depth_scale) || !rgts::positive(depth_max) || !rgts::positive(sdf_trunc) ||
      !rgts::positive(block_size))
    return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const long long samples = (long long)(W / 4) * (H / 4), n = 4 * samples;
  if ((unsigned long long)n >= rg::kMaxItems) return RADEGS_ERR_TOO_LARGE;
  if (n == 0) return hipMemsetAsync(counts3, 0, 3 * sizeof(long long), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if (!depth || !workspace || workspace_bytes < radegs_tsdf_unique_bytes(n) || !rg::aligned16(workspace)) return RADEGS_ERR_INVALID_ARG;
  const rgts::UniqueView w = rgts::unique_carve(n, workspace);
  if (hipMemsetAsync(w.flag, 0, 4, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgts::touch_keys_kernel, dim3(rg::blocks_of((size_t)samples)), dim3(256), 0, s, W, H, depth, rgts::camera_of(cam16), depth_scale,
                     depth_max, sdf_trunc, block_size, w.lo, w.hi, w.flag);
  return rgts::unique_run((uint32_t)n, w, 0u, nullptr, counts3, s);
}

int radegs_tsdf_unique_plan(long long n, const int* coords, long long ngrid, const unsigned long long* grid_keys, void* workspace,
                            size_t workspace_bytes, long long* counts3, void* stream_v) {
  if (n < 0 || ngrid < 0 || !counts3 || (ngrid && !grid_keys)) return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)n >= rg::kMaxItems || (unsigned long long)ngrid >= rg::kMaxItems) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (n == 0) return hipMemsetAsync(counts3, 0, 3 * sizeof(long long), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if (!coords || !workspace || workspace_bytes < radegs_tsdf_unique_bytes(n) || !rg::aligned16(workspace)) return RADEGS_ERR_INVALID_ARG;
  const rgts::UniqueView w = rgts::unique_carve(n, workspace);
  if (hipMemsetAsync(w.flag, 0, 4, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgts::coords_keys_kernel, dim3(rg::blocks_of((size_t)n)), dim3(256), 0, s, (uint32_t)n, coords, w.lo, w.hi, w.flag);
  return rgts::unique_run((uint32_t)n, w, (uint32_t)ngrid, grid_keys, counts3, s);
}

int radegs_tsdf_unique_emit(long long n, const void* workspace, long long n_unique, int* coords_out, void* stream) {
  if (n < 0 || n_unique < 0 || n_unique > n) return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)n >= rg::kMaxItems) return RADEGS_ERR_TOO_LARGE;
  if (n == 0 || n_unique == 0) return 0;
  if (!workspace || !coords_out) return RADEGS_ERR_INVALID_ARG;
  const rgts::UniqueView w = rgts::unique_carve(n, const_cast<void*>(workspace));
  hipLaunchKernelGGL(rgts::unique_emit_kernel, dim3(rg::blocks_of((size_t)n)), dim3(256), 0, static_cast<hipStream_t>(stream), (uint32_t)n, w.sorted,
                     w.first, w.first_incl, (uint32_t)n_unique, coords_out);
  return rg::launch_status();
}

int radegs_tsdf_insert_apply(long long n, const void* workspace, long long ngrid, const unsigned long long* grid_keys, const int* grid_slots,
                             long long n_unique, long long n_new, unsigned long long* new_keys, int* new_slots, int* active_slots,
                             int* active_coords, void* stream_v) {
  if (n < 0 || ngrid < 0 || n_unique < 0 || n_new < 0 || n_new > n_unique || n_unique > n) return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)n >= rg::kMaxItems || (unsigned long long)(ngrid + n_new) >= 0x7FFFFFFFull) return RADEGS_ERR_TOO_LARGE;
  if ((ngrid && (!grid_keys || !grid_slots)) || ((ngrid + n_new) && (!new_keys || !new_slots)) || (n_unique && (!active_slots || !active_coords)) ||
      (n && !workspace))
    return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const rgts::UniqueView w = n ? rgts::unique_carve(n, const_cast<void*>(workspace)) : rgts::UniqueView{};
  const uint32_t total = (uint32_t)(ngrid + n_new);
  if (ngrid)
    hipLaunchKernelGGL(rgts::insert_old_kernel, dim3(rg::blocks_of((size_t)ngrid)), dim3(256), 0, s, (uint32_t)ngrid, grid_keys, grid_slots, (uint32_t)n,
                       w.sorted, w.fresh_incl, total, new_keys, new_slots);
  if (n)
    hipLaunchKernelGGL(rgts::insert_new_kernel, dim3(rg::blocks_of((size_t)n)), dim3(256), 0, s, (uint32_t)n, w.sorted, w.first, w.fresh, w.pos,
                       w.first_incl, w.fresh_incl, (uint32_t)ngrid, grid_slots, (uint32_t)n_unique, total, new_keys, new_slots, active_slots,
                       active_coords);
  return rg::launch_status();
}

int radegs_tsdf_integrate(long long n_active, const int* active_slots, const int* active_coords, long long capacity, int W, int H, const float* depth,
                          const float* color, const float* cam16, float depth_scale, float depth_max, float sdf_trunc, float* tsdf, float* weight,
                          float* block_color, void* stream) {
  if (n_active < 0 || capacity < 0 || W < 1 || H < 1 || (long long)W * H >= (1ll << 31) || !rgts::camera_ok(cam16) || !rgts::positive(depth_scale) ||
      !rgts::positive(depth_max) || !rgts::positive(sdf_trunc) || (color == nullptr) != (block_color == nullptr))
    return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)n_active >= 0x7FFFFFFFull || (unsigned long long)capacity >= 0x7FFFFFFFull) return RADEGS_ERR_TOO_LARGE;
  if (n_active == 0) return 0;
  if (!active_slots || !active_coords || !depth || !tsdf || !weight) return RADEGS_ERR_INVALID_ARG;
  const rgts::Camera c = rgts::camera_of(cam16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (color)
    hipLaunchKernelGGL(rgts::fuse_view_kernel<true>, dim3((unsigned)n_active), dim3(256), 0, s, active_slots, active_coords, (uint32_t)capacity, W, H, depth,
                       color, c, depth_scale, depth_max, sdf_trunc, tsdf, weight, block_color);
  else
    hipLaunchKernelGGL(rgts::fuse_view_kernel<false>, dim3((unsigned)n_active), dim3(256), 0, s, active_slots, active_coords, (uint32_t)capacity, W, H, depth,
                       color, c, depth_scale, depth_max, sdf_trunc, tsdf, weight, block_color);
  return rg::launch_status();
}

size_t radegs_tsdf_extract_bytes(long long n) {
  if (n <= 0 || (unsigned long long)n >= (1ull << 19)) return 0;   // 2^19 blocks: every voxel index below 2^31
  return rgts::extract_carve(n, nullptr).bytes;
}

int radegs_tsdf_extract_plan(long long n, const unsigned long long* keys, const int* slots, const float* tsdf, const float* weight,
                             float weight_threshold, void* workspace, size_t workspace_bytes, long long* counts2, void* stream_v) {
  if (n < 0 || !counts2 || weight_threshold != weight_threshold) return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)n >= (1ull << 19)) return RADEGS_ERR_TOO_LARGE;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (n == 0) return hipMemsetAsync(counts2, 0, 2 * sizeof(long long), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if (!keys || !slots || !tsdf || !weight || !workspace || workspace_bytes < radegs_tsdf_extract_bytes(n) || !rg::aligned16(workspace))
    return RADEGS_ERR_INVALID_ARG;
  const rgts::ExtractView w = rgts::extract_carve(n, workspace);
  if (hipMemsetAsync(w.totals, 0, 16, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgts::extract_count_kernel, dim3((unsigned)n), dim3(256), 0, s, (uint32_t)n, keys, slots, tsdf, weight, weight_threshold, w.info,
                     w.block_nv, w.block_nt, w.totals);
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, w.block_nv, nullptr, w.nv_incl, (size_t)n, s) != hipSuccess) return RADEGS_ERR_HIP;
  if (rg::inclusive_scan_gather_u32(w.temp, w.temp_bytes, w.block_nt, nullptr, w.nt_incl, (size_t)n, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgts::extract_counts_kernel, dim3(1), dim3(1), 0, s, w.totals, counts2);
  return rg::launch_status();
}

int radegs_tsdf_extract_emit(long long n, const unsigned long long* keys, const int* slots, const float* tsdf, const float* block_color,
                             float voxel_size, const void* workspace, long long V, long long F, float* vertices, long long* faces, float* colors,
                             void* stream_v) {
  if (n < 0 || V < 0 || F < 0 || !rgts::positive(voxel_size)) return RADEGS_ERR_INVALID_ARG;
  if ((unsigned long long)n >= (1ull << 19) || (unsigned long long)V >= 0xFFFFFFFFull || (unsigned long long)F >= 0xFFFFFFFFull) return RADEGS_ERR_TOO_LARGE;
  if (n == 0 || (V == 0 && F == 0)) return 0;
  if (!keys || !slots || !tsdf || !workspace || (V && !vertices) || (F && !faces) || (V && (block_color == nullptr) != (colors == nullptr)))
    return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  const rgts::ExtractView w = rgts::extract_carve(n, const_cast<void*>(workspace));
  if (block_color)
    hipLaunchKernelGGL(rgts::extract_vertices_kernel<true>, dim3((unsigned)n), dim3(256), 0, s, (uint32_t)n, keys, slots, tsdf, block_color, voxel_size, w.info,
                       w.nv_incl, w.vbase, (uint32_t)V, vertices, colors);
  else
    hipLaunchKernelGGL(rgts::extract_vertices_kernel<false>, dim3((unsigned)n), dim3(256), 0, s, (uint32_t)n, keys, slots, tsdf, block_color, voxel_size,
                       w.info, w.nv_incl, w.vbase, (uint32_t)V, vertices, colors);
  hipLaunchKernelGGL(rgts::extract_faces_kernel, dim3((unsigned)n), dim3(256), 0, s, (uint32_t)n, keys, slots, tsdf, w.info, w.nt_incl, w.vbase, (uint32_t)F,
                     faces);
  return rg::launch_status();
}

}  // extern "C"
