// radegs_densify.hip -- adaptive density control: the stage of the training iteration that follows the backward,
//     GaussianModel.add_densification_stats + train.py:186's max_radii2D update     every iteration, in place, one launch
//     GaussianModel.densify_and_prune (scene/gaussian_model.py:717-741)             every densification_interval iterations
// densify_and_prune is split in two around the ONE host read it needs (the new row count sizes the new tensors):
//   plan   decide_kernel    one pass over the P input Gaussians: every decision of clone / split / final prune as six 0/1 rows
//          rg::inclusive_scan_gather_u32 (radegs_sort.hip) over the 6 P flags: the four candidate segments laid end to end in
//                           upstream's output order ARE the output order, so one scan numbers every surviving row; the two
//                           extra segments count the clone- and split-selected rows for upstream's report
//          index_kernel     inverts the numbering: source row (and which candidate of it) of every output row + the 4 counts
//   apply  apply_kernel     one pass over the OUTPUT: all 18 arrays (6 parameters, 6 exp_avg, 6 exp_avg_sq) at their final size
// Upstream rewrites all of them four times (cat, cat, mask, mask).  Candidates of source row i, in output order of their segments:
//   0 the row itself (unless split-selected)   1 its clone   2 / 3 its first / second split child
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/radegs.h"
#include "rg_prims.h"
#include "rg_workspace.h"

namespace rgd {

constexpr uint32_t kSegShift = 30, kRowMask = (1u << kSegShift) - 1u;
constexpr int kNumTensors = RADEGS_DENSIFY_NUM_TENSORS, kPerThread = 4, kChunk = 256 * 4 * kPerThread;
enum Kind : int { kCopy = 0, kXyz = 1, kScaling = 2, kMoment = 3 };

// ---------------------------------------------------------------- statistics ----------------------------------------------------------------
// REDUCED = false: one view's screen-space gradient [P,3] (xy signed, column 2 the abs-gradient); visible = mask[i] or radii[i] > 0.
// REDUCED = true:  view_parallel's [P,3] (sum |grad xy|, sum |grad abs|, number of ranks that saw the Gaussian) and radii_max.
template <bool REDUCED>
__global__ void __launch_bounds__(256) stats_kernel(int P, const float* __restrict__ g3, const int* __restrict__ radii, const uint8_t* __restrict__ mask,
                                                    float* __restrict__ accum, float* __restrict__ accum_abs, float* __restrict__ accum_abs_max,
                                                    float* __restrict__ denom, float* __restrict__ max_radii2D) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float c0 = g3[3 * (size_t)i], c1 = g3[3 * (size_t)i + 1], c2 = g3[3 * (size_t)i + 2];
  const int r = radii ? radii[i] : 0;
  float add, add_abs, add_n;
  bool vis;
  if (REDUCED) {
    vis = c2 != 0.0f;
    add = c0; add_abs = c1; add_n = c2;
  } else {
    vis = mask ? mask[i] != 0 : r > 0;
    add = sqrtf(c0 * c0 + c1 * c1); add_abs = fabsf(c2); add_n = 1.0f;
  }
  if (!vis) return;
  accum[i] += add;
  accum_abs[i] += add_abs;
  const float m = accum_abs_max[i];
  accum_abs_max[i] = (m > add_abs || m != m) ? m : add_abs;   // a NaN on either side stays, as in upstream's torch.max (fmaxf would drop it)
  denom[i] += add_n;
  if (max_radii2D && radii) max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
}

// ------------------------------------------------------------------- plan -------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ void __launch_bounds__(256) decide_kernel(int P, const float* __restrict__ accum, const float* __restrict__ accum_abs,
                                                     const float* __restrict__ denom, const float* __restrict__ scaling_raw,
                                                     const float* __restrict__ opacity_raw, float max_grad, const float* __restrict__ q_dev,
                                                     float dense_threshold, float min_opacity, int prune_big, float big_threshold,
                                                     uint32_t* __restrict__ flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float d = denom[i];
  float g = accum[i] / d, ga = accum_abs[i] / d;   // IEEE divide: 0/0 = NaN -> 0, x/0 = Inf stays
  if (g != g) g = 0.0f;
  if (ga != ga) ga = 0.0f;
  const bool hot = fabsf(g) >= max_grad || ga >= *q_dev;
  float smax = 0.0f, cmax = 0.0f;   // largest activated scale of the row itself (= of its clone) and of its split children
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float s = expf(scaling_raw[3 * (size_t)i + k]);
    smax = fmaxf(smax, s);
    cmax = fmaxf(cmax, expf(logf(s / 1.6f)));   // the children are pruned on exp() of the raw value they store
  }
  const bool clone = hot && smax <= dense_threshold, split = hot && smax > dense_threshold;
  const bool faint = sigmoidf(opacity_raw[i]) < min_opacity;
  const bool drop = faint || (prune_big && smax > big_threshold), drop_child = faint || (prune_big && cmax > big_threshold);
  const size_t n = (size_t)P;
  flags[i] = !split && !drop;
  flags[n + i] = clone && !drop;
  flags[2 * n + i] = flags[3 * n + i] = split && !drop_child;
  flags[4 * n + i] = clone;
  flags[5 * n + i] = split;
}

// src_of[output row] = source row | candidate << 30;  counts = {rows out, clone-selected, split-selected, pruned by the final prune}
__global__ void __launch_bounds__(256) index_kernel(uint32_t P, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ incl,
                                                    uint32_t* __restrict__ src_of, int* __restrict__ counts) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;   // position in the four candidate segments
  if (j == 0) {
    const uint32_t out = incl[4 * (size_t)P - 1], clones = incl[5 * (size_t)P - 1] - out, splits = incl[6 * (size_t)P - 1] - incl[5 * (size_t)P - 1];
    counts[0] = (int)out; counts[1] = (int)clones; counts[2] = (int)splits; counts[3] = (int)(P + clones + splits - out);
  }
  if (j >= 4u * P) return;
  if (flags[j]) {
    const uint32_t seg = j / P;
    src_of[incl[j] - 1] = (j - seg * P) | (seg << kSegShift);
  }
}

// ------------------------------------------------------------------- apply ------------------------------------------------------------------
struct Table {
  const float* in[kNumTensors]; float* out[kNumTensors];
  unsigned width[kNumTensors], kind[kNumTensors], block_start[kNumTensors + 1];
  int count;
  unsigned rows_out;
  const float* scaling; const float* rotation; const float* z;   // [P,3] raw, [P,4] raw, [P,3,3]
  const uint32_t* src_of;
};

struct __attribute__((packed, aligned(4))) f4u { float x, y, z, w; };   // four consecutive floats of a row: 4-byte aligned only

// offset of a clone / split child from its source: component c of R(q/|q|) (z o s)
__device__ __forceinline__ float sample_offset(const Table& t, uint32_t s, uint32_t seg, uint32_t c) {
  const float* q = t.rotation + 4 * (size_t)s;
  float w = q[0], x = q[1], y = q[2], z = q[3];
  const float inv = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
  w *= inv; x *= inv; y *= inv; z *= inv;
  float r0, r1, r2;   // row c of the rotation matrix of the unit quaternion (w, x, y, z)
  if (c == 0)      { r0 = 1.0f - 2.0f * (y * y + z * z); r1 = 2.0f * (x * y - w * z); r2 = 2.0f * (x * z + w * y); }
  else if (c == 1) { r0 = 2.0f * (x * y + w * z); r1 = 1.0f - 2.0f * (x * x + z * z); r2 = 2.0f * (y * z - w * x); }
  else             { r0 = 2.0f * (x * z - w * y); r1 = 2.0f * (y * z + w * x); r2 = 1.0f - 2.0f * (x * x + y * y); }
  const float* zz = t.z + 9 * (size_t)s + 3 * (seg - 1);
  const float* sc = t.scaling + 3 * (size_t)s;
  return r0 * (zz[0] * expf(sc[0])) + r1 * (zz[1] * expf(sc[1])) + r2 * (zz[2] * expf(sc[2]));
}

// Flat-element addressing over the output: a thread owns kPerThread groups of four consecutive floats of one output array (one 16-byte
// store each; every array starts 16-byte aligned or takes the word path), a block 4096 floats.  Surviving originals keep their order,
// so a run of output rows whose sources are consecutive is one contiguous piece of the input, shifted: one 16-byte load at 4-byte
// alignment.  Only where the four floats straddle a removed row, a new row or the array's end does the thread go float by float.
// The row table is read for all of a thread's groups before the first of their loads is issued, and those before the first store: the
// table -> data dependency is two memory round trips, and the bytes in flight are what this kernel runs on.
__device__ __forceinline__ void apply_words(const Table& t, const float* __restrict__ in, float* __restrict__ out, uint32_t W, uint32_t kind, uint32_t n,
                                            uint32_t e0, uint32_t r, uint32_t c, uint32_t code, bool wide) {
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    v[k] = 0.0f;
    if (e0 + k < n) {
      const uint32_t seg = code >> kSegShift, s = code & kRowMask;
      float x = 0.0f;
      if (kind != kMoment || seg == 0) x = in[(size_t)s * W + c];   // new rows start with zero moments
      if (kind == kXyz && seg != 0) x = x + sample_offset(t, s, seg, c);
      if (kind == kScaling && seg >= 2) x = logf(expf(x) / 1.6f);
      v[k] = x;
      if (++c == W) { c = 0; r++; if (e0 + k + 1 < n) code = t.src_of[r]; }
    }
  }
  if (wide) {
    *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < 4; k++)
      if (e0 + k < n) out[e0 + k] = v[k];
  }
}

__global__ void __launch_bounds__(256) apply_kernel(const Table t) {
  int ti = 0;
#pragma unroll 1
  while (ti + 1 < t.count && blockIdx.x >= t.block_start[ti + 1]) ti++;
  const float* __restrict__ in = t.in[ti];
  float* __restrict__ out = t.out[ti];
  const uint32_t W = t.width[ti], kind = t.kind[ti];
  const uint32_t n = t.rows_out * W;   // < 2^32 - 4096: checked by the launcher
  const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  const uint32_t base = (blockIdx.x - t.block_start[ti]) * (uint32_t)kChunk;
  uint32_t e0[kPerThread], r0[kPerThread], c0[kPerThread], dr[kPerThread], code0[kPerThread], code3[kPerThread];
#pragma unroll
  for (int u = 0; u < kPerThread; u++) {
    e0[u] = base + u * 1024 + threadIdx.x * 4;
    const bool live = e0[u] < n;
    r0[u] = live ? e0[u] / W : 0u;
    c0[u] = live ? e0[u] - r0[u] * W : 0u;
    uint32_t c3 = c0[u] + 3;
    dr[u] = 0;
    while (c3 >= W) { c3 -= W; dr[u]++; }
    const bool wide = aligned && e0[u] + 3 < n;   // all four floats exist (the row r0 + dr then does too)
    code0[u] = live ? t.src_of[r0[u]] : 0u;
    code3[u] = wide ? t.src_of[r0[u] + dr[u]] : 0xFFFFFFFFu;
  }
  bool fast[kPerThread];
  f4u v[kPerThread];
#pragma unroll
  for (int u = 0; u < kPerThread; u++) {
    // both ends surviving originals (candidate 0: the code IS the source row) whose sources are as far apart as they are: so is
    // every row in between, sources of originals being strictly increasing
    fast[u] = (code0[u] | code3[u]) <= kRowMask && code3[u] - code0[u] == dr[u];
    if (fast[u]) v[u] = *reinterpret_cast<const f4u*>(in + (size_t)code0[u] * W + c0[u]);
  }
#pragma unroll
  for (int u = 0; u < kPerThread; u++)
    if (fast[u]) *reinterpret_cast<float4*>(out + e0[u]) = make_float4(v[u].x, v[u].y, v[u].z, v[u].w);
#pragma unroll
  for (int u = 0; u < kPerThread; u++)
    if (!fast[u] && e0[u] < n) apply_words(t, in, out, W, kind, n, e0[u], r0[u], c0[u], code0[u], code3[u] != 0xFFFFFFFFu);
}

struct Workspace { uint32_t *flags, *incl, *src_of; void* scan_temp; size_t scan_bytes, bytes; };

static Workspace carve(int P, void* base) {
  const size_t n = (size_t)P;
  rg::Carver c(base);
  Workspace v;
  v.scan_bytes = rg::scan_temp_bytes(6 * n);
  v.src_of = c.take<uint32_t>(2 * n);   // first: radegs_densify_apply finds it at the start.  At most 2 P rows come out (clone and split exclude each other)
  v.flags = c.take<uint32_t>(6 * n);
  v.incl = c.take<uint32_t>(6 * n);
  v.scan_temp = c.take<char>(v.scan_bytes);
  v.bytes = c.off;
  return v;
}

}  // namespace rgd

extern "C" {

int radegs_densify_stats(int P, const float* grad_means2D, const int* radii, const unsigned char* visible, float* accum, float* accum_abs,
                         float* accum_abs_max, float* denom, float* max_radii2D, void* stream) {
  if (P < 0) return RADEGS_ERR_INVALID_ARG;
  if (P == 0) return 0;
  if (!grad_means2D || (!radii && !visible) || !accum || !accum_abs || !accum_abs_max || !denom) return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgd::stats_kernel<false>, dim3(rg::blocks_of((size_t)P)), dim3(256), 0, static_cast<hipStream_t>(stream), P, grad_means2D, radii, visible,
                     accum, accum_abs, accum_abs_max, denom, max_radii2D);
  return rg::launch_status();
}

int radegs_densify_stats_reduced(int P, const float* densify_stats, const int* radii_max, float* accum, float* accum_abs, float* accum_abs_max,
                                 float* denom, float* max_radii2D, void* stream) {
  if (P < 0) return RADEGS_ERR_INVALID_ARG;
  if (P == 0) return 0;
  if (!densify_stats || !accum || !accum_abs || !accum_abs_max || !denom) return RADEGS_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rgd::stats_kernel<true>, dim3(rg::blocks_of((size_t)P)), dim3(256), 0, static_cast<hipStream_t>(stream), P, densify_stats, radii_max,
                     static_cast<const uint8_t*>(nullptr), accum, accum_abs, accum_abs_max, denom, max_radii2D);
  return rg::launch_status();
}

size_t radegs_densify_plan_bytes(int P) { return P <= 0 ? 0 : rgd::carve(P, nullptr).bytes; }

int radegs_densify_plan(int P, const float* accum, const float* accum_abs, const float* denom, const float* scaling_raw, const float* opacity_raw,
                        float max_grad, const float* abs_threshold, float dense_threshold, float min_opacity, int prune_big, float big_threshold,
                        void* workspace, size_t workspace_bytes, int* counts4, void* stream_v) {
  if (P < 0 || P > RADEGS_DENSIFY_MAX_P || !counts4) return RADEGS_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream_v);
  if (P == 0) return hipMemsetAsync(counts4, 0, 4 * sizeof(int), s) == hipSuccess ? 0 : RADEGS_ERR_HIP;
  if (!accum || !accum_abs || !denom || !scaling_raw || !opacity_raw || !abs_threshold || !workspace ||
      workspace_bytes < radegs_densify_plan_bytes(P) || !rg::aligned16(workspace))
    return RADEGS_ERR_INVALID_ARG;
  const rgd::Workspace w = rgd::carve(P, workspace);
  hipLaunchKernelGGL(rgd::decide_kernel, dim3(rg::blocks_of((size_t)P)), dim3(256), 0, s, P, accum, accum_abs, denom, scaling_raw, opacity_raw, max_grad,
                     abs_threshold, dense_threshold, min_opacity, prune_big, big_threshold, w.flags);
  if (rg::inclusive_scan_gather_u32(w.scan_temp, w.scan_bytes, w.flags, nullptr, w.incl, 6 * (size_t)P, s) != hipSuccess) return RADEGS_ERR_HIP;
  hipLaunchKernelGGL(rgd::index_kernel, dim3(rg::blocks_of(4 * (size_t)P)), dim3(256), 0, s, (uint32_t)P, w.flags, w.incl, w.src_of, counts4);
  return rg::launch_status();
}

int radegs_densify_apply(int P, int P_out, int rest_floats, const RadegsDensifyTensors* tensors, const float* unit_normals, const void* workspace,
                         void* stream) {
  if (P < 0 || P > RADEGS_DENSIFY_MAX_P || P_out < 0 || (long long)P_out > 2 * (long long)P || rest_floats < 0 || !tensors) return RADEGS_ERR_INVALID_ARG;
  if (P_out == 0) return 0;
  if (!workspace || !unit_normals) return RADEGS_ERR_INVALID_ARG;
  static const unsigned widths[6] = {3, 3, 0, 1, 3, 4};
  static const unsigned kinds[6] = {rgd::kXyz, rgd::kCopy, rgd::kCopy, rgd::kCopy, rgd::kScaling, rgd::kCopy};
  for (int k = 0; k < 6; k++)   // the six parameters are not optional (f_rest only where it has columns); moments are, group by group
    if ((k != 2 || rest_floats > 0) && (!tensors->in[k] || !tensors->out[k])) return RADEGS_ERR_INVALID_ARG;
  rgd::Table t{};
  unsigned long long blocks = 0;
  int n = 0;
  for (int k = 0; k < rgd::kNumTensors; k++) {
    const unsigned W = k % 6 == 2 ? (unsigned)rest_floats : widths[k % 6];
    if (W == 0 || (!tensors->in[k] && !tensors->out[k])) continue;
    if (!tensors->in[k] || !tensors->out[k] || (unsigned long long)P_out * W >= 0xFFFFF000ull) return RADEGS_ERR_INVALID_ARG;   // 32-bit element index
    t.in[n] = tensors->in[k]; t.out[n] = tensors->out[k]; t.width[n] = W; t.kind[n] = k < 6 ? kinds[k] : (unsigned)rgd::kMoment;
    t.block_start[n] = (unsigned)blocks;
    blocks += ((unsigned long long)P_out * W + rgd::kChunk - 1) / rgd::kChunk;
    n++;
  }
  if (blocks > 0x7FFFFFFFull) return RADEGS_ERR_INVALID_ARG;
  t.block_start[n] = (unsigned)blocks;
  t.count = n; t.rows_out = (unsigned)P_out;
  t.scaling = tensors->in[4]; t.rotation = tensors->in[5]; t.z = unit_normals;
  t.src_of = static_cast<const uint32_t*>(workspace);
  hipLaunchKernelGGL(rgd::apply_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), t);
  return rg::launch_status();
}

}  // extern "C"
