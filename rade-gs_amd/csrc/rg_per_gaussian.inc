// rg_per_gaussian.inc -- the kernels with one thread per Gaussian; included by radegs_kernels.hip inside namespace rg (after CamArgs /
// load_camera and kDepthKeyBase, all they share with the binning and blend code).
//
//   forward    preprocess_fwd_kernel<INTE> (rg_preprocess.h), mark_visible_kernel
//   backward   drgb_clamped_kernel, preprocess_bwd_kernel (rg_preprocess_bwd.h) in named phases: SlabMap and the slab_* moves (the SH slab
//              through LDS), AccRecord (the accumulator record as it lies in memory), store_grads
//   view-parallel SH gradient   sh_grad_from_views_kernel (same slab)

// =========================================================================== preprocess ==
struct PreFwdArgs {
  int P, D, M;
  const float* means3D; const float* scales; const float* rotations; const float* cov3D_precomp;
  const float* opacities; const float* shs; const float* colors_precomp;
  CamArgs cam;
  int write_b;
  int* radii; float4* splat_a; float4* splat_b; uint32_t* tiles_touched; uint32_t* depth_key; uint8_t* clamped;
  float4* inte_rec;  // [P][2] {icr0..icr3 | icr4, icr5, well, 0}; INTE kernel only
  uint32_t* rect;    // [P] packed tile rectangle
  uint32_t* key_overflow;   // mapped host word (or null): set when a visible depth key does not fit the 27-bit window of the 3-pass sort
};

template <bool INTE>
__global__ void __launch_bounds__(256) preprocess_fwd_kernel(const PreFwdArgs a) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.P) return;
  const Camera cam = load_camera(a.cam);
  SplatFwd s;
  const float* m = a.means3D + 3 * (size_t)idx;
  const v3 p_orig = mk3(m[0], m[1], m[2]);
  const float* sh = a.shs ? a.shs + (size_t)idx * a.M * 3 : nullptr;
  const float* color_in = a.colors_precomp ? a.colors_precomp + 3 * (size_t)idx : nullptr;
  const float* scale3 = a.scales ? a.scales + 3 * (size_t)idx : nullptr;
  const float* quat4 = a.rotations ? a.rotations + 4 * (size_t)idx : nullptr;
  const float* cov_in = a.cov3D_precomp ? a.cov3D_precomp + 6 * (size_t)idx : nullptr;
  preprocess_fwd<INTE>(p_orig, scale3, quat4, cov_in, a.opacities[idx], a.D, sh, color_in, cam, s);
  a.radii[idx] = s.radius;
  a.tiles_touched[idx] = (uint32_t)s.tiles;
  a.rect[idx] = s.radius > 0 ? s.rect : 0u;
  // positive floats order like unsigned ints; invisible Gaussians sort to the very end
  a.depth_key[idx] = s.radius > 0 ? __float_as_uint(s.depth) : 0xFFFFFFFFu;
  // the depth sort runs three 9-bit passes over (key - bits(0.2f)) when every visible key fits 27 bits, i.e. z < 13 107 (rg_launch.inc);
  // a key outside raises the flag the host looks at before it trusts the order (and redoes the forward with the 4-pass sort)
  if (a.key_overflow && s.radius > 0 && __float_as_uint(s.depth) - kDepthKeyBase >= (1u << 27))
    __hip_atomic_store(a.key_overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (s.radius > 0) {
    float4* ra = a.splat_a + 4 * (size_t)idx;
    ra[0] = make_float4(s.mx, s.my, s.cx, s.cy);
    ra[1] = make_float4(s.cz, s.op, skip_threshold(s.op), s.ts);
    ra[2] = make_float4(s.rgb[0], s.rgb[1], s.rgb[2], s.rp[0]);
    ra[3] = make_float4(s.rp[1], s.nrm[0], s.nrm[1], s.nrm[2]);
    if (a.write_b) {
      float4* rb = a.splat_b + 3 * (size_t)idx;
      rb[0] = make_float4(s.cp[0], s.cp[1], s.cp[2], s.cp[3]);
      rb[1] = make_float4(s.cp[4], s.cp[5], s.vp[0], s.vp[1]);
      rb[2] = make_float4(s.vp[2], 0.f, 0.f, 0.f);
    }
    a.clamped[idx] = (uint8_t)s.clamped;   // bits 0..2: SH clamp flags
    if constexpr (INTE) {
      float4* ri = a.inte_rec + 2 * (size_t)idx;
      ri[0] = make_float4(s.icr[0], s.icr[1], s.icr[2], s.icr[3]);
      ri[1] = make_float4(s.icr[4], s.icr[5], s.well ? 1.0f : 0.0f, 0.f);
    }
  }
}

__global__ void __launch_bounds__(256) mark_visible_kernel(int P, const float* means3D, const float* view, unsigned char* present) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P) return;
  const float* m = means3D + 3 * (size_t)idx;
  v3 pv = xform43(mk3(m[0], m[1], m[2]), view);
  present[idx] = !(pv.z <= 0.2f);
}

// ======================================================================= preprocess, bwd ==
// What the accumulator records hold when preprocess_bwd_kernel reads them (SplatAcc order, 16 | 32 floats; rg_layout.h).
enum class RecordKind : int {
  reference_sums,   // the reference's FINAL per-Gaussian sums, constant factors applied: radegs_backward_from_sums
  blend_sums,       // the reference's sums with the constant factors (1/focal, W/2, H/2) pending: a backward that launched no blend (R == 0)
                    // over its zeroed accumulator.  Not a case of raw_moments: the conversion would change the sign of a zero
  raw_moments,      // components 9..14 are raw moments of h = opacity G dL/dalpha (what every blend backward leaves, rg_streams.inc), the
                    // constant factors pending: the mean2D / conic sums are formed here, once per Gaussian
};

struct PreBwdArgs {
  int P, D, M;
  const float* means3D; const float* scales; const float* rotations; const float* cov3D_precomp; const float* shs;
  const int* radii; const float4* splat_a; const uint8_t* clamped;
  float* acc; int rec;        // the records, `rec` floats each; only `keep` and `rezero` write to them
  CamArgs cam;
  float* dL_dmean2D; float* dL_dcolor; float* dL_dopacity; float* dL_dmean3D; float* dL_dcov3D; float* dL_dsh; float* dL_dscale;
  float* dL_drot;
  float* dL_drgb_clamped;  // optional [P,3]: dL/dRGB with the clamp mask applied (the view-parallel factored exchange)
  int opacity_grad_intended;  // RadegsBwdArgs::opacity_grad_intended (include/radegs.h)
  RecordKind kind;
  int keep;                   // raw_moments: every visible record is written back in the reference's form (debugging / tests: RadegsBwdArgs::keep_sums)
  int rezero;                 // clear every consumed record (RadegsBwdArgs::acc_reuse): the accumulator goes back to its owner all zeros
  int drgb_done;              // dL_drgb_clamped was already written by drgb_clamped_kernel (RadegsBwdArgs::drgb_ready)
  int vec_slab;               // the SH slab moves in 16-byte pieces (3M % 4 == 0, 3M <= 48, shs and dL_dsh 16-byte aligned)
  int first_block;            // this launch covers the Gaussians from first_block * 128 on (RadegsBwdArgs::grad_chunks)
};

// dL/dRGB with the SH clamp mask applied, straight from the blend backward's sums (the first three floats of every accumulator
// record): what the factored view-parallel exchange all-gathers.  Its own kernel so that the collective can start one kernel
// earlier, under preprocess_bwd_kernel (RadegsBwdArgs::drgb_ready).
__global__ void __launch_bounds__(256) drgb_clamped_kernel(int P, const int* __restrict__ radii, const uint8_t* __restrict__ clamped,
                                                           const float* __restrict__ acc, int rec, float* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P) return;
  float r = 0.f, g = 0.f, b = 0.f;
  if (radii[idx] > 0) {
    const unsigned cl = (unsigned)clamped[idx];
    const float* a = acc + (size_t)idx * rec;
    r = a[0] * ((cl & 1u) ? 0.f : 1.f); g = a[1] * ((cl & 2u) ? 0.f : 1.f); b = a[2] * ((cl & 4u) ? 0.f : 1.f);
  }
  out[3 * (size_t)idx] = r; out[3 * (size_t)idx + 1] = g; out[3 * (size_t)idx + 2] = b;
}

// ---- the SH slab ----
// 128 Gaussians per block.  The (P,M,3) SH tensor and its gradient are 192-byte rows at SH degree 3: read or
// written by one thread each they would be 64 different cache lines per instruction.  The block therefore
// moves its contiguous 128-row slab with coalesced accesses through LDS (row stride 3M+1 words: odd, so the
// per-thread row walks are bank-conflict free); sh and dL/dsh share the slab (sh_bwd's access order allows it).
constexpr int kPreBwdThreads = 128;   // 64 / 256 measured in round 4: no difference (DESIGN.md 4.5)
// A block's contiguous [nrows][rowf] slab in global memory, cut into consecutive pieces of WIDTH words (1, or 4: a 16-byte move, rows of
// rowf % 4 == 0 words), and where piece e lies in the LDS slab of row stride rowf + 1.  The piece's row comes from a multiply-high by
// the reciprocal of the run-time row length (exact for the slab's few thousand pieces): a true division per piece cost more than
// everything else the kernel does, and carrying (row, column) from step to step serialises the loads.
template <int WIDTH>
struct SlabMap {
  static_assert(WIDTH == 1 || WIDTH == 4, "words or 16-byte pieces");
  int per_row, stride, count;   // pieces per row; LDS words per row; pieces of the slab
  uint32_t magic;               // ceil(2^32 / per_row): floor(e / per_row) == mulhi(e, magic) for e * per_row < 2^32
  __device__ __forceinline__ SlabMap(int nrows, int rowf)   // rowf == 0: a map with no pieces
      : per_row(rowf >> (WIDTH == 4 ? 2 : 0)), stride(rowf + 1), count(nrows * per_row),
        magic(per_row ? 0xFFFFFFFFu / (uint32_t)per_row + 1u : 0u) {}
  __device__ __forceinline__ int lds_word(int e) const {
    const int g = (int)__umulhi((uint32_t)e, magic);
    return g * stride + (e - g * per_row) * WIDTH;
  }
};

// The slab between global memory and LDS, 128 consecutive words per step.
template <bool TO_LDS>
__device__ __forceinline__ void slab_copy(float* slab, float* gmem, const SlabMap<1>& m, int tid) {
#pragma unroll 4
  for (int e = tid; e < m.count; e += kPreBwdThreads) {
    if constexpr (TO_LDS) slab[m.lds_word(e)] = gmem[e];
    else gmem[e] = slab[m.lds_word(e)];
  }
}

// The same in 16-byte pieces, twelve per thread, the way in split into its two halves so that the loads can be issued ahead of everything
// else (see preprocess_bwd_kernel).  LDS side: row stride 3M + 1 words, so a piece goes in as four words; neighbouring lanes are 4 words
// apart and rows shift by one word, which keeps the 64 lanes of a store on different banks.
constexpr int kSlabVecs = 12;   // 16-byte pieces per thread: 128 rows x 48 floats / 128 threads
__device__ __forceinline__ void slab_load16(float4 (&v)[kSlabVecs], const float* gmem, const SlabMap<4>& m, int tid) {
  const float4* g4 = reinterpret_cast<const float4*>(gmem);
#pragma unroll
  for (int k = 0; k < kSlabVecs; k++) {
    const int e = tid + k * kPreBwdThreads;
    v[k] = e < m.count ? g4[e] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
__device__ __forceinline__ void slab_stage16(float* slab, const float4 (&v)[kSlabVecs], const SlabMap<4>& m, int tid) {
#pragma unroll
  for (int k = 0; k < kSlabVecs; k++) {
    const int e = tid + k * kPreBwdThreads;
    if (e < m.count) {
      float* d = slab + m.lds_word(e);
      d[0] = v[k].x; d[1] = v[k].y; d[2] = v[k].z; d[3] = v[k].w;
    }
  }
}
__device__ __forceinline__ void slab_store16(float* gmem, const float* slab, const SlabMap<4>& m, int tid) {
  float4* g4 = reinterpret_cast<float4*>(gmem);
#pragma unroll
  for (int k = 0; k < kSlabVecs; k++) {
    const int e = tid + k * kPreBwdThreads;
    if (e < m.count) {
      const float* d = slab + m.lds_word(e);
      g4[e] = make_float4(d[0], d[1], d[2], d[3]);   // (non-temporal stores for these rows: no difference, same-box A/B 1.278-1.283 | 1.277-1.280 ms per step)
    }
  }
}

// ---- the accumulator record ----
// One Gaussian's 16 | 32 floats as they lie in memory: four 16-byte pieces, with the coord map two more and one float (SplatAcc order:
// dcolor3 dts | drp2 dnrm2 | dnrm1 dmean2D3 | dconic3 dop | dvp3 dcp1 | dcp4 | dcp1).  All zeros without the coord map's part.
struct AccRecord {
  float4 q[6];
  float last;
  static __device__ __forceinline__ AccRecord zero() {
    AccRecord r;
#pragma unroll
    for (int k = 0; k < 6; k++) r.q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    r.last = 0.f;
    return r;
  }
  static __device__ __forceinline__ AccRecord load(const float* p, int rec) {
    AccRecord r = zero();
    const float4* s = reinterpret_cast<const float4*>(p);
    r.q[0] = s[0]; r.q[1] = s[1]; r.q[2] = s[2]; r.q[3] = s[3];
    if (rec == 32) { r.q[4] = s[4]; r.q[5] = s[5]; r.last = s[6].x; }
    return r;
  }
  static __device__ __forceinline__ void clear(float* p, int rec) {
    float4* w = reinterpret_cast<float4*>(p);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    w[0] = z; w[1] = z; w[2] = z; w[3] = z;
    if (rec == 32) { w[4] = z; w[5] = z; w[6] = z; }
  }
  // RadegsBwdArgs::keep_sums: a raw record goes back in the reference's form (before the W/2, H/2 factors) -- the mean2D / conic sums
  // preprocess_bwd() formed from the moments; every other component stays what the blend left
  __device__ __forceinline__ void store_sums(float* p, const SplatBwd& o) const {
    float4* w = reinterpret_cast<float4*>(p);
    w[2] = make_float4(q[2].x, o.sums_mean2D[0], o.sums_mean2D[1], o.sums_mean2D[2]);
    w[3] = make_float4(o.sums_conic[0], o.sums_conic[1], o.sums_conic[2], q[3].w);
  }
  // The record as preprocess_bwd() takes it: everything the kind decides about it happens here.
  __device__ __forceinline__ SplatAcc to_splat_acc(RecordKind kind, const Camera& cam) const {
    SplatAcc acc;
    acc.dcolor[0] = q[0].x; acc.dcolor[1] = q[0].y; acc.dcolor[2] = q[0].z; acc.dts = q[0].w;
    acc.drp[0] = q[1].x; acc.drp[1] = q[1].y; acc.dnrm[0] = q[1].z; acc.dnrm[1] = q[1].w;
    acc.dnrm[2] = q[2].x; acc.dmean2D[0] = q[2].y; acc.dmean2D[1] = q[2].z; acc.dmean2D[2] = q[2].w;
    acc.dconic[0] = q[3].x; acc.dconic[1] = q[3].y; acc.dconic[2] = q[3].z; acc.dop = q[3].w;
    acc.dvp[0] = q[4].x; acc.dvp[1] = q[4].y; acc.dvp[2] = q[4].z; acc.dcp[0] = q[4].w;
    acc.dcp[1] = q[5].x; acc.dcp[2] = q[5].y; acc.dcp[3] = q[5].z; acc.dcp[4] = q[5].w; acc.dcp[5] = last;
    acc.raw = kind == RecordKind::raw_moments;   // preprocess_bwd() turns the moments into the reference's sums
    // constant factors the blend backward left out of its sums (linear, so they commute with the sum):
    // 1/focal on the plane gradients (backward.cu:917-922,939-940), W/2 and H/2 on mean2D (:1002-1003)
    if (kind != RecordKind::reference_sums) {
      const float ifx = 1.0f / cam.focal_x, ify = 1.0f / cam.focal_y;
      acc.drp[0] *= ifx; acc.drp[1] *= ify;
#pragma unroll
      for (int c = 0; c < 3; c++) { acc.dcp[2 * c] *= ifx; acc.dcp[2 * c + 1] *= ify; }
      acc.half_wh = true;   // W/2, H/2 on mean2D are applied by preprocess_bwd() (after a raw record's conversion)
    }
    return acc;
  }
};

// One Gaussian's rows of the returned tensors (its SH row leaves through the slab).  An invisible Gaussian's are all zero
// (rasterize_points.cu:180-193): the caller passes zeros.
__device__ __forceinline__ void store_grads(const PreBwdArgs& a, size_t i, const SplatBwd& o, const float (&dcolor)[3], unsigned clamp_bits) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    a.dL_dmean2D[3 * i + c] = o.dmean2D[c];
    a.dL_dcolor[3 * i + c] = dcolor[c];
    a.dL_dmean3D[3 * i + c] = o.dmean3D[c];
    a.dL_dscale[3 * i + c] = o.dscale[c];
  }
  a.dL_dopacity[i] = o.dopacity;
  if (a.dL_drgb_clamped && !a.drgb_done) {
#pragma unroll
    for (int c = 0; c < 3; c++) a.dL_drgb_clamped[3 * i + c] = dcolor[c] * (((clamp_bits >> c) & 1u) ? 0.f : 1.f);
  }
#pragma unroll
  for (int c = 0; c < 6; c++) a.dL_dcov3D[6 * i + c] = o.dcov3D[c];
  *reinterpret_cast<float4*>(a.dL_drot + 4 * i) = make_float4(o.drot[0], o.drot[1], o.drot[2], o.drot[3]);
}

// Memory-level parallelism (round 4).  The kernel moves ~670 B per Gaussian and computes for ~5 000 instructions at 3 waves per SIMD:
// what it cannot afford is a chain of dependent memory latencies.  The first version copied the slab with 4-byte loads in a loop the
// compiler unrolled by 8 -- 2 KB in flight per wave, six full latencies per block one after the other -- and only then, behind the
// barrier and the visibility test, asked for the Gaussian's own records: ~6 MB in flight on the whole chip, which at ~1.5 us of loaded
// latency is the 3.5 TB/s it ran at.  Now EVERY global read of a block is issued before anything waits: the slab as 12 x 16 bytes per
// thread (rows of 3M floats with 3M % 4 == 0 and 16-byte aligned tensors, i.e. SH degree 3 and 1; other shapes keep the word loop),
// the accumulator record, mean, scale, rotation and flags of the thread's Gaussian (for invisible ones too: the record is there and
// reading it costs less than waiting for `radii` first).
__global__ void __launch_bounds__(kPreBwdThreads) preprocess_bwd_kernel(const PreBwdArgs a) {
  extern __shared__ float sh_slab[];  // [128][3M+1]
  const int tid = threadIdx.x;
  const int base = ((int)blockIdx.x + a.first_block) * kPreBwdThreads;
  const int idx = base + tid;
  const int nrows = min(kPreBwdThreads, a.P - base);
  const int rowf = a.M * 3;
  const bool have_sh = a.shs != nullptr;
  const bool vec = have_sh && a.vec_slab != 0;   // host: rowf % 4 == 0, rowf <= 4 * kSlabVecs, shs and dL_dsh 16-byte aligned
  const SlabMap<1> words(nrows, rowf);
  const SlabMap<4> pieces(nrows, vec ? rowf : 0);
  const size_t slab_at = (size_t)base * rowf;

  // ---- every global read of the block ----
  float4 v[kSlabVecs];
  if (vec) slab_load16(v, a.shs + slab_at, pieces, tid);
  const bool live = idx < a.P;
  const size_t i = live ? (size_t)idx : 0;
  const bool has_sr = a.scales != nullptr;
  int radius = 0;
  unsigned cflags = 0;
  AccRecord rec = AccRecord::zero();
  float4 rq = make_float4(0.f, 0.f, 0.f, 0.f);
  float m0 = 0.f, m1 = 0.f, m2 = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
  if (live) {
    radius = a.radii[idx];
    rec = AccRecord::load(a.acc + i * a.rec, a.rec);
    // only a visible Gaussian's record can have been touched (it is in no list otherwise)
    if (a.rezero && radius > 0) AccRecord::clear(a.acc + i * a.rec, a.rec);
    m0 = a.means3D[3 * i]; m1 = a.means3D[3 * i + 1]; m2 = a.means3D[3 * i + 2];
    if (has_sr) {
      s0 = a.scales[3 * i]; s1 = a.scales[3 * i + 1]; s2 = a.scales[3 * i + 2];
      rq = *reinterpret_cast<const float4*>(a.rotations + 4 * i);
    }
    cflags = (unsigned)a.clamped[idx];   // bits 0..2: SH clamp flags (written for visible Gaussians only; unused otherwise)
  }

  // ---- the SH rows into the slab ----
  if (vec) slab_stage16(sh_slab, v, pieces, tid);
  else if (have_sh) slab_copy<true>(sh_slab, const_cast<float*>(a.shs) + slab_at, words, tid);
  if (have_sh) __syncthreads();

  // ---- the thread's Gaussian: its SH row becomes its dL/dsh row in place ----
  if (live) {
    float* row = have_sh ? sh_slab + tid * words.stride : nullptr;
    SplatBwd o = {};
    float dcolor[3] = {0.f, 0.f, 0.f};
    if (!(radius > 0)) {  // invisible: every returned row is zero (rasterize_points.cu:180-193)
      if (row) for (int c = 0; c < rowf; c++) row[c] = 0;
    } else {
      const Camera cam = load_camera(a.cam);
      const SplatAcc acc = rec.to_splat_acc(a.kind, cam);
      float sc3[3] = {s0, s1, s2}, rq4[4] = {rq.x, rq.y, rq.z, rq.w};
      float cov[6];
      if (a.cov3D_precomp) {
#pragma unroll
        for (int c = 0; c < 6; c++) cov[c] = a.cov3D_precomp[6 * i + c];
      } else {
        cov3d_from_scale_rot(sc3, cam.scale_modifier, rq4, cov);
      }
      // what the reference's computeCov2DCUDA reads as `conic_opacity[idx].w` is dL_dconic[idx].w (argument slip at
      // rasterizer_impl.cu:568); the stored opacity*coef only with opacity_grad_intended (include/radegs.h)
      // (a raw record holds sum h dy dy there: dL_dconic.w = -1/2 of it, rg_streams.inc)
      const float op_combined = a.opacity_grad_intended ? a.splat_a[4 * i + 1].y
                                                        : (a.kind == RecordKind::raw_moments ? -0.5f * acc.dconic[2] : acc.dconic[2]);
      if (row) {  // rows beyond the active degree stay zero
        const int K = (a.D + 1) * (a.D + 1);
        for (int c = K * 3; c < rowf; c++) row[c] = 0;
      }
      preprocess_bwd(mk3(m0, m1, m2), has_sr ? sc3 : nullptr, has_sr ? rq4 : nullptr, cov, op_combined, a.D, row,
                     cflags & 7u, cam, acc, row, o);
      if (a.keep) rec.store_sums(a.acc + i * a.rec, o);
#pragma unroll
      for (int c = 0; c < 3; c++) dcolor[c] = acc.dcolor[c];
    }
    store_grads(a, i, o, dcolor, cflags & 7u);
  }

  // ---- the slab, now dL/dsh, back out ----
  if (have_sh && a.dL_dsh) {
    __syncthreads();
    if (vec) slab_store16(a.dL_dsh + slab_at, sh_slab, pieces, tid);
    else slab_copy<false>(sh_slab, a.dL_dsh + slab_at, words, tid);
  }
}

// dL/dsh[P,M,3] = scale * sum over views v of  w(dir_v) (x) dRGB_v   -- rebuilds the SH gradient of a view-parallel batch
// from what the ranks all-gathered (12 B per Gaussian per view instead of all-reducing 192 B per Gaussian).
// Same 128-row LDS slab as preprocess_bwd_kernel for the coalesced write-out.
__global__ void __launch_bounds__(kPreBwdThreads) sh_grad_from_views_kernel(int P, int D, int M, int nviews, const float* __restrict__ means3D,
                                                                           const float* __restrict__ campos, const float* __restrict__ drgb,
                                                                           float scale, float* __restrict__ dL_dsh) {
  extern __shared__ float sh_slab[];
  const int tid = threadIdx.x, base = blockIdx.x * kPreBwdThreads, idx = base + tid;
  const int rowf = M * 3;
  const SlabMap<1> words(min(kPreBwdThreads, P - base), rowf);
  if (idx < P) {
    float acc[48];
#pragma unroll
    for (int k = 0; k < 48; k++) acc[k] = 0.f;
    const v3 pos = mk3(means3D[3 * (size_t)idx], means3D[3 * (size_t)idx + 1], means3D[3 * (size_t)idx + 2]);
    for (int v = 0; v < nviews; v++) {
      const float* g = drgb + ((size_t)v * P + idx) * 3;
      const float gr = g[0], gg = g[1], gb = g[2];
      if (gr == 0.f && gg == 0.f && gb == 0.f) continue;  // not visible (or fully clamped) in this view
      const float cp[3] = {campos[3 * v], campos[3 * v + 1], campos[3 * v + 2]};
      float w[16];
      sh_basis(D, pos, cp, w);
#pragma unroll
      for (int k = 0; k < 16; k++) { acc[3 * k] += w[k] * gr; acc[3 * k + 1] += w[k] * gg; acc[3 * k + 2] += w[k] * gb; }
    }
    float* row = sh_slab + tid * words.stride;
    const int K3 = 3 * (D + 1) * (D + 1);
#pragma unroll
    for (int c = 0; c < 48; c++)
      if (c < rowf) row[c] = c < K3 ? acc[c] * scale : 0.f;
    for (int c = 48; c < rowf; c++) row[c] = 0.f;
  }
  __syncthreads();
  slab_copy<false>(sh_slab, dL_dsh + (size_t)base * rowf, words, tid);
}
