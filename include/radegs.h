/* radegs.h -- C ABI of libradegs_hip.so, the MI355X (gfx950) differentiable Gaussian-splat
 * rasterizer behind RaDe-GS's `diff_gaussian_rasterization` operator.
 *
 * This is the drop-in boundary for the one hot path this repository accelerates.  Every entry
 * point replaces one static method of the reference's native interface
 * (DGR = /root/reference/submodules/diff-gaussian-rasterization):
 *
 *   radegs_forward       <-  CudaRasterizer::Rasterizer::forward    DGR/cuda_rasterizer/rasterizer.h:31-63
 *                            (called from RasterizeGaussiansCUDA,    DGR/rasterize_points.cu:36-133)
 *   radegs_backward      <-  CudaRasterizer::Rasterizer::backward   DGR/cuda_rasterizer/rasterizer.h:65-110
 *                            (called from RasterizeGaussiansBackwardCUDA, DGR/rasterize_points.cu:136-246)
 *   radegs_mark_visible  <-  CudaRasterizer::Rasterizer::markVisible DGR/cuda_rasterizer/rasterizer.h:24-29
 *                            (called from markVisible,               DGR/rasterize_points.cu:248-267)
 *   radegs_integrate     <-  CudaRasterizer::Rasterizer::integrate  DGR/cuda_rasterizer/rasterizer.h:112-147
 *                            (called from IntegrateGaussiansToPointsCUDA, DGR/rasterize_points.cu:269-388)
 *
 * Conventions kept from the reference:
 *   - plain device pointers + sizes; NULL means "tensor not provided" (the reference tests
 *     data_ptr()==nullptr: forward.cu:363,407, backward.cu:622,626, rasterizer_impl.cu:394,494,540);
 *   - the three scratch buffers (geometry / binning / image state) are obtained through
 *     allocator callbacks -- the C form of std::function<char*(size_t)> -- so the caller owns
 *     the memory (torch tensors in the Python binding), may keep it for backward, and hands the
 *     same pointers back.  Their internal layout is private and self-describing from (P, R, W*H);
 *   - viewmatrix/projmatrix are the transposed 4x4 float matrices the reference passes;
 *   - image outputs are CHW float32; `radii` is int32[P].
 * Differences, all deliberate:
 *   - every call takes a HIP stream (the reference launches on the legacy default stream);
 *   - errors are returned as negative codes + radegs_last_error() instead of C++ exceptions;
 *   - output images for modes that are switched off are not touched (the binding zero-fills
 *     them, as the reference's torch::full does).
 * No torch types appear here; `stream` is a hipStream_t passed as void*.
 */
#ifndef RADEGS_H_INCLUDED
#define RADEGS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RADEGS_OK 0
#define RADEGS_ERR_INVALID_ARG (-1)
#define RADEGS_ERR_ALLOC (-2)
#define RADEGS_ERR_HIP (-3)
#define RADEGS_ERR_NO_DEVICE (-4)
#define RADEGS_ERR_STATE (-5)   /* an earlier radegs_backward on this thread and device was handed an image buffer that does not hold what
                                   its forward wrote (reused or overwritten state): that call's gradients are invalid */
#define RADEGS_ERR_TOO_LARGE (-6)   /* radegs_tetmesh_*: a size beyond what the 32-bit sort / scan primitives address */

/* Allocator callback: return a DEVICE pointer to at least `nbytes` bytes (256-B aligned), or
 * NULL on failure.  Mirrors the resize lambdas of DGR/rasterize_points.cu:27-33. */
typedef void* (*radegs_alloc_fn)(void* user, size_t nbytes);

typedef struct RadegsFwdArgs {
  int P;              /* number of Gaussians */
  int D;              /* active SH degree */
  int M;              /* SH coefficients per Gaussian in `shs` (rows of the (P,M,3) tensor) */
  int width, height;
  const float* background;      /* [3] device */
  const float* means3D;         /* [P,3] */
  const float* shs;             /* [P,M,3] or NULL */
  const float* colors_precomp;  /* [P,3] or NULL (exactly one of shs / colors_precomp) */
  const float* opacities;       /* [P] */
  const float* scales;          /* [P,3] or NULL */
  const float* rotations;       /* [P,4] (r,x,y,z), not normalised here; or NULL */
  const float* cov3D_precomp;   /* [P,6] or NULL (exactly one of scales+rotations / cov3D) */
  const float* viewmatrix;      /* [16] device, transposed */
  const float* projmatrix;      /* [16] device, transposed */
  const float* cam_pos;         /* [3] device */
  float scale_modifier, tan_fovx, tan_fovy, kernel_size;
  int prefiltered;              /* must be 0 */
  int require_coord, require_depth, debug;
  float* out_color;             /* [3,H,W] */
  /* The five maps below are PRODUCED iff their flag is set.  A map the flags do not produce is all-zero in the reference
   * (torch::full(0), DGR/rasterize_points.cu:71-77): when its pointer is non-NULL the forward ZERO-FILLS it (every pixel, inside the
   * blend kernel -- no separate fill); pass NULL for a map you do not want touched. */
  float* out_coord;             /* [3,H,W]  produced iff require_coord */
  float* out_mcoord;            /* [3,H,W]  produced iff require_coord */
  float* out_depth;             /* [1,H,W]  produced iff require_depth */
  float* out_mdepth;            /* [1,H,W]  produced iff require_depth */
  float* out_alpha;             /* [1,H,W] */
  float* out_normal;            /* [3,H,W]  produced iff require_coord || require_depth */
  int* radii;                   /* [P] */
} RadegsFwdArgs;

/* Returns num_rendered (>= 0) or a negative RADEGS_ERR_*.
 * Host synchronisation: the FIRST call for a (device, width, height) waits for num_rendered in the middle of the forward to
 * size the binning buffer, like rasterizer_impl.cu:354.  Later calls allocate for a capacity predicted from the previous
 * counts, queue the whole forward, and wait only for the 4-byte count at the very end (a mapped host word the emission kernel
 * writes, polled -- neither an event nor a stream sync); a too small prediction is detected there and the forward is redone with
 * exact sizes.  RADEGS_SPECULATE=0 restores the first
 * behaviour for every call.  The allocators may therefore be asked for MORE than the exact state size, and -- on a redo --
 * a second time within one call.  The image-state callback is invoked after the capacity is known (its tail holds the
 * sub-tile entry streams of the blend stage when the scene's splats are small). */
int radegs_forward(const RadegsFwdArgs* args, radegs_alloc_fn geom_alloc, void* geom_user, radegs_alloc_fn binning_alloc,
                   void* binning_user, radegs_alloc_fn image_alloc, void* image_user, void* stream);

typedef struct RadegsBwdArgs {
  size_t struct_size;           /* sizeof(RadegsBwdArgs) of the header the CALLER was compiled against.  The structure has grown at its
                                   tail between releases; radegs_backward / radegs_backward_from_sums refuse a size they do not know
                                   (RADEGS_ERR_INVALID_ARG) instead of reading hooks past the end of a shorter structure */
  int P, D, M, R;               /* R = num_rendered returned by the forward */
  int width, height;
  const float* background;
  const float* means3D;
  const float* shs;
  const float* colors_precomp;
  const float* alphas;          /* out_alpha of the forward */
  const float* scales;
  const float* rotations;
  const float* cov3D_precomp;
  const float* viewmatrix;
  const float* projmatrix;
  const float* cam_pos;
  float scale_modifier, tan_fovx, tan_fovy, kernel_size;
  const int* radii;
  const float* normalmap;       /* out_normal of the forward */
  void* geom_buffer;            /* the three buffers the forward filled */
  void* binning_buffer;
  void* image_buffer;
  const float* dL_dpix;         /* [3,H,W] */
  const float* dL_dpix_coord;   /* [3,H,W] */
  const float* dL_dpix_mcoord;  /* [3,H,W] */
  const float* dL_dpix_depth;   /* [1,H,W] */
  const float* dL_dpix_mdepth;  /* [1,H,W] */
  const float* dL_dalphas;      /* [1,H,W] */
  const float* dL_dpix_normal;  /* [3,H,W] */
  /* outputs; every element is written by the call (no pre-zeroing needed) */
  float* dL_dmean2D;            /* [P,3]  x,y signed, z = abs-grad sum */
  float* dL_dcolor;             /* [P,3] */
  float* dL_dopacity;           /* [P,1] */
  float* dL_dmean3D;            /* [P,3] */
  float* dL_dcov3D;             /* [P,6] */
  float* dL_dsh;                /* [P,M,3] or NULL when M == 0 */
  float* dL_dscale;             /* [P,3] */
  float* dL_drot;               /* [P,4] */
  int require_coord, require_depth, debug;
  /* optional [P,3]: dL/dRGB of the SH colour with the clamp mask applied.  When given, dL_dsh may be NULL (it is then not
   * written): the SH gradient is the outer product basis(dir) x this vector and can be rebuilt with
   * radegs_sh_grad_from_views -- which is how the view-parallel exchange moves 12 instead of 192 bytes per Gaussian. */
  float* dL_drgb_clamped;
  /* 0 (default): the gradient the reference EXECUTES.  Rasterizer::backward passes `(float4*)dL_dconic` in the position of
   * BACKWARD::preprocess's `conic_opacity` parameter (rasterizer_impl.cu:568 vs backward.h:94), so computeCov2DCUDA's
   * `combined_opacity` (backward.cu:179-180) is the accumulated conic gradient dL_dconic[idx].w, not opacity*coef; it scales the
   * derivative of the opacity-compensation factor w.r.t. the 2D covariance (backward.cu:367-375) and from there dL_dcov3D /
   * dL_dmeans3D / dL_dscales / dL_drotations.  Negligible (~1e-6 of the conic term) at the reference's default kernel_size = 0.
   * 1: the derivative the formulas intend (combined_opacity = opacity*coef) -- what an upstream fix would compute. */
  int opacity_grad_intended;
  /* Optional hand-off for a view-parallel caller (needs dL_drgb_clamped): dL_drgb_clamped is final as soon as the blend backward has
   * run, one kernel before everything else -- it is then written by a small kernel of its own and `drgb_ready(drgb_ready_user)` is
   * called ON THE HOST once that kernel is queued on `stream`, BEFORE the per-Gaussian backward (~0.16 ms at 1M Gaussians) is queued:
   * the caller records an event there and starts its all-gather of these 12-byte rows on another stream, under that kernel. */
  void (*drgb_ready)(void* user);
  void* drgb_ready_user;
  /* Optional, for the same caller: with grad_chunks >= 2 the per-Gaussian backward is queued as that many launches over consecutive
   * ranges of Gaussians, and after each one `grads_ready(grads_ready_user, first, count)` is called ON THE HOST: once `stream` reaches
   * that point, rows [first, first + count) of dL_dmean3D / dL_dopacity / dL_dscale / dL_drot (and of every other returned gradient)
   * are final -- the caller records an event and starts that part of its all-reduce on another stream, under the launches that
   * follow.  0 or 1: one launch, no call. */
  int grad_chunks;
  void (*grads_ready)(void* user, int first, int count);
  void* grads_ready_user;
  /* Inspection (tests): 1 = after the call the accumulation scratch holds every visible Gaussian's sums in the order and units of
   * radegs_backward_from_sums' `sums`, except the constant factors listed there (1/focal on the plane sums, W/2 and H/2 on mean2D).
   * Without it the record's mean2D / conic slots may hold the blend backward's private intermediate (raw moments, csrc/rg_streams.inc). */
  int keep_sums;
  /* 1 = the caller promises that the buffer `accum_alloc` is about to hand out is ALL ZEROS, and wants it back all zeros: the call then
   * skips its fill of the scratch (64 | 128 B per Gaussian: 10 us at 1M Gaussians) and the per-Gaussian kernel clears every record it
   * consumes.  Meant for a caller that keeps ONE scratch buffer per (device, stream) across calls: zero it once, pass 1 from then on,
   * and fall back to 0 after any call that returned an error or ran with keep_sums (the buffer is then in an unknown state).
   * 0: the scratch may hold anything; it is filled with zeros first and left as the kernels leave it. */
  int acc_reuse;
} RadegsBwdArgs;

/* `accum_alloc` provides the per-Gaussian accumulation scratch (64 or 128 B per Gaussian). */
int radegs_backward(const RadegsBwdArgs* args, radegs_alloc_fn accum_alloc, void* accum_user, void* stream);
/* radegs_backward with a FIXED summation order: the same gradients up to fp32 rounding, and the same BITS on every run with the same inputs,
 * the same build of this library and the same device model.  (radegs_backward adds each tile's wave totals to the Gaussian's record with
 * atomics, in the order the scheduler happens to run the tiles.)  Here the tile-wide blend backward runs with one wave per tile and
 * STORES every (tile, entry) total as the partial record of that entry's position r in the tile-ordered instance list; a stable sort of
 * (point_list[r], r) then gives every Gaussian its positions in ascending r -- tile order, then depth order -- and one group of lanes per
 * Gaussian adds its partial records in that order, sequentially, from 0.0f.  The order depends on the instance list alone.  The per-Gaussian
 * half, keep_sums, drgb_ready and grad_chunks / grads_ready work as in radegs_backward; acc_reuse keeps its contract too (the scratch of
 * `accum_alloc` comes back all zeros), though this call never needs the zeros: every record of it is written before it is read.
 * Entry streams are never replayed (the tile-wide backward is valid after either forward).  Not promised: the bits of radegs_backward,
 * or the same bits from another build.
 * `scratch`: device memory of at least radegs_backward_ordered_scratch_bytes(P, R, require_coord) bytes, 256-byte aligned, contents
 * irrelevant, free for reuse once `stream` has passed the call.  With r256(x) = x rounded up to a multiple of 256 and REC = 32 with
 * require_coord, else 16, that is
 *     r256(R * REC * 4)  +  2 * r256(R * 4)  +  r256(sort_temp(R))
 * where sort_temp(R) = 2 * (4 R + 256) + 2048 * (ceil(R / 2048) + 1) + 3072 is the radix sort's temporary: the partial records
 * dominate, 64 B per instance (128 B with the coord map), about 0.5 GB at 8 M instances.  A scratch that is NULL with R > 0, or too small,
 * is refused with RADEGS_ERR_INVALID_ARG before anything is queued.  R == 0 needs no scratch. */
size_t radegs_backward_ordered_scratch_bytes(int P, int R, int require_coord);
int radegs_backward_ordered(const RadegsBwdArgs* args, radegs_alloc_fn accum_alloc, void* accum_user, void* scratch, size_t scratch_bytes,
                            void* stream);
/* The SECOND half of radegs_backward on caller-supplied per-Gaussian sums (inspection / parity hook, like radegs_debug_export): the
 * per-Gaussian backward (computeCov2DCUDA + preprocessCUDA backward, DGR/cuda_rasterizer/backward.cu:145-628) runs over `sums` instead
 * of over what the blend backward accumulated.  sums: device [P][16] floats ([P][32] with require_coord) in the order
 *   dL_dcolors[3], dL_dts, dL_dray_planes[2], dL_dnormals[3], dL_dmeans2D[3], dL_dconic.{x,y,w}, dL_dopacity (the render kernel's raw sum,
 *   before backward.cu:395-403 rescales it), and with require_coord: dL_dview_points[3], dL_dcamera_planes[6], 7 unused
 * holding the values the reference's render kernel leaves in those arrays (rasterizer_impl.cu:541-555).  What summation order does
 * to the gradients is thereby taken out of a comparison: fed with the reference's own sums, every returned gradient must equal the
 * reference's (tests/test_gpu_vs_compiled_reference.py).  Of `args`, geom_buffer, radii, means3D, scales + rotations (or cov3D_precomp),
 * shs (when given), the three camera pointers and the gradient outputs are read -- all must be valid device pointers (NULL is refused);
 * `sums` must be 16-byte aligned (the records are read as 16-byte pieces).  Nothing is allocated.  dL_drgb_clamped, drgb_ready and
 * grad_chunks / grads_ready work as in radegs_backward (so that tests reach those launch modes over known sums); keep_sums and
 * acc_reuse are ignored: `sums` is only read. */
int radegs_backward_from_sums(const RadegsBwdArgs* args, const float* sums, void* stream);

/* dL_dsh[P,M,3] = scale * sum_v basis(normalize(means3D - campos[v])) (x) drgb_clamped[v]   (rows beyond (D+1)^2 zero).
 * campos: [nviews,3], drgb_clamped: [nviews,P,3] -- the all-gathered per-view outputs of radegs_backward. */
int radegs_sh_grad_from_views(int P, int D, int M, int nviews, const float* means3D, const float* campos, const float* drgb_clamped,
                              float scale, float* dL_dsh, void* stream);

/* present[i] = 1 iff Gaussian i passes the near-plane test (view z > 0.2). */
int radegs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, unsigned char* present,
                        void* stream);

typedef struct RadegsIntegrateArgs {
  int P, D, M;                  /* Gaussians, as in RadegsFwdArgs */
  int PN;                       /* number of query points */
  int width, height;
  const float* background;      /* [3] */
  const float* means3D;         /* [P,3] */
  const float* shs;             /* [P,M,3] or NULL */
  const float* colors_precomp;  /* [P,3] or NULL */
  const float* opacities;       /* [P] */
  const float* scales;          /* [P,3] or NULL */
  const float* rotations;       /* [P,4] or NULL */
  const float* cov3D_precomp;   /* [P,6] or NULL */
  const float* viewmatrix;      /* [16] transposed */
  const float* projmatrix;      /* [16] transposed */
  const float* cam_pos;         /* [3] */
  const float* points3D;        /* [PN,3] query points (world space) */
  float scale_modifier, tan_fovx, tan_fovy, kernel_size;
  int debug;
  /* outputs; every element is written by the call (initial values of rasterize_points.cu:312-320 included) */
  float* out_color;             /* [9,H,W]: rgb, expected depth, median depth, 0, max depth, alpha, #points in the pixel */
  float* out_alpha_integrated;  /* [PN]   1 for points that do not project into the image */
  float* out_color_integrated;  /* [PN,3] colour of the pixel the point falls in */
  float* out_coordinate2d;      /* [PN,2] projected position in pixels */
  float* out_sdf;               /* [PN]   median-surface depth along the ray minus point depth; -1000 if not projected */
  int* radii;                   /* [P] */
} RadegsIntegrateArgs;

/* Integrates the Gaussians' opacity along the ray of every query point (GOF-style; used by mesh extraction).
 * `point_alloc` provides the point/INTE state (the reference's point + point-binning buffers).  Returns num_rendered.
 * Documented deviations from the reference's undefined behaviour: (1) for ill-conditioned Gaussians (smallest
 * covariance eigenvalue <= 1e-8) the inverse ray-space covariance is ZERO: upstream's shadowed variable
 * (forward.cu:223) stores an uninitialised matrix there; (2) contributor ids are 32-bit (upstream truncates to uint16, wrong only for tile lists longer than
 * 65535 entries); (3) the exponent of the point opacity is clamped at +80 (a non-PSD ill-conditioned matrix would
 * otherwise overflow expf); (4) the reference's cap is KEPT although nothing here needs it: a pixel stops at its 2048th used entry
 * (MAX_NUM_CONTRIBUTORS * 4, forward.cu:1121-1125: the size of the reference's per-thread contributor array; this library only counts).
 * A query point whose projection is not a number (a NaN coordinate, or 0 * inf in the view transform) is NOT projected: it keeps the
 * initial values and is counted in no pixel, as in the reference, whose reject test it fails to pass. */
int radegs_integrate(const RadegsIntegrateArgs* args, radegs_alloc_fn geom_alloc, void* geom_user, radegs_alloc_fn binning_alloc,
                     void* binning_user, radegs_alloc_fn image_alloc, void* image_user, radegs_alloc_fn point_alloc, void* point_user,
                     void* stream);

/* Sizes of the geometry / image state for (P) and (W*H) -- the binning size depends on R and is
 * requested through the callback. */
size_t radegs_geometry_bytes(int P, int require_coord);
size_t radegs_image_bytes(int width, int height);
size_t radegs_binning_bytes(int R);

/* Test/inspection hook: copy a named private array out of the state buffers into `dst`
 * (device memory, dst_bytes large enough).  Names: "point_list" u32[R], "ranges" u32[2*tiles],
 * "n_contrib" u32[2*H*W], "tiles_touched" u32[P], "splat_a" f32[P,16], "splat_b" f32[P,12],
 * "clamped" u8[P] (bits 0..2: SH channel clamped at 0; bit 3: the eigen-solver converged), "depth_key" u32[P], "blk_count" /
 * "blk_consumed" u32[8*tiles] (entry streams), "rect" u32[P] (packed tile rectangle x0 | y0<<8 | w<<16 | h<<24),
 * "tile_keys_sorted" u32[R] (the binning buffer's sorted tile keys: 32-bit keys only, e.g. with the block mask in the top byte; and
 * only after a forward whose binning buffer was sized for exactly R instances, RADEGS_SPECULATE=0: the array's offset depends on the capacity),
 * and after a forward that wrote entry streams "blk_base" / "blk_order" u32[8*tiles], "stream_meta" u32[4] (tag 0x53545247, chunks the
 * lists need, unused, overflow flag) and "blk_chunks": round chunks of 48 words from chunk 0 on -- the LAST array of the image state, so
 * this function cannot know where the buffer ends: it copies exactly dst_bytes, and the caller, who asks for stream_meta[1] * 48 words,
 * must check radegs_image_bytes(width, height) - 256 + dst_bytes against the size of its image buffer (_C.debug_export does).
 * Returns bytes copied or a negative error. */
long long radegs_debug_export(const char* name, int P, int R, int width, int height, int require_coord, const void* geom_buffer,
                              const void* binning_buffer, const void* image_buffer, void* dst, size_t dst_bytes, void* stream);

/* Size of the point state radegs_integrate asks its `point_alloc` for: pure host arithmetic, like the three sizes above. */
size_t radegs_point_bytes(int P, int PN, int width, int height);
/* The same hook for the point state of radegs_integrate (the buffer its `point_alloc` returned, for the same P, PN, width, height).
 * Names: "inte_rec" f32[P,8] ({inverse ray-space covariance, upper triangle, 6 | well-conditioned flag | 0}; rows of Gaussians that were
 * culled are not written), "p2d" f32[PN,2] and "pdepth" f32[PN] (written for projected points only), "ppix" u32[PN] (pixel index, or
 * 0xFFFFFFFF: not projected), "pt_sorted" u32[PN] (point ids grouped by pixel; as many entries as points were projected), "pix_count"
 * u32[H*W] (all zero once the scatter has run), "pix_incl" u32[H*W] (inclusive scan of the per-pixel point counts) and "final_T"
 * f32[H*W].  Same conventions and error returns as radegs_debug_export. */
long long radegs_debug_export_points(const char* name, int P, int PN, int width, int height, const void* point_buffer, void* dst,
                                     size_t dst_bytes, void* stream);

/* Speculative binning (see radegs_forward): forwards that ran on a predicted capacity / those whose prediction was too small and
 * were redone with exact sizes, since the last reset. */
void radegs_binning_stats(unsigned long long* speculative_calls, unsigned long long* misses, int reset);
/* Which blend formulation the last radegs_forward of the calling thread used: 1 = sub-tile entry streams, 0 = tile-wide kernels,
 * -1 = no forward yet (bench.py reports the native decision instead of mirroring the selection rule). */
int radegs_last_forward_used_streams(void);

/* The library reads its environment switches once, at first use.  A host that changes them afterwards --
 * the test-suite does, between cases of one process -- calls this to have them read again. */
void radegs_reload_env(void);

/* Per-stage timing with HIP events recorded on the launch stream (used by bench.py for the live
 * roofline measurement).  enable(1) -> every subsequent forward/backward records an event pair per
 * stage; collect() waits for them, adds each stage's elapsed ms / launch count into the arrays
 * (n >= radegs_profile_num_stages()) and clears the log. */
void radegs_profile_enable(int on);
/* stage >= 0: record events for that stage only (each recorded stage boundary costs ~10 us of stream bubble, so a timed
 * run should select just the kernel it reports); -1: all stages. */
void radegs_profile_select(int stage);
/* With a selected stage: time only every `every`-th launch of it (an event pair costs ~10 us of stream bubble; 1 = every launch). */
void radegs_profile_stride(int every);
int radegs_profile_num_stages(void);
const char* radegs_profile_stage_name(int i);
int radegs_profile_collect(float* ms_total, int* count, int n);

/* The library remembers, by ADDRESS, which image-state buffers hold entry streams written by their forward (radegs_backward replays
 * them only then; otherwise it runs the tile-wide kernels, which are valid after either forward).  Tell it when such a buffer is
 * freed or moved, so that an unrelated buffer landing on the same address later is not mistaken for one.  (The Python binding
 * does this from the tensor's finaliser and on resize.) */
void radegs_forget_image(const void* image_buffer);

const char* radegs_last_error(void);
const char* radegs_version(void);

/* ---------------------------------------------------------------------------------------------------------------
 * The step that follows the rasterizer in every regularised training iteration: two depth (or
 * coordinate) maps -> two normal maps by central differences, and the normal-consistency loss against the rendered
 * normal map.  Replaces, with one kernel per direction, the torch-eager
 *     depths_double_to_points / point_double_to_normal / depth_double_to_normal   utils/graphics_utils.py:97-127
 *     normal_error_map / depth_normal_loss                                        train.py:152-155
 * and their autograd backward.  All maps are float32 device pointers; normal maps are [2,3,H,W] (map 1 first).
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct RadegsNormalArgs {
  int width, height;
  int points;          /* 0: map1/map2 are depth maps [1,H,W] (depth_double_to_normal); 1: coordinate maps [3,H,W] */
  double fovx, fovy;   /* view.FoVx / view.FoVy in radians (used for depth maps only) */
  const float* map1;   /* expected depth / expected coord */
  const float* map2;   /* median depth / median coord */
} RadegsNormalArgs;

int radegs_normals_forward(const RadegsNormalArgs* args, float* out_normals /* [2,3,H,W] */, void* stream);
/* grad_map1/2 have the shape of map1/2; every element is written */
int radegs_normals_backward(const RadegsNormalArgs* args, const float* grad_normals /* [2,3,H,W] */, float* grad_map1, float* grad_map2,
                            void* stream);
/* loss = (1-depth_ratio) * mean(1 - n.N_1) + depth_ratio * mean(1 - n.N_2), means over all H*W pixels (border: N = 0).
 * out_loss3 = {loss, mean error map 1, mean error map 2}; scratch: radegs_normal_loss_scratch_bytes() bytes. */
size_t radegs_normal_loss_scratch_bytes(int width, int height);
int radegs_normal_loss_forward(const RadegsNormalArgs* args, const float* rendered_normal /* [3,H,W] */, float depth_ratio, void* scratch,
                               float* out_loss3, void* stream);
/* upstream: device scalar d(objective)/d(loss) or NULL (= 1) */
int radegs_normal_loss_backward(const RadegsNormalArgs* args, const float* rendered_normal, float depth_ratio, const float* upstream,
                                float* grad_map1, float* grad_map2, float* grad_rendered_normal /* [3,H,W] */, void* stream);
const char* radegs_normals_last_error(void);

/* ---------------------------------------------------------------------------------------------------------------
 * The step that precedes the rasterizer in every render() call: parameter activations fused with
 * the 3D (mip) filter -- GaussianModel.get_scaling_n_opacity_with_3D_filter, scene/gaussian_model.py:156-166.
 *   scales[P,3] = sqrt(exp(scaling_raw)^2 + filter_3D^2);  opacity[P] = sigmoid(opacity_raw) * sqrt(det1/det2)
 * backward: grad_scales / grad_opacity may be NULL (= zero cotangent); filter_3D carries no gradient upstream either.
 * --------------------------------------------------------------------------------------------------------------- */
int radegs_filter3d_forward(int P, const float* scaling_raw /* [P,3] */, const float* opacity_raw /* [P,1] */,
                            const float* filter_3D /* [P,1] */, float* scales_out /* [P,3] */, float* opacity_out /* [P,1] */,
                            void* stream);
int radegs_filter3d_backward(int P, const float* scaling_raw, const float* opacity_raw, const float* filter_3D, const float* grad_scales,
                             const float* grad_opacity, float* grad_scaling_raw /* [P,3] */, float* grad_opacity_raw /* [P,1] */,
                             void* stream);
/* GaussianModel.compute_3D_filter (scene/gaussian_model.py:179-232) over all cameras in one pass.  cameras16: [ncam][16]
 * device floats = R (3x3 row-major as stored: p_cam = p @ R + T), T (3), focal_x, focal_y, width, height.
 * focal_length: max focal_x over the cameras (host).  scratch_distance: [P] floats, scratch_max: 1 uint32 (device).
 * filter_3D[P] = min-depth / focal_length * sqrt(0.2); Gaussians no camera sees get the largest valid depth. */
int radegs_compute_filter3d(int P, const float* xyz, int ncam, const float* cameras16, float focal_length, float* scratch_distance,
                            unsigned* scratch_max, float* filter_3D, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Model activations: the whole pre-step of render() -- raw parameters in, the rasterizer's four
 * per-Gaussian inputs out -- and its backward, one launch each, nothing read back, work enqueued on `stream`.
 *   shs[P,K+1,3]   = cat(f_dc[P,1,3], f_rest[P,K,3]) along dim 1         (the bytes torch.cat writes)
 *   rotations[P,4] = x / fmaxf(sqrtf(((x0^2 + x1^2) + x2^2) + x3^2), 1e-12f)   one rounding per operation, nothing fused
 *   scales, opacity: the bits radegs_filter3d_forward gives on the same inputs
 * backward: each cotangent may be NULL (= zero cotangent; the gradients it alone feeds are written as exact zeros).
 *   g_f_dc / g_f_rest = the two slices of g_shs;  g_scaling_raw / g_opacity_raw: the bits of radegs_filter3d_backward;
 *   g_rotation_raw = (g - y (g.y)) / n for n >= 1e-12f, with g.y = ((g0 y0 + g1 y1) + g2 y2) + g3 y3, else g / 1e-12f.
 * 0 <= K <= RADEGS_MODELIO_MAX_REST; f_rest / g_f_rest are NULL iff K == 0.  P == 0 is legal and launches nothing.
 * f_dc, f_rest, rotation_raw, shs, rotations, g_shs, g_rotations, g_f_dc, g_f_rest and g_rotation_raw are 16-byte
 * aligned.  Anything else returns RADEGS_ERR_INVALID_ARG before a launch.
 * --------------------------------------------------------------------------------------------------------------- */
int radegs_model_activate_forward(int P, int K, const float* f_dc, const float* f_rest, const float* rotation_raw, const float* scaling_raw,
                                  const float* opacity_raw, const float* filter_3D, float* shs, float* rotations, float* scales, float* opacity,
                                  void* stream);
int radegs_model_activate_backward(int P, int K, const float* rotation_raw, const float* scaling_raw, const float* opacity_raw, const float* filter_3D,
                                   const float* g_shs, const float* g_rotations, const float* g_scales, const float* g_opacity, float* g_f_dc,
                                   float* g_f_rest, float* g_rotation_raw, float* g_scaling_raw, float* g_opacity_raw, void* stream);


/* ---------------------------------------------------------------------------------------------------------------
 * The photometric loss that closes every training iteration:
 *     (1 - lambda) * l1_loss(image, gt) + lambda * (1 - ssim(image, gt))      train.py:159, utils/loss_utils.py:17-63
 * image / gt: [C,H,W] float32.  forward writes out_loss3 = {loss, l1, ssim}; when `dmaps` ([3,C,H,W]) is given it also
 * stores the per-pixel SSIM derivative maps the backward consumes.  backward: grad_image = coef2[0] * d l1/d image +
 * coef2[1] * d ssim/d image (coef2: two DEVICE floats, e.g. {g*(1-lambda), -g*lambda} for upstream gradient g).
 * --------------------------------------------------------------------------------------------------------------- */
size_t radegs_photometric_scratch_bytes(int width, int height, int channels);
int radegs_photometric_forward(int width, int height, int channels, const float* image, const float* gt, float lambda_dssim, void* scratch,
                               float* dmaps, float* out_loss3, void* stream);
int radegs_photometric_backward(int width, int height, int channels, const float* image, const float* gt, const float* dmaps,
                                const float* coef2, float* grad_image, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Multi-tensor Adam step: torch.optim.Adam(l, lr=0.0, eps=1e-15) of scene/gaussian_model.py:338-349
 * (no weight decay, no amsgrad) over up to RADEGS_ADAM_MAX_TENSORS parameter tensors in one launch.  `step` is the
 * step count AFTER this update (>= 1); `lr` the group's current learning rate.  All pointers: float32, device.
 * --------------------------------------------------------------------------------------------------------------- */
#define RADEGS_ADAM_MAX_TENSORS 16
typedef struct RadegsAdamTensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  unsigned long long numel;
  float lr;
  double step;
} RadegsAdamTensor;
int radegs_adam_step(int count, const RadegsAdamTensor* tensors, double beta1, double beta2, double eps, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * simple_knn._C.distCUDA2 (scene/gaussian_model.py:315): out[i] = mean of the squared distances from points[i] to its 3
 * nearest neighbours.  The reference imports it from the un-vendored `simple-knn` submodule; restated from that library's
 * published algorithm (Morton order + boxes of 1024 points + exact rejection search).  points: [P,3] float32 device.
 * --------------------------------------------------------------------------------------------------------------- */
size_t radegs_knn_scratch_bytes(int P);
int radegs_knn_mean_dist2(int P, const float* points, void* scratch, float* out /* [P] */, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Adaptive density control: the stage of the training iteration after the backward.  All pointers:
 * device; float32 unless typed otherwise.
 *
 * radegs_densify_stats: GaussianModel.add_densification_stats (scene/gaussian_model.py:743-747) and train.py:186's
 * max_radii2D update for one view, in place, one launch, no host read.  grad_means2D: [P,3] (xy signed, column 2 the
 * abs-gradient).  visible: [P] bytes, or NULL = radii > 0 (then radii is required).  For each visible row
 *   accum += sqrt(gx^2+gy^2); accum_abs += |g2|; accum_abs_max = max(., |g2|); denom += 1; max_radii2D = max(., radii)
 * (max_radii2D or radii NULL: that line is skipped).  Invisible rows are not written.  accum_abs_max propagates NaN as
 * upstream's torch.max does: a NaN |g2|, or a NaN already stored, leaves NaN (C's fmaxf would keep the other operand).
 * radegs_densify_stats_reduced: the same update from view_parallel's rank-reduced [P,3] statistics (sum |grad xy|,
 * sum |grad abs|, number of ranks that saw the Gaussian) and radii_max; rows whose count is 0 are not written;
 * accum_abs_max takes the max with the SUM column (the per-rank maximum is not transmitted).
 *
 * GaussianModel.densify_and_prune (scene/gaussian_model.py:717-741) is plan + apply around the one host read it needs:
 *   radegs_densify_plan   every clone / split / prune decision and the index of every surviving output row.
 *       abs_threshold: DEVICE scalar Q (upstream's torch.quantile);  dense_threshold = percent_dense * extent;
 *       prune_big != 0: also prune max(exp(_scaling)) > big_threshold (= 0.1 * extent; upstream's `if max_screen_size`).
 *       The max_radii2D > max_screen_size term is not an input: upstream zeroes max_radii2D before it reads it.
 *       workspace: radegs_densify_plan_bytes(P) bytes, 16-byte aligned, kept untouched until apply has run.
 *       counts4 (device ints): {rows out, clone-selected, split-selected, pruned by the final prune} -- the last three are
 *       upstream's return tuple.  The caller reads counts4 back, allocates, and calls
 *   radegs_densify_apply  writes all output arrays at P_out = counts4[0] rows in upstream's row order: surviving unsplit
 *       originals, clones, first children, second children.  unit_normals: [P,3,3] standard-normal draws indexed by source
 *       row (slot 0 the clone, 1 / 2 the children): xyz' = xyz + R(q/|q|) (z o exp(_scaling)); children store
 *       _scaling' = log(exp(_scaling) / 1.6); everything else is copied; moments of new rows are zero.
 *       tensors: [0..5] xyz[P,3] f_dc[P,3] f_rest[P,rest_floats] opacity[P,1] scaling[P,3] rotation[P,4], [6..11] their
 *       exp_avg, [12..17] their exp_avg_sq; a moment pair may be NULL (in and out: a group without optimizer state).
 * P = 0 and P_out = 0 are legal and launch nothing.
 * --------------------------------------------------------------------------------------------------------------- */
#define RADEGS_DENSIFY_NUM_TENSORS 18
#define RADEGS_DENSIFY_MAX_P (1 << 29)
typedef struct RadegsDensifyTensors {
  const float* in[RADEGS_DENSIFY_NUM_TENSORS];
  float* out[RADEGS_DENSIFY_NUM_TENSORS];
} RadegsDensifyTensors;
int radegs_densify_stats(int P, const float* grad_means2D /* [P,3] */, const int* radii /* [P] */, const unsigned char* visible /* [P] */,
                         float* accum, float* accum_abs, float* accum_abs_max, float* denom, float* max_radii2D, void* stream);
int radegs_densify_stats_reduced(int P, const float* densify_stats /* [P,3] */, const int* radii_max /* [P] or NULL */, float* accum,
                                 float* accum_abs, float* accum_abs_max, float* denom, float* max_radii2D, void* stream);
size_t radegs_densify_plan_bytes(int P);
int radegs_densify_plan(int P, const float* accum, const float* accum_abs, const float* denom, const float* scaling_raw /* [P,3] */,
                        const float* opacity_raw /* [P,1] */, float max_grad, const float* abs_threshold, float dense_threshold,
                        float min_opacity, int prune_big, float big_threshold, void* workspace, size_t workspace_bytes, int* counts4,
                        void* stream);
int radegs_densify_apply(int P, int P_out, int rest_floats, const RadegsDensifyTensors* tensors, const float* unit_normals /* [P,3,3] */,
                         const void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Mesh extraction: the steps of mesh_extract_tetrahedra.py around radegs_integrate.  All pointers:
 * device; float32 unless typed otherwise.  Every call returns 0 or a negative RADEGS_ERR_*, enqueues on `stream` (a
 * hipStream_t, NULL = the default stream) and neither synchronises nor reads anything back.  Sizes of 0 are legal and
 * launch nothing.
 *
 * Marching tetrahedra (utils/tetmesh.py:97-138, one chunk) is plan + emit around the one host read it needs:
 *   radegs_tetmesh_plan   occ = sdf > 0; a tet is crossing when 0 < sum(occ) < 4; a mesh vertex is one distinct edge
 *       (min, max) whose ends differ in occ, numbered in ascending lexicographic (min, max) order.  tets: [T,4] int32,
 *       16-byte aligned, indices in [0, V) (a tet with an index outside is treated as not crossing).  counts2 (device):
 *       {n_verts, n_faces}.  workspace: radegs_tetmesh_plan_bytes(V, T) bytes, 16-byte aligned, kept untouched until
 *       emit has run; it is sized for the worst case of 4 crossing edges per tet (about 180 bytes per tet).
 *       RADEGS_ERR_TOO_LARGE when 5 T >= 2^32 - 65 536: that bound keeps the crossing-edge instances (at most 4 T) and
 *       the scanned flags inside what the 32-bit primitives address.  V is an int, so V < 2^31.
 *   radegs_tetmesh_emit   n_verts / n_faces: counts2 as read back.  interp_v[v] = (min, max); end_points / end_sdf /
 *       end_scales are vertices / sdf / scales gathered at interp_v (bit-exact copies).  faces: all one-triangle tets in
 *       tet order, then all two-triangle tets in tet order, rows from upstream's 16 x 6 triangle table.
 *       Deviation: above 32 Mi tets upstream works in chunks and its FACE order becomes chunk by chunk; this is always
 *       the single-chunk order (same vertices, same order; same face set).
 * radegs_tetra_points: GaussianModel.get_tetra_points (scene/gaussian_model.py:400-429).  scales3: the 3D-filtered
 *   scales; rotation_raw: [P,4], normalised here; it, out_points and out_scale 16-byte aligned.  out_points: the eight corners of the +-3 sigma box
 *   of Gaussian i at rows 8 i .. 8 i + 7 (binary counting, x most significant: (-,-,-), (-,-,+), ... (+,+,+)), the
 *   centres at rows 8 P ..; out_scale: 3 * max(scales3) per row of out_points.
 * radegs_cull_alpha_accumulate: one view of evaluage_cull_alpha (mesh_extract_tetrahedra.py:42-54).  point_coordinate
 *   [PN,2] is pixel coordinates as radegs_integrate writes them and is NOT modified; mask [H,W] is sampled bilinearly
 *   (align_corners = False, zero padding) after multiplication by gt_mask and masks_extra ([H,W] or NULL each); where the
 *   sample is > 0.5: final_sdf = min(final_sdf, alpha_integrated), weight += 1.
 * radegs_cull_alpha_finish: sdf_out = weight > 0 ? 0.5 - final_sdf : -100.
 * radegs_tetmesh_bisect: one step of the binary search (mesh_extract_tetrahedra.py:93-102) in place; mid_sdf was
 *   evaluated at (left + right) / 2; where mid_sdf and left_sdf have the same strict sign the left end moves, else
 *   (mid_sdf == 0 included) the right end; mid_pts_out: (left + right) / 2 of the new bracket.
 * radegs_tetmesh_filter_plan / _apply: keep vertex v when |l0 - r0| <= scale_l + scale_r on the INITIAL end points
 *   [NV,2,3] and end scales [NV,2]; keep a face when all three of its vertices are kept; kept vertices stay in order and
 *   faces are renumbered (trimesh's update_vertices followed by update_faces).  counts2 (device): {vertices kept,
 *   faces kept}.  workspace: radegs_tetmesh_filter_plan_bytes(NV, NF), 16-byte aligned, untouched until apply has run.
 *   points [NV,3]: the vertex positions to filter (the bisection's result).
 * --------------------------------------------------------------------------------------------------------------- */
size_t radegs_tetmesh_plan_bytes(int V, long long T);
int radegs_tetmesh_plan(int V, long long T, const int* tets /* [T,4] */, const float* sdf /* [V] */, void* workspace, size_t workspace_bytes,
                        long long* counts2, void* stream);
int radegs_tetmesh_emit(int V, long long T, const int* tets, const float* sdf, const float* vertices /* [V,3] */, const float* scales /* [V] */,
                        const void* workspace, long long n_verts, long long n_faces, float* end_points /* [NV,2,3] */, float* end_sdf /* [NV,2] */,
                        float* end_scales /* [NV,2] */, long long* faces /* [NF,3] */, long long* interp_v /* [NV,2] */, void* stream);
int radegs_tetra_points(int P, const float* xyz, const float* scales3, const float* rotation_raw, float* out_points /* [9P,3] */,
                        float* out_scale /* [9P] */, void* stream);
int radegs_cull_alpha_accumulate(long long PN, const float* alpha_integrated, const float* point_coordinate, const float* mask,
                                 const float* gt_mask, const float* masks_extra, int W, int H, float* final_sdf, int* weight, void* stream);
int radegs_cull_alpha_finish(long long PN, const float* final_sdf, const int* weight, float* sdf_out, void* stream);
int radegs_tetmesh_bisect(long long N, float* left_pts, float* right_pts, float* left_sdf, float* right_sdf, const float* mid_sdf,
                          float* mid_pts_out, void* stream);
size_t radegs_tetmesh_filter_plan_bytes(long long NV, long long NF);
int radegs_tetmesh_filter_plan(long long NV, long long NF, const float* end_points, const float* end_scales, const long long* faces,
                               void* workspace, size_t workspace_bytes, long long* counts2, void* stream);
int radegs_tetmesh_filter_apply(long long NV, long long NF, const float* points, const long long* faces, const void* workspace,
                                long long nv_out, long long nf_out, float* out_vertices /* [nv_out,3] */, long long* out_faces /* [nf_out,3] */,
                                void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Mesh evaluation: evaluate_dtu_mesh.py's cull and dtu_eval/eval.py's Chamfer distance.  The same
 * conventions as above: device pointers unless marked (host), 0 or a negative RADEGS_ERR_*, work enqueued on `stream`,
 * nothing read back, sizes of 0 legal.  eval.py's geometry is fp64 here as there; the cull is fp32 as upstream's.
 *
 * radegs_mesheval_sample_count / _emit (eval.py:50-71): per triangle v1, v2, l1, l2, area2 = |v1 x v2|; dropped unless
 *   area2 > 0; thr = density sqrt(l1 l2 / area2), n = floor(l / thr); samples at k = ((i + .5) / n1, (j + .5) / n2),
 *   i <= n1, j <= n2, k0 + k1 < 1 evaluated as two fp64 divisions and one addition; q = (v1 k0 + v2 k1) + p0; order:
 *   triangles in input order, i major, j minor.  counts [F]; totals2 (device): {number of samples as 64 bits, number of
 *   triangles whose n exceeds 30 000 (their count is 0: refuse the mesh)}.  workspace: radegs_mesheval_sample_bytes(F),
 *   16-byte aligned, untouched until emit has run.  M: totals2[0] as read back; out [M,3].  A face with an index
 *   outside [0, V) yields no samples.
 * radegs_mesheval_grid_build: the uniform grid over `points` [N,3]: cell = floor((p - origin) / cell) wrapped into a
 *   32-bit key (11, 11, 10 bits for x, y, z), the cloud sorted by key (stable) and gathered.  origin3 (host).  The
 *   workspace (radegs_mesheval_grid_bytes(N), 16-byte aligned) IS the grid: hand it, with the same N, origin3 and
 *   cell, to the two consumers below.  Cells one key period apart alias; every candidate is decided by its distance.
 * radegs_mesheval_thin_rounds (eval.py:86-94): `rounds` rounds of the thinning over a grid with cell >= radius.  state
 *   [N] by point index: 0 undecided, 1 kept, 2 removed; start from zeros and *undecided = N.  A round removes an
 *   undecided point when a lower-index point within d^2 <= radius^2 is kept and keeps it when all of those are
 *   removed (d^2 = (dx^2 + dy^2) + dz^2).  Call until *undecided reads 0: state == 1 is then the mask eval.py's loop
 *   leaves.  No bound on the number of rounds is implied: a chain of N points needs N.
 * radegs_mesheval_nearest (eval.py:119-134): per query the distance and index of the nearest grid point if the distance
 *   is < max_dist, else inf and -1; equal distances: the lower index.  ceil(max_dist / cell) must not exceed 511.
 * radegs_mesheval_sum_below: out2 = {sum of dist < max_dist, their number}, in a fixed order (repeatable bit for bit).
 * radegs_mesheval_obs_mask (eval.py:102-110): box10 (host) = lo[3], hi[3] (inbound: lo <= p < hi), BB0[3], Res; dims3
 *   (host): the volume's shape; volume: uint8 [d0,d1,d2] row-major.  g = rint((p - BB0) / Res), half to even.  Three
 *   masks of length N: inbound; inbound & g inside the volume; that & volume[g] != 0.
 * radegs_mesheval_above_plane (eval.py:128-130): ((P0 x + P1 y) + P2 z) + P3 > 0; plane4 (host).
 * radegs_mesheval_dilate: binary dilation of mask != 0 [H,W] by the disk x^2 + y^2 <= radius^2, zero outside.
 * radegs_mesheval_cull_vertices (evaluate_dtu_mesh.py:111-133): flags[v] = 1 iff for every camera the vertex projects
 *   outside (-1, 1) or onto a set pixel of that camera's mask (nearest, align_corners = True, half to even).
 *   RadegsCullCamera.m: rows 0-2 of K w2c; masks: all cameras' uint8 masks in one buffer, mask_offset into it.
 * radegs_tetmesh_filter_plan_flags: radegs_tetmesh_filter_plan on ready vertex flags (0 / 1) instead of end points;
 *   radegs_tetmesh_filter_apply follows it the same way.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct RadegsCullCamera {
  float m[12];
  int W, H;
  long long mask_offset;
} RadegsCullCamera;

size_t radegs_mesheval_sample_bytes(long long F);
int radegs_mesheval_sample_count(long long V, long long F, const double* vertices /* [V,3] */, const long long* faces /* [F,3] */, double density,
                                 void* workspace, size_t workspace_bytes, int* counts /* [F] */, unsigned long long* totals2, void* stream);
int radegs_mesheval_sample_emit(long long V, long long F, const double* vertices, const long long* faces, double density, const void* workspace,
                                long long M, double* out /* [M,3] */, void* stream);
size_t radegs_mesheval_grid_bytes(long long N);
int radegs_mesheval_grid_build(long long N, const double* points /* [N,3] */, const double* origin3, double cell, void* workspace,
                               size_t workspace_bytes, void* stream);
int radegs_mesheval_thin_rounds(long long N, const void* grid_workspace, const double* origin3, double cell, double radius, int rounds,
                                unsigned char* state /* [N] */, unsigned* undecided, void* stream);
int radegs_mesheval_nearest(long long N, const void* grid_workspace, const double* origin3, double cell, long long Q,
                            const double* queries /* [Q,3] */, double max_dist, double* dist /* [Q] */, long long* index /* [Q] */, void* stream);
size_t radegs_mesheval_sum_bytes(void);
int radegs_mesheval_sum_below(long long Q, const double* dist, double max_dist, void* workspace, size_t workspace_bytes, double* out2, void* stream);
int radegs_mesheval_obs_mask(long long N, const double* points, const double* box10, const int* dims3, const unsigned char* volume,
                             unsigned char* inbound, unsigned char* grid_inbound, unsigned char* in_obs, void* stream);
int radegs_mesheval_above_plane(long long N, const double* points, const double* plane4, unsigned char* above, void* stream);
int radegs_mesheval_dilate(int W, int H, const unsigned char* mask, int radius, unsigned char* out, void* stream);
int radegs_mesheval_cull_vertices(long long NV, const float* vertices /* [NV,3] */, int ncam, const RadegsCullCamera* cameras,
                                  const unsigned char* masks, unsigned* flags /* [NV] */, void* stream);
int radegs_tetmesh_filter_plan_flags(long long NV, long long NF, const unsigned* vertex_flags, const long long* faces, void* workspace,
                                     size_t workspace_bytes, long long* counts2, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Decoupled appearance loss: train.py:37-58 L1_loss_appearance over scene/appearance_network.py.
 * The trunk (conv1 and the four pixel-shuffle blocks, at most half resolution) stays with the caller; these entry
 * points are everything at full resolution.  Conventions as above: device pointers, float32, 0 or a negative
 * RADEGS_ERR_*, work enqueued on `stream`, nothing read back; every argument is checked before anything is queued.
 *
 * Crop: H = orig_height / 32 * 32, W likewise, top = orig_height / 2 - H / 2, left likewise; orig_height and
 * orig_width in [32, 32768].  image / gt: [3,orig_height,orig_width].
 *
 * radegs_appearance_downsample_forward: down [3,H/32,W/32] = bilinear resize of the crop, align_corners=True, with
 *   torch's index arithmetic (source coordinate = dst * (in-1)/(out-1) in fp32, scale 0 when out == 1).
 * radegs_appearance_downsample_backward: grad_image [3,orig_height,orig_width], written completely (zero where no
 *   output reads).
 * radegs_appearance_head_forward: feat [16,H/2,W/2] (feat_height / feat_width must be exactly H/2, W/2);
 *   W2 [16,16,3,3], b2 [16], W3 [3,16,3,3], b3 [3].  loss[0] = mean |sigmoid(conv3(relu(conv2(bilinear x2 (feat)))))
 *   * crop(image) - crop(gt)|, both convolutions zero-padded at the crop border.  `transformed` (optional,
 *   [3,H,W]) receives the product before the difference: the inference branch.  Writes nothing else of full
 *   resolution.  scratch: radegs_appearance_head_scratch_bytes(.., 0) bytes, 16-byte aligned.
 * radegs_appearance_head_backward: grad_loss: one device float.  Writes grad_feat [16,H/2,W/2], grad_image
 *   [3,orig_height,orig_width] (completely: zero outside the crop; the path through `down` is not included),
 *   grad_W2, grad_b2, grad_W3, grad_b3.  scratch: radegs_appearance_head_scratch_bytes(.., 1) bytes; it holds the
 *   one full-resolution intermediate, the gradient at conv2's pre-activation [16,H,W].
 * No float atomics: two calls on the same inputs return the same bits.  The scratch query returns 0 for a size
 * the calls would refuse.
 * --------------------------------------------------------------------------------------------------------------- */
int radegs_appearance_downsample_forward(int orig_height, int orig_width, const float* image, float* down, void* stream);
int radegs_appearance_downsample_backward(int orig_height, int orig_width, const float* grad_down, float* grad_image, void* stream);
size_t radegs_appearance_head_scratch_bytes(int orig_height, int orig_width, int backward);
int radegs_appearance_head_forward(int orig_height, int orig_width, int feat_height, int feat_width, const float* feat, const float* image, const float* gt,
                                   const float* W2, const float* b2, const float* W3, const float* b3, void* scratch, size_t scratch_bytes,
                                   float* loss, float* transformed, void* stream);
int radegs_appearance_head_backward(int orig_height, int orig_width, int feat_height, int feat_width, const float* feat, const float* image, const float* gt,
                                    const float* W2, const float* b2, const float* W3, const float* b3, const float* grad_loss, void* scratch,
                                    size_t scratch_bytes, float* grad_feat, float* grad_image, float* grad_W2, float* grad_b2, float* grad_W3,
                                    float* grad_b3, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * TSDF fusion: mesh_extract.py:51-105, the DTU route from depth maps to recon.ply, which upstream
 * hands to Open3D's VoxelBlockGrid on the CPU.  Conventions as above: device pointers unless marked (host), 0 or a
 * negative RADEGS_ERR_*, work enqueued on `stream`, nothing read back, sizes of 0 legal.  All device arithmetic is
 * float32, one rounding per operation, products before sums in the order written here.
 *
 * The grid: blocks of 16^3 voxels.  block_size = 16 voxel_size, sdf_trunc = voxel_size trunc_voxel_multiplier (both
 * rounded to float32 once, on the host).  A block's coordinate is floor(world / block_size) per axis, each in
 * [-2^20, 2^20); its key is (z + 2^20) << 42 | (y + 2^20) << 21 | (x + 2^20).  The grid is `keys` [n] ascending and
 * `slots` [n] int: block i's voxels are rows slots[i] of tsdf / weight [capacity][4096] and color
 * [capacity][4096][3], voxel index (z * 16 + y) * 16 + x.
 * cam16 (host): fx, fy, cx, cy, then a 3x4 matrix by rows.
 *
 * radegs_tsdf_touch: the matrix is camera to world.  For every pixel (4i, 4j), i < H / 4, j < W / 4, with
 *   d = depth / depth_scale, 0 < d < depth_max: ray ((x - cx) / fx, (y - cy) / fy, 1); t_min = max(d - sdf_trunc, 0),
 *   t_max = min(d + sdf_trunc, depth_max), step = (t_max - t_min) / 3; the four points ray * (t_min + k step) go to
 *   the world as ((m0 px + m1 py) + m2 pz) + m3 per row and yield one block each.  Then as radegs_tsdf_unique_plan
 *   with an empty grid, over 4 (W / 4) (H / 4) items: size the workspace for that.
 * radegs_tsdf_unique_plan: coords int [n,3].  Sorts the keys (two stable 32-bit passes), marks first occurrences and
 *   looks them up in the grid's keys.  counts3 (device) = {distinct blocks, those not in the grid, 1 if a
 *   coordinate lay outside the 21 bits -- such an item yields no block: refuse the call}.  workspace:
 *   radegs_tsdf_unique_bytes(n), 16-byte aligned, untouched until the calls below have run.
 * radegs_tsdf_unique_emit: coords_out int [n_unique,3], ascending by key; n_unique as read back.
 * radegs_tsdf_insert_apply: new_keys / new_slots [ngrid + n_new]: the grid with the new blocks merged in, the new
 *   block of rank r (in key order) in slot ngrid + r -- the caller provides capacity >= ngrid + n_new and
 *   zero-fills those rows.  active_slots [n_unique], active_coords [n_unique,3]: the listed blocks.
 * radegs_tsdf_integrate: the matrix is world to camera with its rotation part multiplied by voxel_size (in float64,
 *   before the conversion).  One workgroup per listed block.  Per voxel X = 16 b + v (integers, as float32):
 *   p = ((m0 X.x + m1 X.y) + m2 X.z) + m3 per row; skipped unless p.z > 0; u = (fx p.x) / p.z + cx, v likewise;
 *   ui = roundf(u), vi = roundf(v) (half away from zero); skipped unless 0 <= ui < W, 0 <= vi < H;
 *   d = depth[vi][ui] / depth_scale, sdf = d - p.z; skipped unless d > 0, d <= depth_max, sdf >= -sdf_trunc;
 *   s = min(sdf, sdf_trunc) / sdf_trunc; inv = 1 / (w + 1); tsdf = (w tsdf + s) inv; color = (w color + c) inv per
 *   channel (color [H][W][3]); w = w + 1.  color and block_color are both given or both null.
 * radegs_tsdf_extract_plan / _emit: marching cubes over the cells whose eight corners (looked up across block
 *   borders) all have weight > weight_threshold; case bit i = corner i negative (csrc/rg_mc_tables.h, generated by
 *   scripts/make_mc_tables.py).  A voxel owns the edges leaving it along +x, +y, +z; an owned edge carries a vertex
 *   iff a valid cell cuts it: ratio = (0 - tsdf_o) / (tsdf_e - tsdf_o), position voxel_size (X + ratio axis),
 *   colour c_o + ratio (c_e - c_o).  Vertices in (key, voxel, axis) order, faces in (key, voxel of the cell's lowest
 *   corner, table) order.  counts2 (device) = {V, F}; workspace: radegs_tsdf_extract_bytes(n), 16-byte aligned,
 *   untouched until emit has run.  At most 2^19 - 1 blocks.  vertices [V,3], faces [F,3], colors [V,3] or null.
 * --------------------------------------------------------------------------------------------------------------- */
size_t radegs_tsdf_unique_bytes(long long n);
int radegs_tsdf_touch(int W, int H, const float* depth /* [H,W] */, const float* cam16, float depth_scale, float depth_max, float sdf_trunc,
                      float block_size, void* workspace, size_t workspace_bytes, long long* counts3, void* stream);
int radegs_tsdf_unique_plan(long long n, const int* coords /* [n,3] */, long long ngrid, const unsigned long long* grid_keys, void* workspace,
                            size_t workspace_bytes, long long* counts3, void* stream);
int radegs_tsdf_unique_emit(long long n, const void* workspace, long long n_unique, int* coords_out /* [n_unique,3] */, void* stream);
int radegs_tsdf_insert_apply(long long n, const void* workspace, long long ngrid, const unsigned long long* grid_keys, const int* grid_slots,
                             long long n_unique, long long n_new, unsigned long long* new_keys, int* new_slots, int* active_slots,
                             int* active_coords, void* stream);
int radegs_tsdf_integrate(long long n_active, const int* active_slots, const int* active_coords, long long capacity, int W, int H, const float* depth,
                          const float* color, const float* cam16, float depth_scale, float depth_max, float sdf_trunc, float* tsdf, float* weight,
                          float* block_color, void* stream);
size_t radegs_tsdf_extract_bytes(long long n);
int radegs_tsdf_extract_plan(long long n, const unsigned long long* keys, const int* slots, const float* tsdf, const float* weight,
                             float weight_threshold, void* workspace, size_t workspace_bytes, long long* counts2, void* stream);
int radegs_tsdf_extract_emit(long long n, const unsigned long long* keys, const int* slots, const float* tsdf, const float* block_color,
                             float voxel_size, const void* workspace, long long V, long long F, float* vertices, long long* faces, float* colors,
                             void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Tanks-and-Temples evaluation: eval_tnt/run.py with registration.py and evaluation.py, which
 * upstream hands to Open3D on the CPU.  Conventions as above: device pointers unless marked (host), 0 or a negative
 * RADEGS_ERR_*, work enqueued on `stream`, nothing read back, sizes of 0 legal.  All geometry is float64, one
 * rounding per operation, in the order written here.  Nearest neighbours are radegs_mesheval_grid_build / _nearest.
 *
 * radegs_tnteval_centroids (run.py:97): out [F,3] = ((a + b) + c) / 3 per face; a face with an index outside
 *   [0, V) yields NaN.
 * radegs_tnteval_transform: matrix12 (host): rows 0-2 of a 4x4 by rows, finite; out = ((m0 x + m1 y) + m2 z) + m3
 *   per row.  out may be points.
 * radegs_tnteval_crop: the selection polygon volume.  orthogonal_axis 0 / 1 / 2 = "X" / "Y" / "Z"; (u, v, w) =
 *   (1, 2, 0), (0, 2, 1), (0, 1, 2).  polygon_uv [n_polygon,2]: the polygon's u and v coordinates, 3 to 1024
 *   vertices.  keep[i] = 0 if p[w] < axis_min or p[w] > axis_max; otherwise every edge (i, j = (i + 1) % n) with
 *   (poly[i].v > p[v]) != (poly[j].v > p[v]) yields the node
 *   poly[i].u + (p[v] - poly[i].v) / (poly[j].v - poly[i].v) * (poly[j].u - poly[i].u), and keep[i] = 1 iff the
 *   number of nodes < p[u] is odd.
 * radegs_tnteval_voxel_plan / _emit: index = floor((p - origin) / voxel) per axis (origin3 (host): the caller
 *   passes min - 0.5 voxel), each in [0, 2^21); key = ix << 42 | iy << 21 | iz, sorted (stable); counts2 (device) =
 *   {number of occupied voxels M, 1 if an index lay outside the 21 bits: refuse the call}.  emit: means [M,3] = the
 *   voxel's points added in index order, divided by their number; counts [M]; voxels ascending by (ix, iy, iz).
 *   workspace: radegs_tnteval_voxel_bytes(N), 16-byte aligned, untouched until emit has run.
 * radegs_tnteval_pair_sums: over the pairs q with 0 <= index[q] < NT, s = moved[q], t = target[index[q]]:
 *   out18 = {count, sum s [3], sum t [3], sum (dx^2 + dy^2) + dz^2 of s - t, sum (t - mt)(s - ms)^T [3][3] by rows,
 *   sum |s - ms|^2}, ms = sum s / count and mt likewise, formed on the device.  Fixed order: repeatable bit for
 *   bit.  workspace: radegs_tnteval_sums_bytes(), 16-byte aligned.
 * radegs_tnteval_histogram: numpy.histogram over explicit ascending edges [n_edges] (2 to 4096): hist [n_edges - 1],
 *   bin b = edges[b] <= d < edges[b + 1], the last bin closed on both sides, NaN in no bin; below[0] = the number
 *   of d < threshold.  Both are zeroed by the call.
 * --------------------------------------------------------------------------------------------------------------- */
int radegs_tnteval_centroids(long long V, long long F, const double* vertices /* [V,3] */, const long long* faces /* [F,3] */, double* out /* [F,3] */,
                             void* stream);
int radegs_tnteval_transform(long long N, const double* points /* [N,3] */, const double* matrix12, double* out /* [N,3] */, void* stream);
int radegs_tnteval_crop(long long N, const double* points, int orthogonal_axis, double axis_min, double axis_max, int n_polygon, const double* polygon_uv,
                        unsigned char* keep /* [N] */, void* stream);
size_t radegs_tnteval_voxel_bytes(long long N);
int radegs_tnteval_voxel_plan(long long N, const double* points, const double* origin3, double voxel, void* workspace, size_t workspace_bytes,
                              long long* counts2, void* stream);
int radegs_tnteval_voxel_emit(long long N, const double* points, const void* workspace, long long M, double* means /* [M,3] */, int* counts /* [M] */,
                              void* stream);
size_t radegs_tnteval_sums_bytes(void);
int radegs_tnteval_pair_sums(long long Q, const double* moved /* [Q,3] */, long long NT, const double* target /* [NT,3] */, const long long* index /* [Q] */,
                             void* workspace, size_t workspace_bytes, double* out18, void* stream);
int radegs_tnteval_histogram(long long N, const double* dist, int n_edges, const double* edges, double threshold, long long* hist, long long* below,
                             void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Tanks-and-Temples mesh culling: eval_tnt/cull_mesh.py, which upstream hands to pyrender / EGL
 * (the depth maps) and to eager torch (Mesher.point_masks).  Conventions as above: device pointers, 0 or a negative
 * RADEGS_ERR_*, work enqueued on `stream`, nothing read back, sizes of 0 legal.  The faces are then filtered with
 * radegs_tetmesh_filter_plan_flags / radegs_tetmesh_filter_apply.
 *
 * radegs_tntcull_render_begin / _finish: depth [B,H,W] of the mesh as B cameras see it; a pixel no triangle covers
 *   reads 0.  float64, one rounding per operation, in the order written here (DESIGN.md 11 N11 gives the reasons).
 *   w2c [B,12]: rows 0-2 of each world-to-camera matrix by rows; the camera looks down -z, +y is up, image row 0 is
 *   at the top.  Per vertex: X = ((m0 x + m1 y) + m2 z) + m3, Y and Z likewise, d = -Z.
 *   Near clip: Sutherland-Hodgman against d >= znear in camera space, vertex order kept, walking 0 -> 1 -> 2 -> 0; a
 *   quad is fanned from its first vertex.  Where an edge meets the plane: from the end a that is smaller in
 *   (X, then Y, then d), t = (znear - d_a) / (d_b - d_a), X = X_a + t (X_b - X_a), Y likewise, d = znear.
 *   Window: x = fx X / d + cx, y = cy - fy Y / d; pixel (i, j) is sampled at (j + 0.5, i + 0.5).
 *   Edge a -> b at p: from the end that is smaller in (x, then y), (bx - ax)(py - ay) - (by - ay)(px - ax), negated if
 *   that end is b.  area = the edge 0 -> 1 at vertex 2; area == 0 (or NaN): skipped; area < 0: all three values are
 *   negated.  Candidates: the pixel centres of the closed bounding box, j in [ceil(xmin - 0.5), floor(xmax - 0.5)]
 *   cut to [0, W - 1], rows likewise.  Covered iff E0, E1, E2 >= 0 (Ek: the edge opposite vertex k) and
 *   (E0 + E1) + E2 > 0; d = ((E0 + E1) + E2) / ((E0 / d0 + E1 / d1) + E2 / d2); kept iff znear <= d <= zfar; rounded
 *   to float32; a pixel keeps the minimum (a 32-bit unsigned atomic minimum on the bits: independent of face order).
 *   begin clears the maps, sets every triangle up and draws the boxes of at most 256 pixel centres; larger boxes go
 *   to a queue in the workspace, in chunks of 1024 pixel centres; finish drains the queue and resolves untouched
 *   pixels to 0.  Both take the same arguments; depth is not to be read in between.  A chunk that finds the queue
 *   full is drawn by begin itself: any workspace of at least radegs_tntcull_render_bytes(0, 0) bytes (the header)
 *   gives the same maps, radegs_tntcull_render_bytes(F, B) is the size that keeps begin fast.  16-byte aligned.
 *   stats4 (device, may be NULL): {queue chunks asked for, triangles drawn by begin, triangles queued, chunks begin
 *   drew because the queue was full}.  znear > 0, zfar > znear, 2 <= H, W <= 32768, B <= 65535, V, F < 2^31; faces with
 *   an index outside [0, V) draw nothing.
 * radegs_tntcull_count_views (cull_mesh.py:132-170 at forecast_radius 0): counts[i] += the number of the B cameras
 *   that see point i.  float32, one rounding per operation.  w2c [B,12] float32.  Per camera:
 *   cam = ((m0 x + m1 y) + m2 z) + m3 per row; z = z_c + 1e-8; u = (fx x_c + cx z_c) / z, v = (fy y_c + cy z_c) / z;
 *   in_frustum = 0 <= u <= W - 1 and 0 <= v <= H - 1 and z > 0; the depth map [H,W] is sampled bilinearly at
 *   ix = min(W - 1, max(((u / (W - 1) * 2 - 1) + 1) / 2 * (W - 1), 0)), iy likewise (grid_sample, align_corners = True,
 *   border padding): x0 = floor(ix), weights nw = (x0 + 1 - ix)(y0 + 1 - iy), ne = (ix - x0)(y0 + 1 - iy),
 *   sw = (x0 + 1 - ix)(iy - y0), se = (ix - x0)(iy - y0), s = (((0 + nw D[y0][x0]) + ne D[y0][x0 + 1]) +
 *   sw D[y0 + 1][x0]) + se D[y0 + 1][x0 + 1], a neighbour outside the image left out;
 *   seen = in_frustum and (s > 0 ? z < s + eps : true).
 * --------------------------------------------------------------------------------------------------------------- */
size_t radegs_tntcull_render_bytes(long long F, int B);
int radegs_tntcull_render_begin(long long V, long long F, const double* vertices /* [V,3] */, const long long* faces /* [F,3] */, int B,
                                const double* w2c /* [B,12] */, int H, int W, double fx, double fy, double cx, double cy, double znear, double zfar,
                                void* workspace, size_t workspace_bytes, float* depth /* [B,H,W] */, void* stream);
int radegs_tntcull_render_finish(long long V, long long F, const double* vertices, const long long* faces, int B, const double* w2c, int H, int W,
                                 double fx, double fy, double cx, double cy, double znear, double zfar, const void* workspace, size_t workspace_bytes,
                                 float* depth, long long* stats4, void* stream);
int radegs_tntcull_count_views(long long N, const float* points /* [N,3] */, int B, int H, int W, const float* depths /* [B,H,W] */,
                               const float* w2c /* [B,12] */, float fx, float fy, float cx, float cy, float eps, int* counts /* [N] */, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Mesh clean-up: the steps that treat the mesh as a graph, which upstream hands to Open3D
 * (utils/mesh_utils.py:23-44 post_process_mesh, mesh_extract.py:104 compute_vertex_normals) and to trimesh
 * (eval_tnt/cull_mesh.py:186-202 get_connected_mesh).  Conventions as above: device pointers, 0 or a negative
 * RADEGS_ERR_*, work enqueued on `stream`, nothing read back, arguments refused before the first HIP call.
 * faces int64 [F,3], vertices float64 [V,3]; V < 2^31 and F <= 2^30, beyond that RADEGS_ERR_TOO_LARGE; F == 0 launches
 * nothing.  Workspaces are 16-byte aligned.  A face with an index outside [0, V) is never used to address memory: it
 * joins nothing, has area 0, adds to no normal and does not survive a compaction.
 *
 * radegs_meshclean_cluster: triangle_clusters[f] in [0, C) and *n_clusters = C.  The 3 F records (min, max) of the
 *   edges corner k -> corner k + 1 are sorted; a record with equal ends joins nothing; manifold = 0: all triangles of
 *   the records with one key are joined (Open3D's cluster_connected_triangles), manifold = 1: only where exactly two
 *   records have the key (trimesh's face_adjacency; records are counted, so a triangle (a, b, a) brings two).  Clusters
 *   are numbered by ascending smallest triangle index.  The labels do not depend on the order of the atomics.
 * radegs_meshclean_stats: cluster_n_triangles [C]; cluster_area [C] (may be NULL) = the sum of
 *   0.5 * sqrt((nx nx + ny ny) + nz nz), n = (b - a) x (c - a) = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx), one
 *   rounding per operation, over the cluster's triangles in ascending index: consecutive groups of 256 (the last
 *   padded with 0.0) through the 256-wide halving tree, then the group sums added to 0.0 in ascending order;
 *   total_area [1] (may be NULL) = the two-stage fixed-order sum over all triangles in their own order.  C is the value
 *   radegs_meshclean_cluster left in *n_clusters, read by the host in between to size these outputs.
 * radegs_meshclean_compact_plan / _apply: a face is selected unless remove[f] != 0 (remove may be NULL) or
 *   cluster_keep[triangle_clusters[f]] == 0 (cluster_keep may be NULL); drop_unreferenced: only the corners of the
 *   selected faces stay as vertices; drop_degenerate: a selected face with two equal indices goes (after the vertices
 *   were marked).  counts2 = {vertices kept, faces kept}, which the host reads to size kept_vertices [nv] (the old index
 *   of every new vertex) and out_faces [nf,3] (renumbered); both keep the original relative order.
 * radegs_meshclean_vertex_normals: normals [V,3] = per vertex the sum of the n above over its corners in ascending
 *   (triangle, corner) order, starting from 0.0; normalized: divided by len = sqrt((sx sx + sy sy) + sz sz), or
 *   (0, 0, 1) unless len is positive and finite.
 * --------------------------------------------------------------------------------------------------------------- */
size_t radegs_meshclean_cluster_bytes(long long F);
int radegs_meshclean_cluster(long long V, long long F, const long long* faces, int manifold, void* workspace, size_t workspace_bytes,
                             long long* triangle_clusters /* [F] */, long long* n_clusters /* [1] */, void* stream);
size_t radegs_meshclean_stats_bytes(long long F, long long C);
int radegs_meshclean_stats(long long V, long long F, long long C, const double* vertices, const long long* faces, const long long* triangle_clusters,
                           void* workspace, size_t workspace_bytes, long long* cluster_n_triangles /* [C] */, double* cluster_area /* [C] */,
                           double* total_area /* [1] */, void* stream);
size_t radegs_meshclean_compact_bytes(long long V, long long F);
int radegs_meshclean_compact_plan(long long V, long long F, long long C, const long long* faces, const unsigned char* remove /* [F] */,
                                  const long long* triangle_clusters /* [F] */, const unsigned char* cluster_keep /* [C] */, int drop_degenerate,
                                  int drop_unreferenced, void* workspace, size_t workspace_bytes, long long* counts2, void* stream);
int radegs_meshclean_compact_apply(long long V, long long F, const long long* faces, const void* workspace, long long nv_out, long long nf_out,
                                   long long* kept_vertices /* [nv_out] */, long long* out_faces /* [nf_out,3] */, void* stream);
size_t radegs_meshclean_normals_bytes(long long F);
int radegs_meshclean_vertex_normals(long long V, long long F, const double* vertices, const long long* faces, int normalized, void* workspace,
                                    size_t workspace_bytes, double* normals /* [V,3] */, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Delaunay: the tetrahedra of N points, which upstream gets from tetranerf's CGAL binding
 * (mesh_extract_tetrahedra.py:63, cpp.triangulate).  Conventions as above: device pointers unless marked (host), 0 or a
 * negative RADEGS_ERR_*, work enqueued on `stream`, nothing read back, arguments refused before the first HIP call.
 * points float64 [N,3], finite; 4 <= N <= 2^31 - 8 and record_capacity <= 2^32 - 65 537, beyond that
 * RADEGS_ERR_TOO_LARGE.  The workspace is 16-byte aligned, radegs_delaunay_bytes(N, record_capacity) long, and the same
 * for plan and emit: emit reads what plan left in it.
 *
 * Coordinates triangulated (radegs_delaunay_perturb writes them to out [N,3]; plan computes the same):
 *   x' = x + scale * (u - 0.5),  one rounding per operation;  x' = x where scale == 0;
 *   u = (z >> 11) * 2^-53,  z = fin((3 i + axis + 1) * 0x9E3779B97F4A7C15 + seed * 0xD1B54A32D192ED03)  mod 2^64,
 *   fin(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
 *   The caller passes scale = jitter * bounding-box diagonal.
 * Every point clips its own Voronoi cell (rade-gs_amd/csrc/rg_delaunay_cell.h states the predicates, the four ghost
 * generators at infinity that close the cells of hull points, and the error bound behind `uncertain`); a cell's
 * vertices that hold no ghost are the tetrahedra at that point.
 *
 * radegs_delaunay_plan: bounds (host) = {min x, y, z, max x, y, z} of the points, used only to lay the search grid: any
 *   finite box gives the same result.  Appends one record (the ascending quadruple of point indices) per tetrahedron
 *   per corner that found it to the workspace, at most record_capacity of them, and writes counts4 = {records found
 *   (4 T on a consistent input; above record_capacity: nothing past the capacity was written, call again with more
 *   room), points deferred to the one-wave-per-point kernel, predicate values within their error bound, cells that
 *   outgrew the 256 faces / 508 triangles of that kernel}.  The host reads counts4.
 * radegs_delaunay_emit: records = counts4[0] <= record_capacity.  Sorts the records (two passes of the two-word sort),
 *   and writes one row per distinct quadruple, in lexicographic order, to cells int32 [out_capacity,4] (rows past the
 *   capacity are dropped): (a, b, c, d) ascending, c and d exchanged where det[b - a, c - a, d - a] < 0 on x'.
 *   counts2 = {distinct quadruples, those not found exactly four times or with a zero determinant}.
 *
 * Size.  A record costs 16 B and the sort's working arrays 56 B more, and 4 T is about 27 N on scattered points, so the
 * workspace is about 2 KB a point (N = 30 M: 58 GB); the 32-bit sort words bound 4 T below 2^32 - 65 536, N near 150 M.
 * --------------------------------------------------------------------------------------------------------------- */
size_t radegs_delaunay_bytes(long long N, long long record_capacity);
int radegs_delaunay_perturb(long long N, const double* points /* [N,3] */, double scale, unsigned long long seed, double* out /* [N,3] */, void* stream);
int radegs_delaunay_plan(long long N, const double* points /* [N,3] */, const double* bounds /* (host) [6] */, double scale, unsigned long long seed,
                         long long record_capacity, void* workspace, size_t workspace_bytes, long long* counts4, void* stream);
int radegs_delaunay_emit(long long N, long long records, long long record_capacity, void* workspace, size_t workspace_bytes, long long out_capacity,
                         int* cells /* [out_capacity,4] */, long long* counts2, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Image evaluation: what render.py -> metric.py need and upstream takes from torchvision and
 * lpipsPyTorch: the 8-bit round trip of a saved image, PSNR's squared-difference sum, and the LPIPS-VGG trunk and
 * taps.  Conventions as above: device pointers unless marked (host), 0 or a negative RADEGS_ERR_*, work enqueued on
 * `stream`, nothing read back, arguments refused before the first HIP call.  All float32 unless stated; activations
 * are channels-last [N,H,W,C]; H, W <= 32768 and N H W < 2^31 - 64.
 *
 * radegs_imageeval_conv3x3: y = max(conv3x3(x, w) + bias, 0), stride 1, zero padding 1.  Cin a multiple of 16, Cout a
 *   multiple of 64.  Every output element is ONE fmaf chain that starts at the bias, in the K order of
 *   rade-gs_amd/csrc/rg_conv_chain.h (chunks of 16 channels, then the nine taps row by row, then the chunk's channels);
 *   the f32-input MFMA computes it.  packed_weight holds w[co][ci][ky][kx] as [Cout/64][Cin/16][ky*3+kx][ci%16][co%64],
 *   16-byte aligned like x.
 * radegs_imageeval_conv3x3_first: the same chain for Cin = 3 (one chunk) on a planar image [N,3,H,W], with
 *   (image - mean3[c]) / std3[c] applied as a pixel is loaded; a pixel outside the image is 0 after that step.
 *   mean3, std3 (host).  packed_weight is [ky*3+kx][ci][Cout].
 * radegs_imageeval_tap: feat [2,H,W,C] holds the feature maps of the two images, C in {64,128,256,512}.
 *   out[0] (float64) = 1/(H W) sum over pixels of sum_c lin[c] (fx_c/(|fx| + 1e-10) - fy_c/(|fy| + 1e-10))^2, |.| the
 *   channel norm; float32 per pixel, float64 in a fixed order across pixels, so two calls return the same bits.
 *   pooled (may be NULL; needs H, W >= 2) [2,H/2,W/2,C] = the 2x2 max pool, the last row / column of an odd size
 *   dropped.  Workspace: 16-byte aligned, radegs_imageeval_tap_bytes(H, W).
 * radegs_imageeval_quantize: image planar [3,H,W]; u8 [H,W,3] (may be NULL) = trunc(clamp(x * 255 + 0.5, 0, 255)) with
 *   one rounding per operation, NaN -> 0; out [3,H,W] (may be NULL) = u8 / 255.
 * radegs_imageeval_ssd: out[0] (float64) = sum_i float32((a_i - b_i)^2), n >= 1 elements, fixed order.
 * --------------------------------------------------------------------------------------------------------------- */
int radegs_imageeval_conv3x3(int N, int H, int W, int Cin, int Cout, const float* x, const float* packed_weight, const float* bias, float* y, void* stream);
int radegs_imageeval_conv3x3_first(int N, int H, int W, int Cout, const float* image, const float* mean3 /* (host) */, const float* std3 /* (host) */,
                                   const float* packed_weight, const float* bias, float* y, void* stream);
size_t radegs_imageeval_tap_bytes(int H, int W);
int radegs_imageeval_tap(int H, int W, int C, const float* feat, const float* lin /* [C] */, float* pooled, void* workspace, size_t workspace_bytes,
                         double* out, void* stream);
int radegs_imageeval_quantize(int H, int W, const float* image, unsigned char* u8, float* out, void* stream);
size_t radegs_imageeval_ssd_bytes(void);
int radegs_imageeval_ssd(long long n, const float* a, const float* b, void* workspace, size_t workspace_bytes, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Model state: the Gaussian model on its way to and from a file, which upstream does through
 * plyfile and a dozen eager kernels each: GaussianModel.save_ply / load_ply (scene/gaussian_model.py:379-397, 515-559),
 * reset_opacity (495-513) and create_from_pcd after the kNN step (301-328).  Conventions as above: device pointers, 0
 * or a negative RADEGS_ERR_*, work enqueued on `stream`, nothing read back, arguments refused before the first HIP
 * call.  All tensors float32 and contiguous; row counts are long long (20 M records of 252 B pass 4 GB).  Every kernel
 * is one pass without atomics: two calls return the same bits.  Divisions and square roots are IEEE (the unit is built
 * without fast-math, clang's default for HIP keeps float division correctly rounded) and no product is contracted.
 *
 * radegs_modelio_pack: rows [row_begin, row_end) of xyz [P,3], f_dc [P,1,3], f_rest [P,K,3] (K <=
 *   RADEGS_MODELIO_MAX_REST; may be NULL for K = 0), opacity [P,1], scaling [P,3], rotation [P,4] and filter_3D [P,1]
 *   (may be NULL) become records of C = 17 + 3 K (+ 1 with the filter) floats in out [row_end - row_begin, C] (16-byte
 *   aligned), in the file's order: x y z, nx ny nz (zeros), f_dc_0..2, f_rest_0..3K-1 with f_rest_{c K + k} =
 *   f_rest[k][c] (upstream's transpose(1,2).flatten(1)), opacity, scale_0..2, rot_0..3, filter_3D.  Bits are copied.
 * radegs_modelio_unpack: records holds P records of S bytes (1 <= S <= RADEGS_MODELIO_MAX_RECORD), little-endian, at
 *   a 4-byte aligned address, and is readable up to the next multiple of 4 past P S.  columns [D] (device memory, D <=
 *   RADEGS_MODELIO_MAX_COLUMNS, 16-byte aligned): for every row r the value of type src_type at byte src_offset of the
 *   record is written as float32 to dst[r * dst_stride + dst_elem].  F4 with scale = 0 is copied bit for bit; every
 *   other value goes through double: divided by 255.0 where scale != 0 (so U1 gives float(double(u) / 255.0), upstream's
 *   float64 quotient followed by .float()), then rounded to nearest even once (F8 as torch.tensor(float64,
 *   dtype=torch.float)).  A descriptor with an unknown type or that leaves the record reads and writes nothing.
 * radegs_modelio_reset_opacity: per row, float32, expf / logf / sqrtf, one rounding per operation, in upstream's order:
 *   q_k = exp(s_k)^2, coef = sqrt(((q0 q1) q2) / (((q0 + f^2)(q1 + f^2))(q2 + f^2))), cur = (1 / (1 + exp(-o))) coef,
 *   x = min(cur, 0.01) / coef (a NaN passes through), opacity_out = log(x / (1 - x)).  zero_a, zero_b [P] (may be NULL;
 *   the opacity's two Adam moments) are filled with zeros.
 * radegs_modelio_init: f_dc = (colors - 0.5f) / 0.28209479177387814f (RGB2SH, IEEE float division), f_rest [P,K,3] =
 *   0, scaling = log(sqrt(max(dist2, 1e-7f))) in all three columns, rotation (16-byte aligned) = (1, 0, 0, 0), opacity =
 *   opacity_value, which the caller computes once: the float32 log(0.1f / (1 - 0.1f)).  dist2 [P] is
 *   radegs_knn_mean_dist2's output.
 * --------------------------------------------------------------------------------------------------------------- */
#define RADEGS_MODELIO_MAX_REST 79        /* K: the 64-row LDS image of the output tile stays within 64 KB */
#define RADEGS_MODELIO_MAX_RECORD 768     /* S */
#define RADEGS_MODELIO_MAX_COLUMNS 256    /* D */
enum { RADEGS_MODELIO_I1 = 0, RADEGS_MODELIO_U1, RADEGS_MODELIO_I2, RADEGS_MODELIO_U2, RADEGS_MODELIO_I4, RADEGS_MODELIO_U4, RADEGS_MODELIO_F4,
       RADEGS_MODELIO_F8 };
typedef struct RadegsModelioColumn {
  float* dst;             /* the destination tensor's first element */
  long long dst_stride;   /* floats between two of its rows */
  int dst_elem;           /* float within the row */
  int src_offset;         /* byte within the record */
  int src_type;           /* RADEGS_MODELIO_* */
  int scale;              /* 0: the value; 1: the value / 255 */
} RadegsModelioColumn;
int radegs_modelio_pack(long long P, long long row_begin, long long row_end, int K, const float* xyz, const float* f_dc, const float* f_rest,
                        const float* opacity, const float* scaling, const float* rotation, const float* filter_3D, float* out, void* stream);
int radegs_modelio_unpack(long long P, int S, const void* records, int D, const RadegsModelioColumn* columns, void* stream);
int radegs_modelio_reset_opacity(long long P, const float* opacity_raw, const float* scaling_raw, const float* filter_3D, float* opacity_out /* [P] */,
                                 float* zero_a, float* zero_b, void* stream);
int radegs_modelio_init(long long P, int K, const float* colors /* [P,3] */, const float* dist2 /* [P] */, float opacity_value, float* f_dc, float* f_rest,
                        float* opacity, float* scaling, float* rotation, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Scene ingestion: a decoded 8-bit photograph on its way to a training camera, which upstream does
 * per image on one host thread: PIL.Image.resize + / 255 + permute (utils/general_utils.py PILtoTorch, called from
 * utils/camera_utils.py loadCam), the Blender RGBA composite (scene/dataset_readers.py:270-276) and the edge map
 * (scene/cameras.py:59-68).  Conventions as above: device pointers unless marked (host), 0 or a negative
 * RADEGS_ERR_*, work enqueued on `stream`, nothing read back, arguments refused before the first HIP call.  One pass
 * per kernel, no atomics: two calls return the same bits.
 *
 * radegs_sceneio_resize: src uint8 [H, W, C] interleaved, C in {1, 3, 4}, 4-byte aligned; the result is Pillow's 8-bit
 *   `resize` with its default filter (bicubic, a = -0.5, antialiased) applied to every channel on its own.  The filter
 *   coefficients are the caller's: a RadegsSceneioTable (host structure, device arrays) per axis whose size changes,
 *   NULL for an axis that keeps its size.  Per output index i the table holds bounds[2 i] = first source index,
 *   bounds[2 i + 1] = n taps, and n coefficients in fixed point with RADEGS_SCENEIO_PRECISION_BITS fractional bits;
 *   a pass computes clip8((2^21 + sum pixel * k) >> 22) in int32 (the builder of the table asserts 255 sum|k| + 2^21
 *   < 2^31).  The horizontal pass runs first, over source rows [row_first, row_first + rows_mid) only, into mid
 *   [rows_mid, Wout, C]; with a vertical table these must be the rows it reads (first, last), without one all H rows.
 *   The horizontal table's kk is transposed, [ksize, out_size]; the vertical one's is [out_size, ksize]; max_span
 *   (horizontal only) is the largest number of source pixels that 64 consecutive outputs starting at a multiple of 64
 *   read, and must make 4 rows of that many pixels fit into 64 KB.  The resulting byte goes to out_u8 [Hout, Wout, C]
 *   (may be NULL) and, where image is not NULL, through lut [256] (float32: i / 255) to planar float32: channels 0..2
 *   to image [min(C, 3), Hout, Wout], channel 3 to mask [1, Hout, Wout].  Every value of lut lies in [0, 1]: upstream's
 *   clamp(0, 1) is the identity and is not run.
 * radegs_sceneio_composite: rgba uint8 [N, 4] (16-byte aligned) over a white or black background to rgb uint8 [N, 3]
 *   (4-byte aligned), in float64, one rounding per operation: a = A / 255.0, v = (c / 255.0) a + bg (1 - a), byte =
 *   trunc(v 255.0) & 0xFF.
 * radegs_sceneio_edge: image float32 [C, H, W], C in {1, 3}; edge [H, W] = exp(-max over the four neighbours of the
 *   mean over channels of |centre - neighbour|) in the interior, computed in float64 and rounded once, 0 on the
 *   one-pixel border.
 * --------------------------------------------------------------------------------------------------------------- */
#define RADEGS_SCENEIO_PRECISION_BITS 22
typedef struct RadegsSceneioTable {
  const int* bounds;      /* device, [out_size, 2] */
  const int* kk;          /* device, [ksize, out_size] (horizontal) or [out_size, ksize] (vertical) */
  int in_size, out_size, ksize;
  int max_span;           /* horizontal only */
  int first, last;        /* the source indices the table reads: [first, last) */
} RadegsSceneioTable;
int radegs_sceneio_resize(int H, int W, int C, int Hout, int Wout, const unsigned char* src, const RadegsSceneioTable* horizontal /* host */,
                          const RadegsSceneioTable* vertical /* host */, int row_first, int rows_mid, unsigned char* mid, const float* lut,
                          unsigned char* out_u8, float* image, float* mask, void* stream);
int radegs_sceneio_composite(long long N, const unsigned char* rgba, int white_background, unsigned char* rgb, void* stream);
int radegs_sceneio_edge(int C, int H, int W, const float* image, float* edge /* [H,W] */, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Unbounded mesh extraction: GaussianExtractor.extract_mesh_unbounded, utils/mesh_utils.py:162-270
 * with utils/mcube_utils.py -- a TSDF over a contracted cube, sampled densely and meshed crop by crop.  Conventions
 * as for TSDF fusion above: device pointers unless marked (host), 0 or a negative RADEGS_ERR_*, work enqueued on
 * `stream`, nothing read back, sizes of 0 legal.  All device arithmetic is float32, one rounding per operation,
 * products before sums in the order written here; sqrt and / are correctly rounded.  NaN follows IEEE: every
 * comparison with NaN is false, so such a view is skipped.
 *
 * Contraction (of a sample y of the contracted cube to the world point x):
 *   mag = sqrt((y.x y.x + y.y y.y) + y.z y.z); x = y if mag < 1, else (1 / (2 - mag)) (y / mag) per component; then
 *   x = x radius + center per component.  mag >= 2 is legal (the reference's grid reaches |y| = 1.9 sqrt 3): the
 *   result is whatever this arithmetic gives, inf and NaN included.
 * Per-sample truncation (a quirk of the reference, preserved: the norm is taken of the WORLD point, after the
 *   un-normalisation, mesh_utils.py:198-202): n = sqrt((x.x x.x + x.y x.y) + x.z x.z); trunc = trunc5, and
 *   trunc = trunc5 (1 / (2 - min(n, 1.9))) if n > 1.  trunc5 = float32(5 voxel_size), rounded once on the host from
 *   float64.  Without contraction (the colouring pass) x is the input and trunc = trunc5.
 * Per view v = 0 .. V-1, in this order, m = the view's full_proj_transform [4][4] by rows (row-vector convention):
 *   q.c = ((x.x m[0][c] + x.y m[1][c]) + x.z m[2][c]) + m[3][c] for c = 0, 1, 3; z = q.w; px = q.x / z; py = q.y / z.
 *   In view iff -1 < px < 1, -1 < py < 1 and z > 0, all strict.  Bilinear sample, align_corners, border padding:
 *   ix = min(max(((px + 1) / 2) (W - 1), 0), W - 1), x0 = floor(ix), x1 = x0 + 1, likewise iy, y0, y1 with H;
 *   nw = (x1 - ix) (y1 - iy), ne = (ix - x0) (y1 - iy), sw = (x1 - ix) (iy - y0), se = (ix - x0) (iy - y0);
 *   value = (((0 + I[y0][x0] nw) + I[y0][x1] ne) + I[y1][x0] sw) + I[y1][x1] se, a tap with x1 = W or y1 = H
 *   contributing nothing (its term is left out, not multiplied by zero).  sdf = depth - z.  Integrate iff in view
 *   and sdf > -trunc: s = min(max(sdf / trunc, -1), 1); tsdf = (tsdf w + s) / (w + 1); rgb.c = (rgb.c w + colour.c)
 *   / (w + 1) per channel; w = w + 1.  Initially tsdf = 1, w = 1 (one, not zero: a sample seen by n views of constant
 *   colour c ends with c n / (n + 1)), rgb = 0.  V = 0: every tsdf is 1.
 * RadegsUnboundedView (a device array [V]): m, then W, H >= 1, depth [H][W], rgb [3][H][W] or null (such a view
 *   leaves rgb alone); the sizes may differ from view to view.  An entry with W < 1, H < 1 or no depth is skipped.
 * radegs_unbounded_fuse: explicit mode, samples [M,3]; lattice mode, samples null: the M = nx ny nz samples
 *   (ax[lx], ay[ly], az[lz]) at index (lx ny + ly) nz + lz, never materialised.  `mapping` (lattice mode only) picks
 *   how lanes map to samples, RADEGS_UNBOUNDED_ZRUN: a wave is 64 consecutive indices, _BRICK: a wave is a 4x4x4
 *   brick; the results are the same bits.  contract != 0: samples are contracted, as above; radius must be positive.
 *   center3 (host) [3].  tsdf [M]; rgb [M,3] or null.  One thread per sample, all views in one launch, one write.
 * radegs_unbounded_uncontract (after the weld): world [M,3] = the contraction above, then each component v clamped:
 *   -max_range if v < -max_range, max_range if v > max_range, else v (NaN stays).
 *
 * Dense marching cubes over a lattice of nx ny nz values (each >= 2, fewer than 2^31 points) with coordinates ax, ay,
 *   az: level 0; case bit i = corner i < 0 (csrc/rg_mc_tables.h, the table of TSDF fusion; NaN counts as positive);
 *   every cell is valid.  A lattice point owns the edges leaving it along +x, +y, +z; an owned edge carries a vertex
 *   iff its ends differ in sign: t = (0 - v_o) / (v_e - v_o), position c_o + t (c_e - c_o) along the edge's axis and
 *   the lattice's own coordinates along the other two -- taken from the sample coordinates themselves, so two crops
 *   that share a plane produce the same bits there.  Orientation as in TSDF fusion.  Vertices in (lattice index,
 *   axis) order with key ((gx G + gy) G + gz) 3 + axis, g = offset3 + l, 1 <= G <= 2^20, offset3 (host) >= 0,
 *   offset3 + n <= G; faces [F,3] in (lattice index of the cell's lowest corner, table) order, indices into this
 *   call's vertices.  counts2 (device) = {V, F}; workspace: radegs_densemc_bytes (0 for a refused lattice), 16-byte
 *   aligned, untouched between plan and emit.
 * Crops and weld (host side, rade-gs_amd/unbounded_mesh.py): the lattice of crop (i, j, k) is
 *   float32(linspace(xs[i], xs[i+1], crop)) per axis, xs = linspace(-R, R, N + 1) in float64, N = resolution / crop;
 *   adjacent crops share their boundary plane: g = i (crop - 1) + l, G = N (crop - 1) + 1.  The final vertices are
 *   ascending by key, duplicates removed; faces crop-major (i, then j, then k), then as emitted, re-indexed.  Then
 *   radegs_unbounded_uncontract with max_range, then the colouring pass (no contraction, rgb) over the vertices.
 *
 * Deviations from upstream, restated from memory of skimage and trimesh (neither can be read where this was
 * written): skimage's Lewiner tables are replaced by the table above; trimesh's merge_vertices(digits_vertex=6) by
 * the exact key weld; the vertex position is the interpolation of the sample coordinates above, not skimage's
 * origin + index spacing; the crop is a parameter (upstream: 512).
 * --------------------------------------------------------------------------------------------------------------- */
#define RADEGS_UNBOUNDED_ZRUN 0
#define RADEGS_UNBOUNDED_BRICK 1
typedef struct RadegsUnboundedView {
  float m[16];
  int W, H;
  const float* depth;
  const float* rgb;
} RadegsUnboundedView;
int radegs_unbounded_fuse(long long M, const float* samples /* [M,3] or null */, const float* ax, const float* ay, const float* az, int nx, int ny, int nz,
                          int mapping, int V, const RadegsUnboundedView* views /* [V] */, int contract, float radius, const float* center3 /* host */,
                          float trunc5, float* tsdf /* [M] */, float* rgb /* [M,3] or null */, void* stream);
int radegs_unbounded_uncontract(long long M, const float* contracted /* [M,3] */, float radius, const float* center3 /* host */, float max_range,
                                float* world /* [M,3] */, void* stream);
size_t radegs_densemc_bytes(int nx, int ny, int nz);
int radegs_densemc_plan(const float* values /* [nx,ny,nz] */, int nx, int ny, int nz, void* workspace, size_t workspace_bytes, long long* counts2,
                        void* stream);
int radegs_densemc_emit(const float* values, const float* ax, const float* ay, const float* az, int nx, int ny, int nz, const int* offset3 /* host */,
                        long long G, const void* workspace, long long V, long long F, float* vertices /* [V,3] */, long long* keys /* [V] */,
                        long long* faces /* [F,3] */, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Evaluation from files: the step from the files of a geometry evaluation to the tensors of the
 * units above -- what upstream hands to o3d.io.read_point_cloud, trimesh.load and
 * o3d.pipelines.registration.registration_ransac_based_on_correspondence (eval_tnt/registration.py:66-110).
 * Conventions as above: device pointers unless marked (host), 0 or a negative RADEGS_ERR_*, work enqueued on
 * `stream`, nothing read back, arguments refused before the first HIP call, sizes of 0 legal.  fp64, one rounding per
 * operation in the order written here, products before sums, IEEE divide and sqrt.
 *
 * Records: `buffer` (4-byte aligned, readable up to the next multiple of 4 past the last record) holds, from byte
 *   byte_offset (any alignment), little-endian records of S bytes, 1 <= S <= RADEGS_MODELIO_MAX_RECORD.  Types are
 *   RADEGS_MODELIO_*.
 * radegs_evalio_unpack_points: out [N,3] double; column k is the value of type types3[k] at byte offsets3[k] of the
 *   record (both host, refused when the value leaves the record).  Integers and F4 are widened exactly, F8 is copied
 *   bit for bit.
 * radegs_evalio_unpack_faces: a record holds a list length of count_type (I1 .. U4) at count_offset and three indices
 *   of index_type (I4 or U4) from index_offset; whatever else it holds is skipped.  faces [F,3] gets the indices as
 *   read; *bad (device, zeroed by the call) counts the records whose length is not 3 or that hold an index outside
 *   [0, V).  A caller that finds *bad != 0 must not use faces: the records did not have the fixed stride assumed.
 *
 * radegs_evalio_ransac: source, target [N,3], pair i = (source[i], target[i]), N < 2^31; hypotheses h = 0 .. K-1.
 *   Generator: u(seed, h, k) = the high 32 bits of mix(seed 0x9E3779B97F4A7C15 + h 0xD1B54A32D192ED03 +
 *   k 0x8CB92BA72F3D8DD7 + 0x2545F4914F6CDD1D) in 64-bit wrapping arithmetic, mix(z): z ^= z >> 30;
 *   z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.  Draw k = 0 .. ransac_n - 1 of
 *   hypothesis h takes the r-th index of [0, N) not taken by an earlier draw, r = (u(seed, h, k) (N - k)) >> 32: the
 *   sample is a function of (seed, h) alone.
 *   Similarity of a sample (Eigen's umeyama with scaling, what tnt_eval.umeyama computes from radegs_tnteval_pair_sums'
 *   numbers): sums of s and t in draw order, means ms, mt = sum / n; Sigma = (sum (t - mt)(s - ms)^T) / n and var =
 *   (sum (ds0 ds0 + ds1 ds1) + ds2 ds2) / n in draw order; Sigma = U D V^T by RADEGS_EVALIO_RANSAC_SWEEPS sweeps of
 *   one-sided Jacobi rotations over the column pairs (0,1), (0,2), (1,2), singular values descending; S = diag(1, 1,
 *   sign(det U det V)); c = ((D0 + D1) + S2 D2) / var; R = U S V^T; T = [c R | mt - (c R) ms].  The rotation agrees with
 *   any other SVD to rounding only while D1 / D0 is well away from 0.  var = 0 (a sample without extent) or a T that
 *   is not finite: the hypothesis counts 0 inliers.
 *   Evaluation: for i ascending, p = T (s_i, 1) with rows ((m0 x + m1 y) + m2 z) + m3, d2 = (dx dx + dy dy) + dz dz of
 *   p - t_i; where sqrt(d2) < max_dist: counts[h] += 1, sumsq[h] += d2.
 *   Choice: the largest count; among those the smallest sqrt(sumsq / count); among those the smallest h.  Keys are
 *   compared, nothing is accumulated atomically: two calls give the same bits whatever the launch geometry.
 *   out15 = rows 0-2 of T of the chosen hypothesis, its count, its sumsq, h; with every count 0: the identity, 0, 0, -1.
 *   The kernel stages the pairs through LDS RADEGS_EVALIO_RANSAC_CHUNK at a time.
 * --------------------------------------------------------------------------------------------------------------- */
#define RADEGS_EVALIO_RANSAC_CHUNK 256    /* pairs per LDS stage: 12 KB */
#define RADEGS_EVALIO_RANSAC_SWEEPS 8
#define RADEGS_EVALIO_RANSAC_MIN_N 3
#define RADEGS_EVALIO_RANSAC_MAX_N 8
int radegs_evalio_unpack_points(long long N, int S, const void* buffer, long long byte_offset, const int* offsets3 /* host */, const int* types3 /* host */,
                                double* out /* [N,3] */, void* stream);
int radegs_evalio_unpack_faces(long long F, int S, const void* buffer, long long byte_offset, int count_offset, int count_type, int index_offset,
                               int index_type, long long V, long long* faces /* [F,3] */, unsigned int* bad, void* stream);
int radegs_evalio_ransac(long long N, const double* source, const double* target, double max_dist, int ransac_n, long long K, unsigned long long seed,
                         int* counts /* [K] */, double* sumsq /* [K] */, double* out15, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Camera pose refinement (csrc/radegs_pose.hip; the arithmetic is csrc/rg_pose.h, statement for statement, restated in
 * NumPy by tests/pose_restatement.py).  Conventions as above: device pointers, 0 or a negative RADEGS_ERR_*, work
 * enqueued on `stream`, nothing read back, arguments refused before the first HIP call.  fp64, one rounding per
 * operation in the order rg_pose.h writes, IEEE divide and sqrt.
 *
 * radegs_pose_gradient: the gradient of the loss with respect to the camera pose, from the gradients radegs_backward
 *   returned for means3D [P,3], rotations [P,4] (w, x, y, z) and shs [P,M,3] of the same view (campos [3] and
 *   viewmatrix [16] are that view's).  out12 = g_xi[6] then g_tau[6], each (translation, rotation):
 *     xi, world frame:   w2c(xi) = w2c [[Exp(theta), rho], [0, 1]]
 *     tau, camera frame: Exp(tau) w2c = w2c Exp(xi)
 *   g_xi = the sum over the Gaussians of rg_pose.h's row in the order of rg_reduce.h's two-stage sum: a function of P
 *   alone, so two calls give the same bits.  The SH row of a Gaussian is read only where sh_degree > 0 and the three
 *   DC entries of its dL_dsh row are not all zero.  0 <= sh_degree <= 3, (sh_degree + 1)^2 <= M <= 16.  P = 0 gives
 *   zeros.  workspace: radegs_pose_gradient_bytes(P) bytes, 8-byte aligned, contents irrelevant before and after.
 *   The gradient is linear in what the backward returned: with opacity_grad_intended = 0 it inherits the reference's
 *   argument slip (kernel_size > 0 makes that visible).
 *
 * radegs_pose_step: one Adam step on one camera's tau and the retraction master <- Exp(tau) master.
 *   master [4,4] double, the world-to-camera matrix, row-major and NOT transposed; grad6 = g_tau (double, device);
 *   exp_avg, exp_avg_sq [6] float; step >= 1 counts this camera's steps, this one included; bias corrections on the
 *   host in double as radegs_adam_step forms them, lr_translation for tau[0..2], lr_rotation for tau[3..5]; the
 *   update in fp32 as radegs_adam_step's, from a parameter of 0.  Exp: Rodrigues, series coefficients below
 *   |theta| = 1e-8, then one Newton step towards the nearest rotation (rg_pose.h::retract).  proj [16] float is the
 *   camera's projection matrix, stored transposed.  Written in place with vector stores: world_view_transform [16]
 *   (master transposed, rounded), full_proj_transform [16] (view proj in double, rounded once), camera_center [3].
 * --------------------------------------------------------------------------------------------------------------- */
size_t radegs_pose_gradient_bytes(long long P);
int radegs_pose_gradient(long long P, int M, int sh_degree, const float* means3D, const float* rotations, const float* shs, const float* campos,
                         const float* viewmatrix, const float* dL_dmeans3D, const float* dL_drotations, const float* dL_dsh, void* workspace,
                         size_t workspace_bytes, double* out12, void* stream);
int radegs_pose_step(double* master, const double* grad6, float* exp_avg, float* exp_avg_sq, double step, double lr_translation,
                     double lr_rotation, double beta1, double beta2, double eps, const float* proj, float* world_view_transform,
                     float* full_proj_transform, float* camera_center, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Mesh simplification: vertex clustering with quadric error (Lindstrom 2000), the step upstream's
 * users take in Open3D (simplify_vertex_clustering) or MeshLab after post_process_mesh.  Conventions as above: device
 * pointers, 0 or a negative RADEGS_ERR_*, work enqueued on `stream`, nothing read back, arguments refused before the
 * first HIP call.  faces int64 [F,3], vertices float64 [V,3], finite; V < 2^31 and F <= 2^30, beyond that
 * RADEGS_ERR_TOO_LARGE.  Workspaces are 16-byte aligned.  fp64, one rounding per operation in the order written, IEEE
 * divide and sqrt, no float atomics: two calls give the same bits.  A face with an index outside [0, V) is never used
 * to address memory: it adds to no quadric and is flagged for removal.
 *
 * 1. Cells (radegs_simplify_cells).  o = (ox, oy, oz) and h > 0 finite.  c_a = floor((v_a - o_a) / h) per axis; the
 *   caller has made sure 0 <= c_a < 2^RADEGS_SIMPLIFY_CELL_BITS (a value outside is clamped to that range, never
 *   used as it is).  key = cx << 42 | cy << 21 | cz <= max_key, which only sets how many bits are sorted.  The cells
 *   that hold a vertex are numbered 0..K-1 by ascending key (not Open3D's hash-map order).  Outputs: vertex_cell [V];
 *   order [V], the vertices by ascending (key, index); cell_start [V + 1], of which K + 1 entries are written: cell k
 *   is order[cell_start[k] .. cell_start[k + 1]); cell_key [V], K written; *n_cells = K, which the host reads.
 * 2. Averages (radegs_simplify_vertices).  averages [K,3] and attributes_out [K,A]: per cell and component the sum
 *   over its members in ascending vertex index, added to 0.0 one by one, divided by their number.
 * 3. Quadrics (quadric = 1).  Triangle (a, b, c): u = b - a, v = c - a, n = (uy vz - uz vy, uz vx - ux vz,
 *   ux vy - uy vx), len = sqrt((nx nx + ny ny) + nz nz); unless len is positive and finite the triangle contributes
 *   nothing.  w = 0.5 len, n^ = n / len, d = -((n^x ax + n^y ay) + n^z az), wn = w n^ (three products), wd = w d.
 *   Its ten entries, in the order of quadrics [K,10]:
 *     xx = wnx n^x, xy = wnx n^y, xz = wnx n^z, xd = wnx d, yy = wny n^y, yz = wny n^z, yd = wny d, zz = wnz n^z,
 *     zd = wnz d, dd = wd d.
 *   One record per corner: the entries are added to the cell of each of the three corners (twice where two corners
 *   share a cell).
 * 4. Order of the sums: per cell and entry the records in ascending (triangle, corner), added to 0.0 one by one -- a
 *   function of the cell's records alone.  (The kernel gives a cell one wave: 64 records' entries are computed side
 *   by side and then added in this order.)
 *   The solve, per cell: A = [[xx xy xz][xy yy yz][xz yz zz]], b = (xd, yd, zd), m = the average,
 *   g_a = ((A_a0 m_0 + A_a1 m_1) + A_a2 m_2) + b_a.  Cyclic Jacobi on A with R = I: at most
 *   RADEGS_SIMPLIFY_JACOBI_SWEEPS sweeps, none once a01, a02 and a12 are all exactly 0; a sweep visits the pairs
 *   (p, q) = (0,1), (0,2), (1,2), r the third index, and leaves a pair with a_pq == 0 alone; otherwise
 *     theta = (a_qq - a_pp) / (2 a_pq);  t = (theta < 0 ? -1 : 1) / (|theta| + sqrt(theta theta + 1));
 *     c = 1 / sqrt(t t + 1);  s = t c;  a_pp -= t a_pq (one product, then the difference);  a_qq += that product;
 *     a_pq = 0;  (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq);  for k = 0, 1, 2:
 *     (R_kp, R_kq) = (c R_kp - s R_kq, s R_kp + c R_kq).
 *   lambda_i = a_ii afterwards, r_i = column i of R, lambda_max = the largest (compared with >, starting from
 *   lambda_0).  x = m; for i = 0, 1, 2 with lambda_i > 1e-3 lambda_max (Lindstrom's cut):
 *     coef = ((R_0i g_0 + R_1i g_1) + R_2i g_2) / lambda_i;  x_a = x_a - coef R_ai.
 *   x = m instead unless lambda_max is positive and finite, x is finite and, on every axis,
 *   o_a + c_a h <= x_a <= o_a + (c_a + 1) h (a product, then a sum; c_a from the cell's key).  positions [K,3] = x.
 * 5. Faces (radegs_simplify_faces).  cell_faces [F,3] = the corners' cell numbers, rotated so that the smallest comes
 *   first (the orientation stays); remove [F] = 1 where two corners share a cell (the row is then 0 0 0).
 *   remove_duplicates: of the faces with the same rotated triple only the one of lowest index stays (opposite
 *   orientations are different triples); the triples are sorted LSD: the third number, then stable by (second, first).
 * 6. Compaction is radegs_meshclean_compact_plan / _apply on (K, cell_faces, remove): output faces keep the ascending
 *   order of their input face.  radegs_simplify_face_source reads that plan's workspace (of
 *   radegs_meshclean_compact_bytes(K, F)) after the plan: face_source [nf_out] = the input face of every output face.
 * --------------------------------------------------------------------------------------------------------------- */
#define RADEGS_SIMPLIFY_CELL_BITS 21
#define RADEGS_SIMPLIFY_JACOBI_SWEEPS 8
size_t radegs_simplify_cells_bytes(long long V);
int radegs_simplify_cells(long long V, const double* vertices, double ox, double oy, double oz, double h, long long max_key, void* workspace,
                          size_t workspace_bytes, long long* vertex_cell /* [V] */, int* order /* [V] */, int* cell_start /* [V + 1] */,
                          long long* cell_key /* [V] */, long long* n_cells /* [1] */, void* stream);
size_t radegs_simplify_vertices_bytes(long long F);
int radegs_simplify_vertices(long long V, long long F, long long K, int A, const double* vertices, const long long* faces,
                             const double* attributes /* [V,A] */, const long long* vertex_cell, const int* order, const int* cell_start,
                             const long long* cell_key, double ox, double oy, double oz, double h, int quadric, void* workspace,
                             size_t workspace_bytes, double* averages /* [K,3] */, double* attributes_out /* [K,A] */, double* quadrics /* [K,10] */,
                             double* positions /* [K,3] */, void* stream);
size_t radegs_simplify_faces_bytes(long long F);
int radegs_simplify_faces(long long V, long long F, long long K, const long long* faces, const long long* vertex_cell, int remove_duplicates,
                          void* workspace, size_t workspace_bytes, long long* cell_faces /* [F,3] */, unsigned char* remove /* [F] */, void* stream);
int radegs_simplify_face_source(long long K, long long F, const void* compact_workspace, long long nf_out, long long* face_source /* [nf_out] */,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RADEGS_H_INCLUDED */
