"""`_C` -- binding of libradegs_hip.so (C ABI: include/radegs.h) with the call surface of the
reference's pybind module (DGR/ext.cpp:15-19):

    rasterize_gaussians(...)            DGR/rasterize_points.h:18-42  / rasterize_points.cu:36-133
    rasterize_gaussians_backward(...)   DGR/rasterize_points.h:43-76  / rasterize_points.cu:136-246
    mark_visible(...)                   DGR/rasterize_points.h:78-81  / rasterize_points.cu:248-267
    integrate_gaussians_to_points(...)  DGR/rasterize_points.h:83-110 / rasterize_points.cu:269-388

Same positional arguments, same return tuples (note the forward's output order differs from the
Python operator's 8-tuple, exactly as upstream).  torch is used for device memory and the current
HIP stream only; no torch type crosses the C boundary.

There is NO CPU path and no fallback: a missing library or a non-GPU tensor raises.
"""
import contextlib
import ctypes
import os
import threading
import weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("RADEGS_LIB") or os.path.join(_HERE, "libradegs_hip.so")   # RADEGS_LIB: A/B runs of two builds

_ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
_F = ctypes.POINTER(ctypes.c_float)


class RadegsFwdArgs(ctypes.Structure):
    _fields_ = [("P", ctypes.c_int), ("D", ctypes.c_int), ("M", ctypes.c_int), ("width", ctypes.c_int), ("height", ctypes.c_int),
                ("background", ctypes.c_void_p), ("means3D", ctypes.c_void_p), ("shs", ctypes.c_void_p),
                ("colors_precomp", ctypes.c_void_p), ("opacities", ctypes.c_void_p), ("scales", ctypes.c_void_p),
                ("rotations", ctypes.c_void_p), ("cov3D_precomp", ctypes.c_void_p), ("viewmatrix", ctypes.c_void_p),
                ("projmatrix", ctypes.c_void_p), ("cam_pos", ctypes.c_void_p),
                ("scale_modifier", ctypes.c_float), ("tan_fovx", ctypes.c_float), ("tan_fovy", ctypes.c_float),
                ("kernel_size", ctypes.c_float),
                ("prefiltered", ctypes.c_int), ("require_coord", ctypes.c_int), ("require_depth", ctypes.c_int), ("debug", ctypes.c_int),
                ("out_color", ctypes.c_void_p), ("out_coord", ctypes.c_void_p), ("out_mcoord", ctypes.c_void_p),
                ("out_depth", ctypes.c_void_p), ("out_mdepth", ctypes.c_void_p), ("out_alpha", ctypes.c_void_p),
                ("out_normal", ctypes.c_void_p), ("radii", ctypes.c_void_p)]


class RadegsBwdArgs(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("P", ctypes.c_int), ("D", ctypes.c_int), ("M", ctypes.c_int), ("R", ctypes.c_int), ("width", ctypes.c_int),
                ("height", ctypes.c_int),
                ("background", ctypes.c_void_p), ("means3D", ctypes.c_void_p), ("shs", ctypes.c_void_p),
                ("colors_precomp", ctypes.c_void_p), ("alphas", ctypes.c_void_p), ("scales", ctypes.c_void_p),
                ("rotations", ctypes.c_void_p), ("cov3D_precomp", ctypes.c_void_p), ("viewmatrix", ctypes.c_void_p),
                ("projmatrix", ctypes.c_void_p), ("cam_pos", ctypes.c_void_p),
                ("scale_modifier", ctypes.c_float), ("tan_fovx", ctypes.c_float), ("tan_fovy", ctypes.c_float),
                ("kernel_size", ctypes.c_float),
                ("radii", ctypes.c_void_p), ("normalmap", ctypes.c_void_p), ("geom_buffer", ctypes.c_void_p),
                ("binning_buffer", ctypes.c_void_p), ("image_buffer", ctypes.c_void_p),
                ("dL_dpix", ctypes.c_void_p), ("dL_dpix_coord", ctypes.c_void_p), ("dL_dpix_mcoord", ctypes.c_void_p),
                ("dL_dpix_depth", ctypes.c_void_p), ("dL_dpix_mdepth", ctypes.c_void_p), ("dL_dalphas", ctypes.c_void_p),
                ("dL_dpix_normal", ctypes.c_void_p),
                ("dL_dmean2D", ctypes.c_void_p), ("dL_dcolor", ctypes.c_void_p), ("dL_dopacity", ctypes.c_void_p),
                ("dL_dmean3D", ctypes.c_void_p), ("dL_dcov3D", ctypes.c_void_p), ("dL_dsh", ctypes.c_void_p),
                ("dL_dscale", ctypes.c_void_p), ("dL_drot", ctypes.c_void_p),
                ("require_coord", ctypes.c_int), ("require_depth", ctypes.c_int), ("debug", ctypes.c_int),
                ("dL_drgb_clamped", ctypes.c_void_p), ("opacity_grad_intended", ctypes.c_int),
                ("drgb_ready", ctypes.c_void_p), ("drgb_ready_user", ctypes.c_void_p),
                ("grad_chunks", ctypes.c_int), ("grads_ready", ctypes.c_void_p), ("grads_ready_user", ctypes.c_void_p),
                ("keep_sums", ctypes.c_int), ("acc_reuse", ctypes.c_int)]


class RadegsIntegrateArgs(ctypes.Structure):
    _fields_ = [("P", ctypes.c_int), ("D", ctypes.c_int), ("M", ctypes.c_int), ("PN", ctypes.c_int), ("width", ctypes.c_int),
                ("height", ctypes.c_int),
                ("background", ctypes.c_void_p), ("means3D", ctypes.c_void_p), ("shs", ctypes.c_void_p),
                ("colors_precomp", ctypes.c_void_p), ("opacities", ctypes.c_void_p), ("scales", ctypes.c_void_p),
                ("rotations", ctypes.c_void_p), ("cov3D_precomp", ctypes.c_void_p), ("viewmatrix", ctypes.c_void_p),
                ("projmatrix", ctypes.c_void_p), ("cam_pos", ctypes.c_void_p), ("points3D", ctypes.c_void_p),
                ("scale_modifier", ctypes.c_float), ("tan_fovx", ctypes.c_float), ("tan_fovy", ctypes.c_float),
                ("kernel_size", ctypes.c_float), ("debug", ctypes.c_int),
                ("out_color", ctypes.c_void_p), ("out_alpha_integrated", ctypes.c_void_p), ("out_color_integrated", ctypes.c_void_p),
                ("out_coordinate2d", ctypes.c_void_p), ("out_sdf", ctypes.c_void_p), ("radii", ctypes.c_void_p)]


for _s in (RadegsFwdArgs, RadegsBwdArgs, RadegsIntegrateArgs):
    _s._names = frozenset(name for name, _ in _s._fields_)

# every symbol include/radegs.h declares
EXPORTED_SYMBOLS = ("radegs_forward", "radegs_backward", "radegs_backward_ordered", "radegs_backward_ordered_scratch_bytes", "radegs_backward_from_sums", "radegs_mark_visible", "radegs_integrate", "radegs_sh_grad_from_views", "radegs_geometry_bytes", "radegs_image_bytes",
                    "radegs_binning_bytes", "radegs_debug_export", "radegs_point_bytes", "radegs_debug_export_points", "radegs_forget_image", "radegs_last_error", "radegs_version", "radegs_profile_enable",
                    "radegs_profile_select", "radegs_profile_stride", "radegs_binning_stats", "radegs_reload_env", "radegs_last_forward_used_streams", "radegs_profile_num_stages", "radegs_profile_stage_name", "radegs_profile_collect",
                    # fused pre/post steps (bound in graphics_utils.py / gaussian_model_ops.py)
                    "radegs_normals_forward", "radegs_normals_backward", "radegs_normal_loss_scratch_bytes",
                    "radegs_normal_loss_forward", "radegs_normal_loss_backward", "radegs_normals_last_error",
                    "radegs_filter3d_forward", "radegs_filter3d_backward", "radegs_compute_filter3d",
                    "radegs_model_activate_forward", "radegs_model_activate_backward",
                    "radegs_photometric_scratch_bytes",
                    "radegs_photometric_forward", "radegs_photometric_backward", "radegs_adam_step", "radegs_knn_scratch_bytes",
                    "radegs_knn_mean_dist2", "radegs_densify_stats", "radegs_densify_stats_reduced", "radegs_densify_plan_bytes",
                    "radegs_densify_plan", "radegs_densify_apply",
                    # decoupled appearance loss (bound in loss_utils.py)
                    "radegs_appearance_downsample_forward", "radegs_appearance_downsample_backward", "radegs_appearance_head_scratch_bytes",
                    "radegs_appearance_head_forward", "radegs_appearance_head_backward",
                    # mesh extraction (bound in tetmesh.py)
                    "radegs_tetmesh_plan_bytes", "radegs_tetmesh_plan", "radegs_tetmesh_emit", "radegs_tetra_points",
                    "radegs_cull_alpha_accumulate", "radegs_cull_alpha_finish", "radegs_tetmesh_bisect", "radegs_tetmesh_filter_plan_bytes",
                    "radegs_tetmesh_filter_plan", "radegs_tetmesh_filter_apply",
                    # mesh evaluation (bound in mesh_eval.py)
                    "radegs_mesheval_sample_bytes", "radegs_mesheval_sample_count", "radegs_mesheval_sample_emit", "radegs_mesheval_grid_bytes",
                    "radegs_mesheval_grid_build", "radegs_mesheval_thin_rounds", "radegs_mesheval_nearest", "radegs_mesheval_sum_bytes",
                    "radegs_mesheval_sum_below", "radegs_mesheval_obs_mask", "radegs_mesheval_above_plane", "radegs_mesheval_dilate",
                    "radegs_mesheval_cull_vertices", "radegs_tetmesh_filter_plan_flags",
                    # TSDF fusion (bound in tsdf.py)
                    "radegs_tsdf_unique_bytes", "radegs_tsdf_touch", "radegs_tsdf_unique_plan", "radegs_tsdf_unique_emit", "radegs_tsdf_insert_apply",
                    "radegs_tsdf_integrate", "radegs_tsdf_extract_bytes", "radegs_tsdf_extract_plan", "radegs_tsdf_extract_emit",
                    # Tanks-and-Temples evaluation (bound in tnt_eval.py)
                    "radegs_tnteval_centroids", "radegs_tnteval_transform", "radegs_tnteval_crop", "radegs_tnteval_voxel_bytes",
                    "radegs_tnteval_voxel_plan", "radegs_tnteval_voxel_emit", "radegs_tnteval_sums_bytes", "radegs_tnteval_pair_sums",
                    "radegs_tnteval_histogram",
                    # Tanks-and-Temples mesh culling (bound in tnt_cull.py)
                    "radegs_tntcull_render_bytes", "radegs_tntcull_render_begin", "radegs_tntcull_render_finish", "radegs_tntcull_count_views",
                    # mesh clean-up (bound in mesh_clean.py)
                    "radegs_meshclean_cluster_bytes", "radegs_meshclean_cluster", "radegs_meshclean_stats_bytes", "radegs_meshclean_stats",
                    "radegs_meshclean_compact_bytes", "radegs_meshclean_compact_plan", "radegs_meshclean_compact_apply",
                    "radegs_meshclean_normals_bytes", "radegs_meshclean_vertex_normals",
                    # Delaunay tetrahedralisation (bound in delaunay.py)
                    "radegs_delaunay_bytes", "radegs_delaunay_perturb", "radegs_delaunay_plan", "radegs_delaunay_emit",
                    # image evaluation (bound in image_eval.py)
                    "radegs_imageeval_conv3x3", "radegs_imageeval_conv3x3_first", "radegs_imageeval_tap_bytes", "radegs_imageeval_tap",
                    "radegs_imageeval_quantize", "radegs_imageeval_ssd_bytes", "radegs_imageeval_ssd",
                    # model state (bound in model_io.py)
                    "radegs_modelio_pack", "radegs_modelio_unpack", "radegs_modelio_reset_opacity", "radegs_modelio_init",
                    # scene ingestion (bound in scene_io.py)
                    "radegs_sceneio_resize", "radegs_sceneio_composite", "radegs_sceneio_edge",
                    # unbounded mesh extraction (bound in unbounded_mesh.py)
                    "radegs_unbounded_fuse", "radegs_unbounded_uncontract", "radegs_densemc_bytes", "radegs_densemc_plan", "radegs_densemc_emit",
                    # evaluation from files (bound in eval_io.py)
                    "radegs_evalio_unpack_points", "radegs_evalio_unpack_faces", "radegs_evalio_ransac",
                    # camera pose refinement (prototypes below, called from pose_opt.py)
                    "radegs_pose_gradient_bytes", "radegs_pose_gradient", "radegs_pose_step",
                    # mesh simplification (bound in mesh_simplify.py)
                    "radegs_simplify_cells_bytes", "radegs_simplify_cells", "radegs_simplify_vertices_bytes", "radegs_simplify_vertices",
                    "radegs_simplify_faces_bytes", "radegs_simplify_faces", "radegs_simplify_face_source")

_lib = None
# test hook: when True, the per-Gaussian accumulation scratch of the last backward is kept in LAST_ACC
KEEP_ACC = False
# False (default): the backward the reference executes, including its argument slip in the opacity-compensation gradient
# (include/radegs.h::RadegsBwdArgs.opacity_grad_intended).  True (or RADEGS_OPACITY_GRAD=intended in the environment): the derivative
# the reference's formulas intend.  Differs only for kernel_size > 0.
OPACITY_GRAD_INTENDED = os.environ.get("RADEGS_OPACITY_GRAD", "").lower() == "intended"
LAST_ACC = None
LAST_POINT_STATE = None
# RADEGS_DETERMINISTIC=1 (read here and again by reload_env(), like the library's own RADEGS_* switches) or set_deterministic_backward(True):
# rasterize_gaussians_backward calls radegs_backward_ordered -- per-Gaussian sums in a fixed order, bit-identical gradients run to run
# (include/radegs.h).  torch.use_deterministic_algorithms is NOT consulted: following it would change what existing callers get.
DETERMINISTIC = os.environ.get("RADEGS_DETERMINISTIC", "0") == "1"
# with KEEP_ACC, after an ordered backward: (partial records as a float32 view [R, 16 | 32], R) -- one record per position of point_list
LAST_PARTIALS = None
# Optional allocator for the 8 gradient tensors of the backward: callable(name, shape, dtype, device) -> tensor
# or None.  A data-parallel caller points it at slices of ONE flat bucket so that the gradient all-reduce needs no
# gather copy (rade-gs_amd/view_parallel.GradBucket).  Default: plain torch.empty.
# Installed PER DEVICE with set_grad_allocator(device, fn): autograd runs every device's backward on its own worker thread,
# so one process driving several GPUs must not share a single hook.  The module attribute GRAD_ALLOCATOR is the fallback for
# devices without their own entry (one process per GPU, the deployment this library is built for, needs nothing else).
GRAD_ALLOCATOR = None
_GRAD_ALLOCATORS = {}
_HOOK_LOCK = threading.Lock()


def set_grad_allocator(device, fn):
    """Install (fn) or remove (None) the gradient allocator of one device; see GRAD_ALLOCATOR."""
    idx = torch.device(device).index
    if idx is None:
        idx = torch.cuda.current_device()
    with _HOOK_LOCK:
        if fn is None:
            _GRAD_ALLOCATORS.pop(idx, None)
        else:
            _GRAD_ALLOCATORS[idx] = fn


def set_deterministic_backward(flag):
    """Switch the fixed-order backward on or off for this process (see DETERMINISTIC); returns the previous value.  reload_env() sets it
    from the environment again."""
    global DETERMINISTIC
    prev = DETERMINISTIC
    DETERMINISTIC = bool(flag)
    return prev


def _grad_allocator_for(dev):
    with _HOOK_LOCK:
        return _GRAD_ALLOCATORS.get(dev.index, GRAD_ALLOCATOR)


# The allocator may also (a) return a (P,3) tensor for the extra name "dL_drgb_clamped" -- the backward then fills it with
# dL/dRGB (clamp mask applied) -- and (b) return SKIP_GRAD for "dL_dsh": the (P,M,3) SH gradient is then not written and
# comes back as None (it is basis(dir) x dL_drgb_clamped; view_parallel.FactoredGradExchange rebuilds the batch sum).
SKIP_GRAD = object()
# (c) if the allocator OBJECT has a method `drgb_ready()` (the allocator is then a bound method of it), the backward calls it on the
# host as soon as the kernel that writes dL_drgb_clamped is queued -- before the per-Gaussian backward -- so that an all-gather of
# those rows can run under that kernel (include/radegs.h::RadegsBwdArgs.drgb_ready).
_READY_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p)
_GRADS_READY_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int, ctypes.c_int)


def _c_hook(fn_type, fn, errors):
    """The Python callable `fn` as a C hook of type `fn_type` (it is not handed the hook's leading user pointer; the other arguments arrive
    as ints).  An exception it raises must not unwind through the C frame: it is appended to `errors`, and the caller re-raises it once
    the native call has returned.  fn None: no hook."""
    if fn is None:
        return None

    def _call(_user, *args):
        try:
            fn(*(int(x) for x in args))
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)
    return fn_type(_call)


def _args(struct, **fields):
    """An argument structure from keyword fields (struct_size filled in where there is one; a field not named is 0 / NULL).  A tensor stands
    for its device pointer, None for NULL, a hook made by _c_hook for its C address.  The structure keeps the values alive."""
    unknown = fields.keys() - struct._names
    if unknown:
        raise TypeError(f"{struct.__name__} has no field {sorted(unknown)}")
    values = {name: v.data_ptr() if isinstance(v, torch.Tensor) else ctypes.cast(v, ctypes.c_void_p) if isinstance(v, ctypes._CFuncPtr) else v
              for name, v in fields.items()}
    if "struct_size" in struct._names:
        values["struct_size"] = ctypes.sizeof(struct)
    a = struct(**values)
    a.keep = fields
    return a


_I, _SZ, _VP, _ULL = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)
# the rasterizer's own entry points: {name: (restype, [argtypes])}.  Every other module keeps such a table for the symbols it calls and hands
# it to bind(); together the tables cover EXPORTED_SYMBOLS (tests/test_signatures.py), so no function is ever called with ctypes' defaults
_SIGNATURES = {
    "radegs_forward": (_I, [ctypes.POINTER(RadegsFwdArgs)] + [_ALLOC_FN, _VP] * 3 + [_VP]),
    "radegs_backward": (_I, [ctypes.POINTER(RadegsBwdArgs), _ALLOC_FN, _VP, _VP]),
    "radegs_backward_ordered": (_I, [ctypes.POINTER(RadegsBwdArgs), _ALLOC_FN, _VP, _VP, _SZ, _VP]),
    "radegs_backward_ordered_scratch_bytes": (_SZ, [_I, _I, _I]),
    "radegs_backward_from_sums": (_I, [ctypes.POINTER(RadegsBwdArgs), _VP, _VP]),
    "radegs_integrate": (_I, [ctypes.POINTER(RadegsIntegrateArgs)] + [_ALLOC_FN, _VP] * 4 + [_VP]),
    "radegs_sh_grad_from_views": (_I, [_I] * 4 + [_VP] * 3 + [ctypes.c_float, _VP, _VP]),
    "radegs_mark_visible": (_I, [_I] + [_VP] * 5),
    "radegs_geometry_bytes": (_SZ, [_I, _I]),
    "radegs_image_bytes": (_SZ, [_I, _I]),
    "radegs_binning_bytes": (_SZ, [_I]),
    "radegs_debug_export": (ctypes.c_longlong, [ctypes.c_char_p] + [_I] * 5 + [_VP] * 4 + [_SZ, _VP]),
    "radegs_point_bytes": (_SZ, [_I] * 4),
    "radegs_debug_export_points": (ctypes.c_longlong, [ctypes.c_char_p] + [_I] * 4 + [_VP] * 2 + [_SZ, _VP]),
    "radegs_forget_image": (None, [_VP]),
    "radegs_last_error": (ctypes.c_char_p, []),
    "radegs_version": (ctypes.c_char_p, []),
    "radegs_binning_stats": (None, [_ULL, _ULL, _I]),
    "radegs_reload_env": (None, []),
    "radegs_last_forward_used_streams": (_I, []),
    "radegs_profile_enable": (None, [_I]),
    "radegs_profile_select": (None, [_I]),
    "radegs_profile_stride": (None, [_I]),
    "radegs_profile_num_stages": (_I, []),
    "radegs_profile_stage_name": (ctypes.c_char_p, [_I]),
    "radegs_profile_collect": (_I, [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(_I), _I]),
    "radegs_pose_gradient_bytes": (_SZ, [ctypes.c_longlong]),
    "radegs_pose_gradient": (_I, [ctypes.c_longlong, _I, _I] + [_VP] * 9 + [_SZ, _VP, _VP]),
    "radegs_pose_step": (_I, [_VP] * 4 + [ctypes.c_double] * 6 + [_VP] * 5),
}
_bound = set()   # id() of the tables (module-level dicts, never freed) already set on the library
_BIND_LOCK = threading.Lock()


def bind(signatures):
    """Loads libradegs_hip.so (built in-tree by rade-gs_amd/build.py; fails loudly) on first use, sets the module's table
    {"radegs_x": (restype, [argtypes...]), ...} on it, once, and returns the library."""
    global _lib
    if id(signatures) not in _bound:
        with _BIND_LOCK:
            if _lib is None:
                if not os.path.exists(_LIB_PATH):
                    raise RuntimeError(f"{_LIB_PATH} is missing: build it with `python rade-gs_amd/build.py` "
                                       "(there is no CPU or PyTorch fallback for this operator)")
                _lib = ctypes.CDLL(_LIB_PATH)
            for name, (restype, argtypes) in signatures.items():
                fn = getattr(_lib, name)
                fn.restype, fn.argtypes = restype, argtypes
            _bound.add(id(signatures))
    return _lib


def library():
    """libradegs_hip.so with the rasterizer's entry points bound."""
    return bind(_SIGNATURES)


def _check(rc, what):
    if rc < 0:
        # whatever failed, the cached scratches are no longer known to be zero (RADEGS_ERR_STATE in particular is reported one call late: the
        # backward it belongs to has poisoned its scratch with NaN): the next backward starts from a fresh one
        _ACC_SCRATCH.clear()
        _ORDERED_SCRATCH.clear()
        raise RuntimeError(f"{what} failed ({rc}): {library().radegs_last_error().decode()}")
    return rc


def _require_gpu(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"diff_gaussian_rasterization (MI355X build): `{name}` must be a GPU tensor -- "
                           "this operator has no CPU implementation")


def _f32(t, name):
    """contiguous float32 view of an input; empty tensor == 'not provided' == NULL (reference convention)."""
    if t is None or t.numel() == 0:
        return None
    _require_gpu(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"`{name}` must be float32")
    return t.contiguous()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _forget_image(holder):
    """The native side remembers which image-state buffers hold entry streams by ADDRESS (the backward replays them only for a
    buffer whose forward wrote them).  An address must leave that set when its buffer moves or dies, or a later, unrelated buffer
    landing on it would be taken for a stream image: called on resize and from the tensor's finaliser."""
    try:
        if holder[0] and _lib is not None:
            _lib.radegs_forget_image(ctypes.c_void_p(holder[0]))
    except Exception:   # interpreter shutdown: the library may already be gone; nothing left to protect then
        pass
    holder[0] = 0


# Test knob (tests/test_gpu_poison.py): every buffer the native side is about to fill -- the produced maps, radii, the three state
# buffers -- is first overwritten with 0xFF bytes / NaN, so a kernel that reads something this call has not written, or leaves a
# pixel unwritten, shows up in the results instead of hiding behind whatever the allocator's recycled memory happened to hold.
_POISON = os.environ.get("RADEGS_DEBUG_POISON", "0") == "1"
# RADEGS_ACC_REUSE=0: a fresh accumulation scratch per backward, filled with zeros by the call (the behaviour before round 6); default:
# one scratch per (device, stream), handed back zeroed by the backward itself (RadegsBwdArgs.acc_reuse)
ACC_REUSE = os.environ.get("RADEGS_ACC_REUSE", "1") != "0"
ACC_REUSE_MAX_BYTES = 256 << 20


class _Resizable:
    """uint8 device tensor grown on request from the native side (the resize lambda of
    DGR/rasterize_points.cu:27-33).  image=True: the tensor is an image-state buffer (see _forget_image)."""

    def __init__(self, device, image=False):
        self.tensor = torch.empty(0, dtype=torch.uint8, device=device)
        self.error = None
        holder = [0]
        if image:
            weakref.finalize(self.tensor, _forget_image, holder)

        def _cb(_user, nbytes):
            # every request stands for itself: the native side may retry with a smaller size after a failed one (alloc_image's
            # fallback to the tile-wide formulation, rg_launch.inc), and a stale error must not outlive the retry that succeeded
            self.error = None
            try:
                self.tensor.resize_(int(nbytes))
                if _POISON:
                    self.tensor.fill_(0xFF)
                if image and self.tensor.data_ptr() != holder[0]:
                    _forget_image(holder)
                    holder[0] = self.tensor.data_ptr()
                return self.tensor.data_ptr()
            except Exception as ex:  # surfaces as RADEGS_ERR_ALLOC
                self.error = ex
                return 0

        self.cb = _ALLOC_FN(_cb)

    def release(self):
        """Drop the ctypes callback once the native call has returned: it closes over `self`, and the cycle would keep the
        tensor (hundreds of MB of device memory at 1M+ Gaussians) alive until Python's cyclic GC happens to run."""
        self.cb = None


class _Fixed:
    """allocator callback over a tensor that already exists (the cached accumulation scratch)"""

    def __init__(self, tensor):
        self.tensor = tensor
        self.error = None

        def _cb(_user, nbytes):
            if int(nbytes) > self.tensor.numel():
                self.error = RuntimeError(f"accumulation scratch of {self.tensor.numel()} B asked for {int(nbytes)} B")
                return 0
            return self.tensor.data_ptr()

        self.cb = _ALLOC_FN(_cb)

    def release(self):
        self.cb = None


# held for the whole of a backward that uses a cached scratch: ctypes drops the GIL during the native call, and two host threads queueing
# backwards on ONE stream would otherwise interleave their kernels over the same buffer.  Re-entrant, because an exchange hook runs on the
# calling thread inside the native call, and a call of this module that fails there clears the caches (_check).
_SCRATCH_LOCK = threading.RLock()


class _ScratchCache:
    """uint8 scratch buffers of the backward, one per key = (device index, stream handle), at most 8; every access is made under
    _SCRATCH_LOCK.  zeroed=True: a buffer is all zeros when it is made and the backward hands it back so (RadegsBwdArgs.acc_reuse);
    zeroed=False: the contents are irrelevant between calls."""

    def __init__(self, zeroed):
        self._alloc = torch.zeros if zeroed else torch.empty
        self._buffers = {}

    @contextlib.contextmanager
    def lease(self, key, nbytes, device):
        """Takes the lock and yields the buffer of `key`, grown to `nbytes`; the lock is held until the block ends."""
        with _SCRATCH_LOCK:
            t = self._buffers.get(key)
            if t is None or t.numel() < nbytes:
                if t is None and len(self._buffers) >= 8:
                    self._buffers.clear()
                del t
                self._buffers.pop(key, None)    # let go of the smaller one before its replacement is allocated
                t = self._buffers[key] = self._alloc(max(int(nbytes), 1), dtype=torch.uint8, device=device)
            yield t

    def drop(self, key):
        """Inside a lease whose call failed: the buffer is in an unknown state, the next call starts from a fresh one."""
        self._buffers.pop(key, None)

    def clear(self):
        with _SCRATCH_LOCK:
            self._buffers.clear()

    def values(self):
        with _SCRATCH_LOCK:
            return list(self._buffers.values())

    def __len__(self):
        return len(self.values())


_ACC_SCRATCH = _ScratchCache(zeroed=True)        # the per-Gaussian accumulators, all zeros between calls
_ORDERED_SCRATCH = _ScratchCache(zeroed=False)   # the ordered backward's partial records and sorted positions


def _zero_maps(channels, H, W, device):
    """All-zero maps for the outputs a call does not produce (the reference returns torch.full(0) maps whatever the flags,
    rasterize_points.cu:71-77): FRESH memory every call, like the reference -- ONE zero-filled allocation (one ~6 us fill at 1080p
    instead of five) handed out as disjoint tensors that merely share its storage.  They are built with `set_`, not by slicing:
    slices would be autograd VIEWS of one base, and an autograd Function that returns several views of one tensor makes every
    later in-place edit of them raise ("Output N of ... is a view and is being modified inplace"); the reference's separate
    torch.full tensors allow `depth[mask] = 0` / `normal *= x`, so these must too (tests/test_cabi.py)."""
    total = sum(channels)
    if total == 0:
        return []
    flat = torch.zeros(total * H * W, dtype=torch.float32, device=device)
    storage = flat.untyped_storage()
    out, off = [], 0
    for c in channels:
        t = torch.empty(0, dtype=torch.float32, device=device)
        t.set_(storage, off * H * W, (c, H, W))     # own tensor, own version counter, no `_base`: not a view for autograd
        out.append(t)
        off += c
    return out


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _gaussian_fields(means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size,
                     sh, degree, campos):
    """The fields RadegsFwdArgs, RadegsBwdArgs and RadegsIntegrateArgs share: the Gaussians and the camera as contiguous float32 tensors
    (None: not provided), P, D, M and the four scalars."""
    shs = _f32(sh, "shs")
    return dict(P=int(means3D.size(0)), D=int(degree), M=int(sh.size(1)) if shs is not None else 0, means3D=_f32(means3D, "means3D"), shs=shs,
                colors_precomp=_f32(colors, "colors_precomp"), scales=_f32(scales, "scales"), rotations=_f32(rotations, "rotations"),
                cov3D_precomp=_f32(cov3D_precomp, "cov3D_precomp"), viewmatrix=_f32(viewmatrix, "viewmatrix"),
                projmatrix=_f32(projmatrix, "projmatrix"), cam_pos=_f32(campos, "campos"), scale_modifier=float(scale_modifier),
                tan_fovx=float(tan_fovx), tan_fovy=float(tan_fovy), kernel_size=float(kernel_size))


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                        projmatrix, tan_fovx, tan_fovy, kernel_size, image_height, image_width, sh, degree, campos, prefiltered,
                        require_coord, require_depth, debug):
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")  # rasterize_points.cu:60-62
    _require_gpu(means3D, "means3D")
    L = library()
    dev = means3D.device
    P, H, W = int(means3D.size(0)), int(image_height), int(image_width)
    require_coord, require_depth = bool(require_coord), bool(require_depth)
    fo = dict(dtype=torch.float32, device=dev)
    live = P != 0

    geo = require_coord or require_depth
    # (channels, produced by this call) in the order color, depth, mdepth, coord, mcoord, alpha, normal
    spec = [(3, True), (1, require_depth), (1, require_depth), (3, require_coord), (3, require_coord), (1, True), (3, geo)]
    # A map the flags do not produce is all-zero in the reference (torch::full(0), rasterize_points.cu:71-77) and FRESH memory on every call.
    # The library zero-fills whatever unproduced map it is handed (include/radegs.h: inside the blend kernel, no separate fill), so a live call
    # allocates all seven uninitialised; only the call that launches nothing (P == 0) fills them here.
    if live:
        maps = [torch.empty((c, H, W), **fo) for c, _ in spec]
    else:
        maps = _zero_maps([c for c, _ in spec], H, W, dev)
    out_color, out_depth, out_mdepth, out_coord, out_mcoord, out_alpha, out_normal = maps
    radii = torch.empty(P, dtype=torch.int32, device=dev) if live else torch.zeros(P, dtype=torch.int32, device=dev)
    if _POISON and live:
        for m in maps:   # the unproduced ones too: the library must overwrite them with zeros
            m.fill_(float("nan"))
        radii.fill_(-0x01010102)
    geom, binning, img = _Resizable(dev), _Resizable(dev), _Resizable(dev, image=True)
    rendered = 0
    if live:
        a = _args(RadegsFwdArgs, width=W, height=H, background=_f32(background, "bg"), opacities=_f32(opacity, "opacities"),
                  prefiltered=int(bool(prefiltered)), require_coord=int(require_coord), require_depth=int(require_depth), debug=int(bool(debug)),
                  out_color=out_color, out_coord=out_coord, out_mcoord=out_mcoord, out_depth=out_depth, out_mdepth=out_mdepth,
                  out_alpha=out_alpha, out_normal=out_normal, radii=radii,
                  **_gaussian_fields(means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                                     tan_fovy, kernel_size, sh, degree, campos))
        with torch.cuda.device(dev):
            rc = L.radegs_forward(ctypes.byref(a), geom.cb, None, binning.cb, None, img.cb, None, _stream(dev))
        for r in (geom, binning, img):
            r.release()
            if r.error is not None:
                raise r.error
        rendered = _check(rc, "radegs_forward")
    return (rendered, out_color, out_coord, out_mcoord, out_alpha, out_normal, out_depth, out_mdepth, radii, geom.tensor,
            binning.tensor, img.tensor)


def _alloc_grads(grad_alloc, P, M, dev):
    """The eight gradients of the backward in its return order, then dL_drgb_clamped (None unless the allocator supplies it).  Each comes
    from the device's allocator hook where that returns a tensor; dL_dsh is None where the hook answered SKIP_GRAD (see SKIP_GRAD)."""
    fo = dict(dtype=torch.float32, device=dev)

    def hooked(name, shape):
        t = grad_alloc(name, shape, torch.float32, dev)
        if t is not None:
            assert t.shape == torch.Size(shape) and t.is_contiguous() and t.dtype == torch.float32 and t.device == dev
        return t

    def mk(name, shape):
        t = hooked(name, shape) if P != 0 and grad_alloc is not None else None
        if t is not None:
            return t
        if P != 0 and _POISON:
            return torch.full(shape, float("nan"), **fo)
        return torch.empty(shape, **fo) if P != 0 else torch.zeros(shape, **fo)

    dL_dmeans3D, dL_dmeans2D, dL_dcolors = mk("dL_dmeans3D", (P, 3)), mk("dL_dmeans2D", (P, 3)), mk("dL_dcolors", (P, 3))
    dL_dopacity, dL_dcov3D = mk("dL_dopacity", (P, 1)), mk("dL_dcov3D", (P, 6))
    drgb = hooked("dL_drgb_clamped", (P, 3)) if P != 0 and M != 0 and grad_alloc is not None else None
    skip_dsh = drgb is not None and grad_alloc("dL_dsh", (P, M, 3), torch.float32, dev) is SKIP_GRAD
    dL_dsh = None if skip_dsh else mk("dL_dsh", (P, M, 3))
    dL_dscales, dL_drotations = mk("dL_dscales", (P, 3)), mk("dL_drotations", (P, 4))
    return dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, drgb


def _exchange_hooks(grad_alloc, drgb, errors):
    """{drgb_ready, grads_ready, grad_chunks} of RadegsBwdArgs from the object the allocator is a bound method of: `drgb_ready()` is called
    on the host as soon as the kernel that writes dL_drgb_clamped is queued, `grads_ready(first, count)` after each of `grad_chunks`
    launches of the per-Gaussian backward, so that the owner's exchange of those rows runs under the launches that follow."""
    owner = getattr(grad_alloc, "__self__", None)
    hooks = {}
    if owner is not None and drgb is not None and callable(getattr(owner, "drgb_ready", None)) and getattr(owner, "early_drgb", False):
        hooks["drgb_ready"] = _c_hook(_READY_FN, owner.drgb_ready, errors)
    if owner is not None and callable(getattr(owner, "grads_ready", None)) and int(getattr(owner, "grad_chunks", 0) or 0) > 1 \
            and getattr(owner, "early_grads", False):
        hooks["grad_chunks"] = int(owner.grad_chunks)
        hooks["grads_ready"] = _c_hook(_GRADS_READY_FN, owner.grads_ready, errors)
    return hooks


def _run_backward(L, a, dev, ordered, hook_errors):
    """radegs_backward, or radegs_backward_ordered, over the prepared arguments `a`; returns (rc, the accumulator's holder).  The accumulator
    is ONE all-zero buffer per (device, stream), handed back all-zero by every successful call (RadegsBwdArgs.acc_reuse) -- unless its
    contents are wanted afterwards (KEEP_ACC, _POISON, the ordered backward: every record written by the call) or it is too large: then the
    call gets a fresh one.  The ordered backward's scratch is cached in the same way.  A failed call drops what it leased."""
    global LAST_PARTIALS
    coord = bool(a.require_coord)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(torch.cuda.current_stream(dev).cuda_stream))
    if ordered:
        cache, nbytes = _ORDERED_SCRATCH, int(L.radegs_backward_ordered_scratch_bytes(a.P, a.R, int(coord)))
        cached = a.R > 0
    else:
        # (above ACC_REUSE_MAX_BYTES the clearing stores cost the per-Gaussian kernel more than the fill they replace: C4, 5 M Gaussians with
        # the coord map = 640 MB, same-box A/B: preprocess_bwd +0.13 ms against a 0.08-ms fill)
        cache, nbytes = _ACC_SCRATCH, a.P * (128 if coord else 64)
        cached = not (KEEP_ACC or _POISON or not ACC_REUSE or nbytes > ACC_REUSE_MAX_BYTES)
    with cache.lease(key, nbytes, dev) if cached else contextlib.nullcontext() as buf:
        a.acc_reuse = int(cached and not ordered)
        acc = _Fixed(buf) if a.acc_reuse else _Resizable(dev)
        with torch.cuda.device(dev):
            if ordered:
                rc = L.radegs_backward_ordered(ctypes.byref(a), acc.cb, None, _ptr(buf), nbytes if cached else 0, _stream(dev))
            else:
                rc = L.radegs_backward(ctypes.byref(a), acc.cb, None, _stream(dev))
        acc.release()
        ok = rc == 0 and acc.error is None and not hook_errors
        if cached and not ok:
            cache.drop(key)
        if ordered and KEEP_ACC and ok:
            rec = 32 if coord else 16
            part = torch.empty((0, rec), dtype=torch.float32, device=dev) if buf is None else buf[:a.R * rec * 4].view(torch.float32).view(a.R, rec).clone()
            LAST_PARTIALS = (part, a.R)
    return rc, acc


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                                 projmatrix, tan_fovx, tan_fovy, kernel_size, dL_dout_color, dL_dout_coord, dL_dout_mcoord,
                                 dL_dout_depth, dL_dout_mdepth, dL_dout_alpha, dL_dout_normal, normalmap, sh, degree, campos,
                                 geomBuffer, R, binningBuffer, imageBuffer, alphas, require_coord, require_depth, debug):
    global LAST_ACC
    _require_gpu(means3D, "means3D")
    L = library()
    dev = means3D.device
    P = int(means3D.size(0))
    M = int(sh.size(1)) if (sh is not None and sh.numel() != 0) else 0
    grad_alloc = _grad_allocator_for(dev)
    *grads, drgb = _alloc_grads(grad_alloc, P, M, dev)
    dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations = grads
    if P != 0:
        g = _gaussian_fields(means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                             kernel_size, sh, degree, campos)
        if g["scales"] is not None and g["rotations"] is None:
            raise RuntimeError("scales given without rotations")
        gb, bb, ib = geomBuffer.contiguous(), binningBuffer.contiguous(), imageBuffer.contiguous()
        hook_errors = []
        ordered = DETERMINISTIC     # read once: another thread may flip the switch while this call runs
        a = _args(RadegsBwdArgs, R=int(R), width=int(dL_dout_color.size(2)), height=int(dL_dout_color.size(1)),
                  background=_f32(background, "bg"), alphas=_f32(alphas, "alphas"), radii=radii.contiguous(), normalmap=_f32(normalmap, "normalmap"),
                  geom_buffer=gb if gb.numel() else None, binning_buffer=bb if bb.numel() else None, image_buffer=ib if ib.numel() else None,
                  dL_dpix=_f32(dL_dout_color, "dL_dcolor"), dL_dpix_coord=_f32(dL_dout_coord, "dL_dcoord"),
                  dL_dpix_mcoord=_f32(dL_dout_mcoord, "dL_dmcoord"), dL_dpix_depth=_f32(dL_dout_depth, "dL_ddepth"),
                  dL_dpix_mdepth=_f32(dL_dout_mdepth, "dL_dmdepth"), dL_dalphas=_f32(dL_dout_alpha, "dL_dalpha"),
                  dL_dpix_normal=_f32(dL_dout_normal, "dL_dnormal"),
                  dL_dmean2D=dL_dmeans2D, dL_dcolor=dL_dcolors, dL_dopacity=dL_dopacity, dL_dmean3D=dL_dmeans3D, dL_dcov3D=dL_dcov3D,
                  dL_dsh=dL_dsh if M else None, dL_dscale=dL_dscales, dL_drot=dL_drotations,
                  require_coord=int(bool(require_coord)), require_depth=int(bool(require_depth)), debug=int(bool(debug)),
                  dL_drgb_clamped=drgb, opacity_grad_intended=int(bool(OPACITY_GRAD_INTENDED)), keep_sums=int(bool(KEEP_ACC)),
                  **g, **_exchange_hooks(grad_alloc, drgb, hook_errors))
        rc, acc = _run_backward(L, a, dev, ordered, hook_errors)
        if acc.error is not None:
            raise acc.error
        if hook_errors:
            raise hook_errors[0]
        _check(rc, "radegs_backward_ordered" if ordered else "radegs_backward")
        if KEEP_ACC:
            LAST_ACC = acc.tensor.view(torch.float32)
        if g["scales"] is None:  # precomputed covariance: scale/rotation grads are identically zero
            dL_dscales.zero_()
            dL_drotations.zero_()
    return tuple(grads)


def backward_from_sums(sums, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                       tan_fovy, kernel_size, image_height, image_width, sh, degree, campos, geomBuffer, require_coord, *,
                       grad_chunks=0, grads_ready=None, want_drgb=False, drgb_ready=None, keep_sums=False):
    """Test hook (radegs_backward_from_sums, include/radegs.h): the per-Gaussian half of the backward over caller-supplied per-Gaussian
    sums [P, 16 | 32] (the reference's render-kernel sums, its constant factors included).  Returns the 8-tuple of
    rasterize_gaussians_backward.

    The keyword arguments reach the launch modes of RadegsBwdArgs: grad_chunks >= 2 with grads_ready = callable(first, count): that many
    launches over consecutive ranges of Gaussians, the callable called on the host after each one; want_drgb: a NaN-filled (P,3)
    dL_drgb_clamped is allocated and returned as a NINTH element; drgb_ready = callable(): dL_drgb_clamped is written by its own kernel
    and the callable is called once that kernel is queued (implies want_drgb); keep_sums goes into the structure as it is (the library
    only reads `sums`).  An exception raised by a callable is re-raised after the native call has returned."""
    _require_gpu(means3D, "means3D")
    L = library()
    dev = means3D.device
    P = int(means3D.size(0))
    M = int(sh.size(1)) if (sh is not None and sh.numel() != 0) else 0
    fo = dict(dtype=torch.float32, device=dev)
    rec = 32 if require_coord else 16
    sm = _f32(sums, "sums")
    if tuple(sm.shape) != (P, rec):
        raise RuntimeError(f"sums must be ({P}, {rec})")
    out = [torch.full(s, float("nan"), **fo) for s in ((P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, max(M, 1), 3), (P, 3), (P, 4))]
    dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations = out
    want_drgb = bool(want_drgb) or drgb_ready is not None
    drgb = torch.full((P, 3), float("nan"), **fo) if want_drgb else None
    cb_err = []
    g = _gaussian_fields(means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                         kernel_size, sh, degree, campos)
    a = _args(RadegsBwdArgs, width=int(image_width), height=int(image_height), radii=radii.contiguous(), geom_buffer=geomBuffer.contiguous(),
              dL_dmean2D=dL_dmeans2D, dL_dcolor=dL_dcolors, dL_dopacity=dL_dopacity, dL_dmean3D=dL_dmeans3D, dL_dcov3D=dL_dcov3D,
              dL_dsh=dL_dsh if M else None, dL_dscale=dL_dscales, dL_drot=dL_drotations, require_coord=int(bool(require_coord)),
              dL_drgb_clamped=drgb, opacity_grad_intended=int(bool(OPACITY_GRAD_INTENDED)), drgb_ready=_c_hook(_READY_FN, drgb_ready, cb_err),
              grad_chunks=int(grad_chunks), grads_ready=_c_hook(_GRADS_READY_FN, grads_ready, cb_err), keep_sums=int(bool(keep_sums)), **g)
    with torch.cuda.device(dev):
        rc = L.radegs_backward_from_sums(ctypes.byref(a), _ptr(sm), _stream(dev))
    if cb_err:
        raise cb_err[0]
    _check(rc, "radegs_backward_from_sums")
    if g["scales"] is None:
        dL_dscales.zero_()
        dL_drotations.zero_()
    out = (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, (dL_dsh if M else None), dL_dscales, dL_drotations)
    return out + (drgb,) if want_drgb else out


def sh_grad_from_views(means3D, campos_all, drgb_all, degree, M, scale=1.0, out=None):
    """dL_dsh[P,M,3] = scale * sum_v basis(dir_v) (x) drgb_all[v]  (radegs_sh_grad_from_views; campos_all [V,3], drgb_all [V,P,3])."""
    _require_gpu(means3D, "means3D")
    L = library()
    dev = means3D.device
    P, V = int(means3D.size(0)), int(drgb_all.size(0))
    m3, cp, dr = _f32(means3D, "means3D"), _f32(campos_all, "campos_all"), _f32(drgb_all, "drgb_all")
    if V and (tuple(drgb_all.shape) != (V, P, 3) or tuple(campos_all.shape) != (V, 3)):
        raise RuntimeError("campos_all must be (V,3) and drgb_all (V,P,3)")
    if out is None:
        out = torch.empty((P, int(M), 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = L.radegs_sh_grad_from_views(P, int(degree), int(M), V, _ptr(m3), _ptr(cp), _ptr(dr), float(scale), _ptr(out), _stream(dev))
    _check(rc, "radegs_sh_grad_from_views")
    return out


def mark_visible(means3D, viewmatrix, projmatrix):
    _require_gpu(means3D, "means3D")
    L = library()
    dev = means3D.device
    P = int(means3D.size(0))
    present = torch.zeros(P, dtype=torch.bool, device=dev)
    if P != 0:
        m3, vm, pm = _f32(means3D, "means3D"), _f32(viewmatrix, "viewmatrix"), _f32(projmatrix, "projmatrix")
        with torch.cuda.device(dev):
            rc = L.radegs_mark_visible(P, _ptr(m3), _ptr(vm), _ptr(pm), ctypes.c_void_p(present.data_ptr()), _stream(dev))
        _check(rc, "radegs_mark_visible")
    return present


def integrate_gaussians_to_points(background, points3D, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                                  view2gaussian_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, kernel_size, subpixel_offset,
                                  image_height, image_width, sh, degree, campos, prefiltered, debug):
    """IntegrateGaussiansToPointsCUDA (DGR/rasterize_points.cu:269-388).  `view2gaussian_precomp`, `subpixel_offset` and
    `prefiltered` are accepted and -- exactly as upstream's kernels do -- never read.  Returns the upstream 10-tuple
    (num_rendered, out_color[9,H,W], out_alpha_integrated[PN], out_color_integrated[PN,3], out_coordinate2d[PN,2],
    out_sdf[PN], radii[P], geomBuffer, binningBuffer, imgBuffer); the point-state buffer is dropped like upstream's."""
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    if points3D.dim() != 2 or points3D.size(1) != 3:
        raise RuntimeError("points3D must have dimensions (num_points, 3)")
    _require_gpu(means3D, "means3D")
    _require_gpu(points3D, "points3D")
    L = library()
    dev = means3D.device
    P, PN, H, W = int(means3D.size(0)), int(points3D.size(0)), int(image_height), int(image_width)
    fo = dict(dtype=torch.float32, device=dev)
    out_color = torch.empty((9, H, W), **fo)
    radii = torch.empty(P, dtype=torch.int32, device=dev)
    out_alpha_integrated = torch.empty((PN,), **fo)
    out_color_integrated = torch.empty((PN, 3), **fo)
    out_coordinate2d = torch.empty((PN, 2), **fo)
    out_sdf = torch.empty((PN,), **fo)
    geom, binning, img, pts = _Resizable(dev), _Resizable(dev), _Resizable(dev), _Resizable(dev)
    a = _args(RadegsIntegrateArgs, PN=PN, width=W, height=H, background=_f32(background, "bg"), opacities=_f32(opacity, "opacities"),
              points3D=_f32(points3D, "points3D"), debug=int(bool(debug)), out_color=out_color, out_alpha_integrated=out_alpha_integrated,
              out_color_integrated=out_color_integrated, out_coordinate2d=out_coordinate2d, out_sdf=out_sdf, radii=radii,
              **_gaussian_fields(means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                                 kernel_size, sh, degree, campos))
    with torch.cuda.device(dev):
        rc = L.radegs_integrate(ctypes.byref(a), geom.cb, None, binning.cb, None, img.cb, None, pts.cb, None, _stream(dev))
    for r in (geom, binning, img, pts):
        r.release()
        if r.error is not None:
            raise r.error
    rendered = _check(rc, "radegs_integrate")
    global LAST_POINT_STATE
    LAST_POINT_STATE = pts.tensor if KEEP_ACC else None
    return (rendered, out_color, out_alpha_integrated, out_color_integrated, out_coordinate2d, out_sdf, radii, geom.tensor,
            binning.tensor, img.tensor)


def debug_export(name, dtype, numel, P, R, W, H, require_coord, geomBuffer, binningBuffer, imageBuffer):
    """Test hook: copy a private state array (see radegs_debug_export in include/radegs.h)."""
    L = library()
    dev = geomBuffer.device
    dst = torch.empty(numel, dtype=dtype, device=dev)
    if name == "blk_chunks":
        # the last array of the image state, copied at the size asked for: it starts where a state without stream storage ends, less
        # the layout's 256 bytes of tail padding (csrc/rg_layout.h: kTailPad)
        end = int(L.radegs_image_bytes(int(W), int(H))) - 256 + dst.numel() * dst.element_size()
        have = imageBuffer.numel() * imageBuffer.element_size()
        if end > have:
            raise RuntimeError(f"debug_export: blk_chunks of {dst.numel() * dst.element_size()} bytes would end at byte {end} of an image state of {have}")
    with torch.cuda.device(dev):
        n = L.radegs_debug_export(name.encode(), int(P), int(R), int(W), int(H), int(bool(require_coord)),
                                  ctypes.c_void_p(geomBuffer.data_ptr()) if geomBuffer.numel() else None,
                                  ctypes.c_void_p(binningBuffer.data_ptr()) if binningBuffer.numel() else None,
                                  ctypes.c_void_p(imageBuffer.data_ptr()) if imageBuffer.numel() else None,
                                  ctypes.c_void_p(dst.data_ptr()), dst.numel() * dst.element_size(), _stream(dev))
    if n < 0:
        raise RuntimeError(L.radegs_last_error().decode())
    return dst


def point_bytes(P, PN, W, H):
    """Size of the point state an integrate call of these sizes allocates (radegs_point_bytes)."""
    return int(library().radegs_point_bytes(int(P), int(PN), int(W), int(H)))


def debug_export_points(name, dtype, numel, P, PN, W, H, pointBuffer=None):
    """Test hook: copy a private array of the point state (see radegs_debug_export_points in include/radegs.h).  pointBuffer None: the
    state the last integrate_gaussians_to_points left in LAST_POINT_STATE (kept under KEEP_ACC)."""
    L = library()
    buf = LAST_POINT_STATE if pointBuffer is None else pointBuffer
    if buf is None:
        raise RuntimeError("debug_export_points: no point state (set KEEP_ACC before integrate_gaussians_to_points)")
    have, need = buf.numel() * buf.element_size(), point_bytes(P, PN, W, H)
    if have < need:
        raise RuntimeError(f"debug_export_points: a point state of {have} bytes, (P, PN, W, H) = {(P, PN, W, H)} needs {need}")
    dev = buf.device
    dst = torch.empty(numel, dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        n = L.radegs_debug_export_points(name.encode(), int(P), int(PN), int(W), int(H), ctypes.c_void_p(buf.data_ptr()),
                                         ctypes.c_void_p(dst.data_ptr()), dst.numel() * dst.element_size(), _stream(dev))
    if n < 0:
        raise RuntimeError(L.radegs_last_error().decode())
    return dst


def binning_stats(reset=False):
    """(speculative forwards, forwards redone because the predicted capacity was too small) since the last reset."""
    calls, misses = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
    library().radegs_binning_stats(ctypes.byref(calls), ctypes.byref(misses), int(bool(reset)))
    return int(calls.value), int(misses.value)


def reload_env():
    """Have the library read its RADEGS_* environment switches again (it reads them once, at first use); RADEGS_DETERMINISTIC, which this
    module reads, with them."""
    global DETERMINISTIC
    DETERMINISTIC = os.environ.get("RADEGS_DETERMINISTIC", "0") == "1"
    library().radegs_reload_env()


def last_forward_used_streams():
    """The blend formulation of this thread's last forward: True = sub-tile entry streams, False = tile-wide kernels, None = none yet."""
    v = library().radegs_last_forward_used_streams()
    return None if v < 0 else bool(v)


def profile_enable(on=True, only=None, every=1):
    """Per-stage HIP-event timing on the launch stream.  `only` = a stage name: record that stage alone (every recorded stage
    boundary costs ~10 us of stream bubble, so a timed run selects just the kernel it reports), `every` = n: every n-th launch."""
    L = library()
    sel = -1
    if only is not None:
        names = [L.radegs_profile_stage_name(i).decode() for i in range(L.radegs_profile_num_stages())]
        sel = names.index(only)
    L.radegs_profile_select(sel)
    L.radegs_profile_stride(int(every) if only is not None else 1)
    L.radegs_profile_enable(int(bool(on)))


def profile_collect():
    """{stage name: (total ms, launches)} since the last collect (HIP events on the launch stream)."""
    L = library()
    n = L.radegs_profile_num_stages()
    ms = (ctypes.c_float * n)()
    cnt = (ctypes.c_int * n)()
    L.radegs_profile_collect(ms, cnt, n)
    return {L.radegs_profile_stage_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(n)}
