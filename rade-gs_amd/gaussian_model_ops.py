"""HIP-backed mirror of GaussianModel.get_scaling_n_opacity_with_3D_filter (scene/gaussian_model.py:156-166), the
per-Gaussian step gaussian_renderer.render() runs right before the rasterizer (gaussian_renderer/__init__.py:63).
SURVEY 8f N3.  One streaming kernel per direction instead of ~10 / ~20 eager torch kernels.  GPU only.

Also the HIP-backed adaptive density control of the same class: add_densification_stats,
densify_and_prune and patch_gaussian_model, which installs both on the reference's GaussianModel."""
import ctypes
import functools

import torch

import geom_host as gh
import model_io as _model_io
from diff_gaussian_rasterization import _C

DENSIFY_NUM_TENSORS = 18


class RadegsDensifyTensors(ctypes.Structure):
    _fields_ = [("inp", ctypes.c_void_p * DENSIFY_NUM_TENSORS), ("out", ctypes.c_void_p * DENSIFY_NUM_TENSORS)]


_I, _VP, _FL = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
_SIGNATURES = {
    "radegs_filter3d_forward": (_I, [_I] + [_VP] * 6),
    "radegs_filter3d_backward": (_I, [_I] + [_VP] * 8),
    "radegs_compute_filter3d": (_I, [_I, _VP, _I, _VP, _FL, _VP, _VP, _VP, _VP]),
    "radegs_model_activate_forward": (_I, [_I, _I] + [_VP] * 11),
    "radegs_model_activate_backward": (_I, [_I, _I] + [_VP] * 14),
    "radegs_densify_stats": (_I, [_I] + [_VP] * 9),
    "radegs_densify_stats_reduced": (_I, [_I] + [_VP] * 8),
    "radegs_densify_plan_bytes": (ctypes.c_size_t, [_I]),
    "radegs_densify_plan": (_I, [_I] + [_VP] * 5 + [_FL, _VP, _FL, _FL, _I, _FL, _VP, ctypes.c_size_t, _VP, _VP]),
    "radegs_densify_apply": (_I, [_I, _I, _I, ctypes.POINTER(RadegsDensifyTensors), _VP, _VP, _VP]),
    **_model_io.SIGNATURES,      # patch_gaussian_model_io installs the methods that run on them
}


def _lib():
    return _C.bind(_SIGNATURES)


_call = functools.partial(gh.call, _SIGNATURES)


def _prep(t, name, cols):
    _C._require_gpu(t, name)
    if t.dtype != torch.float32 or t.dim() != 2 or t.size(1) != cols:
        raise RuntimeError(f"`{name}` must be float32 of shape (P,{cols})")
    return t.contiguous()


class _ScalingOpacity3DFilter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling_raw, opacity_raw, filter_3D):
        sc, op, f3 = _prep(scaling_raw, "_scaling", 3), _prep(opacity_raw, "_opacity", 1), _prep(filter_3D, "filter_3D", 1)
        P = sc.size(0)
        if op.size(0) != P or f3.size(0) != P:
            raise RuntimeError("_scaling, _opacity and filter_3D must have the same number of rows")
        scales, opacity = torch.empty_like(sc), torch.empty_like(op)
        _call("radegs_filter3d_forward", sc.device, P, sc, op, f3, scales, opacity)
        ctx.save_for_backward(sc, op, f3)
        ctx.set_materialize_grads(False)     # an output that nothing downstream uses arrives as None, not as a tensor of zeros
        return scales, opacity

    @staticmethod
    def backward(ctx, g_scales, g_opacity):
        sc, op, f3 = ctx.saved_tensors
        if g_scales is None and g_opacity is None:
            return None, None, None
        gs = None if g_scales is None else g_scales.contiguous()
        go = None if g_opacity is None else g_opacity.contiguous()
        g_sc, g_op = torch.empty_like(sc), torch.empty_like(op)
        _call("radegs_filter3d_backward", sc.device, sc.size(0), sc, op, f3, gs, go, g_sc, g_op)
        return g_sc, g_op, None


def scaling_n_opacity_with_3D_filter(scaling_raw, opacity_raw, filter_3D):
    """(scales[P,3], opacity[P,1]) = GaussianModel.get_scaling_n_opacity_with_3D_filter evaluated on the raw parameters
    `_scaling` (log-space), `_opacity` (logit) and the `filter_3D` buffer.  Differentiable w.r.t. the two parameters."""
    return _ScalingOpacity3DFilter.apply(scaling_raw, opacity_raw, filter_3D)


def _prep3(t, name, cols):
    """`t` as the activation kernels address it: float32 (P, K, 3) with K == `cols` (any K when None), contiguous and 16-byte aligned"""
    _C._require_gpu(t, name)
    if t.dtype != torch.float32 or t.dim() != 3 or t.size(2) != 3 or (cols is not None and t.size(1) != cols):
        raise RuntimeError(f"`{name}` must be float32 of shape (P,{'K' if cols is None else cols},3)")
    return _aligned(t.contiguous())


def _aligned(t):
    """a contiguous tensor whose first byte lies on a 16-byte boundary (a view into the middle of a buffer is copied)"""
    return t.clone() if t.numel() and t.data_ptr() % 16 else t


class _ModelActivations(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f_dc, f_rest, rotation_raw, scaling_raw, opacity_raw, filter_3D):
        out = model_activations_forward(f_dc, f_rest, rotation_raw, scaling_raw, opacity_raw, filter_3D)
        ctx.save_for_backward(rotation_raw, scaling_raw, opacity_raw, filter_3D)
        ctx.K = f_rest.size(1)
        ctx.set_materialize_grads(False)     # an output that nothing downstream uses arrives as None, not as a tensor of zeros
        return out

    @staticmethod
    def backward(ctx, g_shs, g_rotations, g_scales, g_opacity):
        rot, sc, op, f3 = ctx.saved_tensors
        if g_shs is None and g_rotations is None and g_scales is None and g_opacity is None:
            return None, None, None, None, None, None
        return model_activations_backward(ctx.K, rot, sc, op, f3, g_shs, g_rotations, g_scales, g_opacity) + (None,)


def _param(t, name, tail):
    """a raw parameter as the activation kernels address it: on the GPU, float32, (P,) + tail, contiguous; nothing is copied on the way in"""
    _C._require_gpu(t, name)
    if t.dtype != torch.float32 or t.dim() != len(tail) + 1 or any(x is not None and x != y for x, y in zip(tail, t.shape[1:])):
        raise RuntimeError(f"`{name}` must be float32 of shape (P,{','.join('K' if x is None else str(x) for x in tail)})")
    if not t.is_contiguous():
        raise RuntimeError(f"`{name}` must be a contiguous {t.dtype} GPU tensor with {t.size(0)} rows")
    return t


def _outputs(out, shapes, dev):
    if out is None:
        return tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in shapes)
    out = tuple(out)
    if len(out) != len(shapes):
        raise RuntimeError(f"`out` must hold {len(shapes)} tensors")
    for t, s in zip(out, shapes):
        _C._require_gpu(t, "out")
        if t.dtype != torch.float32 or tuple(t.shape) != s or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f"`out` must hold contiguous float32 tensors of shapes {shapes} on the inputs' device")
    return out


def model_activations_forward(f_dc, f_rest, rotation_raw, scaling_raw, opacity_raw, filter_3D, out=None):
    """radegs_model_activate_forward without autograd: (shs, rotations, scales, opacity).  `out`: four tensors to write into instead of
    new ones (contiguous, of those shapes; the first two 16-byte aligned)."""
    dc, rest = _param(f_dc, "_features_dc", (1, 3)), _param(f_rest, "_features_rest", (None, 3))
    rot, sc = _param(rotation_raw, "_rotation", (4,)), _param(scaling_raw, "_scaling", (3,))
    op, f3 = _param(opacity_raw, "_opacity", (1,)), _param(filter_3D, "filter_3D", (1,))
    P, K, dev = dc.size(0), rest.size(1), dc.device
    if any(t.size(0) != P for t in (rest, rot, sc, op, f3)):
        raise RuntimeError("_features_dc, _features_rest, _rotation, _scaling, _opacity and filter_3D must have the same number of rows")
    if any(t.device != dev for t in (rest, rot, sc, op, f3)):
        raise RuntimeError("_features_dc, _features_rest, _rotation, _scaling, _opacity and filter_3D must be on the same device")
    dc, rest, rot = _aligned(dc.detach()), _aligned(rest.detach()), _aligned(rot.detach())
    shs, rotations, scales, opacity = _outputs(out, ((P, K + 1, 3), (P, 4), (P, 3), (P, 1)), dev)
    _call("radegs_model_activate_forward", dev, P, K, dc, rest if K else None, rot, sc, op, f3, shs, rotations, scales, opacity)
    return shs, rotations, scales, opacity


def model_activations_backward(K, rotation_raw, scaling_raw, opacity_raw, filter_3D, g_shs, g_rotations, g_scales, g_opacity, out=None):
    """radegs_model_activate_backward: the gradients (g_f_dc [P,1,3], g_f_rest [P,K,3], g_rotation_raw, g_scaling_raw, g_opacity_raw) of the
    cotangents of model_activations' four outputs, each of which may be None (= zero).  `out`: five tensors to write into instead of new
    ones (contiguous, of those shapes; the first three 16-byte aligned)."""
    rot = _aligned(_param(rotation_raw, "_rotation", (4,)).detach())
    sc, op, f3 = _param(scaling_raw, "_scaling", (3,)), _param(opacity_raw, "_opacity", (1,)), _param(filter_3D, "filter_3D", (1,))
    P, dev = rot.size(0), rot.device
    if sc.size(0) != P or op.size(0) != P or f3.size(0) != P:
        raise RuntimeError("_rotation, _scaling, _opacity and filter_3D must have the same number of rows")
    gsh = None if g_shs is None else _prep3(g_shs, "grad of shs", K + 1)
    gr = None if g_rotations is None else _aligned(_prep(g_rotations, "grad of rotations", 4))
    gs = None if g_scales is None else _prep(g_scales, "grad of scales", 3)
    go = None if g_opacity is None else _prep(g_opacity, "grad of opacity", 1)
    for g, n in ((gsh, "shs"), (gr, "rotations"), (gs, "scales"), (go, "opacity")):
        if g is not None and g.size(0) != P:
            raise RuntimeError(f"grad of {n} must have {P} rows")
    out = _outputs(out, ((P, 1, 3), (P, K, 3), (P, 4), (P, 3), (P, 1)), dev)
    g_dc, g_rest, g_rot, g_sc, g_op = out
    _call("radegs_model_activate_backward", dev, P, K, rot, sc, op, f3, gsh, gr, gs, go, g_dc, g_rest if K else None, g_rot, g_sc, g_op)
    return out


def model_activations(f_dc, f_rest, rotation_raw, scaling_raw, opacity_raw, filter_3D):
    """(shs[P,K+1,3], rotations[P,4], scales[P,3], opacity[P,1]) = (GaussianModel.get_features, get_rotation,
    *get_scaling_n_opacity_with_3D_filter) from the raw parameters: everything render() does between the model and the rasterizer, one
    launch forward and one backward (csrc/radegs_activate.hip).  Differentiable w.r.t. the five parameters; `filter_3D` carries none."""
    return _ModelActivations.apply(f_dc, f_rest, rotation_raw, scaling_raw, opacity_raw, filter_3D)


@torch.no_grad()
def compute_3D_filter(xyz, cameras):
    """GaussianModel.compute_3D_filter (scene/gaussian_model.py:179-232): returns the (P,1) `filter_3D` buffer for the
    Gaussian centres `xyz` and an iterable of cameras (attributes R, T, image_width, image_height, FoVx, FoVy), all cameras
    in one kernel instead of ~15 torch kernels per camera.

    A point that no camera sees takes the largest distance over the points that are seen, as upstream.  When no camera sees ANY point,
    upstream raises (it takes `.max()` of an empty selection); this returns a filter of exactly 0 for every point instead."""
    import math

    import numpy as np
    _C._require_gpu(xyz, "xyz")
    x = _prep(xyz.detach(), "xyz", 3)
    rows, focal_length = [], 0.0
    for cam in cameras:
        W, H = cam.image_width, cam.image_height
        fx = W / (2 * math.tan(cam.FoVx / 2.))
        fy = H / (2 * math.tan(cam.FoVy / 2.))
        rows.append(np.concatenate([np.asarray(cam.R, dtype=np.float32).reshape(9), np.asarray(cam.T, dtype=np.float32).reshape(3),
                                    np.array([fx, fy, W, H], dtype=np.float32)]))
        focal_length = max(focal_length, fx)
    if not rows:
        raise RuntimeError("compute_3D_filter needs at least one camera")
    table = torch.from_numpy(np.stack(rows)).to(x.device)
    P = x.size(0)
    dist = torch.empty(P, dtype=torch.float32, device=x.device)
    mx = torch.empty(1, dtype=torch.int32, device=x.device)
    out = torch.empty((P, 1), dtype=torch.float32, device=x.device)
    _call("radegs_compute_filter3d", x.device, P, x, len(rows), table, float(focal_length), dist, mx, out)
    return out


# ---- adaptive density control (scene/gaussian_model.py:717-747, train.py:186-187) ----
# upstream's optimizer group name -> model attribute, in the order of RadegsDensifyTensors
_DENSIFY_PARAMS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"), ("scaling", "_scaling"),
                   ("rotation", "_rotation"))
_STATS = ("xyz_gradient_accum", "xyz_gradient_accum_abs", "xyz_gradient_accum_abs_max", "denom")


def _rows(t, name, P, dtype=torch.float32):
    """a per-Gaussian array as the kernels address it: on the GPU, `dtype`, contiguous, P rows"""
    _C._require_gpu(t, name)
    if t.dtype != dtype or t.dim() < 1 or t.size(0) != P or not t.is_contiguous():
        raise RuntimeError(f"`{name}` must be a contiguous {dtype} GPU tensor with {P} rows")
    return t


def _stat_rows(model, P):
    stats = [_rows(getattr(model, n), n, P) for n in _STATS]
    for n, t in zip(_STATS, stats):
        if t.numel() != P:
            raise RuntimeError(f"`{n}` must have one element per Gaussian")
    return stats


@torch.no_grad()
def add_densification_stats(model, viewspace_point_tensor, update_filter=None, radii=None):
    """GaussianModel.add_densification_stats for one view, in place, as one launch with no host read-back (upstream's boolean-mask
    indexing blocks the host once per statement).  `viewspace_point_tensor`: the rasterizer's means2D input after backward (its
    `.grad` is read) or the [P,3] gradient itself.  `update_filter`: bool / uint8 [P], or None = `radii > 0`.  With `radii` (int32
    [P]) the same launch also does train.py:186's `max_radii2D = max(max_radii2D, radii)` on the visible rows."""
    g = viewspace_point_tensor.grad if viewspace_point_tensor.grad is not None else viewspace_point_tensor
    P = model.xyz_gradient_accum.shape[0]
    g = _rows(g, "viewspace_point_tensor.grad", P)
    if g.dim() != 2 or g.size(1) != 3:
        raise RuntimeError("`viewspace_point_tensor.grad` must be (P,3)")
    if update_filter is None and radii is None:
        raise RuntimeError("add_densification_stats needs `update_filter` or `radii`")
    mask = None
    if update_filter is not None:
        if update_filter.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError("`update_filter` must be a bool or uint8 mask")
        mask = _rows(update_filter, "update_filter", P, update_filter.dtype).view(torch.uint8)
    rad = None if radii is None else _rows(radii, "radii", P, torch.int32)
    mr = None if radii is None else _rows(model.max_radii2D, "max_radii2D", P)
    _call("radegs_densify_stats", g.device, P, g, rad, mask, *_stat_rows(model, P), mr)


@torch.no_grad()
def add_reduced_densification_stats(model, densify_stats, radii_max=None):
    """The same update from the statistics view_parallel hands out already reduced over the ranks
    (`FactoredGradExchange(...)["densify_stats"]` [P,3]: sum |grad xy|, sum |grad abs|, number of ranks that saw the Gaussian, and
    `["radii_max"]` int32 [P]).  xyz_gradient_accum_abs_max takes the max with the summed column."""
    P = model.xyz_gradient_accum.shape[0]
    st = _rows(densify_stats, "densify_stats", P)
    if st.dim() != 2 or st.size(1) != 3:
        raise RuntimeError("`densify_stats` must be (P,3)")
    rad = None if radii_max is None else _rows(radii_max, "radii_max", P, torch.int32)
    mr = None if radii_max is None else _rows(model.max_radii2D, "max_radii2D", P)
    _call("radegs_densify_stats_reduced", st.device, P, st, rad, *_stat_rows(model, P), mr)


def densify_plan(accum, accum_abs, denom, scaling_raw, opacity_raw, max_grad, abs_threshold, dense_threshold, min_opacity, big_threshold=None):
    """radegs_densify_plan: returns (workspace, counts) -- counts is a DEVICE int32[4] = rows out, clone-selected, split-selected,
    pruned; `abs_threshold` a device scalar.  Nothing is read back."""
    P = scaling_raw.shape[0]
    dev = scaling_raw.device
    for t, n in ((accum, "accum"), (accum_abs, "accum_abs"), (denom, "denom"), (scaling_raw, "_scaling"), (opacity_raw, "_opacity")):
        _rows(t, n, P)
    _C._require_gpu(abs_threshold, "abs_threshold")
    if abs_threshold.dtype != torch.float32 or abs_threshold.numel() != 1:
        raise RuntimeError("`abs_threshold` must be one float32 on the GPU")
    nbytes = _lib().radegs_densify_plan_bytes(P)
    ws = gh.workspace(nbytes, dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    _call("radegs_densify_plan", dev, P, accum, accum_abs, denom, scaling_raw, opacity_raw, float(max_grad), abs_threshold, float(dense_threshold),
          float(min_opacity), int(big_threshold is not None), float(big_threshold or 0.0), ws, nbytes, counts)
    return ws, counts


def densify_apply(workspace, P_out, params, exp_avg, exp_avg_sq, unit_normals):
    """radegs_densify_apply: `params` the six parameter tensors in upstream's order (xyz, f_dc, f_rest, opacity, scaling, rotation),
    `exp_avg` / `exp_avg_sq` six tensors or None each.  Returns three lists of new tensors with P_out rows (None where None came in)."""
    P = params[0].shape[0]
    dev = params[0].device
    t = RadegsDensifyTensors()
    outs = []
    for j, group in enumerate((params, exp_avg, exp_avg_sq)):
        res = []
        for k, x in enumerate(group):
            if x is None:
                if j == 0:
                    raise RuntimeError("densify_apply needs all six parameter tensors")
                res.append(None)
                continue
            _rows(x, _DENSIFY_PARAMS[k][1], P)
            if x.shape != params[k].shape:
                raise RuntimeError(f"moment of `{_DENSIFY_PARAMS[k][1]}` does not have its parameter's shape")
            o = torch.empty((P_out,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
            if x.numel() and o.numel():
                t.inp[6 * j + k], t.out[6 * j + k] = x.data_ptr(), o.data_ptr()
            res.append(o)
        outs.append(res)
    widths = [x[0].numel() if P else 0 for x in params]
    if P and [widths[k] for k in (0, 1, 3, 4, 5)] != [3, 3, 1, 3, 4]:
        raise RuntimeError("parameter shapes must be xyz (P,3), f_dc (P,1,3), f_rest (P,M,3), opacity (P,1), scaling (P,3), rotation (P,4)")
    if P_out:
        z = _rows(unit_normals, "unit_normals", P)
        if tuple(z.shape) != (P, 3, 3):
            raise RuntimeError("`unit_normals` must be (P,3,3)")
        _call("radegs_densify_apply", dev, P, P_out, widths[2], ctypes.byref(t), z, workspace)
    return outs


@torch.no_grad()
def densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, unit_normals=None):
    """GaussianModel.densify_and_prune: clone, split, prune and the final prune as one plan, ONE host read (the new row count) and one
    pass that writes the six parameters and their twelve Adam moments at their final size; upstream rewrites them four times.
    Returns upstream's tuple (cloned, split, pruned).  `unit_normals` [P,3,3]: the standard-normal draws upstream takes from
    torch.normal (slot 0 the clone's, 1 / 2 the split children's, by source row); drawn with torch.randn when None.
    As upstream, the `max_radii2D > max_screen_size` prune never fires (densification_postfix zeroes max_radii2D before the prune
    reads it): `max_screen_size` only switches the world-size prune on.  `filter_3D` is left to the caller (train.py:196-199)."""
    params = [getattr(model, a) for _, a in _DENSIFY_PARAMS]
    P = params[0].shape[0]
    dev = params[0].device
    for (_, a), p in zip(_DENSIFY_PARAMS, params):
        _rows(p, a, P)
    if P == 0:
        return 0, 0, 0
    groups = {g["name"]: g for g in model.optimizer.param_groups if g.get("name") in dict(_DENSIFY_PARAMS)}
    states = []
    for (name, a), p in zip(_DENSIFY_PARAMS, params):
        if name not in groups or len(groups[name]["params"]) != 1 or groups[name]["params"][0] is not p:
            raise RuntimeError(f"optimizer group `{name}` must hold exactly the model's `{a}`")
        states.append(model.optimizer.state.get(p, None) or None)
    accum, accum_abs, denom = (_rows(getattr(model, n), n, P) for n in ("xyz_gradient_accum", "xyz_gradient_accum_abs", "denom"))
    # Q as upstream computes it, on the device: no host read
    grads = accum / denom
    grads = torch.where(grads.isnan(), torch.zeros_like(grads), grads)                  # not `x[mask] = 0`: that is a nonzero() and a host wait
    grads_abs = accum_abs / denom
    grads_abs = torch.where(grads_abs.isnan(), torch.zeros_like(grads_abs), grads_abs)
    ratio = (torch.norm(grads, dim=-1) >= max_grad).float().mean()
    Q = torch.quantile(grads_abs.reshape(-1), 1 - ratio)
    ws, counts = densify_plan(accum, accum_abs, denom, model._scaling, model._opacity, max_grad, Q, model.percent_dense * extent, min_opacity,
                              0.1 * extent if max_screen_size else None)
    P_out, cloned, split, pruned = counts.tolist()          # the one host read
    if unit_normals is None:
        unit_normals = torch.randn((P, 3, 3), dtype=torch.float32, device=dev)
    new_p, new_m, new_v = densify_apply(ws, P_out, [p.data for p in params], [s["exp_avg"] if s else None for s in states],
                                        [s["exp_avg_sq"] if s else None for s in states], unit_normals)
    for k, (name, a) in enumerate(_DENSIFY_PARAMS):
        group, old = groups[name], params[k]
        new = torch.nn.Parameter(new_p[k].requires_grad_(True))
        if states[k] is not None:
            st = states[k]
            st["exp_avg"], st["exp_avg_sq"] = new_m[k], new_v[k]
            del model.optimizer.state[old]
            model.optimizer.state[new] = st
        group["params"][0] = new
        setattr(model, a, new)
    for n in _STATS:
        setattr(model, n, torch.zeros((P_out, 1), dtype=torch.float32, device=dev))
    model.max_radii2D = torch.zeros((P_out,), dtype=torch.float32, device=dev)
    return cloned, split, pruned


def patch_gaussian_model(cls, appearance_network=False):
    """Installs the two functions above on the reference's GaussianModel class under upstream's method names and signatures, so that
    train.py's `gaussians.add_densification_stats(viewspace_point_tensor, visibility_filter)` and
    `gaussians.densify_and_prune(max_grad, min_opacity, extent, size_threshold)` run on the HIP kernels.  Returns `cls`.

    appearance_network=True also wraps `training_setup`: after upstream's own has built the optimizer,
    `self.appearance_network` is replaced by appearance_network.AppearanceNetwork.adopt(...) of it -- the same Parameter objects, so the
    optimizer group keeps pointing at live parameters.

    The model's state I/O is installed by patch_gaussian_model_io below; this function leaves those four methods alone."""
    def _add_densification_stats(self, viewspace_point_tensor, update_filter):
        return add_densification_stats(self, viewspace_point_tensor, update_filter)

    def _densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
        return densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size)

    cls.add_densification_stats = _add_densification_stats
    cls.densify_and_prune = _densify_and_prune
    if appearance_network:
        from appearance_network import AppearanceNetwork
        upstream_setup = cls.training_setup

        def _training_setup(self, *args, **kwargs):
            out = upstream_setup(self, *args, **kwargs)
            self.appearance_network = AppearanceNetwork.adopt(self.appearance_network)
            return out

        cls.training_setup = _training_setup
    return cls


def patch_gaussian_model_io(cls):
    """Installs model_io's save_model_ply, load_model_ply, create_from_pcd and reset_model_opacity on the reference's
    GaussianModel class as `save_ply(path)`, `load_ply(path)`, `create_from_pcd(pcd, spatial_lr_scale)` and `reset_opacity()`: no plyfile,
    one kernel each instead of a dozen.  A function of its own, not a keyword of patch_gaussian_model: that function's signature is what its
    callers and tests know, and it touches none of these four methods.  Returns `cls`; the two compose in either order."""
    def _save_ply(self, path):
        return _model_io.save_model_ply(self, path)

    def _load_ply(self, path):
        return _model_io.load_model_ply(self, path)

    def _create_from_pcd(self, pcd, spatial_lr_scale):
        return _model_io.create_from_pcd(self, pcd, spatial_lr_scale)

    def _reset_opacity(self):
        return _model_io.reset_model_opacity(self)

    cls.save_ply, cls.load_ply, cls.create_from_pcd, cls.reset_opacity = _save_ply, _load_ply, _create_from_pcd, _reset_opacity
    return cls
