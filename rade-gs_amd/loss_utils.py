"""HIP-backed mirror of the reference's photometric loss:

    l1_loss(network_output, gt)        utils/loss_utils.py:17-18
    ssim(img1, img2)                   utils/loss_utils.py:31-63   (window 11, size_average=True)
    photometric_loss(image, gt, lambda_dssim)  =  (1-l)*l1_loss + l*(1-ssim)     train.py:159, fused

(C,H,W) float32 GPU tensors; `gt` may carry a leading batch dimension of 1 as train.py passes it.  Differentiable
w.r.t. the first argument only (the ground-truth image is data).  One tiled kernel per direction through
libradegs_hip.so (radegs_photometric_*).  GPU only: there is no CPU path.

And of the decoupled appearance loss:

    l1_loss_appearance(image, gt_image, gaussians, view_idx, return_transformed_image=False)       train.py:37-58

with the appearance network's trunk (conv1 and the four pixel-shuffle blocks, at most half resolution) in torch and everything at
full resolution in the HIP head kernels (radegs_appearance_*)."""
import ctypes
import functools

import torch

import geom_host as gh
import image_eval
from diff_gaussian_rasterization import _C

_I, _VP, _SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
_SIGNATURES = {
    "radegs_photometric_scratch_bytes": (_SZ, [_I, _I, _I]),
    "radegs_photometric_forward": (_I, [_I, _I, _I, _VP, _VP, ctypes.c_float, _VP, _VP, _VP, _VP]),
    "radegs_photometric_backward": (_I, [_I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "radegs_appearance_downsample_forward": (_I, [_I, _I, _VP, _VP, _VP]),
    "radegs_appearance_downsample_backward": (_I, [_I, _I, _VP, _VP, _VP]),
    "radegs_appearance_head_scratch_bytes": (_SZ, [_I, _I, _I]),
    "radegs_appearance_head_forward": (_I, [_I] * 4 + [_VP] * 8 + [_SZ, _VP, _VP, _VP]),
    "radegs_appearance_head_backward": (_I, [_I] * 4 + [_VP] * 9 + [_SZ] + [_VP] * 7),
    **image_eval.SIGNATURES,      # the evaluation metrics next to the training losses; image_eval.ssim runs on the ssim below
}


def _lib():
    return _C.bind(_SIGNATURES)


_call = functools.partial(gh.call, _SIGNATURES)


def _prep(img, gt):
    _C._require_gpu(img, "image")
    _C._require_gpu(gt, "gt")
    if gt.dim() == img.dim() + 1 and gt.size(0) == 1:
        gt = gt[0]
    if img.dim() != 3 or gt.shape != img.shape:
        raise RuntimeError(f"image and gt must both be (C,H,W); got {tuple(img.shape)} and {tuple(gt.shape)}")
    if img.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError("image and gt must be float32")
    return img.contiguous(), gt.contiguous()


class _Photometric(torch.autograd.Function):
    """returns (loss, l1, ssim); the backward folds the three upstream gradients into two coefficients"""

    @staticmethod
    def forward(ctx, image, gt, lambda_dssim):
        a, b = _prep(image, gt)
        C, H, W = a.shape
        dev = a.device
        need = ctx.needs_input_grad[0]
        scratch = gh.workspace(_lib().radegs_photometric_scratch_bytes(W, H, C), dev)
        dmaps = torch.empty((3, C, H, W), dtype=torch.float32, device=dev) if need else None
        out = torch.empty(3, dtype=torch.float32, device=dev)
        _call("radegs_photometric_forward", dev, W, H, C, a, b, float(lambda_dssim), scratch, dmaps, out)
        ctx.lam = float(lambda_dssim)
        ctx.save_for_backward(a, b, dmaps)
        ctx.mark_non_differentiable()
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_loss, g_l1, g_ssim):
        a, b, dmaps = ctx.saved_tensors
        coef = torch.stack([g_loss * (1.0 - ctx.lam) + g_l1, g_ssim - g_loss * ctx.lam]).to(torch.float32).contiguous()
        grad = torch.empty_like(a)
        C, H, W = a.shape
        _call("radegs_photometric_backward", a.device, W, H, C, a, b, dmaps, coef, grad)
        return grad, None, None


def photometric_loss(image, gt, lambda_dssim=0.2):
    """(1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt)) -- train.py:159."""
    return _Photometric.apply(image, gt, lambda_dssim)[0]


def l1_loss(network_output, gt):
    return _Photometric.apply(network_output, gt, 0.0)[1]


def ssim(img1, img2, window_size=11, size_average=True):
    if window_size != 11 or not size_average:
        raise NotImplementedError("only the configuration train.py uses (window_size=11, size_average=True) is built")
    return _Photometric.apply(img1, img2, 1.0)[2]


# ---- decoupled appearance loss (train.py:37-58) ----
def _appearance_image(t, name):
    _C._require_gpu(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"`{name}` must be float32")
    if t.dim() != 3 or t.size(0) != 3:
        raise RuntimeError(f"`{name}` must be (3,H,W); got {tuple(t.shape)}")
    if t.size(1) < 32 or t.size(2) < 32:
        raise RuntimeError(f"`{name}` is {t.size(1)}x{t.size(2)}: the centre crop to multiples of 32 would be empty")
    return t.contiguous()


def appearance_crop(origH, origW):
    """(H, W, top, left) of train.py:40-44's centre crop"""
    H, W = origH // 32 * 32, origW // 32 * 32
    return H, W, origH // 2 - H // 2, origW // 2 - W // 2


class _AppearanceDownsample(torch.autograd.Function):
    """[3,origH,origW] -> [3,H/32,W/32]: the bilinear (align_corners=True) resize of the centre crop"""

    @staticmethod
    def forward(ctx, image):
        a = _appearance_image(image, "image")
        H, W, _, _ = appearance_crop(a.size(1), a.size(2))
        down = torch.empty((3, H // 32, W // 32), dtype=torch.float32, device=a.device)
        _call("radegs_appearance_downsample_forward", a.device, a.size(1), a.size(2), a, down)
        ctx.shape = tuple(a.shape)
        return down

    @staticmethod
    def backward(ctx, g_down):
        g = g_down.to(torch.float32).contiguous()
        grad = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        _call("radegs_appearance_downsample_backward", g.device, ctx.shape[1], ctx.shape[2], g, grad)
        return grad


def _head_args(feat, image, gt, W2, b2, W3, b3):
    a, b = _appearance_image(image, "image"), _appearance_image(gt, "gt_image")
    if a.shape != b.shape:
        raise RuntimeError(f"image and gt_image must have the same shape; got {tuple(a.shape)} and {tuple(b.shape)}")
    H, W, _, _ = appearance_crop(a.size(1), a.size(2))
    for t, name, shape in ((feat, "features", (16, H // 2, W // 2)), (W2, "conv2.weight", (16, 16, 3, 3)), (b2, "conv2.bias", (16,)),
                           (W3, "conv3.weight", (3, 16, 3, 3)), (b3, "conv3.bias", (3,))):
        _C._require_gpu(t, name)
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise RuntimeError(f"`{name}` must be float32 of shape {shape}; got {t.dtype} {tuple(t.shape)}")
    return [feat.contiguous(), a, b, W2.contiguous(), b2.contiguous(), W3.contiguous(), b3.contiguous()]


def _head_forward(args, want_transformed):
    feat, a = args[0], args[1]
    dev = feat.device
    nbytes = _lib().radegs_appearance_head_scratch_bytes(a.size(1), a.size(2), 0)
    scratch = gh.workspace(nbytes, dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    out = torch.empty((3, 2 * feat.size(1), 2 * feat.size(2)), dtype=torch.float32, device=dev) if want_transformed else None
    _call("radegs_appearance_head_forward", dev, a.size(1), a.size(2), feat.size(1), feat.size(2), *args, scratch, nbytes, loss, out)
    return loss[0], out


class _AppearanceHead(torch.autograd.Function):
    """loss = mean |sigmoid(conv3(relu(conv2(bilinear x2 (features))))) * crop(image) - crop(gt)|; differentiable w.r.t. the features, the
    image and the four parameter tensors.  The gradient of `image` is the full-size tensor, zero outside the crop."""

    @staticmethod
    def forward(ctx, feat, image, gt, W2, b2, W3, b3):
        args = _head_args(feat, image, gt, W2, b2, W3, b3)
        loss, _ = _head_forward(args, False)
        ctx.save_for_backward(*args)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        args = ctx.saved_tensors
        feat, a = args[0], args[1]
        dev = feat.device
        g = g_loss.to(torch.float32).reshape(1).contiguous()
        nbytes = _lib().radegs_appearance_head_scratch_bytes(a.size(1), a.size(2), 1)
        scratch = gh.workspace(nbytes, dev)
        grads = [torch.empty_like(t) for t in (feat, a, args[3], args[4], args[5], args[6])]
        _call("radegs_appearance_head_backward", dev, a.size(1), a.size(2), feat.size(1), feat.size(2), *args, g, scratch, nbytes, *grads)
        return grads[0], grads[1], None, grads[2], grads[3], grads[4], grads[5]


def appearance_downsample(image):
    return _AppearanceDownsample.apply(image)


def appearance_head_loss(features, image, gt_image, conv2_weight, conv2_bias, conv3_weight, conv3_bias):
    return _AppearanceHead.apply(features, image, gt_image, conv2_weight, conv2_bias, conv3_weight, conv3_bias)


def _appearance_layers(net):
    """the seven convolutions of an appearance network (ours or the reference's own class), reached by attribute"""
    import torch.nn as nn
    convs = [net.conv1, net.up1.conv, net.up2.conv, net.up3.conv, net.up4.conv, net.conv2, net.conv3]
    for c, cin, cout in ((convs[5], 16, 16), (convs[6], 16, 3)):
        if not (isinstance(c, nn.Conv2d) and tuple(c.kernel_size) == (3, 3) and tuple(c.padding) == (1, 1) and tuple(c.stride) == (1, 1)
                and tuple(c.dilation) == (1, 1) and c.groups == 1 and c.in_channels == cin and c.out_channels == cout and c.bias is not None
                and c.padding_mode == "zeros"):
            raise NotImplementedError("the fused appearance head is built for conv2 = 3x3 16->16 and conv3 = 3x3 16->3, padding 1, with bias; "
                                      f"got {c}")
    return convs


def l1_loss_appearance(image, gt_image, gaussians, view_idx, return_transformed_image=False):
    """train.py:37-58's L1_loss_appearance: same arguments and result.  Reads `gaussians.get_apperance_embedding(view_idx)` (upstream's
    spelling) and `gaussians.appearance_network` (appearance_network.AppearanceNetwork or the reference's class).  The inference branch
    (`return_transformed_image=True`) is supported under torch.no_grad() only."""
    net = gaussians.appearance_network
    convs = _appearance_layers(net)
    image, gt_image = _appearance_image(image, "image"), _appearance_image(gt_image, "gt_image")
    if return_transformed_image and torch.is_grad_enabled():
        raise RuntimeError("l1_loss_appearance(return_transformed_image=True) is the inference branch: call it under torch.no_grad()")
    embedding = gaussians.get_apperance_embedding(view_idx)
    origH, origW = image.shape[1:]
    H, W, _, _ = appearance_crop(origH, origW)
    down = _AppearanceDownsample.apply(image)
    x = torch.cat([down, embedding[None].repeat(H // 32, W // 32, 1).permute(2, 0, 1)], dim=0)[None]
    x = torch.relu(convs[0](x))
    for blk in (net.up1, net.up2, net.up3, net.up4):
        x = blk(x)
    feat = x[0]
    w = (convs[5].weight, convs[5].bias, convs[6].weight, convs[6].bias)
    if not return_transformed_image:
        return _AppearanceHead.apply(feat, image, gt_image, *w)
    _, transformed = _head_forward(_head_args(feat, image, gt_image, *w), True)
    return torch.nn.functional.interpolate(transformed[None], size=(origH, origW), mode="bilinear", align_corners=True)[0]
