"""HIP-backed image-quality evaluation: the novel-view numbers of render.py -> metric.py -- the 8-bit round trip of a saved
render (torchvision's save_image -> PNG -> to_tensor), utils/image_utils.py:17-19 psnr, utils/loss_utils.py ssim on the (1,3,H,W) pairs
metric.py hands it, and lpipsPyTorch's LPIPS with the VGG-16 trunk.  GPU only, float32, every cross-thread sum in a fixed order: two calls
return the same bits.  The thirteen convolutions run on the f32-input MFMA, one fmaf chain per output element (csrc/rg_conv_chain.h).
Weights are read from files the caller provides; nothing is ever fetched.  include/radegs.h, "Image evaluation", is the specification and
tests/imageeval_restatement.py restates it in torch and NumPy.  torchvision is not readable where this was written: the rounding rule of
save_image and the division of to_tensor are from memory of its source."""
import ctypes
import functools
import json
import os

import torch

import geom_host as gh
from diff_gaussian_rasterization import _C
from geom_host import i32, ll, sz, vp

SIGNATURES = {
    "radegs_imageeval_conv3x3": (i32, [i32] * 5 + [vp] * 5),
    "radegs_imageeval_conv3x3_first": (i32, [i32] * 4 + [vp, gh.pf32, gh.pf32, vp, vp, vp, vp]),
    "radegs_imageeval_tap_bytes": (sz, [i32, i32]),
    "radegs_imageeval_tap": (i32, [i32, i32, i32, vp, vp, vp, vp, sz, vp, vp]),
    "radegs_imageeval_quantize": (i32, [i32, i32, vp, vp, vp, vp]),
    "radegs_imageeval_ssd_bytes": (sz, []),
    "radegs_imageeval_ssd": (i32, [ll, vp, vp, vp, sz, vp, vp]),
}
_SIGNATURES = SIGNATURES

# torchvision's vgg16().features: index of each convolution, its channels, and the convolutions a tap follows (relu1_2, 2_2, 3_3, 4_3, 5_3)
VGG_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512), (19, 512, 512),
             (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
TAP_AFTER = (1, 3, 6, 9, 12)
TAP_CHANNELS = (64, 128, 256, 512, 512)
MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)      # lpipsPyTorch/modules/networks.py:41-44
MIN_SIDE = 16                                              # below it the fourth pool of the reference leaves an empty map
VGG_FILES, LIN_FILES = ("vgg16-397923af.pth", "vgg16.pth"), ("vgg.pth", "lpips_vgg.pth")
WEIGHTS_ENV = "RADEGS_LPIPS_WEIGHTS"
_CHUNK, _BN = 16, 64                                        # csrc/rg_conv_chain.h kChunk, radegs_imageeval.hip kBN

_ACT_SCRATCH = _C._ScratchCache(zeroed=False)               # the trunk's two activation buffers and the tap workspace, per (device, stream)


def _lib():
    return gh.bind(_SIGNATURES)


_call = functools.partial(gh.call, _SIGNATURES)


def _align(n):
    return (int(n) + 255) & ~255


def _image(t, name):
    """a contiguous float32 (3,H,W) GPU view of a (3,H,W) or (1,3,H,W) tensor"""
    _C._require_gpu(t, name)
    if t.dim() == 4 and t.size(0) == 1:
        t = t[0]
    if t.dim() != 3 or t.size(0) != 3:
        raise RuntimeError(f"`{name}` must be (3,H,W) or (1,3,H,W), got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"`{name}` must be float32")
    return t.detach().contiguous()


def _pair(a, b):
    a, b = _image(a, "a"), _image(b, "b")
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f"the two images differ in shape or device: {tuple(a.shape)} and {tuple(b.shape)}")
    return a, b


# ------------------------------------------------------------------- 8-bit round trip, PSNR, SSIM -------------------------------------------------------------------
def _quantize(image, want_u8, want_float):
    x = _image(image, "image")
    dev, (_, H, W) = x.device, x.shape
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    out = torch.empty_like(x) if want_float else None
    _call("radegs_imageeval_quantize", dev, H, W, x, u8, out)
    return u8, out


@torch.no_grad()
def quantize(image):
    """What an image reads back as after save_image -> PNG -> to_tensor: trunc(clamp(x * 255 + 0.5, 0, 255)) / 255, in the input's shape."""
    out = _quantize(image, False, True)[1]
    return out.view(image.shape)


@torch.no_grad()
def to_uint8(image):
    """The (H,W,3) uint8 image save_image writes."""
    return _quantize(image, True, False)[0]


@torch.no_grad()
def psnr(a, b):
    """utils/image_utils.py:17-19 on a (1,3,H,W) pair: (1,1), 20 log10(1 / sqrt(mse)); identical images give inf."""
    a, b = _pair(a, b)
    dev, n = a.device, a.numel()
    nbytes = _lib().radegs_imageeval_ssd_bytes()
    ws, out = gh.workspace(nbytes, dev), torch.empty(1, dtype=torch.float64, device=dev)
    _call("radegs_imageeval_ssd", dev, n, a, b, ws, nbytes, out)
    mse = (out / n).to(torch.float32).view(1, 1)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def ssim(a, b):
    """loss_utils.ssim (window 11, mean) on a (1,3,H,W) or (3,H,W) pair."""
    import loss_utils
    a, b = _pair(a, b)
    return loss_utils.ssim(a, b)


# ------------------------------------------------------------------------------ weights ------------------------------------------------------------------------------
def _vgg_state(state):
    """{conv position 0..12: (weight [Cout,Cin,3,3], bias [Cout])} from torchvision's vgg16 keys; classifier keys are ignored"""
    out = {}
    for k, (idx, cin, cout) in enumerate(VGG_CONVS):
        w, b = state.get(f"features.{idx}.weight"), state.get(f"features.{idx}.bias")
        if w is None or b is None:
            raise KeyError(f"the VGG-16 state dict lacks features.{idx}.weight / .bias")
        if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
            raise ValueError(f"features.{idx}: expected {(cout, cin, 3, 3)} and {(cout,)}, got {tuple(w.shape)} and {tuple(b.shape)}")
        out[k] = (w.detach().to(torch.float32), b.detach().to(torch.float32))
    return out


def _lin_state(state):
    """[five (C,) tensors] from the original LPIPS keys (lin{k}.model.1.weight) or the reference's renamed ones ({k}.1.weight)"""
    out = []
    for k, c in enumerate(TAP_CHANNELS):
        w = state.get(f"lin{k}.model.1.weight")
        if w is None:
            w = state.get(f"{k}.1.weight")
        if w is None:
            raise KeyError(f"the LPIPS state dict lacks lin{k}.model.1.weight / {k}.1.weight")
        if w.numel() != c:
            raise ValueError(f"lin{k}: expected {c} weights, got {tuple(w.shape)}")
        out.append(w.detach().to(torch.float32).reshape(c))
    return out


def _find(directory, names):
    for n in names:
        p = os.path.join(directory, n)
        if os.path.isfile(p):
            return p
    return None


def load_lpips_weights(vgg_path=None, lin_path=None):
    """(vgg_state, lin_state) for LPIPS(...), read with torch.load(weights_only=True) from the two paths or, for a path not given, from the
    directory RADEGS_LPIPS_WEIGHTS names (vgg16-397923af.pth or vgg16.pth: torchvision's VGG-16; vgg.pth or lpips_vgg.pth: the LPIPS v0.1
    linear heads).  A missing file is an error that names both; nothing is downloaded."""
    directory = os.environ.get(WEIGHTS_ENV)
    if directory:
        vgg_path = vgg_path or _find(directory, VGG_FILES)
        lin_path = lin_path or _find(directory, LIN_FILES)
    if not vgg_path or not lin_path or not os.path.isfile(vgg_path) or not os.path.isfile(lin_path):
        raise FileNotFoundError(
            "LPIPS needs two weight files and neither is ever downloaded: torchvision's VGG-16 state dict "
            f"({' or '.join(VGG_FILES)}; got {vgg_path!r}) and the LPIPS v0.1 VGG linear heads ({' or '.join(LIN_FILES)}; got {lin_path!r}).  "
            f"Pass both paths or set {WEIGHTS_ENV} to the directory that holds them (now {directory!r}).")
    vgg = torch.load(vgg_path, map_location="cpu", weights_only=True)
    lin = torch.load(lin_path, map_location="cpu", weights_only=True)
    _vgg_state(vgg), _lin_state(lin)      # refuse a wrong file here, by name
    return vgg, lin


def _pack(w):
    """the order the kernels read (include/radegs.h): first layer (Cin = 3) [tap][ci][co]; others [co / 64][ci / 16][tap][ci % 16][co % 64]"""
    cout, cin = w.shape[:2]
    if cin == 3:
        return w.permute(2, 3, 1, 0).reshape(27, cout).contiguous()
    return w.reshape(cout // _BN, _BN, cin // _CHUNK, _CHUNK, 9).permute(0, 2, 4, 3, 1).contiguous()


# ------------------------------------------------------------------------------- kernels -------------------------------------------------------------------------------
def _conv(dev, N, H, W, cin, cout, src, packed, bias, dst, mean=MEAN, std=STD):
    """one layer into dst; Cin = 3 is the first layer: src is the planar image, z-scored on load"""
    if cin == 3:
        mean, std = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        _call("radegs_imageeval_conv3x3_first", dev, N, H, W, cout, src, mean, std, packed, bias, dst)
    else:
        _call("radegs_imageeval_conv3x3", dev, N, H, W, cin, cout, src, packed, bias, dst)


def _tap(dev, H, W, C, feat, lin, pooled, ws, ws_bytes, out):
    _call("radegs_imageeval_tap", dev, H, W, C, feat, lin, pooled, ws, ws_bytes, out)


def _floats(buf, offset, *shape):
    n = 1
    for s in shape:
        n *= s
    return buf[offset:offset + 4 * n].view(torch.float32).view(*shape)


@torch.no_grad()
def conv3x3_relu(x, weight, bias, first=False, mean=MEAN, std=STD):
    """One layer on its own (tests, the benchmark): x channels-last (N,H,W,Cin) float32 -- or, with first=True, a planar (N,3,H,W) image that
    is z-scored with `mean` and `std` on load -- weight (Cout,Cin,3,3), bias (Cout,); returns channels-last (N,H,W,Cout)."""
    _C._require_gpu(x, "x")
    x = x.detach().contiguous()
    dev, cout, cin = x.device, weight.shape[0], weight.shape[1]
    if first != (cin == 3) or x.dim() != 4 or x.shape[1 if first else 3] != cin or x.dtype != torch.float32:
        raise RuntimeError(f"x {tuple(x.shape)} does not fit weight {tuple(weight.shape)}")
    N, H, W = (x.shape[0], x.shape[2], x.shape[3]) if first else x.shape[:3]
    packed, b = _pack(weight.detach().to(dev, torch.float32)), bias.detach().to(dev, torch.float32).contiguous()
    y = torch.empty((N, H, W, cout), dtype=torch.float32, device=dev)
    _conv(dev, N, H, W, cin, cout, x, packed, b, y, mean, std)
    return y


@torch.no_grad()
def tap_pool(feat, lin, pool=True):
    """One tap on its own (tests): feat channels-last (2,H,W,C) holding the two images' maps, lin (C,).  Returns (the layer's scalar as a
    float64 (1,) tensor, the pooled maps (2,H//2,W//2,C) or None)."""
    _C._require_gpu(feat, "feat")
    feat, dev = feat.detach().contiguous(), feat.device
    _, H, W, C = feat.shape
    if feat.shape[0] != 2 or feat.dtype != torch.float32 or lin.numel() != C:
        raise RuntimeError("`feat` must be float32 (2,H,W,C) and `lin` (C,)")
    nbytes = _lib().radegs_imageeval_tap_bytes(H, W)
    ws, out = gh.workspace(nbytes, dev), torch.empty(1, dtype=torch.float64, device=dev)
    pooled = torch.empty((2, H // 2, W // 2, C), dtype=torch.float32, device=dev) if pool else None
    _tap(dev, H, W, C, feat, lin.detach().to(dev, torch.float32).contiguous(), pooled, ws, nbytes, out)
    return out, pooled


class LPIPS:
    """lpipsPyTorch.modules.lpips.LPIPS with net_type='vgg', version '0.1', evaluation only.  vgg_state: torchvision's vgg16 state dict;
    lin_state: the LPIPS linear heads under either key spelling (load_lpips_weights returns both).  Weights are packed once per device."""

    def __init__(self, vgg_state, lin_state):
        self._convs, self._lin = _vgg_state(vgg_state), _lin_state(lin_state)
        self._packed = {}

    def to(self, device):
        return self

    def eval(self):
        return self

    def _on(self, dev):
        p = self._packed.get(dev)
        if p is None:
            p = self._packed[dev] = ([(_pack(w.to(dev)), b.to(dev).contiguous()) for _, (w, b) in sorted(self._convs.items())],
                                     [l.to(dev).contiguous() for l in self._lin])
        return p

    def _run(self, batch, want_maps=False):
        """batch (2,3,H,W) contiguous.  Returns (the five layer scalars, float64 (5,); the first image's five ReLU maps if asked for)."""
        dev, (N, _, H, W) = batch.device, batch.shape
        if H < MIN_SIDE or W < MIN_SIDE:
            raise ValueError(f"LPIPS-VGG needs H, W >= {MIN_SIDE} (the reference's fourth pool would leave an empty map), got {H}x{W}")
        convs, lins = self._on(dev)
        half, ws_bytes = _align(4 * N * H * W * 64), int(_lib().radegs_imageeval_tap_bytes(H, W))
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        out, maps = torch.empty(5, dtype=torch.float64, device=dev), []
        with _ACT_SCRATCH.lease(key, 2 * half + _align(ws_bytes), dev) as buf:
            ws = buf[2 * half:]
            src, cur, h, w, tap = batch, 0, H, W, 0
            for k, (_, cin, cout) in enumerate(VGG_CONVS):
                dst = _floats(buf, cur * half, N, h, w, cout)
                _conv(dev, N, h, w, cin, cout, src, convs[k][0], convs[k][1], dst)
                src, cur = dst, 1 - cur
                if k != TAP_AFTER[tap]:
                    continue
                last = tap == 4
                pooled = None if last else _floats(buf, cur * half, N, h // 2, w // 2, cout)
                _tap(dev, h, w, cout, src, lins[tap], pooled, ws, ws_bytes, out[tap:])
                if want_maps:
                    maps.append(src[:1].permute(0, 3, 1, 2).clone())
                if not last:
                    src, cur, h, w = pooled, 1 - cur, h // 2, w // 2
                tap += 1
        return out, maps

    @torch.no_grad()
    def forward_layers(self, x, y):
        """the five per-layer terms, float32 (5,); x and y go through the trunk as one batch of two"""
        x, y = _pair(x, y)
        return self._run(torch.stack([x, y]))[0].to(torch.float32)

    @torch.no_grad()
    def forward(self, x, y):
        layers = self.forward_layers(x, y)
        total = layers[0]
        for k in range(1, 5):
            total = total + layers[k]
        return total.view(1, 1, 1, 1)

    __call__ = forward

    @torch.no_grad()
    def features(self, x):
        """the five tapped ReLU maps (relu1_2 .. relu5_3) before normalisation, (1,C,h,w) each, for tests"""
        x = _image(x, "x")
        return self._run(torch.stack([x, x]), True)[1]


_DEFAULT = {}     # weights directory -> LPIPS read from it (an LPIPS packs once per device itself)


def default_lpips():
    """the network of the files RADEGS_LPIPS_WEIGHTS names, read once per directory"""
    directory = os.environ.get(WEIGHTS_ENV)
    net = _DEFAULT.get(directory)
    if net is None:
        net = _DEFAULT[directory] = LPIPS(*load_lpips_weights())
    return net


# ------------------------------------------------------------------------------ metric.py ------------------------------------------------------------------------------
@torch.no_grad()
def evaluate_views(renders, gts, lpips=None, names=None):
    """metric.py:67-86 on lists of (1,3,H,W) or (3,H,W) GPU images: {"SSIM", "PSNR", "LPIPS": means; "per_view": {metric: {name: value}}},
    averaged the way the reference does (torch.tensor(list).mean(), float32).  lpips: an LPIPS; None reads RADEGS_LPIPS_WEIGHTS."""
    if len(renders) != len(gts) or not renders:
        raise RuntimeError("`renders` and `gts` must be two lists of the same, non-zero length")
    net = default_lpips() if lpips is None else lpips
    names = [f"{i:05d}.png" for i in range(len(renders))] if names is None else list(names)
    ssims, psnrs, lpipss = [], [], []
    for r, g in zip(renders, gts):
        ssims.append(ssim(r, g))
        psnrs.append(psnr(r, g))
        lpipss.append(net.forward(r, g))
    res, per_view = {}, {}
    for key, vals in (("SSIM", ssims), ("PSNR", psnrs), ("LPIPS", lpipss)):
        t = torch.tensor([float(v) for v in vals])
        res[key] = t.mean().item()
        per_view[key] = dict(zip(names, t.tolist()))
    res["per_view"] = per_view
    return res


def _pil():
    try:
        from PIL import Image
    except ImportError as ex:
        raise ImportError("image_eval.render_set / evaluate read and write PNG files through Pillow (PIL), which is not installed; "
                          "quantize, psnr, ssim, LPIPS and evaluate_views need no image files") from ex
    return Image


def save_png(image, path):
    """torchvision.utils.save_image of one (3,H,W) image: the 8-bit rounding on the GPU, the PNG container by Pillow"""
    _pil().fromarray(to_uint8(image).cpu().numpy()).save(path)


def load_png(path, device="cuda"):
    """metric.py:31: to_tensor(Image.open(path))[None, :3] on `device`"""
    import numpy as np
    a = np.asarray(_pil().open(path))
    if a.ndim == 2:
        a = a[:, :, None].repeat(3, axis=2)
    # divided on the host as to_tensor does, by a true IEEE division: torch's GPU division by a scalar was seen to be one ulp off u8 / 255
    # for some of the 256 values
    planar = np.ascontiguousarray(np.moveaxis(a[:, :, :3], 2, 0)).astype(np.float32) / np.float32(255)
    return torch.from_numpy(planar).to(device).unsqueeze(0)


def render_set(model_path, name, iteration, views, render_fn):
    """render.py:24-35: writes <model_path>/<name>/ours_<iteration>/{renders,gt}/00000.png ...; render_fn(view) returns the (3,H,W) render
    (the reference's render(view, gaussians, pipeline, background, kernel_size)["render"]), view.original_image is the ground truth."""
    _pil()
    base = os.path.join(model_path, name, f"ours_{iteration}")
    render_path, gts_path = os.path.join(base, "renders"), os.path.join(base, "gt")
    os.makedirs(render_path, exist_ok=True)
    os.makedirs(gts_path, exist_ok=True)
    for idx, view in enumerate(views):
        save_png(render_fn(view), os.path.join(render_path, f"{idx:05d}.png"))
        save_png(view.original_image[0:3, :, :], os.path.join(gts_path, f"{idx:05d}.png"))


def evaluate(model_paths, lpips=None, device="cuda"):
    """metric.py:36-91: for every <scene>/test/<method>/{renders,gt} writes <scene>/results.json ({method: {"SSIM","PSNR","LPIPS"}}) and
    <scene>/per_view.json ({method: {metric: {file name: value}}}) and returns {scene: results}.  Errors are raised, not swallowed."""
    _pil()
    out = {}
    for scene_dir in model_paths:
        full, per_view = {}, {}
        test_dir = os.path.join(scene_dir, "test")
        for method in sorted(os.listdir(test_dir)):
            renders_dir, gt_dir = os.path.join(test_dir, method, "renders"), os.path.join(test_dir, method, "gt")
            names = sorted(os.listdir(renders_dir))
            renders = [load_png(os.path.join(renders_dir, n), device) for n in names]
            gts = [load_png(os.path.join(gt_dir, n), device) for n in names]
            res = evaluate_views(renders, gts, lpips, names)
            per_view[method] = res.pop("per_view")
            full[method] = res
        with open(os.path.join(scene_dir, "results.json"), "w") as fp:
            json.dump(full, fp, indent=True)
        with open(os.path.join(scene_dir, "per_view.json"), "w") as fp:
            json.dump(per_view, fp, indent=True)
        out[scene_dir] = full
    return out
