"""The image-evaluation unit (rade-gs_amd/image_eval.py, include/radegs.h "Image evaluation") in this file's own torch / NumPy words, in
float32 and float64: the 8-bit round trip, PSNR, the VGG-16 tap features and LPIPS -- and the convolution once more as a host fmaf chain in
the documented K order (libradegs_conv_chain_check.so, which build.py compiles with g++ from csrc/rg_conv_chain.h).  Also the rule the
seeded weights are drawn by: only the seed travels with the golden files."""
import ctypes
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_LIB = os.path.join(ROOT, "rade-gs_amd", "diff_gaussian_rasterization", "libradegs_conv_chain_check.so")

VGG_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512), (19, 512, 512),
             (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512))
TAP_AFTER = (1, 3, 6, 9, 12)
TAP_CHANNELS = (64, 128, 256, 512, 512)
MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)
U = 2.0 ** -24


# ------------------------------------------------------------------------- seeded weights -------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def seeded_weights(seed):
    """(vgg state dict under torchvision's keys, lin state dict under the original LPIPS keys), float32, drawn from default_rng(seed) in this
    order: per convolution the He-scaled weight, standard_normal * sqrt(2 / (9 Cin)), then the bias, uniform(-0.05, 0.05); then per tap the
    non-negative linear head, uniform(0, 2 / C)."""
    rng = np.random.default_rng(seed)
    vgg, lin = {}, {}
    for idx, cin, cout in VGG_CONVS:
        vgg[f"features.{idx}.weight"] = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32))
        vgg[f"features.{idx}.bias"] = torch.from_numpy(rng.uniform(-0.05, 0.05, cout).astype(np.float32))
    for k, c in enumerate(TAP_CHANNELS):
        lin[f"lin{k}.model.1.weight"] = torch.from_numpy(rng.uniform(0.0, 2.0 / c, (1, c, 1, 1)).astype(np.float32))
    return vgg, lin


def image_pair(seed, H, W):
    """two (1,3,H,W) float32 images in [0,1]: smooth structure plus noise, the second a disturbed copy of the first"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([0.5 + 0.4 * np.sin(0.31 * xx + 0.17 * yy + c) * np.cos(0.23 * yy - 0.05 * xx * c) for c in range(3)])
    a = np.clip(base + 0.05 * rng.standard_normal(base.shape), 0, 1)
    b = np.clip(a + 0.08 * rng.standard_normal(base.shape) + 0.03, 0, 1)
    return a[None].astype(np.float32), b[None].astype(np.float32)


# -------------------------------------------------------------------- quantise, PSNR ---------------------------------------------------------------------
def quantize_u8(x):
    """(3,H,W) float32 -> (H,W,3) uint8: trunc(clamp(x * 255 + 0.5, 0, 255)), float32 with one rounding per operation; NaN -> 0"""
    x = np.asarray(x, np.float32)
    t = x * np.float32(255.0)
    t = t + np.float32(0.5)
    t = np.where(t >= 0, np.minimum(t, np.float32(255.0)), np.float32(0.0))     # NaN fails t >= 0
    return np.ascontiguousarray(np.moveaxis(t.astype(np.int32).astype(np.uint8), 0, 2))


def quantize(x):
    """what the saved image reads back as: u8 / 255 in float32, (3,H,W)"""
    return np.moveaxis(quantize_u8(x), 2, 0).astype(np.float32) / np.float32(255.0)


def mse(a, b, dtype=torch.float64):
    a, b = torch.as_tensor(a).to(dtype), torch.as_tensor(b).to(dtype)
    return ((a - b) ** 2).reshape(-1).mean()


def psnr(a, b, dtype=torch.float64):
    return 20 * torch.log10(1.0 / torch.sqrt(mse(a, b, dtype)))


# ---------------------------------------------------------------------- VGG taps, LPIPS ----------------------------------------------------------------------
def vgg_features(x, vgg, dtype=torch.float64):
    """the five tapped ReLU maps (before normalisation) of a (1,3,H,W) image"""
    x = torch.as_tensor(x).to(dtype)
    mean, std = torch.tensor(MEAN, dtype=torch.float32).to(dtype).view(1, 3, 1, 1), torch.tensor(STD, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    x = (x - mean) / std
    out = []
    for k, (idx, _, _) in enumerate(VGG_CONVS):
        x = F.relu(F.conv2d(x, vgg[f"features.{idx}.weight"].to(dtype), vgg[f"features.{idx}.bias"].to(dtype), padding=1))
        if k in TAP_AFTER:
            out.append(x)
            if len(out) < 5:
                x = F.max_pool2d(x, 2)
    return out


def tap_term(fx, fy, lin, dtype=torch.float64):
    """one layer's scalar from two (1,C,H,W) maps and the (C,) head"""
    fx, fy, lin = fx.to(dtype), fy.to(dtype), torch.as_tensor(lin).to(dtype).reshape(1, -1, 1, 1)
    eps = 1e-10       # a Python scalar as in the reference: rounded to the tensor's type when added
    nx = fx / (torch.sqrt((fx ** 2).sum(1, keepdim=True)) + eps)
    ny = fy / (torch.sqrt((fy ** 2).sum(1, keepdim=True)) + eps)
    return (lin * (nx - ny) ** 2).sum(1).mean()


def lpips_layers(x, y, vgg, lin, dtype=torch.float64):
    """(five layer scalars, their sum) as a float64 array"""
    fx, fy = vgg_features(x, vgg, dtype), vgg_features(y, vgg, dtype)
    layers = [tap_term(a, b, lin[f"lin{k}.model.1.weight"], dtype) for k, (a, b) in enumerate(zip(fx, fy))]
    total = layers[0]
    for v in layers[1:]:
        total = total + v
    return np.array([float(v) for v in layers] + [float(total)], np.float64)


# ----------------------------------------------------------------------- the host chain -----------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _chain_lib():
    if not os.path.exists(CHAIN_LIB):
        raise RuntimeError(f"{CHAIN_LIB} is missing: build it with `python rade-gs_amd/build.py`")
    L = ctypes.CDLL(CHAIN_LIB)
    L.radegs_conv_chain_host.restype = ctypes.c_int
    L.radegs_conv_chain_host.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p]
    return L


def chain_conv(x, weight, bias, relu=True):
    """x channels-last (N,H,W,Cin) float32, weight (Cout,Cin,3,3), bias (Cout,): the fmaf chain of csrc/rg_conv_chain.h on the host,
    channels-last (N,H,W,Cout)"""
    x, w, b = (np.ascontiguousarray(np.asarray(t, np.float32)) for t in (x, weight, bias))
    N, H, W, cin = x.shape
    cout = w.shape[0]
    assert w.shape == (cout, cin, 3, 3) and b.shape == (cout,)
    y = np.empty((N, H, W, cout), np.float32)
    rc = _chain_lib().radegs_conv_chain_host(N, H, W, cin, cout, x.ctypes.data, w.ctypes.data, b.ctypes.data, int(relu), y.ctypes.data)
    assert rc == 0
    return y


def zscore_channels_last(image):
    """a planar (N,3,H,W) float32 image -> the first layer's input, (x - mean) / std in float32, channels-last"""
    x = np.asarray(image, np.float32)
    z = (x - np.array(MEAN, np.float32).reshape(1, 3, 1, 1)) / np.array(STD, np.float32).reshape(1, 3, 1, 1)
    return np.ascontiguousarray(np.moveaxis(z, 1, 3))


def conv_f64(x, weight, bias):
    """the same layer in float64 with torch: (N,H,W,Cout), and sum |w||x| per output for the bound"""
    xt = torch.from_numpy(np.moveaxis(np.asarray(x, np.float64), 3, 1).copy())
    wt, bt = torch.from_numpy(np.asarray(weight, np.float64)), torch.from_numpy(np.asarray(bias, np.float64))
    y = F.relu(F.conv2d(xt, wt, bt, padding=1)).permute(0, 2, 3, 1).numpy()
    mag = F.conv2d(xt.abs(), wt.abs(), None, padding=1).permute(0, 2, 3, 1).numpy()
    return y, mag


def chain_bound(mag, result, cin):
    """|err| <= gamma_K * sum |w||x| + one ulp of the result, gamma_K = K u / (1 - K u), u = 2^-24, K = 9 Cin + 1"""
    K = 9 * cin + 1
    gamma = K * U / (1 - K * U)
    return gamma * mag + np.spacing(np.abs(np.asarray(result, np.float32))).astype(np.float64)
