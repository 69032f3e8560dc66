"""The decoupled appearance loss written out in torch on the CPU, from the formulae of DESIGN 11 "N8" -- test infrastructure.

    crop      H = origH//32*32, W = origW//32*32, top = origH//2 - H//2, left = origW//2 - W//2
    down      = bilinear(crop(image), (H/32, W/32), align_corners=True)                                   downsample()
    F         = up4(up3(up2(up1(relu(conv1(cat(down, embedding repeated over the pixels)))))))            trunk()
                up_i = relu(conv_i(pixel_shuffle(x, 2)))
    U         = bilinear x2 (F), align_corners=True
    A         = relu(conv2(U)),  M = sigmoid(conv3(A))       3x3, zero padding at the crop border
    loss      = mean |M * crop(image) - crop(gt)|                                                          head()

Every function takes the dtype to compute in (float64: the arbiter's exact value; float32: one more evaluation of the reference's
arithmetic) and returns every intermediate the fixtures of tests/golden/make_golden_appearance.py hold, as numpy arrays."""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAM_NAMES = ["conv1.weight", "conv1.bias", "up1.conv.weight", "up1.conv.bias", "up2.conv.weight", "up2.conv.bias", "up3.conv.weight", "up3.conv.bias",
               "up4.conv.weight", "up4.conv.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias"]
HEAD_NAMES = PARAM_NAMES[10:]
CASES = ("37x45", "63x95", "70x101", "99x167", "zeros64x64")


def crop_of(origH, origW):
    H, W = origH // 32 * 32, origW // 32 * 32
    return H, W, origH // 2 - H // 2, origW // 2 - W // 2


def _t(x, dtype, grad=True):
    t = torch.as_tensor(np.asarray(x)).detach().to(dtype).clone()
    return t.requires_grad_(grad)


def _np(t):
    return None if t is None else t.detach().numpy().copy()


def _downsample(image):
    H, W, top, left = crop_of(image.shape[1], image.shape[2])
    crop = image[:, top:top + H, left:left + W]
    return F.interpolate(crop[None], size=(H // 32, W // 32), mode="bilinear", align_corners=True)[0]


def _trunk(down, embedding, p):
    hd, wd = down.shape[1:]
    x = torch.cat([down, embedding[:, None, None].expand(-1, hd, wd)], dim=0)[None]
    x = torch.relu(F.conv2d(x, p["conv1.weight"], p["conv1.bias"], padding=1))
    for i in range(1, 5):
        x = torch.relu(F.conv2d(F.pixel_shuffle(x, 2), p[f"up{i}.conv.weight"], p[f"up{i}.conv.bias"], padding=1))
    return x[0]


def _head(feat, image, gt, p):
    H, W, top, left = crop_of(image.shape[1], image.shape[2])
    U = F.interpolate(feat[None], scale_factor=2, mode="bilinear", align_corners=True)
    A = torch.relu(F.conv2d(U, p["conv2.weight"], p["conv2.bias"], padding=1))
    M = torch.sigmoid(F.conv2d(A, p["conv3.weight"], p["conv3.bias"], padding=1))[0]
    transformed = M * image[:, top:top + H, left:left + W]
    return (transformed - gt[:, top:top + H, left:left + W]).abs().mean(), transformed


def downsample(image, grad_down=None, dtype=torch.float64):
    """-> {"down", "dimage"}: the 32x down-sampling alone; dimage for the cotangent `grad_down` (ones when None)"""
    img = _t(image, dtype)
    down = _downsample(img)
    g = torch.ones_like(down) if grad_down is None else torch.as_tensor(np.asarray(grad_down)).to(dtype)
    down.backward(g)
    return {"down": _np(down), "dimage": _np(img.grad)}


def head(feat, image, gt, params, grad_loss=1.0, dtype=torch.float64):
    """-> {"loss", "transformed", "dF", "dimage", "dW2", "db2", "dW3", "db3"}: the full-resolution head alone (dimage: the direct path)"""
    p = {k: _t(params[k], dtype) for k in HEAD_NAMES}
    f, img = _t(feat, dtype), _t(image, dtype)
    loss, transformed = _head(f, img, _t(gt, dtype, False), p)
    (loss * grad_loss).backward()
    return {"loss": _np(loss), "transformed": _np(transformed), "dF": _np(f.grad), "dimage": _np(img.grad), "dW2": _np(p["conv2.weight"].grad),
            "db2": _np(p["conv2.bias"].grad), "dW3": _np(p["conv3.weight"].grad), "db3": _np(p["conv3.bias"].grad)}


def stage(image, gt, embedding, params, grad_loss=1.0, dtype=torch.float64):
    """The whole stage.  -> {"loss", "down", "F", "transformed", "dimage", "dembedding", "dF", "dW2", "db2", "dW3", "db3",
    "dtrunk": {parameter name: gradient}}"""
    p = {k: _t(params[k], dtype) for k in PARAM_NAMES}
    img, emb = _t(image, dtype), _t(embedding, dtype)
    down = _downsample(img)
    feat = _trunk(down, emb, p)
    feat.retain_grad()
    loss, transformed = _head(feat, img, _t(gt, dtype, False), p)
    (loss * grad_loss).backward()
    return {"loss": _np(loss), "down": _np(down), "F": _np(feat), "transformed": _np(transformed), "dimage": _np(img.grad), "dembedding": _np(emb.grad),
            "dF": _np(feat.grad), "dW2": _np(p["conv2.weight"].grad), "db2": _np(p["conv2.bias"].grad), "dW3": _np(p["conv3.weight"].grad),
            "db3": _np(p["conv3.bias"].grad), "dtrunk": {k: _np(p[k].grad) for k in PARAM_NAMES[:10]}}


def transformed_full(image, gt, embedding, params, dtype=torch.float64):
    """the inference branch: the transformed crop resized to the image's size"""
    with torch.no_grad():
        p = {k: _t(params[k], dtype, False) for k in PARAM_NAMES}
        img = _t(image, dtype, False)
        _, tr = _head(_trunk(_downsample(img), _t(embedding, dtype, False), p), img, _t(gt, dtype, False), p)
        return _np(F.interpolate(tr[None], size=tuple(img.shape[1:]), mode="bilinear", align_corners=True)[0])


# ---- fixtures: arrays spread over appearance_<case>.<n>.npz parts (no committed file of this repository may exceed 1 MiB) ----
def load_parts(stem):
    out = {}
    paths = sorted(glob.glob(os.path.join(GOLDEN, stem + ".*.npz")))
    assert paths, "no fixture parts for " + stem
    for path in paths:
        with np.load(path) as z:
            for k in z.files:
                out[k] = z[k]
    return out


def load_weights():
    """-> (names in the reference's state-dict order, {name: float32 array})"""
    z = load_parts("appearance_weights")
    names = [str(n) for n in z["names"]]
    return names, {n: z[n] for n in names}


def load_case(case):
    return load_parts("appearance_" + case)
