"""Generates tests/golden/imageeval_metrics.npz.  Build container only (needs the reference's sources).

The reference's own code, RUN on the CPU, not copied: utils/image_utils.py psnr, utils/loss_utils.py ssim and lpipsPyTorch's LPIPS('vgg')
(its forward, with hooks on its five linear heads so that the layer terms are recorded next to their sum).  torchvision is
not installed: a stub module provides models.vgg16(...), whose `features` is the Sequential of the public VGG-16 layer list, and
torch.hub.load_state_dict_from_url is replaced BEFORE anything is constructed, so no call can reach outside.  The weights are drawn from
numpy.random.default_rng(SEED) by tests/imageeval_restatement.py's seeded_weights: only the seed and that rule travel, not 58 MB of weights.

Per shape (16x16, 37x45, 64x80) the file holds the 8-bit input pair, the reference's float32 and float64 layer terms / total / PSNR / MSE /
SSIM, and the reference's own float32-against-float64 deviation under 1 and under 16 threads."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import imageeval_restatement as ir  # noqa: E402
from make_golden_mesheval import save  # noqa: E402

SEED = 7
SHAPES = ((16, 16), (37, 45), (64, 80))
VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")     # the public layer list ("D")


def no_network(*args, **kwargs):
    raise AssertionError("the golden generator must not reach outside")


def stub_torchvision(vgg_state):
    def vgg16(*args, **kwargs):
        layers, cin = [], 3
        for v in VGG16_CFG:
            if v == "M":
                layers.append(torch.nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [torch.nn.Conv2d(cin, v, kernel_size=3, padding=1), torch.nn.ReLU(inplace=True)]
                cin = v
        net = types.SimpleNamespace(features=torch.nn.Sequential(*layers))
        net.features.load_state_dict({k[len("features."):]: v for k, v in vgg_state.items()})
        return net
    tv, models = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
    models.vgg16 = vgg16
    models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1="IMAGENET1K_V1")
    models.alexnet = models.squeezenet1_1 = no_network
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models


def load_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_layers(net, x, y):
    """The reference's forward, run as it is, with a hook on each of its five linear heads that keeps the head's output map: a layer's
    term is that map's spatial mean, the total is what the forward returns."""
    kept = []
    hooks = [head.register_forward_hook(lambda module, args, out: kept.append(out)) for head in net.lin]
    try:
        total = net(x, y)
    finally:
        for h in hooks:
            h.remove()
    assert len(kept) == 5 and total.shape == (1, 1, 1, 1)
    layers = [float(m.mean((2, 3))) for m in kept]
    assert abs(sum(layers) - float(total)) <= 1e-6 * float(total)
    return np.array(layers + [float(total)], np.float64)


def main():
    vgg, lin = ir.seeded_weights(SEED)
    torch.hub.load_state_dict_from_url = lambda *a, **k: dict(lin)      # the original key spelling; get_state_dict renames it
    torch.hub.download_url_to_file = no_network
    stub_torchvision(vgg)
    sys.path.insert(0, REF)
    import lpipsPyTorch
    assert lpipsPyTorch.__file__.startswith(REF)
    from lpipsPyTorch.modules.lpips import LPIPS
    image_utils = load_file("ref_image_utils", os.path.join(REF, "utils", "image_utils.py"))
    loss_utils = load_file("ref_loss_utils", os.path.join(REF, "utils", "loss_utils.py"))
    with torch.no_grad():
        net32 = LPIPS("vgg").eval()
        net64 = LPIPS("vgg").eval().double()
        data = dict(seed=np.asarray(SEED), shapes=np.asarray(SHAPES))
        for H, W in SHAPES:
            a, b = ir.image_pair(1000 + H, H, W)
            ua, ub = ir.quantize_u8(a[0]), ir.quantize_u8(b[0])                   # what metric.py reads from the PNG files
            x32 = torch.from_numpy(np.moveaxis(ua, 2, 0).astype(np.float32) / np.float32(255))[None]
            y32 = torch.from_numpy(np.moveaxis(ub, 2, 0).astype(np.float32) / np.float32(255))[None]
            x32, y32 = x32.contiguous(), y32.contiguous()
            x64, y64 = x32.double(), y32.double()
            tag = f"{H}x{W}_"
            torch.set_num_threads(1)
            l64 = reference_layers(net64, x64, y64)
            l32_1 = reference_layers(net32, x32, y32)
            torch.set_num_threads(16)
            l32_16 = reference_layers(net32, x32, y32)
            data[tag + "a_u8"], data[tag + "b_u8"] = ua, ub
            data[tag + "lpips_f64"], data[tag + "lpips_f32"] = l64, l32_1
            data[tag + "lpips_f32_dev_1thread"] = np.abs(l32_1 - l64) / np.abs(l64)
            data[tag + "lpips_f32_dev_16threads"] = np.abs(l32_16 - l64) / np.abs(l64)
            mse64 = float(((x64 - y64) ** 2).view(1, -1).mean(1))
            p64, p32 = float(image_utils.psnr(x64, y64)), float(image_utils.psnr(x32, y32))
            s64, s32 = float(loss_utils.ssim(x64, y64)), float(loss_utils.ssim(x32, y32))
            assert float(image_utils.psnr(x32, x32)) == float("inf")
            data[tag + "mse_f64"], data[tag + "psnr_f64"], data[tag + "psnr_f32"] = np.asarray(mse64), np.asarray(p64), np.asarray(p32)
            data[tag + "ssim_f64"], data[tag + "ssim_f32"] = np.asarray(s64), np.asarray(s32)
            print(tag, "lpips f64", l64, "f32 dev", data[tag + "lpips_f32_dev_1thread"].max(), data[tag + "lpips_f32_dev_16threads"].max(),
                  "psnr", p64, p32, "ssim", s64, s32)
    save("imageeval_metrics.npz", **data)


if __name__ == "__main__":
    main()
