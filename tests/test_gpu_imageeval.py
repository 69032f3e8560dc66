"""GPU tier of the image evaluation: image_eval.py and the kernels of csrc/radegs_imageeval.hip.  The convolution is held to
equality: exactly torch's CPU result on integer data, where no summation order can matter, and exactly the host fmaf chain of
csrc/rg_conv_chain.h on random data, because the f32-input MFMA is that chain.  Pooled maps, the 8-bit round trip and repeated sums are
exact too.  LPIPS, PSNR and SSIM are compared with what the reference's own code wrote (tests/golden/imageeval_metrics.npz) inside the
project's image band, 1e-4 relative (SSIM: the 5e-6 of the fused-step tests)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_eval as ie
import imageeval_restatement as ir

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "imageeval_metrics.npz"))
SEED = int(GOLDEN["seed"])
_NET = {}

# N = 2 everywhere: 5x7 is smaller than a tile and all border, 37x45 has tails in both directions and more than one block
CONV_CASES = [(3, 64, 5, 7), (64, 64, 5, 7), (64, 128, 5, 7), (3, 64, 37, 45), (64, 64, 37, 45), (64, 128, 37, 45), (256, 256, 9, 11), (512, 512, 4, 5),
              (512, 512, 2, 2), (512, 512, 1, 1)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def net():
    if "net" not in _NET:
        _NET["net"] = ie.LPIPS(*ir.seeded_weights(SEED))
    return _NET["net"]


def golden_pair(H, W):
    tag = f"{H}x{W}_"
    return [dev((np.moveaxis(GOLDEN[tag + k], 2, 0).astype(np.float32) / np.float32(255))[None]) for k in ("a_u8", "b_u8")]


def run_conv(x, w, b, cin, **kw):
    """x: planar (N,3,H,W) for the first layer, channels-last otherwise; returns channels-last numpy"""
    return ie.conv3x3_relu(dev(x), dev(w), dev(b), first=cin == 3, **kw).cpu().numpy()


# ----------------------------------------------------------------------------- convolution -----------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,H,W", CONV_CASES)
def test_conv_on_integer_data_equals_torch_exactly(cin, cout, H, W):
    """|w|, |x| <= 3 and |b| <= 8: every partial sum is an integer below 9 * 512 * 9 + 8 < 2^24, exact in float32 in any order.  Drawn at
    random, the weights differ across taps, input and output channels, so a transposed tap or swapped operand cannot pass."""
    rng = np.random.default_rng(100 + cin + cout + H)
    w = rng.integers(-3, 4, (cout, cin, 3, 3)).astype(np.float32)
    b = rng.integers(-8, 9, cout).astype(np.float32)
    x = rng.integers(-3, 4, (2, cin, H, W)).astype(np.float32)          # planar
    want = F.relu(F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), padding=1)).permute(0, 2, 3, 1).numpy()
    if cin == 3:
        got = run_conv(x, w, b, cin, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
    else:
        got = run_conv(np.moveaxis(x, 1, 3), w, b, cin)
    assert got.shape == want.shape and np.array_equal(got, want), float(np.abs(got - want).max())
    assert (want > 0).any() and (want == 0).any()


@pytest.mark.parametrize("cin,cout,H,W", CONV_CASES)
def test_conv_on_random_data_equals_the_host_chain(cin, cout, H, W):
    rng = np.random.default_rng(200 + cin + cout + H)
    w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = rng.uniform(-0.05, 0.05, cout).astype(np.float32)
    if cin == 3:
        img = rng.uniform(-0.3, 1.3, (2, 3, H, W)).astype(np.float32)     # negatives after the z-score, and exact zeros before it
        img[:, :, ::3, ::2] = np.float32(0.0)
        got, x = run_conv(img, w, b, cin), ir.zscore_channels_last(img)
    else:
        x = np.maximum(rng.standard_normal((2, H, W, cin)), 0).astype(np.float32)
        got = run_conv(x, w, b, cin)
    chain = ir.chain_conv(x, w, b)
    want, mag = ir.conv_f64(x, w, b)
    err, bound = np.abs(got.astype(np.float64) - want), ir.chain_bound(mag, got, cin)
    differ = int((got != chain).sum())
    print(f"{cin}->{cout} {H}x{W}: {differ} of {got.size} outputs differ from the host chain; error over the gamma_K bound {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
    assert differ == 0, float(np.abs(got - chain).max())               # equal as floats: -0 == +0


def test_first_layer_pads_with_zero_in_the_normalised_space():
    """An image equal to `mean` normalises to exactly 0, so every output, border included, is the bias chain fmaf(0, w, bias) = bias; a
    border padded with (0 - mean) / std would add weights to it."""
    rng = np.random.default_rng(5)
    w = rng.standard_normal((64, 3, 3, 3)).astype(np.float32)
    b = rng.uniform(0.1, 1.0, 64).astype(np.float32)
    b[::2] *= -1
    img = np.broadcast_to(np.array(ie.MEAN, np.float32).reshape(1, 3, 1, 1), (2, 3, 6, 9)).copy()
    got = run_conv(img, w, b, 3)
    assert np.array_equal(got, np.broadcast_to(np.maximum(b, 0), got.shape))


# ----------------------------------------------------------------------------- pool + tap -----------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C,pool", [(37, 45, 64, True), (18, 22, 128, True), (9, 11, 256, True), (4, 5, 512, True), (2, 2, 512, False)])
def test_tap_and_pool(H, W, C, pool):
    rng = np.random.default_rng(300 + H)
    f = np.maximum(rng.standard_normal((2, H, W, C)), 0).astype(np.float32)
    f[0, H // 2, W // 2] = 0                     # all channels zero in x only
    f[:, 0, W - 1] = 0                           # and in both
    lin = rng.uniform(0, 2.0 / C, C).astype(np.float32)
    out1, pooled1 = ie.tap_pool(dev(f), dev(lin), pool)
    out2, pooled2 = ie.tap_pool(dev(f), dev(lin), pool)
    a, b = out1.cpu().numpy(), out2.cpu().numpy()
    assert np.isfinite(a).all() and a.tobytes() == b.tobytes()
    t = torch.from_numpy(f).permute(0, 3, 1, 2)
    want = float(ir.tap_term(t[:1], t[1:], lin))
    print(f"{H}x{W}x{C}: tap {float(a[0]):.9e}, float64 {want:.9e}, off by {abs(float(a[0]) - want) / want:.2e}")
    assert abs(float(a[0]) - want) <= 1e-4 * want
    if pool:
        assert pooled1.shape == (2, H // 2, W // 2, C)
        assert torch.equal(pooled1.cpu(), F.max_pool2d(t, 2).permute(0, 2, 3, 1)) and torch.equal(pooled1, pooled2)
    else:
        assert pooled1 is None


# --------------------------------------------------------------------------- LPIPS end to end ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(16, 16), (37, 45), (64, 80)])
def test_lpips_against_the_reference_golden(H, W):
    x, y = golden_pair(H, W)
    want = GOLDEN[f"{H}x{W}_lpips_f64"]
    layers = net().forward_layers(x, y)
    total = net().forward(x, y)
    assert total.shape == (1, 1, 1, 1) and total.dtype == torch.float32 and layers.shape == (5,)
    got = np.concatenate([layers.cpu().numpy().astype(np.float64), [float(total)]])
    dev_hip = np.abs(got - want) / np.abs(want)
    dev_ref = np.maximum(GOLDEN[f"{H}x{W}_lpips_f32_dev_1thread"], GOLDEN[f"{H}x{W}_lpips_f32_dev_16threads"])
    print(f"{H}x{W}: HIP off float64 by {np.array2string(dev_hip, precision=2)}; the reference's float32 by {np.array2string(dev_ref, precision=2)}")
    assert (dev_hip <= 1e-4).all()
    again = net().forward_layers(x, y)
    assert torch.equal(layers, again)
    assert float(net().forward(x, x)) == 0.0 and float(net().forward(x[0], x[0])) == 0.0


def test_lpips_features_are_the_vgg_taps():
    x, _ = golden_pair(37, 45)
    got = net().features(x)
    want = ir.vgg_features(x.cpu(), ir.seeded_weights(SEED)[0])
    assert [tuple(g.shape) for g in got] == [(1, 64, 37, 45), (1, 128, 18, 22), (1, 256, 9, 11), (1, 512, 4, 5), (1, 512, 2, 2)]
    for g, w in zip(got, want):
        assert float((g.cpu().double() - w).abs().max()) <= 1e-4 * float(w.abs().max())


def test_lpips_refuses_what_the_reference_cannot_pool():
    x = torch.rand(1, 3, 15, 40, device=DEV)
    with pytest.raises(ValueError):
        net().forward(x, x)
    with pytest.raises(ValueError):
        net().forward(x.transpose(2, 3).contiguous(), x.transpose(2, 3).contiguous())


# ------------------------------------------------------------------------- quantise, PSNR, SSIM -------------------------------------------------------------------------
def test_quantize_equals_the_restatement_exactly():
    k = np.arange(0, 255, dtype=np.float64)
    edge = ((k + 0.5) / 255).astype(np.float32)
    vals = np.concatenate([np.nextafter(edge, np.float32(-1)), edge, np.nextafter(edge, np.float32(2)),
                           np.float32([-0.0, 0.0, -1.0, -1e-8, 1.0, 1.5, 300.0, 0.999999, np.nextafter(np.float32(1), np.float32(0))]),
                           np.random.default_rng(1).uniform(-0.1, 1.1, 2000).astype(np.float32)])
    x = np.resize(vals, (3, 31, 97)).copy()
    x[1] = x[1, ::-1]
    want_u8, want = ir.quantize_u8(x), ir.quantize(x)
    u8, q = ie.to_uint8(dev(x)), ie.quantize(dev(x))
    assert u8.dtype == torch.uint8 and u8.shape == (31, 97, 3) and np.array_equal(u8.cpu().numpy(), want_u8)
    assert q.shape == (3, 31, 97) and np.array_equal(q.cpu().numpy(), want)
    assert ie.quantize(dev(x)[None]).shape == (1, 3, 31, 97)
    assert set(np.unique(want_u8)) == set(range(256))


@pytest.mark.parametrize("H,W", [(16, 16), (37, 45), (64, 80)])
def test_psnr_and_ssim_against_the_reference_golden(H, W):
    import loss_utils
    x, y = golden_pair(H, W)
    tag = f"{H}x{W}_"
    p = ie.psnr(x, y)
    assert p.shape == (1, 1)
    mse = 10.0 ** (-float(p) / 10.0)
    print(f"{H}x{W}: PSNR {float(p):.6f} dB (reference float64 {float(GOLDEN[tag + 'psnr_f64']):.6f}), SSIM {float(ie.ssim(x, y)):.7f} ({float(GOLDEN[tag + 'ssim_f64']):.7f})")
    assert abs(mse - float(GOLDEN[tag + "mse_f64"])) <= 1e-4 * float(GOLDEN[tag + "mse_f64"])
    assert math.isinf(float(ie.psnr(x, x))) and float(ie.psnr(x, x)) > 0
    s = ie.ssim(x, y)
    assert torch.equal(s, loss_utils.ssim(x[0], y[0])) and torch.equal(s, ie.ssim(x[0], y[0]))
    assert abs(float(s) - float(GOLDEN[tag + "ssim_f64"])) <= 5e-6
    with pytest.raises(RuntimeError):
        loss_utils.ssim(x, y)                      # the training loss keeps refusing the batched pair


# ------------------------------------------------------------------------------ evaluate ------------------------------------------------------------------------------
def test_evaluate_on_a_directory_of_png_pairs(tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    import lpipsPyTorch
    vgg, lin = ir.seeded_weights(SEED)
    wdir = tmp_path / "weights"
    wdir.mkdir()
    torch.save(vgg, wdir / "vgg16.pth")
    torch.save(lin, wdir / "vgg.pth")
    monkeypatch.setenv(ie.WEIGHTS_ENV, str(wdir))
    scene = tmp_path / "scene"

    class View:
        pass
    views = []
    for i in range(3):
        a, b = ir.image_pair(50 + i, 37, 45)
        v = View()
        v.original_image, v.render = dev(b[0]), dev(a[0])
        views.append(v)
    ie.render_set(str(scene), "test", 30000, views, lambda v: v.render)
    names = ["00000.png", "00001.png", "00002.png"]
    base = scene / "test" / "ours_30000"
    assert sorted(os.listdir(base / "renders")) == names and sorted(os.listdir(base / "gt")) == names
    renders = [ie.load_png(str(base / "renders" / n), DEV) for n in names]
    gts = [ie.load_png(str(base / "gt" / n), DEV) for n in names]
    for v, r, g in zip(views, renders, gts):        # the PNG holds the 8-bit round trip
        assert torch.equal(r[0], ie.quantize(v.render)) and torch.equal(g[0], ie.quantize(v.original_image))
    want = ie.evaluate_views(renders, gts, net(), names)
    got = ie.evaluate([str(scene)])[str(scene)]
    full, per_view = json.load(open(scene / "results.json")), json.load(open(scene / "per_view.json"))
    assert list(full) == ["ours_30000"] and sorted(full["ours_30000"]) == ["LPIPS", "PSNR", "SSIM"] and got == full
    for key in ("SSIM", "PSNR", "LPIPS"):
        assert full["ours_30000"][key] == want[key]
        assert per_view["ours_30000"][key] == want["per_view"][key] and sorted(per_view["ours_30000"][key]) == names
        vals = torch.tensor([want["per_view"][key][n] for n in names])
        assert want[key] == vals.mean().item()
    d = lpipsPyTorch.lpips(renders[0], gts[0], net_type="vgg")
    assert d.shape == (1, 1, 1, 1) and torch.equal(d, net().forward(renders[0], gts[0]))
    assert abs(float(d) - want["per_view"]["LPIPS"]["00000.png"]) == 0.0
    with pytest.raises(NotImplementedError):
        lpipsPyTorch.lpips(renders[0], gts[0], net_type="alex")
