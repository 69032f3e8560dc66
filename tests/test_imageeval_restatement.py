"""CPU tier of the image evaluation: tests/imageeval_restatement.py against the fixture the reference's own code wrote
(tests/golden/imageeval_metrics.npz), the host fmaf-chain convolution against float64 inside the derivable bound, and image_eval's weight
loader, which reads files and never fetches."""
import os
import re

import numpy as np
import pytest
import torch

import imageeval_restatement as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "imageeval_metrics.npz"))
SHAPES = [tuple(s) for s in GOLDEN["shapes"]]


def pair(H, W, dtype):
    tag = f"{H}x{W}_"
    out = []
    for k in ("a_u8", "b_u8"):
        out.append(torch.from_numpy(np.moveaxis(GOLDEN[tag + k], 2, 0).astype(np.float32) / np.float32(255))[None].contiguous().to(dtype))
    return out


def test_the_fixture_holds_the_issue_shapes_and_a_deviation_record():
    assert SHAPES == [(16, 16), (37, 45), (64, 80)] and int(GOLDEN["seed"]) == 7
    for H, W in SHAPES:
        for k in ("lpips_f32_dev_1thread", "lpips_f32_dev_16threads"):
            d = GOLDEN[f"{H}x{W}_{k}"]
            assert d.shape == (6,) and (d < 1e-5).all()


@pytest.mark.parametrize("H,W", SHAPES)
def test_lpips_restatement_equals_the_reference_in_float64(H, W):
    vgg, lin = ir.seeded_weights(7)
    x, y = pair(H, W, torch.float64)
    got, want = ir.lpips_layers(x, y, vgg, lin, torch.float64), GOLDEN[f"{H}x{W}_lpips_f64"]
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (got, want)


@pytest.mark.parametrize("H,W", SHAPES)
def test_lpips_restatement_in_float32_stays_inside_the_reference_deviation(H, W):
    """The restatement does the reference's float32 operations; what may differ between two machines is the order in which the CPU
    convolution adds, which is what the reference's own 1-thread and 16-thread runs differ by.  The bound is the largest deviation the
    reference itself shows anywhere in the fixture."""
    vgg, lin = ir.seeded_weights(7)
    bound = max(float(GOLDEN[f"{h}x{w}_{k}"].max()) for h, w in SHAPES for k in ("lpips_f32_dev_1thread", "lpips_f32_dev_16threads"))
    x, y = pair(H, W, torch.float32)
    want, threads = GOLDEN[f"{H}x{W}_lpips_f64"], torch.get_num_threads()
    try:
        for n in (1, 16):                  # the two settings the fixture was recorded under
            torch.set_num_threads(n)
            dev = np.abs(ir.lpips_layers(x, y, vgg, lin, torch.float32) - want) / np.abs(want)
            print(f"{H}x{W}, {n} threads: float32 restatement off float64 by {dev.max():.2e}, the reference's own largest {bound:.2e}")
            assert (dev <= bound).all(), (n, dev, bound)
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("H,W", SHAPES)
def test_psnr_restatement_equals_the_reference(H, W):
    x, y = pair(H, W, torch.float64)
    tag = f"{H}x{W}_"
    assert abs(float(ir.mse(x, y)) - float(GOLDEN[tag + "mse_f64"])) <= 1e-12 * float(GOLDEN[tag + "mse_f64"])
    assert abs(float(ir.psnr(x, y)) - float(GOLDEN[tag + "psnr_f64"])) <= 1e-12 * float(GOLDEN[tag + "psnr_f64"])
    x32, y32 = pair(H, W, torch.float32)
    assert abs(float(ir.psnr(x32, y32, torch.float32)) - float(GOLDEN[tag + "psnr_f32"])) <= 1e-5
    assert float(ir.psnr(x32, x32, torch.float32)) == float("inf")


def test_quantize_restatement_on_the_rounding_edges():
    k = np.arange(0, 255, dtype=np.float64)
    edge = ((k + 0.5) / 255).astype(np.float32)
    x = np.concatenate([np.nextafter(edge, np.float32(-1)), edge, np.nextafter(edge, np.float32(2)), np.float32([-0.0, -1.0, -1e-8, 1.0, 1.5, 0.999999, np.nan])])
    x = np.resize(x, (3, 1, x.size))
    u = ir.quantize_u8(x)
    t = x[0, 0].astype(np.float32) * np.float32(255) + np.float32(0.5)
    want = np.where(np.isnan(t), 0, np.clip(np.nan_to_num(t), 0, 255)).astype(np.int64)
    assert np.array_equal(u[0, :, 0].astype(np.int64), want)
    assert u.min() == 0 and u.max() == 255
    assert np.array_equal(ir.quantize(x)[0, 0], u[0, :, 0].astype(np.float32) / np.float32(255))


# ------------------------------------------------------------------------ the host chain ------------------------------------------------------------------------
CHAIN_CASES = [(3, 64, 5, 7), (64, 64, 5, 7), (64, 128, 5, 7), (256, 256, 3, 4)]


def chain_case(cin, cout, H, W, seed=11):
    rng = np.random.default_rng(seed + cin + cout)
    w = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = rng.uniform(-0.05, 0.05, cout).astype(np.float32)
    if cin == 3:
        img = rng.uniform(-0.2, 1.2, (2, 3, H, W)).astype(np.float32)
        img[:, :, 0, 0] = np.float32(0.0)
        x = ir.zscore_channels_last(img)
    else:
        x = np.maximum(rng.standard_normal((2, H, W, cin)), 0).astype(np.float32)
    return x, w, b


@pytest.mark.parametrize("cin,cout,H,W", CHAIN_CASES)
def test_host_chain_convolution_stays_inside_the_gamma_bound(cin, cout, H, W):
    x, w, b = chain_case(cin, cout, H, W)
    got = ir.chain_conv(x, w, b)
    want, mag = ir.conv_f64(x, w, b)
    err, bound = np.abs(got.astype(np.float64) - want), ir.chain_bound(mag, got, cin)
    print(f"{cin}->{cout} {H}x{W}: largest error over its bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert float(err.max()) > 0       # the comparison is not vacuous: float32 rounding is there


def test_host_chain_order_is_the_documented_one():
    """The order shows in float32: all products are 1 except one of 2^25, whose ulp is 4.  The ones before it add up exactly, every one after
    it is absorbed, so the centre pixel of a 3x3 image of ones reads 2^25 + k where k is the large term's position in the chain (a multiple
    of 4 here).  k is written out from the header's comment, not taken from its code."""
    cin = 32
    x = np.ones((1, 3, 3, cin), np.float32)
    for ci, ky, kx in ((0, 0, 0), (16, 0, 0), (4, 2, 1), (28, 1, 2), (12, 2, 2)):
        w = np.ones((1, cin, 3, 3), np.float32)
        w[0, ci, ky, kx] = 2.0 ** 25
        k = ((ci // 16) * 9 + ky * 3 + kx) * 16 + ci % 16
        got = float(ir.chain_conv(x, w, np.zeros(1, np.float32))[0, 1, 1, 0])
        assert got == 2.0 ** 25 + k, (ci, ky, kx, got - 2.0 ** 25, k)


# --------------------------------------------------------------------------- the loader ---------------------------------------------------------------------------
def test_loader_reads_all_three_key_spellings(tmp_path, monkeypatch):
    import image_eval as ie
    vgg, lin = ir.seeded_weights(7)
    vgg_small = dict(vgg)
    vgg_small["classifier.0.weight"] = torch.zeros(2, 2)                         # ignored
    renamed = {k.replace("lin", "").replace("model.", ""): v for k, v in lin.items()}      # the reference's get_state_dict
    assert sorted(renamed) == [f"{k}.1.weight" for k in range(5)]
    torch.save(vgg_small, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    torch.save(renamed, tmp_path / "renamed.pth")
    monkeypatch.setenv(ie.WEIGHTS_ENV, str(tmp_path))
    v1, l1 = ie.load_lpips_weights()
    v2, l2 = ie.load_lpips_weights(lin_path=str(tmp_path / "renamed.pth"))
    convs = ie._vgg_state(v1)
    assert len(convs) == 13 and all(torch.equal(convs[k][0], vgg[f"features.{idx}.weight"]) for k, (idx, _, _) in enumerate(ie.VGG_CONVS))
    for a, b, (key, want) in zip(ie._lin_state(l1), ie._lin_state(l2), sorted(lin.items())):
        assert torch.equal(a, want.reshape(-1)) and torch.equal(b, a)
    net = ie.LPIPS(v1, l2)                                                      # constructing needs no GPU and no network
    assert len(net._convs) == 13 and len(net._lin) == 5


def test_missing_files_raise_and_name_both(tmp_path, monkeypatch):
    import image_eval as ie
    monkeypatch.delenv(ie.WEIGHTS_ENV, raising=False)
    with pytest.raises(FileNotFoundError) as e:
        ie.load_lpips_weights()
    assert "vgg16" in str(e.value) and "vgg.pth" in str(e.value) and ie.WEIGHTS_ENV in str(e.value)
    monkeypatch.setenv(ie.WEIGHTS_ENV, str(tmp_path))
    torch.save(ir.seeded_weights(7)[0], tmp_path / "vgg16.pth")                  # one of the two is not enough
    with pytest.raises(FileNotFoundError) as e:
        ie.load_lpips_weights()
    assert "vgg.pth" in str(e.value)
    import lpipsPyTorch
    with pytest.raises(FileNotFoundError):
        lpipsPyTorch.LPIPS("vgg")


def test_only_vgg_is_built():
    import lpipsPyTorch
    for net_type in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError):
            lpipsPyTorch.lpips(None, None, net_type=net_type)
        with pytest.raises(NotImplementedError):
            lpipsPyTorch.LPIPS(net_type)
    with pytest.raises(NotImplementedError):
        lpipsPyTorch.lpips(None, None)                                          # the reference's default is 'alex'


def test_no_download_path_exists():
    pkg = os.path.join(ROOT, "rade-gs_amd")
    for rel in ("image_eval.py", os.path.join("lpipsPyTorch", "__init__.py")):
        src = open(os.path.join(pkg, rel)).read()
        for word in ("load_state_dict_from_url", "urlopen", "hub"):
            assert not re.search(word, src), (rel, word)
    assert os.listdir(os.path.join(pkg, "lpipsPyTorch")).count("__init__.py") == 1


def test_pillow_is_asked_for_by_name(monkeypatch):
    import builtins

    import image_eval as ie
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    with pytest.raises(ImportError, match="Pillow"):
        ie.evaluate([])
