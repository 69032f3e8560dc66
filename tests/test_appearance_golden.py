"""CPU tier of the decoupled appearance loss: tests/appearance_restatement.py -- the stage written out from DESIGN 11
"N8"'s formulae -- against the fixtures the reference's own code wrote (tests/golden/make_golden_appearance.py), and the module's
parameter names / state-dict compatibility with the reference's class."""
import numpy as np
import pytest
import torch

import appearance_restatement as R
from arbiter import failed_criteria, tensor_stats

TENSORS = ("loss", "F", "down", "dimage", "dembedding", "dF", "dW2", "db2", "dW3", "db3")


def criteria_ac(got, ref32, f64):
    """the scale-relative criteria of tests/arbiter.py (B and D are absolute 1e-5: vacuous at these magnitudes, not relied on)"""
    st = tensor_stats(got, {"ref32": ref32}, f64)
    return [c for c in failed_criteria(st) if c[0][0] in "AC"], st


@pytest.fixture(scope="module")
def weights():
    return R.load_weights()


@pytest.mark.parametrize("case", R.CASES)
def test_restatement_reproduces_the_reference(case, weights):
    z = R.load_case(case)
    s64 = R.stage(z["image"], z["gt"], z["embedding"], weights[1], dtype=torch.float64)
    s32 = R.stage(z["image"], z["gt"], z["embedding"], weights[1], dtype=torch.float32)
    for k in TENSORS:
        f64 = z[k + "_f64"]
        assert s64[k].size == f64.size and s64[k].dtype == np.float64 and (k == "loss" or s64[k].shape == f64.shape), k
        assert np.abs(s64[k].reshape(f64.shape) - f64).max() <= 1e-12 * (np.abs(f64).max() + 1e-30), (case, k)
        failed, st = criteria_ac(s32[k], z[k + "_f32"], f64)
        assert not failed, (case, k, failed)
    H, W, top, left = R.crop_of(*z["image"].shape[1:])
    outside = np.ones(z["image"].shape[1:], bool)
    outside[top:top + H, left:left + W] = False
    assert not z["dimage_f64"][:, outside].any() and not s64["dimage"][:, outside].any()
    if case == "37x45":
        assert (H, W, top, left) == (32, 32, 2, 6) and z["down_f32"].shape == (3, 1, 1) and z["F_f32"].shape == (16, 16, 16)
        for n in R.PARAM_NAMES[:10]:
            failed, st = criteria_ac(s32["dtrunk"][n], z[f"dtrunk.{n}_f32"], s64["dtrunk"][n])
            assert not failed, (n, failed)
    if case.startswith("zeros"):
        assert not z["image"][:, 10:30, 20:50].any() and not z["gt"][:, 10:30, 20:50].any()
        assert not z["dimage_f64"][:, 12:28, 22:48].any()                       # sign(0) = 0 there, and nothing reaches `down`


def test_head_and_downsample_alone_compose_to_the_stage(weights):
    z = R.load_case("63x95")
    s = R.stage(z["image"], z["gt"], z["embedding"], weights[1], grad_loss=0.8)
    h = R.head(s["F"], z["image"], z["gt"], weights[1], grad_loss=0.8)
    for k in ("loss", "dF", "dW2", "db2", "dW3", "db3"):
        assert np.allclose(h[k], s[k], rtol=1e-12, atol=0), k
    d = R.downsample(z["image"])
    assert np.array_equal(d["down"], s["down"])
    assert np.allclose(s["dF"], 0.8 * z["dF_f64"], rtol=1e-10, atol=1e-18)


def test_module_has_the_reference_parameter_names_and_loads_its_state_dict(weights):
    from appearance_network import AppearanceNetwork, UpsampleBlock
    names, w = weights
    net = AppearanceNetwork(3 + 64, 3)
    assert [n for n, _ in net.named_parameters()] == names == R.PARAM_NAMES
    assert list(net.state_dict()) == names
    for n, p in net.named_parameters():
        assert tuple(p.shape) == w[n].shape, n
    net.load_state_dict({n: torch.from_numpy(w[n]) for n in names}, strict=True)
    assert isinstance(net.up1, UpsampleBlock) and net.up4.conv.out_channels == 16
    z = R.load_case("37x45")
    x = torch.cat([torch.from_numpy(z["down_f32"]), torch.from_numpy(z["embedding"])[:, None, None]], 0)[None]
    with torch.no_grad():
        feat = net.trunk(x)[0].numpy()
        m = net(x)
    failed, _ = criteria_ac(feat, z["F_f32"], z["F_f64"])
    assert not failed, failed
    assert tuple(m.shape) == (1, 3, 32, 32) and float(m.min()) > 0 and float(m.max()) < 1


def test_default_initialisation_is_conv2d_default():
    from appearance_network import AppearanceNetwork
    torch.manual_seed(5)
    a = AppearanceNetwork(67, 3)
    torch.manual_seed(5)
    convs = [torch.nn.Conv2d(i, o, 3, stride=1, padding=1) for i, o in ((67, 256), (64, 128), (32, 64), (16, 32), (8, 16), (16, 16), (16, 3))]
    mine = [a.conv1, a.up1.conv, a.up2.conv, a.up3.conv, a.up4.conv, a.conv2, a.conv3]
    for c, m in zip(convs, mine):
        assert torch.equal(c.weight, m.weight) and torch.equal(c.bias, m.bias)


def test_adopt_shares_parameters():
    from appearance_network import AppearanceNetwork

    class Block(torch.nn.Module):
        def __init__(self, i, o):
            super().__init__()
            self.conv = torch.nn.Conv2d(i // 4, o, 3, padding=1)

    class Other(torch.nn.Module):           # a module of the reference's shape that is not our class
        def __init__(self):
            super().__init__()
            self.conv1 = torch.nn.Conv2d(67, 256, 3, padding=1)
            self.up1, self.up2, self.up3, self.up4 = Block(256, 128), Block(128, 64), Block(64, 32), Block(32, 16)
            self.conv2, self.conv3 = torch.nn.Conv2d(16, 16, 3, padding=1), torch.nn.Conv2d(16, 3, 3, padding=1)

    other = Other()
    net = AppearanceNetwork.adopt(other)
    assert isinstance(net, AppearanceNetwork)
    mine, theirs = dict(net.named_parameters()), dict(other.named_parameters())
    assert list(mine) == R.PARAM_NAMES and set(mine) == set(theirs)
    assert all(mine[n] is theirs[n] for n in mine)
    assert tuple(net(torch.zeros(1, 67, 1, 1)).shape) == (1, 3, 32, 32)
    with pytest.raises(TypeError):
        AppearanceNetwork.adopt(torch.nn.Linear(2, 2))
