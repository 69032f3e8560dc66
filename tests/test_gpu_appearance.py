"""GPU tier of the decoupled appearance loss: loss_utils.l1_loss_appearance and the two autograd Functions under it against
the fixtures the reference's own code wrote and against tests/appearance_restatement.py evaluated on the CPU of the same box.

Yardstick: tests/arbiter.py as it stands, criteria A (rms error against float64 <= 1.35 x the reference's own fp32 error + 1e-7 of the
tensor's scale) and C (worst element <= 3 x the reference's + 2e-6).  B and D are absolute 1e-5 and vacuous for gradients of 1e-7..1e-2:
they are not relied on.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import appearance_restatement as R
from arbiter import failed_criteria, tensor_stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VIEW, VIEWS = 2, 4
GRADS = ("dF", "dimage", "dW2", "db2", "dW3", "db3")


def check(label, got, ref32, f64, failures):
    got = np.asarray(got, np.float64).reshape(np.shape(f64))
    assert np.isfinite(got).all(), label
    st = tensor_stats(got, {"ref32": ref32}, f64)
    failed = [c for c in failed_criteria(st) if c[0][0] in "AC"]
    print(f"{label:28s} scale {st['scale']:.3e}  rms hip {st['err_hip']:.3e} ref {st['err_ref']:.3e}  max hip {st['max_hip']:.3e} ref {st['max_ref']:.3e}"
          f"  {'MISSES ' + repr(failed) if failed else 'ok'}")
    failures += [(label,) + tuple(c) for c in failed]


@pytest.fixture(scope="module")
def weights():
    return R.load_weights()[1]


def gpu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


class ReferenceShaped(torch.nn.Module):
    """a module with the reference's attribute structure that is not appearance_network.AppearanceNetwork"""

    class Block(torch.nn.Module):
        def __init__(self, i, o):
            super().__init__()
            self.pixel_shuffle, self.conv, self.relu = torch.nn.PixelShuffle(2), torch.nn.Conv2d(i // 4, o, 3, stride=1, padding=1), torch.nn.ReLU()

        def forward(self, x):
            return self.relu(self.conv(self.pixel_shuffle(x)))

    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(67, 256, 3, stride=1, padding=1)
        self.up1, self.up2, self.up3, self.up4 = (self.Block(i, o) for i, o in ((256, 128), (128, 64), (64, 32), (32, 16)))
        self.conv2, self.conv3 = torch.nn.Conv2d(16, 16, 3, stride=1, padding=1), torch.nn.Conv2d(16, 3, 3, stride=1, padding=1)


class Gaussians:
    def __init__(self, net, table):
        self.appearance_network, self._appearance_embeddings = net, table

    def get_apperance_embedding(self, idx):
        return self._appearance_embeddings[idx]


def make_gaussians(weights, embedding, reference_shaped=False):
    from appearance_network import AppearanceNetwork
    net = ReferenceShaped() if reference_shaped else AppearanceNetwork(3 + 64, 3)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()}, strict=True)
    table = torch.randn(VIEWS, 64, generator=torch.Generator().manual_seed(3))
    table[VIEW] = torch.from_numpy(embedding)
    return Gaussians(net.to(DEV), torch.nn.Parameter(table.to(DEV)))


# ---- 1. every fixture case end to end ----
@pytest.mark.parametrize("case", R.CASES)
def test_l1_loss_appearance_reproduces_the_reference(case, weights):
    import loss_utils as lu
    z = R.load_case(case)
    g = make_gaussians(weights, z["embedding"], reference_shaped=case in ("63x95", "zeros64x64"))
    image, gt = gpu(z["image"], True), gpu(z["gt"])
    seen = {}

    def keep_features(module, args, out):
        out.retain_grad()
        seen["F"] = out

    handle = g.appearance_network.up4.register_forward_hook(keep_features)
    loss = lu.l1_loss_appearance(image, gt, g, VIEW)
    loss.backward()
    handle.remove()
    torch.cuda.synchronize()
    net = g.appearance_network
    got = {"loss": loss, "F": seen["F"][0], "dimage": image.grad, "dembedding": g._appearance_embeddings.grad[VIEW], "dF": seen["F"].grad[0],
           "dW2": net.conv2.weight.grad, "db2": net.conv2.bias.grad, "dW3": net.conv3.weight.grad, "db3": net.conv3.bias.grad}
    failures = []
    for k, v in got.items():
        check(f"{case} {k}", v.detach().cpu().numpy(), z[k + "_f32"], z[k + "_f64"], failures)
    if case == "37x45":                       # the trunk's parameter gradients (torch / MIOpen), exact value from the restatement
        s64 = R.stage(z["image"], z["gt"], z["embedding"], weights)
        for n, p in net.named_parameters():
            if not n.startswith(("conv2", "conv3")):
                check(f"{case} d {n}", p.grad.cpu().numpy(), z[f"dtrunk.{n}_f32"], s64["dtrunk"][n], failures)
    rows = g._appearance_embeddings.grad.cpu().numpy()
    assert not rows[[i for i in range(VIEWS) if i != VIEW]].any() and rows[VIEW].any()      # only the view's row
    H, W, top, left = R.crop_of(*z["image"].shape[1:])
    outside = np.ones(z["image"].shape[1:], bool)
    outside[top:top + H, left:left + W] = False
    assert not image.grad.cpu().numpy()[:, outside].any()                                    # exactly zero outside the crop
    if case.startswith("zeros"):
        assert not image.grad.cpu().numpy()[:, 12:28, 22:48].any()                           # sign(0) = 0 and M * 0
    assert not failures, failures


# ---- 2. the down-sampling alone ----
@pytest.mark.parametrize("shape", [(37, 45), (63, 95), (70, 101), (99, 167), (64, 64), (64, 32), (75, 130)], ids=lambda s: "%dx%d" % s)
def test_downsample_functions(shape):
    import loss_utils as lu
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    image = rng.random((3,) + shape, dtype=np.float32)
    H, W, top, left = R.crop_of(*shape)
    gd = rng.standard_normal((3, H // 32, W // 32)).astype(np.float32)
    r64, r32 = R.downsample(image, gd), R.downsample(image, gd, dtype=torch.float32)
    x = gpu(image, True)
    down = lu.appearance_downsample(x)
    down.backward(gpu(gd))
    torch.cuda.synchronize()
    assert tuple(down.shape) == (3, H // 32, W // 32)
    failures = []
    check("down", down.detach().cpu().numpy(), r32["down"], r64["down"], failures)
    check("dimage", x.grad.cpu().numpy(), r32["dimage"], r64["dimage"], failures)
    gi = x.grad.cpu().numpy()                                                                 # the same <= 4 pixels per output, nothing else
    assert not gi[(r64["dimage"] == 0) & (r32["dimage"] == 0)].any() and (gi != 0).sum() <= 4 * gd.size
    assert not failures, failures


# ---- 3. the head alone ----
HEAD_CROPS = {"32x32": (37, 45), "64x96": (70, 101), "96x32": (99, 40)}
VARIANTS = ("default", "alive", "dead", "g0.8")


@pytest.fixture(scope="module")
def head_inputs():
    out = {}
    for name, (oh, ow) in HEAD_CROPS.items():
        rng = np.random.default_rng(oh)
        H, W, _, _ = R.crop_of(oh, ow)
        out[name] = (0.5 * np.abs(rng.standard_normal((16, H // 2, W // 2))).astype(np.float32) * (rng.random((16, H // 2, W // 2)) < 0.7).astype(np.float32),
                     rng.random((3, oh, ow), dtype=np.float32), rng.random((3, oh, ow), dtype=np.float32))
    return out


def run_head(feat, image, gt, params, grad_loss):
    import loss_utils as lu
    f, x = gpu(feat, True), gpu(image, True)
    p = [gpu(params[k], True) for k in R.HEAD_NAMES]
    loss = lu.appearance_head_loss(f, x, gpu(gt), *p)
    (loss * grad_loss).backward()
    torch.cuda.synchronize()
    return {"loss": loss.detach(), "dF": f.grad, "dimage": x.grad, "dW2": p[0].grad, "db2": p[1].grad, "dW3": p[2].grad, "db3": p[3].grad}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("crop", list(HEAD_CROPS))
def test_head_functions(crop, variant, weights, head_inputs):
    feat, image, gt = head_inputs[crop]
    params = {k: weights[k].copy() for k in R.HEAD_NAMES}
    if variant == "alive":
        params["conv2.bias"] += 1.0           # every unit alive: a halo that forgets A's zero padding shows at the border, far above C
    if variant == "dead":
        params["conv2.bias"][:] = -10.0       # every unit dead
    grad_loss = 0.8 if variant == "g0.8" else 1.0
    r64 = R.head(feat, image, gt, params, grad_loss)
    r32 = R.head(feat, image, gt, params, grad_loss, dtype=torch.float32)
    got = {k: v.cpu().numpy() for k, v in run_head(feat, image, gt, params, grad_loss).items()}
    failures = []
    for k in ("loss",) + GRADS:
        if variant == "dead" and k in ("dF", "dW2", "db2", "dW3"):
            assert not r64[k].any() and not got[k].any(), k                                   # exactly zero
            continue
        check(f"{crop} {variant} {k}", got[k], r32[k], r64[k], failures)
    if variant == "alive":
        a64 = torch.relu(torch.nn.functional.conv2d(torch.nn.functional.interpolate(torch.from_numpy(feat).double()[None], scale_factor=2, mode="bilinear",
                                                                                       align_corners=True),
                                                    torch.from_numpy(params["conv2.weight"]).double(), torch.from_numpy(params["conv2.bias"]).double(), padding=1))
        assert float((a64 > 0).double().mean()) > 0.99
    if variant == "dead":
        assert got["db3"].any()
    H, W, top, left = R.crop_of(*image.shape[1:])
    outside = np.ones(image.shape[1:], bool)
    outside[top:top + H, left:left + W] = False
    assert not got["dimage"][:, outside].any()
    assert not failures, failures


def test_head_functions_where_workgroups_walk_several_tiles(weights):
    """Crop 512x544: 18 x 19 = 342 forward tiles and 19 x 20 = 380 backward tiles for at most 256 workgroups, so workgroups take a second
    tile: the grid stride, the barrier between two tiles of one workgroup and the weight-gradient accumulators that live across them.
    Every size above takes one tile per workgroup."""
    oh, ow = 523, 551
    rng = np.random.default_rng(oh)
    H, W, top, left = R.crop_of(oh, ow)
    assert (H, W) == (512, 544) and -(-H // 30) * -(-W // 30) > 256 and -(-H // 28) * -(-W // 28) > 256
    feat = (0.5 * np.abs(rng.standard_normal((16, H // 2, W // 2))) * (rng.random((16, H // 2, W // 2)) < 0.7)).astype(np.float32)
    image, gt = rng.random((3, oh, ow), dtype=np.float32), rng.random((3, oh, ow), dtype=np.float32)
    params = {k: weights[k].copy() for k in R.HEAD_NAMES}
    params["conv2.bias"] += 0.2
    r64 = R.head(feat, image, gt, params, 0.8)
    r32 = R.head(feat, image, gt, params, 0.8, dtype=torch.float32)
    got = {k: v.cpu().numpy() for k, v in run_head(feat, image, gt, params, 0.8).items()}
    failures = []
    for k in ("loss",) + GRADS:
        check(f"512x544 {k}", got[k], r32[k], r64[k], failures)
    outside = np.ones(image.shape[1:], bool)
    outside[top:top + H, left:left + W] = False
    assert not got["dimage"][:, outside].any()
    assert not failures, failures


# ---- 4. determinism ----
def test_two_runs_are_bit_identical(weights):
    z = R.load_case("70x101")
    s = R.stage(z["image"], z["gt"], z["embedding"], weights, dtype=torch.float32)
    params = {k: weights[k] for k in R.HEAD_NAMES}
    a = run_head(s["F"], z["image"], z["gt"], params, 1.0)
    b = run_head(s["F"].copy(), z["image"].copy(), z["gt"].copy(), params, 1.0)
    for k in ("loss",) + GRADS:
        assert torch.equal(a[k], b[k]), k
    import loss_utils as lu
    gd = np.random.default_rng(4).standard_normal((3, 2, 3)).astype(np.float32)
    downs = []
    for img in (z["image"], z["image"].copy()):
        x = gpu(img, True)
        d = lu.appearance_downsample(x)
        d.backward(gpu(gd.copy()))
        downs.append((d.detach(), x.grad))
    assert torch.equal(downs[0][0], downs[1][0]) and torch.equal(downs[0][1], downs[1][1]) and downs[0][1].any()


# ---- 5. nothing waits for the device ----
def test_functions_do_not_synchronize(weights):
    import loss_utils as lu
    z = R.load_case("63x95")
    s = R.stage(z["image"], z["gt"], z["embedding"], weights, dtype=torch.float32)
    args = [gpu(s["F"], True), gpu(z["image"], True), gpu(z["gt"])] + [gpu(weights[k], True) for k in R.HEAD_NAMES]
    gd = torch.ones(3, 1, 2, device=DEV)
    lu.appearance_head_loss(*args).backward()                                                # warm-up: code objects, allocator
    lu.appearance_downsample(args[1]).backward(gd)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = lu.appearance_head_loss(*args)
        loss.backward()
        down = lu.appearance_downsample(args[1])
        down.backward(gd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert abs(float(loss) - float(s["loss"])) < 1e-5


# ---- 6. adopt() and the inference branch ----
def test_adopted_network_and_the_inference_branch(weights):
    import loss_utils as lu
    from appearance_network import AppearanceNetwork
    z = R.load_case("70x101")
    g = make_gaussians(weights, z["embedding"], reference_shaped=True)
    theirs = dict(g.appearance_network.named_parameters())
    g.appearance_network = AppearanceNetwork.adopt(g.appearance_network)
    mine = dict(g.appearance_network.named_parameters())
    assert list(mine) == R.PARAM_NAMES and all(mine[n] is theirs[n] for n in mine)
    image, gt = gpu(z["image"]), gpu(z["gt"])
    with pytest.raises(RuntimeError, match="no_grad"):
        lu.l1_loss_appearance(image, gt, g, VIEW, return_transformed_image=True)
    with torch.no_grad():
        out = lu.l1_loss_appearance(image, gt, g, VIEW, return_transformed_image=True)
        loss = lu.l1_loss_appearance(image, gt, g, VIEW)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(image.shape)
    failures = []
    check("transformed image", out.cpu().numpy(), R.transformed_full(z["image"], z["gt"], z["embedding"], weights, dtype=torch.float32),
          R.transformed_full(z["image"], z["gt"], z["embedding"], weights), failures)
    check("loss under no_grad", loss.cpu().numpy(), z["loss_f32"], z["loss_f64"], failures)
    assert not failures, failures


def test_refusals_on_the_device(weights):
    import loss_utils as lu
    z = R.load_case("37x45")
    g = make_gaussians(weights, z["embedding"])
    image, gt = gpu(z["image"]), gpu(z["gt"])
    with pytest.raises(RuntimeError, match="crop"):
        lu.l1_loss_appearance(image[:, :31], gt[:, :31], g, VIEW)
    with pytest.raises(RuntimeError, match="float32"):
        lu.l1_loss_appearance(image.double(), gt.double(), g, VIEW)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        lu.l1_loss_appearance(image.cpu(), gt.cpu(), g, VIEW)
