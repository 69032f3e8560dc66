"""Times the decoupled appearance loss at 3 x 1200 x 1600 -- the size the reference's own scene/appearance_network.py uses --
forward + backward through autograd, in one process on one GPU:
  (a) loss_utils.l1_loss_appearance: trunk in torch / MIOpen, everything at full resolution in the HIP head kernels;
  (b) the same stage in eager torch on the same GPU (tests/appearance_restatement.py's formulation moved to the device): the yardstick.
Also the head alone (fused Function | eager), the trunk alone (down-sampling + conv1 + four blocks, forward + backward), the two native head
calls on their own and the allocator's peak memory of (a) and (b).  The two formulations alternate; every figure is the median of REPS individually timed repetitions taken after the clock has
settled.  GPU box only.

    python scripts/gpu_appearance_bench.py [--out FILE] [--reps N] [--height H --width W]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "rade-gs_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch

import appearance_restatement as R
import loss_utils as lu
from appearance_network import AppearanceNetwork
from diff_gaussian_rasterization import _C

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--height", type=int, default=1200)
ap.add_argument("--width", type=int, default=1600)
opt = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU"
assert opt.reps >= 20
dev = torch.device("cuda:0")
OH, OW = opt.height, opt.width
H, W, top, left = R.crop_of(OH, OW)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def settle(seconds=1.5):
    """keep the GPU busy until its clock has settled"""
    x = torch.randn(4096, 4096, device=dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(20):
            x = (x @ x).clamp_(-1, 1)
        torch.cuda.synchronize()


def timed(fn, n):
    """n individually timed repetitions (device events around each), ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def alternate(fns, n, warm=3):
    """{name: median ms} with the formulations alternating in blocks of five repetitions"""
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    settle()
    out = {k: [] for k in fns}
    for _ in range((n + 4) // 5):
        for k, f in fns.items():
            out[k] += timed(f, 5)
    return {k: (statistics.median(v), min(v), max(v), len(v)) for k, v in out.items()}


gen = torch.Generator(device=dev).manual_seed(1)
image = torch.rand(3, OH, OW, device=dev, generator=gen).requires_grad_(True)
gt = torch.rand(3, OH, OW, device=dev, generator=gen)
torch.manual_seed(2)
net = AppearanceNetwork(3 + 64, 3).to(dev)
table = torch.nn.Parameter(0.5 * torch.randn(8, 64, device=dev))
params = dict(net.named_parameters())


class Gaussians:
    appearance_network = net

    def get_apperance_embedding(self, idx):
        return table[idx]


def zero_grads():
    image.grad = None
    table.grad = None
    for p in params.values():
        p.grad = None


def fused():
    zero_grads()
    lu.l1_loss_appearance(image, gt, Gaussians(), 3).backward()


def eager_loss():
    feat = R._trunk(R._downsample(image), table[3], params)
    return R._head(feat, image, gt, params)[0]


def eager():
    zero_grads()
    eager_loss().backward()


with torch.no_grad():
    feat0 = R._trunk(R._downsample(image), table[3], params).contiguous()
feat = feat0.clone().requires_grad_(True)
gfeat = torch.randn_like(feat0) * 1e-6
head_w = [params[k] for k in R.HEAD_NAMES]


def head_fused():
    zero_grads(); feat.grad = None
    lu.appearance_head_loss(feat, image, gt, *head_w).backward()


def head_eager():
    zero_grads(); feat.grad = None
    R._head(feat, image, gt, params)[0].backward()


def trunk_fused():
    zero_grads()
    x = torch.cat([lu.appearance_downsample(image), table[3][:, None, None].expand(-1, H // 32, W // 32)], 0)[None]
    net.trunk(x)[0].backward(gfeat)


def trunk_eager():
    zero_grads()
    R._trunk(R._downsample(image), table[3], params).backward(gfeat)


# the native calls on their own
L = lu._lib()
args = [feat0, image.detach(), gt] + [p.detach() for p in head_w]
fb, bb = L.radegs_appearance_head_scratch_bytes(OH, OW, 0), L.radegs_appearance_head_scratch_bytes(OH, OW, 1)
scratch = torch.empty(bb, dtype=torch.uint8, device=dev)
loss1, g1 = torch.empty(1, device=dev), torch.ones(1, device=dev)
outs = [torch.empty_like(t) for t in (feat0, image, *head_w)]
ptr, stream = _C._ptr, _C._stream(dev)


def native_fwd():
    rc = L.radegs_appearance_head_forward(OH, OW, H // 2, W // 2, *[ptr(t) for t in args], ptr(scratch), fb, ptr(loss1), None, stream)
    assert rc == 0


def native_bwd():
    rc = L.radegs_appearance_head_backward(OH, OW, H // 2, W // 2, *[ptr(t) for t in args], ptr(g1), ptr(scratch), bb, *[ptr(t) for t in outs], stream)
    assert rc == 0


def peak(fn):
    zero_grads()
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


say(f"decoupled appearance loss, image 3 x {OH} x {OW}, crop {H} x {W}, {torch.cuda.get_device_name(0)}; medians of {opt.reps} repetitions (min .. max), ms")
# agreement of the two formulations at this size, before anything is timed
fused()
got = {"dimage": image.grad.clone(), "dtable": table.grad.clone(), **{k: p.grad.clone() for k, p in params.items()}}
lf = float(lu.l1_loss_appearance(image, gt, Gaussians(), 3).detach())
eager()
le = float(eager_loss().detach())
ref = {"dimage": image.grad, "dtable": table.grad, **{k: p.grad for k, p in params.items()}}
diffs = {k: float((got[k] - ref[k]).abs().max() / (ref[k].abs().max() + 1e-30)) for k in got}
worst = max(diffs.values())
say(f"loss fused {lf:.7f} eager {le:.7f}; largest |fused - eager| per tensor, relative to the tensor's largest element: "
    + ", ".join(f"{k} {v:.1e}" for k, v in diffs.items()))
res = dict(height=OH, width=OW, reps=opt.reps, loss_fused=lf, loss_eager=le, worst_grad_diff=worst)
for title, fns in (("whole stage, forward + backward", {"fused": fused, "eager": eager}),
                   ("head alone (up-sampling, conv2, conv3, product, L1), forward + backward", {"fused": head_fused, "eager": head_eager}),
                   ("trunk alone (down-sampling, conv1, four blocks), forward + backward", {"fused": trunk_fused, "eager": trunk_eager}),
                   ("native head calls (weight repack + kernels, no torch around them)", {"forward": native_fwd, "backward": native_bwd})):
    r = alternate(fns, opt.reps)
    res[title] = r
    say(title + ": " + "; ".join(f"{k} {m:.3f} ({lo:.3f} .. {hi:.3f})" for k, (m, lo, hi, _) in r.items())
        + (f"  -> eager / fused = {r['eager'][0] / r['fused'][0]:.2f}" if "eager" in r else ""))
mac = (16 * 16 + 16 * 3) * 9 * H * W
say(f"head forward: {mac / 1e9:.2f} G multiply-adds -> {2 * mac / (res['native head calls (weight repack + kernels, no torch around them)']['forward'][0] * 1e-3) / 1e12:.1f} TFLOP/s fp32 achieved")
pf, pe = peak(fused), peak(eager)
res.update(peak_extra_bytes_fused=pf, peak_extra_bytes_eager=pe)
say(f"peak extra memory of one forward + backward: fused {pf / 1e6:.0f} MB, eager {pe / 1e6:.0f} MB")
say(json.dumps(res))
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    open(opt.out, "w").write("\n".join(lines) + "\n")
