"""Times LPIPS-VGG of image_eval.py on one 1600x1200 pair (workload C3's size) with seeded weights, end to end and per convolution, next to
the same pair through an eager-torch restatement (F.conv2d, i.e. MIOpen) in the same process.  Needs a GPU.

    python scripts/gpu_imageeval_bench.py [--out profiles/imageeval_bench.json] [--width 1600 --height 1200] [--iters 5]

Times are device events around `iters` calls after a warm-up of every shape; FLOP counts are 2 * N * H * W * 9 * Cin * Cout per layer, from
the shapes; the share of peak is against the 157.3 TFLOP/s f32 matrix peak of the MI355X.  The two paths are also compared: the HIP
result must be inside 1e-4 relative of the eager one, or the timing is of something else."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rade-gs_amd"))
import image_eval as ie  # noqa: E402

PEAK_F32_MATRIX = 157.3e12


def seeded_weights(seed):
    rng = np.random.default_rng(seed)
    vgg, lin = {}, {}
    for idx, cin, cout in ie.VGG_CONVS:
        vgg[f"features.{idx}.weight"] = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32))
        vgg[f"features.{idx}.bias"] = torch.from_numpy(rng.uniform(-0.05, 0.05, cout).astype(np.float32))
    for k, c in enumerate(ie.TAP_CHANNELS):
        lin[f"lin{k}.model.1.weight"] = torch.from_numpy(rng.uniform(0.0, 2.0 / c, (1, c, 1, 1)).astype(np.float32))
    return vgg, lin


def timed(fn, iters):
    """mean milliseconds of fn() over `iters` calls, device events, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def eager_lpips(x, y, vgg, lin):
    """lpipsPyTorch's forward in eager torch, float32, the pair as one batch of two"""
    mean, std = torch.tensor(ie.MEAN, device=x.device).view(1, 3, 1, 1), torch.tensor(ie.STD, device=x.device).view(1, 3, 1, 1)
    t = (torch.cat([x, y]) - mean) / std
    total, tap = None, 0
    for k, (idx, _, _) in enumerate(ie.VGG_CONVS):
        t = F.relu(F.conv2d(t, vgg[f"features.{idx}.weight"], vgg[f"features.{idx}.bias"], padding=1))
        if k == ie.TAP_AFTER[tap]:
            n = t / (torch.sqrt((t ** 2).sum(1, keepdim=True)) + 1e-10)
            term = (lin[f"lin{tap}.model.1.weight"] * (n[:1] - n[1:]) ** 2).sum(1, keepdim=True).mean((2, 3), True)
            total = term if total is None else total + term
            if tap < 4:
                t = F.max_pool2d(t, 2)
            tap += 1
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imageeval_bench.json"))
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this benchmark measures on a GPU and there is none")
    dev = torch.device("cuda:0")
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    H, W = args.height, args.width
    vgg, lin = seeded_weights(args.seed)
    net = ie.LPIPS(vgg, lin)
    vgg_d, lin_d = {k: v.to(dev) for k, v in vgg.items()}, {k: v.to(dev) for k, v in lin.items()}
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    x = torch.rand(1, 3, H, W, generator=g).to(dev)
    y = (x + 0.05 * torch.randn(1, 3, H, W, generator=g).to(dev)).clamp(0, 1)
    x, y = ie.quantize(x), ie.quantize(y)

    with torch.no_grad():
        hip_value, eager_value = float(net.forward(x, y)), float(eager_lpips(x, y, vgg_d, lin_d))
        rel = abs(hip_value - eager_value) / abs(eager_value)
        assert rel <= 1e-4, (hip_value, eager_value)
        hip_ms = timed(lambda: net.forward(x, y), args.iters)
        eager_ms = timed(lambda: eager_lpips(x, y, vgg_d, lin_d), args.iters)
        hip_ms2 = timed(lambda: net.forward(x, y), args.iters)          # alternated once more: the spread between two windows of the same code
        eager_ms2 = timed(lambda: eager_lpips(x, y, vgg_d, lin_d), args.iters)

        convs, _ = net._on(dev)
        layers, h, w, tap = [], H, W, 0
        for k, (idx, cin, cout) in enumerate(ie.VGG_CONVS):
            if k == 0:
                src_hip = torch.cat([x, y]).contiguous()
                src_eager = src_hip
            else:
                src_eager = torch.rand(2, cin, h, w, device=dev)
                src_hip = src_eager.permute(0, 2, 3, 1).contiguous()
            dst = torch.empty(2, h, w, cout, device=dev)
            wk, bk = vgg_d[f"features.{idx}.weight"], vgg_d[f"features.{idx}.bias"]
            ms = timed(lambda: ie._conv(dev, 2, h, w, cin, cout, src_hip, convs[k][0], convs[k][1], dst), args.iters)
            ms_eager = timed(lambda: F.relu(F.conv2d(src_eager, wk, bk, padding=1)), args.iters)
            flop = 2.0 * 2 * h * w * 9 * cin * cout
            layers.append(dict(conv=f"features.{idx}", cin=cin, cout=cout, height=h, width=w, flop=flop, hip_ms=ms, hip_tflops=flop / ms / 1e9,
                               hip_share_of_f32_matrix_peak=flop / (ms * 1e-3) / PEAK_F32_MATRIX, eager_ms=ms_eager, eager_tflops=flop / ms_eager / 1e9))
            del src_eager, src_hip, dst
            if k == ie.TAP_AFTER[tap]:
                if tap < 4:
                    h, w = h // 2, w // 2
                tap += 1
    total_flop = sum(l["flop"] for l in layers)
    result = dict(workload=f"LPIPS-VGG, one {W}x{H} pair, seeded weights (seed {args.seed}), float32", device=torch.cuda.get_device_name(0),
                  iters=args.iters, timing="device events around `iters` calls after one warm-up call of the same shapes; two windows each, alternated",
                  lpips_hip=hip_value, lpips_eager=eager_value, relative_difference=rel,
                  hip_end_to_end_ms=[hip_ms, hip_ms2], eager_torch_end_to_end_ms=[eager_ms, eager_ms2],
                  conv_flop_total=total_flop, hip_end_to_end_tflops=total_flop / min(hip_ms, hip_ms2) / 1e9,
                  hip_conv_ms_sum=sum(l["hip_ms"] for l in layers), eager_conv_ms_sum=sum(l["eager_ms"] for l in layers),
                  f32_matrix_peak_tflops=PEAK_F32_MATRIX / 1e12, layers=layers,
                  note="per-layer eager times are F.conv2d + relu on NCHW input (MIOpen picks the algorithm); the end-to-end figures include the "
                       "taps, pools and launch gaps of each path; not measured: kernel-trace times, other image sizes")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(result, fp, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "layers"}))
    for l in layers:
        print(f"{l['conv']:12s} {l['cin']:3d}->{l['cout']:3d} {l['height']}x{l['width']}: HIP {l['hip_ms']:.3f} ms {l['hip_tflops']:.1f} TF/s"
              f" ({100 * l['hip_share_of_f32_matrix_peak']:.0f} % of peak), eager {l['eager_ms']:.3f} ms {l['eager_tflops']:.1f} TF/s")


if __name__ == "__main__":
    main()
