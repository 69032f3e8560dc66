"""Times unbounded mesh extraction on the GPU.

    python scripts/gpu_unbounded_bench.py [--out profiles/unbounded_bench.json] [--views 32] [--crop 512] [--resolution 1024] [--repeats 3]

Run without `--step` it is a driver: each step below runs in a child process of its own under its own time limit, and the first one that
fails, faults or runs out of time ends the run (nothing more is started on the device).  The scene is synthetic: `--views` cameras on a
sphere around an analytic sphere, 1600x1063 depth maps with a far wall, smooth colour maps -- nothing is read from any file.
  crop    one `--crop`^3 lattice of the contracted cube against all views: radegs_unbounded_fuse in both lane mappings (z-runs, 4x4x4
          bricks), device events, median of `--repeats` after one untimed call; then an eager-torch loop that does what upstream does for
          that crop -- the samples materialised, chunks of 256^3, per view the three maps copied from host memory, the matrix product,
          three grid_sample calls (depth, colour, normal) and the masked running average -- in the same process on the same GPU, once
          untimed and once timed.  That loop is the yardstick: the parent commit has no such path.  The two results are compared.
  whole   extract_mesh_unbounded at `--resolution` in crops of `--crop`, split into fuse, marching cubes, weld and colouring (host clock
          around device synchronisation), once untimed at a quarter of the resolution and once timed.
Rates: sample-views per second = lattice points x views / kernel time.  Traffic implied by that rate: every sample-view that is in view
gathers four float32 taps (16 B) through the vector L1 / L2 -- an upper bound, the in-view share is recorded next to it; HBM sees the
tsdf written once (4 B per sample) and each map at least once per launch.  No threshold: recorded, including where eager torch wins."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rade-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
WIDTH, HEIGHT, FOV = 1600, 1063, 0.9
SPHERE_RADIUS, CAMERA_DISTANCE, WALL = 0.25, 2.0, 6.0
STEP_LIMIT_S = {"crop": 420, "whole": 420}


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, np.cross(z, x), z])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def scene(n_views, dev):
    """views on a spiral around the sphere: ([View], depths [H,W], colours [3,H,W], normals [3,H,W]) on the device, and the cloud"""
    import torch
    fovy = 2 * math.atan(math.tan(FOV / 2) * HEIGHT / WIDTH)
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[3, 2], P[2, 2], P[2, 3] = 1 / math.tan(FOV / 2), 1 / math.tan(fovy / 2), 1.0, 100.0 / 99.99, -1.0 / 99.99
    ys, xs = torch.meshgrid(torch.arange(HEIGHT, device=dev, dtype=torch.float64), torch.arange(WIDTH, device=dev, dtype=torch.float64), indexing="ij")
    ndx, ndy = (2 * xs / (WIDTH - 1) - 1) * math.tan(FOV / 2), (2 * ys / (HEIGHT - 1) - 1) * math.tan(fovy / 2)

    class View:
        pass
    views, depths, colours, normals = [], [], [], []
    for k in range(n_views):
        h = -0.8 + 1.6 * (k + 0.5) / n_views
        a = 2.399963 * k
        eye = CAMERA_DISTANCE * np.array([math.sqrt(1 - h * h) * math.cos(a), math.sqrt(1 - h * h) * math.sin(a), h])
        E = look_at(eye)
        v = View()
        v.world_view_transform = torch.from_numpy(E.T.astype(np.float32))
        v.full_proj_transform = torch.from_numpy((E.T @ P.T).astype(np.float32))
        views.append(v)
        Rt = torch.from_numpy(E[:3, :3].T.copy()).to(dev)
        dirs = torch.stack([ndx, ndy, torch.ones_like(ndx)], -1) @ Rt.T
        o = torch.from_numpy(eye).to(dev)
        qa, qb, qc = (dirs * dirs).sum(-1), 2 * (dirs @ o), float(eye @ eye) - SPHERE_RADIUS ** 2
        disc = qb * qb - 4 * qa * qc
        t = (-qb - disc.clamp(min=0).sqrt()) / (2 * qa)
        depths.append(torch.where(disc > 0, t, torch.full_like(t, WALL)).float().contiguous())
        colours.append(torch.stack([0.5 + 0.5 * torch.sin(0.01 * xs + k), 0.5 + 0.5 * torch.cos(0.013 * ys), 0.5 + 0.25 * torch.sin(0.007 * (xs + ys))]).float().contiguous())
        normals.append(torch.zeros((3, HEIGHT, WIDTH), device=dev))
    rng = np.random.default_rng(5)
    d = rng.standard_normal((100000, 3))
    xyz = torch.from_numpy((0.45 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)).to(dev)
    return views, depths, colours, normals, xyz


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def eager_crop(axes, views, host_maps, center, radius, voxel_size, dev):
    """what upstream does for one crop, in eager torch (utils/mesh_utils.py:171-232 and mcube_utils.py:50-68, restated)"""
    import torch
    import torch.nn.functional as Fn
    xx, yy, zz = torch.meshgrid(*axes, indexing="ij")
    points = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1)
    mats = [v.full_proj_transform.to(dev) for v in views]
    c = torch.from_numpy(np.asarray(center, np.float32)).to(dev)
    out = []
    for y in torch.split(points, 256 ** 3, dim=0):
        mag = torch.linalg.norm(y, ord=2, dim=-1)[..., None]
        x = torch.where(mag < 1, y, (1 / (2 - mag)) * (y / mag)) * radius + c
        norm = torch.linalg.norm(x, dim=-1)
        far = norm > 1
        trunc = 5 * voxel_size * torch.ones_like(x[:, 0])
        trunc[far] *= 1 / (2 - norm[far].clamp(max=1.9))
        tsdf, rgbs, w = torch.ones_like(x[:, 0]), torch.zeros((x.shape[0], 3), device=dev), torch.ones_like(x[:, 0])
        for m, (d_host, c_host, n_host) in zip(mats, host_maps):
            q = torch.cat([x, torch.ones_like(x[..., :1])], dim=-1) @ m
            z = q[..., -1:]
            pix = q[..., :2] / z
            mask = ((pix > -1.0) & (pix < 1.0) & (z > 0)).all(dim=-1)
            grid = pix[None, None]
            sd = Fn.grid_sample(d_host.to(dev)[None], grid, mode="bilinear", padding_mode="border", align_corners=True).reshape(-1, 1)
            sc = Fn.grid_sample(c_host.to(dev)[None], grid, mode="bilinear", padding_mode="border", align_corners=True).reshape(3, -1).T
            Fn.grid_sample(n_host.to(dev)[None], grid, mode="bilinear", padding_mode="border", align_corners=True).reshape(3, -1).T
            sdf = (sd - z).flatten()
            mask = mask & (sdf > -trunc)
            s = torch.clamp(sdf / trunc, min=-1.0, max=1.0)[mask]
            wm = w[mask]
            wp = wm + 1
            tsdf[mask] = (tsdf[mask] * wm + s) / wp
            rgbs[mask] = (rgbs[mask] * wm[:, None] + sc[mask]) / wp[:, None]
            w[mask] = wp
        out.append(tsdf)
    return torch.cat(out)


def step_crop(args):
    import torch
    import unbounded_mesh as um
    dev = torch.device("cuda:0")
    views, depths, colours, normals, xyz = scene(args.views, dev)
    stack = um.ViewStack(views, [d[None] for d in depths], colours)
    center, radius = um.scene_normalisation(stack.world_view)
    voxel = radius * 2 / args.resolution
    R = um.contracted_bound(xyz, center, radius)
    axes = [torch.from_numpy(a).to(dev) for a in um.crop_axes(R, args.resolution, args.crop)]
    lattice = (axes[len(axes) // 2],) * 3 if len(axes) > 1 else (axes[0],) * 3        # a crop next to the centre: the sphere's surface runs through it
    M = args.crop ** 3
    res = {"crop": args.crop, "views": args.views, "map": [HEIGHT, WIDTH], "samples": M, "sample_views": M * args.views}
    outs = {}
    for name, mapping in (("zrun", um.ZRUN), ("brick", um.BRICK)):
        fn = lambda: um.fuse_samples(stack, lattice, voxel, center, radius, contract=True, mapping=mapping)
        outs[name] = fn()
        torch.cuda.synchronize()
        ms = sorted(event_ms(fn)[0] for _ in range(args.repeats))
        med = ms[len(ms) // 2]
        rate = M * args.views / (med * 1e-3)
        res[name] = {"kernel_ms_median": round(med, 3), "kernel_ms_min": round(ms[0], 3), "kernel_ms_max": round(ms[-1], 3),
                     "sample_views_per_s": rate, "gather_bytes_per_s_upper_bound": 16 * rate,
                     "hbm_bytes_per_launch_at_least": 4 * M + sum(4 * d.numel() for d in depths)}
        print(name, res[name], flush=True)
    res["mappings_same_bits"] = bool(torch.equal(outs["zrun"].view(torch.int32), outs["brick"].view(torch.int32)))
    res["integrated_share"] = float((outs["zrun"] != 1).float().mean())
    host_maps = [(d[None].cpu(), c.cpu(), n.cpu()) for d, c, n in zip(depths, colours, normals)]
    eager = lambda: eager_crop(lattice, views, host_maps, center, float(np.float32(radius)), voxel, dev)
    ref = eager()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = eager()
    torch.cuda.synchronize()
    res["eager_torch_s"] = time.perf_counter() - t0
    diff = (ref - outs["zrun"]).abs()
    res["eager_vs_kernel"] = {"max_abs_diff": float(diff.max()), "share_above_1e-4": float((diff > 1e-4).float().mean())}
    res["speedup_over_eager"] = {n: res["eager_torch_s"] * 1e3 / res[n]["kernel_ms_median"] for n in ("zrun", "brick")}
    print("eager", res["eager_torch_s"], res["eager_vs_kernel"], flush=True)
    return res


def step_whole(args):
    import torch
    import unbounded_mesh as um
    dev = torch.device("cuda:0")
    views, depths, colours, _, xyz = scene(args.views, dev)
    stack = um.ViewStack(views, [d[None] for d in depths], colours)
    um.extract_mesh_unbounded(stack, xyz, args.resolution // 4, args.crop // 4)        # untimed: code objects, allocator
    timings = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v, f, c = um.extract_mesh_unbounded(stack, xyz, args.resolution, args.crop, timings=timings)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    sv = args.resolution ** 3 * args.views
    res = {"resolution": args.resolution, "crop": args.crop, "views": args.views, "mapping": "brick" if um.DEFAULT_MAPPING == um.BRICK else "zrun",
           "total_s": total, "stages_s": timings, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
           "fuse_sample_views_per_s": sv / timings["fuse"], "peak_memory_bytes": int(torch.cuda.max_memory_allocated(dev))}
    print("whole", res, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unbounded_bench.json"))
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--crop", type=int, default=512)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step", choices=("crop", "whole"))
    args = ap.parse_args()
    if args.step:
        res = {"crop": step_crop, "whole": step_whole}[args.step](args)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    result = {"device": "MI355X (gfx950)", "command": " ".join(sys.argv)}
    for step in ("crop", "whole"):
        part = args.out + "." + step
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--out", part, "--views", str(args.views), "--crop", str(args.crop),
               "--resolution", str(args.resolution), "--repeats", str(args.repeats)]
        try:
            rc = subprocess.run(cmd, timeout=STEP_LIMIT_S[step]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:       # a failed, faulted or overdue step: nothing more is started on the device
            result[step] = {"failed": rc}
            with open(args.out, "w") as fh:
                json.dump(result, fh, indent=1)
            print(f"step {step} ended with {rc}: stopping", flush=True)
            return 1
        with open(part) as fh:
            result[step] = json.load(fh)
        os.remove(part)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
