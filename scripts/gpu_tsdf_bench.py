"""Times TSDF fusion (tsdf.VoxelBlockGrid: touch, integrate, extract) on the GPU against an eager-torch restatement of the integrate step
on the same GPU.  Upstream's own path (Open3D's VoxelBlockGrid on CPU:0) cannot run here: Open3D is not installed.

    python scripts/gpu_tsdf_bench.py [--out profiles/tsdf_bench.json] [--views 49] [--width 800] [--height 600] [--voxel 0.002]

The scene is SYNTHETIC and closed: a sphere of radius 0.5 seen by `views` cameras spread over a sphere of radius 2, analytic z-depth,
colour a smooth function of the hit point.  49 views at 800x600 is DTU at `-r 2`; the object's size in voxels is an estimate of a DTU
scan's, not a measurement.  The output says so.

Touch and integrate are timed per view with the host clock around calls that end in a device synchronise (each contains its one host
read), after one untimed fusion of all views.  The integrate KERNEL alone is timed with device events over repeats on the last view's
blocks and set against its bytes: blocks x 4096 voxels x bytes per voxel x 2 (every attribute read and written once).  That figure is
an upper bound of the traffic: a voxel that fails one of the tests (behind the camera, outside the image, no depth, behind the surface by
more than the truncation) moves nothing, so the number of voxels the view updates is reported beside it; and the last view's blocks are
small enough to stay in the 256 MiB Infinity Cache between repeats.  Both make the quotient an optimistic share of the HBM roof."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rade-gs_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

RADIUS, CAMERA_DISTANCE = 0.5, 2.0
CENTRE = np.array([0.013, -0.007, 0.021])
HBM_ROOF_TBS = 6.3            # achievable streaming rate of an MI355X (8 TB/s is the specification)


def look_at(eye, target, up):
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, y, z])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def make_views(n, W, H, dev):
    """[(depth [H,W], colour [H,W,3], K, E)] on the device; the cameras on a Fibonacci sphere"""
    focal = 0.9 * (H / 2) / math.tan(math.asin(RADIUS / CAMERA_DISTANCE))       # the sphere fills 90 % of the image height
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]], np.float64)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    rays = torch.stack([(xs - K[0, 2]) / focal, (ys - K[1, 2]) / focal, torch.ones_like(xs)], -1)
    views = []
    for i in range(n):
        zc = 1 - 2 * (i + 0.5) / n
        phi = i * math.pi * (3 - math.sqrt(5))
        d = np.array([math.sqrt(1 - zc * zc) * math.cos(phi), math.sqrt(1 - zc * zc) * math.sin(phi), zc])
        E = look_at(CENTRE + CAMERA_DISTANCE * d, CENTRE, np.array([0.0, 0.0, 1.0]) if abs(zc) < 0.9 else np.array([0.0, 1.0, 0.0]))
        Rt, o = torch.from_numpy(E[:3, :3].T.copy()).to(dev), torch.from_numpy(-E[:3, :3].T @ E[:3, 3]).to(dev)
        dirs = rays @ Rt.T
        oc = o - torch.from_numpy(CENTRE).to(dev)
        a, b, c = (dirs * dirs).sum(-1), 2 * (dirs @ oc), float(oc @ oc) - RADIUS * RADIUS
        disc = b * b - 4 * a * c
        t = (-b - torch.sqrt(disc.clamp_min(0))) / (2 * a)
        hit = (disc > 0) & (t > 0)
        t = torch.where(hit, t, torch.zeros_like(t))
        p = o + t[..., None] * dirs
        colour = torch.where(hit[..., None], 0.5 + 0.5 * torch.sin(7.0 * p + torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64, device=dev)), torch.zeros_like(p))
        views.append((t.float().contiguous(), colour.float().contiguous(), K, E))
    return views


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def fuse(views, voxel, depth_max):
    import tsdf
    grid = tsdf.VoxelBlockGrid(voxel_size=voxel, block_count=50000, with_color=True, device=views[0][0].device)
    touch, integrate, lists = [], [], []
    for depth, colour, K, E in views:
        blocks, dt = timed(lambda: grid.compute_unique_block_coordinates(depth, K, E, depth_max=depth_max))
        _, di = timed(lambda: grid.integrate(blocks, depth, colour, K, E, depth_max=depth_max))
        touch.append(dt)
        integrate.append(di)
        lists.append(blocks)
    mesh, de = timed(lambda: grid.extract_triangle_mesh(3.0))
    return grid, lists, mesh, touch, integrate, de


def eager_integrate(coords, tsdf_rows, weight_rows, color_rows, depth, colour, K, E, voxel, depth_max, trunc_multiplier=8.0):
    """the integrate step of include/radegs.h in eager torch ops on [n,4096] tensors (out of place: returns the three new tensors)"""
    dev = depth.device
    H, W = depth.shape
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    R, t = f32(E[:3, :3] * voxel), f32(E[:3, 3])
    fx, fy, cx, cy = (float(np.float32(v)) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    trunc = float(np.float32(voxel * trunc_multiplier))
    v = torch.arange(4096, device=dev)
    offsets = torch.stack([v & 15, (v >> 4) & 15, v >> 8], -1)
    X = (16 * coords.long()[:, None, :] + offsets[None]).float()
    p = [((R[k, 0] * X[..., 0] + R[k, 1] * X[..., 1]) + R[k, 2] * X[..., 2]) + t[k] for k in range(3)]
    ok = p[2] > 0
    u, w_ = (fx * p[0]) / p[2] + cx, (fy * p[1]) / p[2] + cy
    ui, vi = torch.sign(u) * torch.floor(u.abs() + 0.5), torch.sign(w_) * torch.floor(w_.abs() + 0.5)
    ok &= (ui >= 0) & (ui < W) & (vi >= 0) & (vi < H)
    pix = torch.where(ok, vi * W + ui, torch.zeros_like(ui)).long()
    d = depth.reshape(-1)[pix]
    sdf = d - p[2]
    ok &= (d > 0) & ~(d > depth_max) & ~(sdf < -trunc)
    s = torch.clamp(sdf, max=trunc) / trunc
    inv = 1.0 / (weight_rows + 1.0)
    new_t = torch.where(ok, (weight_rows * tsdf_rows + s) * inv, tsdf_rows)
    new_c = torch.where(ok[..., None], (weight_rows[..., None] * color_rows + colour.reshape(-1, 3)[pix]) * inv[..., None], color_rows)
    new_w = torch.where(ok, weight_rows + 1.0, weight_rows)
    return new_t, new_w, new_c, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.json"))
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--voxel", type=float, default=0.002)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_tsdf_bench: no GPU -- nothing is measured without one")
    import tsdf
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda:0")
    depth_max = 8.0
    views = make_views(args.views, args.width, args.height, dev)
    fuse(views, args.voxel, depth_max)                                          # untimed: first launches, allocator
    grid, lists, mesh, touch, integrate, extract = fuse(views, args.voxel, depth_max)
    vertices, faces, colors = mesh
    # the integrate kernel alone, and the eager restatement, on the last view's blocks (all present by now)
    depth, colour, K, E = views[-1]
    blocks = lists[-1]
    n = blocks.shape[0]
    L = tsdf._lib()
    nbytes = L.radegs_tsdf_unique_bytes(n)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    stream = _C._stream(dev)
    assert L.radegs_tsdf_unique_plan(n, _C._ptr(blocks), grid.n, _C._ptr(grid.keys), _C._ptr(ws), nbytes, _C._ptr(counts), stream) == 0
    n_unique, n_new, bad = counts.tolist()
    assert n_unique == n and n_new == 0 and not bad
    keys, slots = torch.empty_like(grid.keys), torch.empty_like(grid.slots)
    active_slots = torch.empty(n, dtype=torch.int32, device=dev)
    active_coords = torch.empty((n, 3), dtype=torch.int32, device=dev)
    assert L.radegs_tsdf_insert_apply(n, _C._ptr(ws), grid.n, _C._ptr(grid.keys), _C._ptr(grid.slots), n, 0, _C._ptr(keys), _C._ptr(slots),
                                      _C._ptr(active_slots), _C._ptr(active_coords), stream) == 0
    m = E[:3].copy()
    m[:, :3] *= args.voxel
    cam = tsdf._camera16(K, m)
    trunc = args.voxel * 8.0
    rows = active_slots.long()
    t_rows, w_rows, c_rows = grid.tsdf[rows].clone(), grid.weight[rows].clone(), grid.color[rows].clone()

    def kernel():
        assert L.radegs_tsdf_integrate(n, _C._ptr(active_slots), _C._ptr(active_coords), grid.capacity, args.width, args.height, _C._ptr(depth), _C._ptr(colour),
                                       cam, 1.0, depth_max, trunc, _C._ptr(grid.tsdf), _C._ptr(grid.weight), _C._ptr(grid.color), stream) == 0

    def eager():
        return eager_integrate(active_coords, t_rows, w_rows, c_rows, depth, colour, K, E, args.voxel, depth_max)

    def device_ms(fn):
        fn()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(args.repeats):
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_time(stop))
        return float(np.median(times)), float(np.min(times))

    # the two agree before either is timed (the kernel on a copy of the same rows)
    before = (grid.tsdf[rows].clone(), grid.weight[rows].clone(), grid.color[rows].clone())
    kernel()
    want = eager()
    agree = bool(torch.equal(grid.tsdf[rows], want[0]) and torch.equal(grid.weight[rows], want[1]) and torch.equal(grid.color[rows], want[2]))
    differ = dict(weight_voxels=int((grid.weight[rows] != want[1]).sum()), tsdf_voxels=int((grid.tsdf[rows] != want[0]).sum()),
                  tsdf_max_abs=float((grid.tsdf[rows] - want[0]).abs().max()), color_max_abs=float((grid.color[rows] - want[2]).abs().max()))
    updated = int(want[3].sum())
    grid.tsdf[rows], grid.weight[rows], grid.color[rows] = before
    kernel_ms, kernel_min = device_ms(kernel)
    eager_ms, eager_min = device_ms(eager)
    whole_call = []
    for _ in range(5):
        whole_call.append(timed(lambda: grid.integrate(blocks, depth, colour, K, E, depth_max=depth_max))[1])
    bytes_per_voxel = 4 + 4 + 12
    kernel_bytes = n * 4096 * bytes_per_voxel * 2
    result = dict(note="SYNTHETIC closed scene: a sphere of radius %.2f, %d views at %dx%d, voxel %.4f; the object's size in voxels is an estimate of a DTU "
                       "scan's, no DTU data was available.  Upstream's Open3D CPU path cannot run here; the comparison is an eager-torch restatement of "
                       "the integrate step on the same GPU." % (RADIUS, args.views, args.width, args.height, args.voxel),
                  device=torch.cuda.get_device_name(0), views=args.views, image=[args.width, args.height], voxel_size=args.voxel,
                  blocks=int(grid.n), blocks_last_view=int(n), vertices=int(vertices.shape[0]), triangles=int(faces.shape[0]),
                  touch_ms_per_view=dict(median=1e3 * float(np.median(touch)), max=1e3 * float(np.max(touch))),
                  integrate_ms_per_view=dict(median=1e3 * float(np.median(integrate)), max=1e3 * float(np.max(integrate)),
                                             includes="sort of the listed blocks, the host read, the insertion and the kernel"),
                  integrate_call_ms_blocks_present=1e3 * float(np.median(whole_call)),
                  extract_ms=1e3 * extract, fuse_total_ms=1e3 * (sum(touch) + sum(integrate) + extract),
                  integrate_kernel=dict(ms_median=kernel_ms, ms_min=kernel_min, bytes=kernel_bytes, tb_per_s=kernel_bytes / (kernel_ms * 1e-3) / 1e12,
                                        hbm_roof_tb_per_s=HBM_ROOF_TBS, fraction_of_roof=kernel_bytes / (kernel_ms * 1e-3) / 1e12 / HBM_ROOF_TBS,
                                        updated_voxels=updated, updated_bytes=updated * bytes_per_voxel * 2,
                                        updated_tb_per_s=updated * bytes_per_voxel * 2 / (kernel_ms * 1e-3) / 1e12,
                                        note="bytes = blocks x 4096 x %d B per voxel x 2, an upper bound: only the updated voxels move their %d B twice; "
                                             "the last view's blocks (%.0f MB) stay in the 256 MiB Infinity Cache between repeats" %
                                             (bytes_per_voxel, bytes_per_voxel, n * 4096 * bytes_per_voxel / 1e6)),
                  eager_integrate=dict(ms_median=eager_ms, ms_min=eager_min, equals_kernel_bit_for_bit=agree, differs_from_kernel=differ,
                                       note="a timing baseline in torch's own kernels; its last bits are torch's"),
                  hip_not_slower_than_eager=bool(kernel_ms <= eager_ms), speedup_over_eager=eager_ms / kernel_ms)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
