"""Times the Tanks-and-Temples mesh culling (tnt_cull.cull_mesh's stages) on the GPU, and the vertex test against an eager-torch restatement
of Mesher.point_masks on the same GPU.  For the depth render there is nothing to compare with: upstream renders through pyrender / EGL,
which this box does not have, so the render is reported against the HBM roof instead.

    python scripts/gpu_tntcull_bench.py [--out profiles/tntcull_bench.json] [--faces 10000000] [--views 150] [--view-batch 10]

The scene is SYNTHETIC: a bumpy unit sphere triangulated as a latitude / longitude grid of about `faces` triangles in grid order (a
marching-tetrahedra mesh is also spatially coherent, but this is an estimate of one, not one), on a floor of two large triangles that
every camera sees (they take the queued path), and `views` cameras on a ring of radius 3 looking at the centre, 1920 x 1080 with the
reference's Tanks-and-Temples intrinsics.  A triangle of the sphere covers about a tenth of a pixel.

Stages are timed with device events around the C entry points, per batch of views, after one untimed batch.  Bytes of the triangle
stream per view: 24 for a face's three int64 indices plus 72 for its three gathered float64 vertices."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rade-gs_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W = 1080, 1920
K = (1163.8678928442187, 1172.793101201448, 962.3120628412543, 542.0667209577691)
HBM_PEAK = 8.0e12            # bytes / s, the MI355X's nominal figure
STREAM_BYTES_PER_FACE = 3 * 8 + 3 * 24


def make_scene(n_faces, n_views, seed=0):
    rng = np.random.default_rng(seed)
    nlat = int(np.sqrt(n_faces / 4))
    nlon = 2 * nlat
    th, ph = np.meshgrid(np.pi * np.arange(nlat + 1) / nlat, 2 * np.pi * np.arange(nlon) / nlon, indexing="ij")
    r = (1.0 + 0.1 * np.sin(3 * th) * np.cos(4 * ph) + 0.06 * np.cos(5 * th + 1.0)) * (1 + 0.0005 * rng.standard_normal(th.shape))
    verts = (np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1) * r[..., None]).reshape(-1, 3)
    a, b = np.meshgrid(np.arange(nlat), np.arange(nlon), indexing="ij")
    at = lambda i, j: i * nlon + (j % nlon)
    faces = np.concatenate([np.stack([at(a, b), at(a + 1, b), at(a + 1, b + 1)], -1).reshape(-1, 3),
                            np.stack([at(a, b), at(a + 1, b + 1), at(a, b + 1)], -1).reshape(-1, 3)], 0)
    n = verts.shape[0]
    floor = np.array([[-3.0, -3.0, -1.3], [3.0, -3.0, -1.3], [3.0, 3.0, -1.3], [-3.0, 3.0, -1.3]])
    faces = np.concatenate([faces, [[n, n + 1, n + 2], [n, n + 2, n + 3]]], 0)
    verts = np.concatenate([verts, floor], 0)
    poses = []
    for k in range(n_views):                                   # OpenCV poses: x right, y down, z forward
        t = 2 * np.pi * k / n_views
        eye = np.array([3.0 * np.cos(t), 3.0 * np.sin(t), 0.6 + 0.4 * np.sin(3 * t)])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, np.cross(fwd, right), fwd, eye
        poses.append(m)
    return verts.astype(np.float32), faces.astype(np.int64), np.stack(poses)


def eager_seen(points, depth, w2c, eps=0.005):
    """cull_mesh.py:132-170 for one camera at forecast_radius 0, restated with the same torch calls (no forecast terms)"""
    ones = torch.ones_like(points[:, :1])
    cam = (w2c @ torch.cat([points, ones], dim=1).reshape(-1, 4, 1))[:, :3]
    Kt = torch.eye(3, device=points.device)
    Kt[0, 0], Kt[1, 1], Kt[0, 2], Kt[1, 2] = K
    uv = Kt @ cam
    z = uv[:, -1:] + 1e-8
    uv = uv[:, :2] / z
    u, v, z = uv[:, 0, 0], uv[:, 1, 0], z[:, 0, 0]
    inside = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1) & (z > 0)
    grid = torch.stack([u / (W - 1) * 2.0 - 1.0, v / (H - 1) * 2.0 - 1.0], dim=-1).reshape(1, 1, -1, 2)
    s = torch.nn.functional.grid_sample(depth.reshape(1, 1, H, W), grid, padding_mode="border", align_corners=True).reshape(-1)
    return inside & torch.where(s > 0.0, z < s + eps, torch.ones_like(inside))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tntcull_bench.json"))
    ap.add_argument("--faces", type=int, default=10_000_000)
    ap.add_argument("--views", type=int, default=150)
    ap.add_argument("--view-batch", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_tntcull_bench: no GPU -- nothing is measured without one")
    import tnt_cull as tcu
    from diff_gaussian_rasterization import _C
    dev = "cuda:0"
    verts, faces, c2w = make_scene(args.faces, args.views)
    v32, f = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    v64 = v32.double()
    V, F = v32.shape[0], f.shape[0]
    render_w2c, test_w2c = tcu._world_to_camera(c2w, "opencv"), tcu._world_to_camera(c2w)
    L = tcu._lib()
    counts = torch.zeros(V, dtype=torch.int32, device=dev)
    stats, total = torch.zeros(4, dtype=torch.int64, device=dev), np.zeros(4, np.int64)
    ms = dict(render_setup_and_small_boxes=0.0, render_queued_and_resolve=0.0, vertex_test=0.0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    stream = _C._stream(torch.device(dev))
    depths_kept = None
    for rnd in ("warm-up", "timed"):
        for b in range(0, args.views if rnd == "timed" else args.view_batch, args.view_batch):
            w = render_w2c[b:b + args.view_batch]
            B = w.shape[0]
            depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
            nbytes = L.radegs_tntcull_render_bytes(F, B)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            cams64, cams32 = tcu._cameras_to(dev, w, torch.float64), tcu._cameras_to(dev, test_w2c[b:b + B], torch.float32)
            a = (V, F, _C._ptr(v64), _C._ptr(f), B, _C._ptr(cams64), H, W, *K, 0.01, 20.0, _C._ptr(ws), nbytes, _C._ptr(depth))
            ev[0].record()
            tcu._check(L.radegs_tntcull_render_begin(*a, stream), "render_begin")
            ev[1].record()
            tcu._check(L.radegs_tntcull_render_finish(*a, _C._ptr(stats), stream), "render_finish")
            ev[2].record()
            tcu._check(L.radegs_tntcull_count_views(V, _C._ptr(v32), B, H, W, _C._ptr(depth), _C._ptr(cams32), *K, 0.005,
                                                    _C._ptr(counts if rnd == "timed" else torch.zeros_like(counts)), stream), "count_views")
            ev[3].record()
            torch.cuda.synchronize()
            if rnd == "timed":
                for key, i in zip(ms, range(3)):
                    ms[key] += ev[i].elapsed_time(ev[i + 1])
                total += stats.cpu().numpy()
                if b == 0:
                    depths_kept = depth
    n = args.views
    render_ms = (ms["render_setup_and_small_boxes"] + ms["render_queued_and_resolve"]) / n
    # the eager restatement, camera by camera as upstream, on the first batch's maps (the same work per camera for the others)
    Bk = depths_kept.shape[0]
    w32 = torch.from_numpy(test_w2c[:Bk]).to(dev, torch.float32)
    eager_counts = torch.zeros(V, dtype=torch.int32, device=dev)
    for k in range(Bk):
        eager_seen(v32, depths_kept[k], w32[k])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(Bk):
        eager_counts += eager_seen(v32, depths_kept[k], w32[k]).int()
    e1.record()
    torch.cuda.synchronize()
    eager_ms = e0.elapsed_time(e1) / Bk
    ours = torch.zeros(V, dtype=torch.int32, device=dev)
    tcu._count(v32, depths_kept, test_w2c[:Bk], K, 0.005, ours)
    kept_v, kept_f = tcu.cull_mesh(v32, f, c2w, pose="opencv", view_batch=args.view_batch)
    covered = float((depths_kept[0] > 0).float().mean())
    result = dict(
        note="SYNTHETIC scene: a bumpy unit sphere as a lat / lon grid in grid order plus a two-triangle floor, ring cameras at radius 3, 1920 x 1080, "
             "the reference's intrinsics; an estimate of a marching-tetrahedra mesh, not one.  No render reference exists on this box (no EGL).",
        device=torch.cuda.get_device_name(0), sizes=dict(vertices=V, faces=F, views=n, view_batch=args.view_batch, H=H, W=W),
        ms_per_view=dict(render=render_ms, render_setup_and_small_boxes=ms["render_setup_and_small_boxes"] / n,
                         render_queued_and_resolve=ms["render_queued_and_resolve"] / n, vertex_test=ms["vertex_test"] / n,
                         vertex_test_eager_torch=eager_ms),
        ratio_eager_torch_over_kernel_vertex_test=eager_ms / (ms["vertex_test"] / n),
        render_million_triangles_per_second=F / render_ms / 1e3,
        triangle_stream=dict(bytes_per_view=F * STREAM_BYTES_PER_FACE, hbm_peak_bytes_per_second=HBM_PEAK,
                             fraction_of_hbm_peak=F * STREAM_BYTES_PER_FACE / (render_ms * 1e-3) / HBM_PEAK,
                             fraction_of_hbm_peak_setup_kernel_alone=F * STREAM_BYTES_PER_FACE / (ms["render_setup_and_small_boxes"] / n * 1e-3) / HBM_PEAK),
        split=dict(queue_chunks=int(total[0]), triangles_drawn_in_place=int(total[1]), triangles_queued=int(total[2]),
                   chunks_drawn_in_place_queue_full=int(total[3]), triangle_view_pairs=F * n),
        first_view_fraction_of_pixels_covered=covered,
        vertex_test_points_where_eager_torch_counts_differ=int((ours != eager_counts).sum()), vertex_test_views_compared=Bk,
        cull=dict(vertices_kept=int(kept_v.shape[0]), faces_kept=int(kept_f.shape[0])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
