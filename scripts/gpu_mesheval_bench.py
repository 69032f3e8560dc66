"""Times mesh evaluation (mesh_eval.dtu_chamfer's stages) on the GPU and, where sklearn can be imported, the same stages through the
reference's own calls (sklearn's kd-tree with n_jobs=16 and the Python thinning loop of dtu_eval/eval.py).

    python scripts/gpu_mesheval_bench.py [--out profiles/mesheval_bench.json] [--area 1e5] [--stl 3000000] [--ref-budget 180]

The scan is SYNTHETIC: a bumpy sphere of about `area` mm^2 sampled at 0.2 mm and a ground-truth cloud of `stl` points around it.  Those
proportions are an estimate of a DTU scan's, not a measurement: no DTU data was available when this was written.  The output says so.

Each GPU stage is timed with the host clock around work that ends in a device synchronise (the stages contain their own host reads),
after one untimed run of the whole pipeline at the same size.  The reference side first runs on a spherical cap holding a tenth of the
surface (same densities); if ten times that fits `--ref-budget` seconds it runs at the full size, otherwise the tenth is what is
reported, with the fraction stated."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rade-gs_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

DENSITY, MAX_DIST, PATCH = 0.2, 20.0, 60.0


def make_scan(area, n_stl, seed=0):
    rng = np.random.default_rng(seed)
    R = float(np.sqrt(area / (4 * np.pi)))
    centre = np.array([50.0, -100.0, 650.0])
    edge = 0.7                                                   # mm: triangles a few samples across, as an extracted mesh's
    nlat, nlon = int(np.pi * R / edge), int(2 * np.pi * R / edge)
    th, ph = np.meshgrid(np.pi * np.arange(nlat + 1) / nlat, 2 * np.pi * np.arange(nlon) / nlon, indexing="ij")
    rad = R * (1 + 0.01 * np.sin(9 * th) * np.cos(7 * ph))
    verts = (np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1) * rad[..., None]).reshape(-1, 3) + centre
    verts = verts.astype(np.float32).astype(np.float64)
    a, b = np.meshgrid(np.arange(nlat), np.arange(nlon), indexing="ij")
    at = lambda i, j: i * nlon + (j % nlon)
    faces = np.concatenate([np.stack([at(a, b), at(a + 1, b), at(a + 1, b + 1)], -1).reshape(-1, 3),
                            np.stack([at(a, b), at(a + 1, b + 1), at(a, b + 1)], -1)[1:].reshape(-1, 3)], 0)
    d = rng.standard_normal((n_stl, 3))
    stl = centre + d / np.linalg.norm(d, axis=1, keepdims=True) * (R + 0.5 * rng.standard_normal((n_stl, 1)))
    half = int(np.ceil(R)) + 10
    BB = np.array([centre - half, centre + half])
    vol = np.ones((2 * half + 1,) * 3, np.uint8)
    vol[:, :, : half // 2] = 0                                   # the observation volume leaves the bottom quarter out
    plane = np.array([0.0, 0.0, 1.0, -(centre[2] - 0.8 * R)])
    return dict(vertices=verts, faces=faces, stl=stl, BB=BB, Res=1.0, vol=vol, plane=plane, R=R, centre=centre)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def gpu_side(scan, dev):
    import mesh_eval as me
    v, f, stl = (torch.from_numpy(scan[k]).to(dev) for k in ("vertices", "faces", "stl"))
    vol = torch.from_numpy(scan["vol"]).to(dev)
    times, keep_for_ref = {}, {}
    for run in ("warm-up", "timed"):
        t = {}
        (cloud, _), t["sample"] = timed(lambda: me.sample_mesh_points(v, f, DENSITY))
        perm = torch.randperm(cloud.shape[0], generator=torch.Generator(device=dev).manual_seed(1), device=dev)
        (down, keep, _), t["thin"] = timed(lambda: me.downsample_points(cloud, DENSITY, perm=perm))
        (inb, gin, obs), t["obs_mask"] = timed(lambda: me.obs_mask_select(down, vol, scan["BB"], scan["Res"], PATCH))
        data_in, data_in_obs = down[inb], down[obs]
        cell = MAX_DIST / me.NN_CELLS_PER_MAX_DIST
        (d2s, _), t["d2s"] = timed(lambda: me.PointGrid(stl, cell).nearest(data_in_obs, MAX_DIST))
        above, t["plane"] = timed(lambda: me.above_plane(stl, scan["plane"]))
        stl_above = stl[above]
        (s2d, _), t["s2d"] = timed(lambda: me.PointGrid(data_in, cell).nearest(stl_above, MAX_DIST))
        sums, t["means"] = timed(lambda: torch.stack([me.mean_below(d2s, MAX_DIST), me.mean_below(s2d, MAX_DIST)]).cpu().numpy())
        times[run] = t
        sizes = dict(triangles=int(f.shape[0]), cloud=int(cloud.shape[0]), kept=int(down.shape[0]), data_in=int(data_in.shape[0]),
                     data_in_obs=int(data_in_obs.shape[0]), stl=int(stl.shape[0]), stl_above=int(stl_above.shape[0]))
        keep_for_ref = dict(shuffled=cloud[perm].cpu().numpy(), keep=keep.cpu().numpy(), data_in=data_in.cpu().numpy(), data_in_obs=data_in_obs.cpu().numpy(),
                            stl_above=stl_above.cpu().numpy(), mean_d2s=float(sums[0, 0] / sums[0, 1]), mean_s2d=float(sums[1, 0] / sums[1, 1]))
    return times["timed"], times["warm-up"], sizes, keep_for_ref


def reference_side(scan, g, fraction):
    """eval.py's own calls on the cap z >= z0 that holds `fraction` of the sphere; returns times and whether the results agree"""
    import sklearn.neighbors as skln
    z0 = scan["centre"][2] + scan["R"] * (1 - 2 * fraction) if fraction < 1 else -np.inf
    cap = lambda p: p[p[:, 2] >= z0]
    shuffled, stl = cap(g["shuffled"]), cap(scan["stl"])
    t, out = {}, {}
    nn = skln.NearestNeighbors(n_neighbors=1, radius=DENSITY, algorithm="kd_tree", n_jobs=16)
    t0 = time.perf_counter()
    nn.fit(shuffled)
    lists = nn.radius_neighbors(shuffled, radius=DENSITY, return_distance=False)
    t["thin_radius_neighbors"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    mask = np.ones(shuffled.shape[0], dtype=np.bool_)
    for curr, idxs in enumerate(lists):
        if mask[curr]:
            mask[idxs] = 0
            mask[curr] = 1
    t["thin_loop"] = time.perf_counter() - t0
    t["thin"] = t["thin_radius_neighbors"] + t["thin_loop"]
    if fraction >= 1:
        out["thin_mask_equal"] = bool(np.array_equal(mask, g["keep"]))
    del lists
    queries = cap(g["data_in_obs"])
    t0 = time.perf_counter()
    nn.fit(stl)
    d, _ = nn.kneighbors(queries, n_neighbors=1, return_distance=True)
    t["d2s"] = time.perf_counter() - t0
    if fraction >= 1:
        out["mean_d2s_rel_diff"] = float(abs(d[d < MAX_DIST].mean() - g["mean_d2s"]) / g["mean_d2s"])
    cloud, queries = cap(g["data_in"]), cap(g["stl_above"])
    t0 = time.perf_counter()
    nn.fit(cloud)
    d, _ = nn.kneighbors(queries, n_neighbors=1, return_distance=True)
    t["s2d"] = time.perf_counter() - t0
    if fraction >= 1:
        out["mean_s2d_rel_diff"] = float(abs(d[d < MAX_DIST].mean() - g["mean_s2d"]) / g["mean_s2d"])
    out.update(fraction=fraction, seconds=t, points=int(shuffled.shape[0]), stl=int(stl.shape[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesheval_bench.json"))
    ap.add_argument("--area", type=float, default=1e5)
    ap.add_argument("--stl", type=int, default=3_000_000)
    ap.add_argument("--ref-budget", type=float, default=180.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_mesheval_bench: no GPU -- nothing is measured without one")
    dev = "cuda:0"
    scan = make_scan(args.area, args.stl)
    gpu, warm, sizes, g = gpu_side(scan, dev)
    result = dict(note="SYNTHETIC scan: a bumpy sphere of about %.0f mm^2 at 0.2 mm and %d ground-truth points; these proportions are an estimate of a "
                       "DTU scan's, no DTU data was available" % (args.area, args.stl),
                  device=torch.cuda.get_device_name(0), sizes=sizes, gpu_seconds=gpu, gpu_seconds_first_run=warm, gpu_total=sum(gpu.values()),
                  mean_d2s=g["mean_d2s"], mean_s2d=g["mean_s2d"])
    try:
        import sklearn  # noqa: F401
    except ImportError:
        result["reference"] = "unavailable: sklearn cannot be imported here"
    else:
        tenth = reference_side(scan, g, 0.1)
        result["reference_tenth"] = tenth
        estimate = 10 * sum(tenth["seconds"][k] for k in ("thin", "d2s", "s2d"))
        if estimate <= args.ref_budget:
            result["reference"] = reference_side(scan, g, 1.0)
        else:
            result["reference"] = dict(tenth, note="the full size was estimated at %.0f s, beyond the %.0f s budget: times are for a tenth of the surface" % (estimate, args.ref_budget))
        ref = result["reference"]
        scale = 1.0 / ref["fraction"]
        result["ratio_reference_over_gpu"] = {k: scale * ref["seconds"][k] / gpu[k] for k in ("thin", "d2s", "s2d")}
        if ref["fraction"] < 1:
            result["ratio_note"] = "reference times scaled linearly from the stated fraction"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
