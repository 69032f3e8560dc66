"""Times the Tanks-and-Temples evaluation (tnt_eval.evaluate's stages) on the GPU and the same nearest-neighbour work through scipy's
cKDTree with workers=16 -- the path of tests/tnteval_restatement.py, standing in for Open3D's kd-tree, which is not installed.

    python scripts/gpu_tnteval_bench.py [--out profiles/tnteval_bench.json] [--mesh-vertices 700000] [--gt 4000000] [--ref-budget 180]

The scene is SYNTHETIC: a bumpy unit sphere, a mesh of `mesh-vertices` vertices (three times that many points with the centroids), a
ground-truth cloud of `gt` points, tau = 0.005 (mesh points about tau / 2 apart, scan points about tau / 3), 2 % of the mesh's points
floating more than 80 tau off the surface, a concave crop polygon that keeps a little over half of both clouds, and an initial alignment off
by 1 degree, 0.5 % of scale and 2 tau.  Those proportions are an ESTIMATE of a Tanks-and-Temples scan's (whose clouds hold 10^6..10^7
points after the crop), not a measurement: no such data was available when this was written.  The output says so.

Each GPU stage is timed with the host clock around work that ends in a device synchronise (the stages contain their own host reads), after
one untimed run of the whole pipeline at the same size.  The kd-tree side repeats, per registration round, one evaluation (tree build
apart) on the clouds the GPU produced and multiplies by the number of evaluations the GPU ran, and runs the two final distance passes
unbounded, as upstream does.  If its estimate exceeds `--ref-budget` seconds the queries are cut to a stated fraction and scaled."""
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

TAU = 0.005


def make_scene(n_vertices, n_gt, seed=0):
    rng = np.random.default_rng(seed)
    radius = lambda th, ph: 1.0 + 0.1 * np.sin(3 * th) * np.cos(4 * ph) + 0.06 * np.cos(5 * th + 1.0)
    nlat = int(np.sqrt(n_vertices / 2))
    nlon = 2 * nlat
    th, ph = np.meshgrid(np.pi * (np.arange(nlat + 1)) / nlat, 2 * np.pi * np.arange(nlon) / nlon, indexing="ij")
    r = radius(th, ph) * (1 + 0.002 * rng.standard_normal(th.shape))
    verts = (np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1) * r[..., None]).reshape(-1, 3)
    a, b = np.meshgrid(np.arange(nlat), np.arange(nlon), indexing="ij")
    at = lambda i, j: i * nlon + (j % nlon)
    faces = np.concatenate([np.stack([at(a, b), at(a + 1, b), at(a + 1, b + 1)], -1).reshape(-1, 3),
                            np.stack([at(a, b), at(a + 1, b + 1), at(a, b + 1)], -1).reshape(-1, 3)], 0)
    n_float = verts.shape[0] // 50                                   # floaters: 2 % of the vertices, each a tiny triangle of its own
    d = rng.standard_normal((n_float, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    base = d * rng.uniform(1.7, 2.1, (n_float, 1))
    tri = (base[:, None, :] + 1e-3 * rng.standard_normal((n_float, 3, 3))).reshape(-1, 3)
    faces = np.concatenate([faces, verts.shape[0] + np.arange(3 * n_float).reshape(-1, 3)], 0)
    verts = np.concatenate([verts, tri], 0)
    d = rng.standard_normal((n_gt, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    gt = d * (radius(np.arccos(np.clip(d[:, 2], -1, 1)), np.arctan2(d[:, 1], d[:, 0])) + 0.0005 * rng.standard_normal(n_gt))[:, None]
    c, s = np.cos(np.radians(1.0)), np.sin(np.radians(1.0))
    init = np.eye(4)
    init[:3, :3] = 1.005 * np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    init[:3, 3] = np.array([1.2, -1.0, 1.2]) * TAU
    polygon = np.array([[-2.3, 0.0, -2.3], [2.3, 0.0, -2.2], [2.2, 0.0, 2.3], [0.2, 0.0, 0.4], [-2.2, 0.0, 2.2]])
    return dict(vertices=verts.astype(np.float32).astype(np.float64), faces=faces.astype(np.int64), gt=gt.astype(np.float32).astype(np.float64),
                init=init, volume=("Y", -0.4, 2.5, polygon))


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def registration(te, t, tag, pcd, gt, init, vol, voxel, threshold, cell=None):
    """one round with its stages timed apart; the result as tnt_eval's own registration_* returns it"""
    (s_crop, _), t[tag + "_crop_source"] = timed(lambda: te.crop_points(pcd, vol, init))
    (t_crop, _), t[tag + "_crop_target"] = timed(lambda: te.crop_points(gt, vol))
    if voxel is None:
        s, tg = te._uniform(s_crop), te._uniform(t_crop)
    else:
        (s, _), t[tag + "_voxel_source"] = timed(lambda: te.voxel_down_sample(s_crop, voxel))
        (tg, _), t[tag + "_voxel_target"] = timed(lambda: te.voxel_down_sample(t_crop, voxel))
    reg, t[tag + "_icp"] = timed(lambda: te.icp(s, tg, threshold, max_iter=20, cell=cell))
    reg["transformation"] = reg["transformation"] @ init
    reg["s"], reg["t"] = s, tg
    return reg


def gpu_side(scene, dev):
    import tnt_eval as te
    v, f, gt = (torch.from_numpy(scene[k]).to(dev) for k in ("vertices", "faces", "gt"))
    vol = te.CropVolume(*scene["volume"])
    times, out = {}, None
    for run in ("warm-up", "timed"):
        t = {}
        pcd, t["mesh_points"] = timed(lambda: te.mesh_points(v, f))
        r2 = registration(te, t, "r2", pcd, gt, scene["init"], vol, TAU, 80 * TAU)
        r3 = registration(te, t, "r3", pcd, gt, r2["transformation"], vol, TAU / 2, 20 * TAU)
        r = registration(te, t, "r", pcd, gt, r3["transformation"], vol, None, 2 * TAU)
        (s_crop, _), t["eval_crop_source"] = timed(lambda: te.crop_points(pcd, vol, r["transformation"]))
        (t_crop, _), t["eval_crop_target"] = timed(lambda: te.crop_points(gt, vol))
        (s, _), t["eval_voxel_source"] = timed(lambda: te.voxel_down_sample(s_crop, TAU / 2))
        (tg, _), t["eval_voxel_target"] = timed(lambda: te.voxel_down_sample(t_crop, TAU / 2))
        cut = te.distance_cut(TAU, 5)
        (d1, _), t["eval_dist_source_to_target"] = timed(lambda: te.cloud_distances(s, tg, cut))
        (d2, _), t["eval_dist_target_to_source"] = timed(lambda: te.cloud_distances(tg, s, cut))
        scores, t["eval_histogram"] = timed(lambda: te.precision_recall(d1, d2, TAU))
        times[run] = t
        out = dict(r2=r2, r3=r3, r=r, s=s, t=tg, scores=scores[:3])
    cells = {}                                                       # the first round's hopeless queries against the choice of `cell`
    s, tg = out["r2"]["s"], out["r2"]["t"]
    for per in (4, 8, 16, 32):
        te.icp(s, tg, 80 * TAU, max_iter=1, cell=80 * TAU / per)
        _, sec = timed(lambda: te.icp(s, tg, 80 * TAU, max_iter=1, cell=80 * TAU / per))
        cells["max_dist/%d" % per] = sec / 2                         # two evaluations
    return times["timed"], times["warm-up"], out, cells


def kdtree_side(out, budget):
    from scipy.spatial import cKDTree
    res, clouds = {}, {}
    plan = [("r2", 80 * TAU), ("r3", 20 * TAU), ("r", 2 * TAU)]
    for tag, _ in plan:
        clouds[tag] = (out[tag]["s"].cpu().numpy(), out[tag]["t"].cpu().numpy())
    s_eval, t_eval = out["s"].cpu().numpy(), out["t"].cpu().numpy()
    t0 = time.perf_counter()
    probe = cKDTree(clouds["r2"][1])
    build = time.perf_counter() - t0
    n_probe = min(20000, clouds["r2"][0].shape[0])
    t0 = time.perf_counter()
    probe.query(clouds["r2"][0][:n_probe], k=1, distance_upper_bound=80 * TAU, workers=16)
    per_query = (time.perf_counter() - t0) / n_probe
    total_queries = sum(clouds[tag][0].shape[0] for tag, _ in plan) + s_eval.shape[0] + t_eval.shape[0]
    estimate = per_query * total_queries + 5 * build
    fraction = 1.0 if estimate <= budget else max(budget / estimate, 0.01)
    res["fraction_of_queries"] = fraction
    sub = lambda q: q if fraction >= 1 else q[np.random.default_rng(1).choice(q.shape[0], max(int(q.shape[0] * fraction), 1), replace=False)]
    for tag, max_dist in plan:
        s, tg = clouds[tag]
        t0 = time.perf_counter()
        tree = cKDTree(tg)
        res[tag + "_tree_build"] = time.perf_counter() - t0
        q = sub(s)
        t0 = time.perf_counter()
        tree.query(q, k=1, distance_upper_bound=max_dist, workers=16)
        res[tag + "_one_evaluation"] = (time.perf_counter() - t0) / fraction
        res[tag + "_evaluations"] = len(out[tag]["history"])
        res[tag + "_icp"] = res[tag + "_tree_build"] + res[tag + "_one_evaluation"] * res[tag + "_evaluations"]
    for name, cloud, queries in (("eval_dist_source_to_target", t_eval, s_eval), ("eval_dist_target_to_source", s_eval, t_eval)):
        t0 = time.perf_counter()
        tree = cKDTree(cloud)
        build = time.perf_counter() - t0
        q = sub(queries)
        t0 = time.perf_counter()
        tree.query(q, k=1, workers=16)
        res[name] = build + (time.perf_counter() - t0) / fraction
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tnteval_bench.json"))
    ap.add_argument("--mesh-vertices", type=int, default=700_000)
    ap.add_argument("--gt", type=int, default=4_000_000)
    ap.add_argument("--ref-budget", type=float, default=180.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_tnteval_bench: no GPU -- nothing is measured without one")
    dev = "cuda:0"
    scene = make_scene(args.mesh_vertices, args.gt)
    gpu, warm, out, cells = gpu_side(scene, dev)
    sizes = dict(mesh_vertices=int(scene["vertices"].shape[0]), mesh_faces=int(scene["faces"].shape[0]), gt=int(scene["gt"].shape[0]))
    for tag in ("r2", "r3", "r"):
        sizes[tag] = dict(source=int(out[tag]["s"].shape[0]), target=int(out[tag]["t"].shape[0]), evaluations=len(out[tag]["history"]),
                          fitness=out[tag]["fitness"], inlier_rmse=out[tag]["inlier_rmse"])
    sizes["eval"] = dict(source=int(out["s"].shape[0]), target=int(out["t"].shape[0]))
    result = dict(note="SYNTHETIC scene: a bumpy unit sphere, tau = %g, %d mesh vertices (+ centroids), %d ground-truth points, 2 %% floaters; these "
                       "proportions are an estimate of a Tanks-and-Temples scan's, no such data was available" % (TAU, sizes["mesh_vertices"], sizes["gt"]),
                  device=torch.cuda.get_device_name(0), sizes=sizes, scores=[float(x) for x in out["scores"]], gpu_seconds=gpu,
                  gpu_seconds_first_run=warm, gpu_total=sum(gpu.values()), r2_seconds_per_evaluation_by_cell=cells)
    ref = kdtree_side(out, args.ref_budget)
    result["ckdtree_workers16_seconds"] = ref
    keys = ("r2_icp", "r3_icp", "r_icp", "eval_dist_source_to_target", "eval_dist_target_to_source")
    result["ratio_ckdtree_over_gpu"] = {k: ref[k] / gpu[k] for k in keys}
    result["ratio_note"] = ("kd-tree ICP rounds = tree build + one evaluation's query x the evaluations the GPU ran (the sums and the SVD are not in "
                            "it); queries cut to the stated fraction are scaled linearly")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
