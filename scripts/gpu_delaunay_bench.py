"""Times delaunay.triangulate on the GPU, stage by stage, and on the same box's host scipy.spatial.Delaunay (Qhull, one thread) over the
same points: the disclosed comparison, CGAL (which upstream calls through tetranerf) is not on this box.

    python scripts/gpu_delaunay_bench.py [--out profiles/delaunay_bench.json] [--points 1000000] [--gaussians 1000000] [--repeats 3] [--no-host] [--single]

Two inputs: `points` uniform random float32 points in the unit cube, and the 9 P box points tetmesh.tetra_points makes of synth_scene's
`gaussians` Gaussians (a frustum-filling SYNTHETIC scene, not a trained one).  Stages, each wall clock with a device synchronisation either
side, host reads and allocations included: `bounds` (the box and the float64 copy), `plan` (perturb, grid, both cell kernels: the records),
`emit` (two sorts, run lengths, oriented rows), and `triangulate`, the public call as a caller sees it.  Median of `repeats` calls after one
untimed call.  `--single` instead runs the stages ONCE per input, with no untimed call before them and no retry, for inputs where a call takes
minutes, and then the public call once, which retries where the first attempt was inconsistent.  There is no threshold: the numbers are recorded, with how many points the one-wave-per-point kernel had to finish."""
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


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(x, 3) for x in out]


def measure_single(points):
    """one attempt at the default jitter and seed, the stages of triangulate called once each; no retry, so `inconsistent` is reported as found"""
    import delaunay
    ms = {}

    def stage(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms[name] = (time.perf_counter() - t0) * 1e3
        return out
    p, (box, diag) = stage("bounds", lambda: (lambda q: (q, delaunay._bounds(q)))(delaunay._points(points)))
    ws, nbytes, capacity, (records, deferred, uncertain, overflow) = stage("plan", lambda: delaunay._plan(p, box, 1e-9 * diag, 0))
    print(json.dumps(dict(plan_ms=ms["plan"], records=records, deferred=deferred, uncertain=uncertain, overflow=overflow)), flush=True)
    _, unique, inconsistent = stage("emit", lambda: delaunay._emit(p.shape[0], ws, nbytes, capacity, records))
    del ws
    public = {}
    try:                                   # the public call, retries and all, once
        _, info = stage("triangulate", lambda: delaunay.triangulate(points, return_info=True))
        public = dict(retries=int(info["retries"]), tets=int(info["tets"]), uncertain=int(info["uncertain"]), inconsistent=int(info["inconsistent"]))
    except RuntimeError as e:
        public = dict(refused=str(e))
    return dict(public_call=public, points=int(points.shape[0]), single_call=True, tets=int(unique), records=int(records), inconsistent=int(inconsistent), uncertain=int(uncertain),
                deferred=int(deferred), overflow=int(overflow), workspace_bytes=int(nbytes), record_capacity=int(capacity), gpu_ms=ms)


def measure(points, repeats, host, single=False):
    import delaunay
    if single:
        return measure_single(points)
    state = {}

    def bounds():
        state["p"] = delaunay._points(points)
        state["bounds"], state["diag"] = delaunay._bounds(state["p"])

    def plan():
        state["plan"] = delaunay._plan(state["p"], state["bounds"], 1e-9 * state["diag"], 0)

    def emit():
        ws, nbytes, capacity, counts = state["plan"]
        state["emit"] = delaunay._emit(state["p"].shape[0], ws, nbytes, capacity, counts[0])

    ms, runs = {}, {}
    for name, fn in (("bounds", bounds), ("plan", plan), ("emit", emit), ("triangulate", lambda: delaunay.triangulate(points))):
        ms[name], runs[name] = timed(fn, repeats)
    _, nbytes, capacity, (records, deferred, uncertain, overflow) = state["plan"]
    cells, unique, inconsistent = state["emit"]
    out = dict(points=int(points.shape[0]), tets=int(unique), records=int(records), inconsistent=int(inconsistent), uncertain=int(uncertain),
               deferred=int(deferred), overflow=int(overflow), workspace_bytes=int(nbytes), record_capacity=int(capacity), gpu_ms=ms, gpu_ms_runs=runs)
    if host:
        from scipy.spatial import Delaunay
        X = delaunay.perturbed(points).cpu().numpy()
        t0 = time.perf_counter()
        tri = Delaunay(X)
        out["host_scipy"] = dict(seconds=time.perf_counter() - t0, tets=int(tri.simplices.shape[0]), coplanar=int(tri.coplanar.size))
        out["ratio_host_scipy_over_gpu_triangulate"] = out["host_scipy"]["seconds"] * 1e3 / ms["triangulate"]
        if tri.simplices.shape[0] == unique:
            out["host_scipy"]["same_cells_as_gpu"] = bool(np.array_equal(np.unique(np.sort(tri.simplices, axis=1), axis=0), np.sort(cells.cpu().numpy(), axis=1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delaunay_bench.json"))
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--single", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_delaunay_bench: no GPU -- nothing is measured without one")
    import synth_scene
    import tetmesh
    dev = "cuda:0"
    result = dict(
        note="GPU times are wall clock around the call, synchronised, host reads and allocations included; median of the listed runs after one "
             "untimed call.  `plan` holds both cell kernels; `deferred` is the number of points the one-wave-per-point kernel finished, each by a scan "
             "of all points.  The host figure is scipy.spatial.Delaunay (Qhull, one thread) on this box's CPU over the same perturbed float64 "
             "points; CGAL is not installed here and was not timed.  The tetra cloud comes from a SYNTHETIC frustum-filling scene.",
        device=torch.cuda.get_device_name(0), host_cpus_available=len(os.sched_getaffinity(0)))
    if args.points:
        uniform = torch.from_numpy(np.random.default_rng(0).random((args.points, 3)).astype(np.float32)).to(dev)
        result["uniform"] = measure(uniform, args.repeats, not args.no_host, args.single)
        print(json.dumps(result["uniform"]), flush=True)
    if args.gaussians:
        scene = synth_scene.make_scene(args.gaussians, 1280, 720)
        cloud, _ = tetmesh.tetra_points(scene.means3D.to(dev), scene.scales.to(dev), scene.rotations.to(dev))
        result["tetra_cloud"] = dict(gaussians=args.gaussians, **measure(cloud, args.repeats, False, args.single))
        print(json.dumps(result["tetra_cloud"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
