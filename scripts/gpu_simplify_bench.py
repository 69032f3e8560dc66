"""Times mesh_simplify.simplify_vertex_clustering on the GPU, stage by stage and as a whole, at three voxel sizes (about 10x, 100x and 1000x
fewer faces) and both contractions, and the NumPy restatement of the whole call (tests/simplify_restatement.py) on the same box's host: the
disclosed comparison (Open3D and MeshLab, which upstream's users call, are not on this box).

    python scripts/gpu_simplify_bench.py [--out profiles/simplify_bench.json] [--faces 4000000] [--floaters 2000] [--repeats 7] [--no-host]

The mesh is the SYNTHETIC one of scripts/gpu_meshclean_bench.py: a jittered grid sheet of about `faces` triangles in grid order plus detached
strips, float32 vertices.  Stage times are device events around each stage of the call (a stage is several kernels: its sorts and scans
included), the whole call is wall clock around the public function with a device synchronisation either side, host reads and allocations
included: medians of `repeats` runs after two untimed ones.  There is no threshold: the numbers are recorded."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rade-gs_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from gpu_meshclean_bench import make_mesh  # noqa: E402

VOXELS = (3.2, 10.0, 31.6)      # the sheet has unit spacing: a cell of side s folds about s^2 faces into one


def event_ms(fn, repeats, warmup=2):
    """(median ms, runs) of fn on the device, by events on the current stream"""
    out = []
    for i in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return float(np.median(out)), [round(x, 3) for x in out]


def wall_ms(fn, repeats, warmup=2):
    out = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(x, 3) for x in out]


def run_lengths(vertex_cell, faces, K):
    """corner records and vertices per cell: what the per-cell kernels walk"""
    rec = torch.bincount(vertex_cell[faces.reshape(-1)], minlength=K).double()
    mem = torch.bincount(vertex_cell, minlength=K).double()
    q = torch.tensor([0.5, 0.9, 0.99], dtype=torch.float64, device=rec.device)
    stat = lambda t: dict(mean=float(t.mean()), p50=float(torch.quantile(t, q[0])), p90=float(torch.quantile(t, q[1])), p99=float(torch.quantile(t, q[2])),
                          max=float(t.max()), share_of_cells_with_at_most_8=float((t <= 8).double().mean()))
    return dict(corner_records_per_cell=stat(rec), vertices_per_cell=stat(mem))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_bench.json"))
    ap.add_argument("--faces", type=int, default=4_000_000)
    ap.add_argument("--floaters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_simplify_bench: no GPU -- nothing is measured without one")
    import mesh_simplify as ms
    import simplify_restatement as sr
    dev = "cuda:0"
    verts, faces = make_mesh(args.faces, args.floaters)
    colours = np.random.default_rng(2).uniform(0.0, 1.0, verts.shape).astype(np.float32)
    v, f, a = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(colours).to(dev)
    v64, a64 = v.double(), a.double()
    lo, hi = ms._bounds(v64)
    for _ in range(3):                                   # the clock settles on real work before anything is timed
        ms.simplify_vertex_clustering(v, f, VOXELS[1], attributes=a)
    torch.cuda.synchronize()
    sizes = []
    for h in VOXELS:
        origin, max_key = ms._grid(lo, hi, h, None)
        cells = ms._cells(v64, origin, h, max_key)
        cell_faces, remove = ms._cell_faces(f, v.shape[0], cells, True)
        ws, nv, nf = ms._compact_plan(cells.K, cell_faces, remove, True)
        stage, runs = {}, {}

        def record(name, fn):
            stage[name], runs[name] = event_ms(fn, args.repeats)
        record("cells", lambda: ms._cells(v64, origin, h, max_key))
        record("faces_with_duplicate_search", lambda: ms._cell_faces(f, v.shape[0], cells, True))
        record("faces_without_duplicate_search", lambda: ms._cell_faces(f, v.shape[0], cells, False))
        record("compact_plan", lambda: ms._compact_plan(cells.K, cell_faces, remove, True))
        record("compact_apply_and_face_source", lambda: ms._compact_apply(cells.K, cell_faces, ws, nv, nf))
        record("vertices_average", lambda: ms._cell_vertices(v64, f, a64, cells, origin, h, 0))
        record("vertices_quadric", lambda: ms._cell_vertices(v64, f, a64, cells, origin, h, 1))
        whole, whole_runs = {}, {}
        for contraction in ms.CONTRACTIONS:
            whole[contraction], whole_runs[contraction] = wall_ms(lambda: ms.simplify_vertex_clustering(v, f, h, contraction, attributes=a), args.repeats)
        entry = dict(voxel_size=h, cells=cells.K, vertices_out=nv, faces_out=nf, reduction=float(f.shape[0]) / max(nf, 1),
                     run_lengths=run_lengths(cells.vertex_cell, f, cells.K), stage_ms=stage, stage_ms_runs=runs,
                     whole_call_ms=whole, whole_call_ms_runs=whole_runs)
        if not args.no_host:
            t0 = time.perf_counter()
            want = sr.simplify_vertex_clustering(verts, faces, h, "quadric", attributes=colours)
            entry["host_numpy_restatement_quadric_ms"] = (time.perf_counter() - t0) * 1e3
            got = ms.simplify_vertex_clustering(v, f, h, "quadric", attributes=a)
            entry["gpu_equals_the_restatement_bit_for_bit"] = bool(all(np.array_equal(g.cpu().numpy().view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
                                                                       for g, w in zip(got, want)))
        sizes.append(entry)
        print(json.dumps(entry), flush=True)
    result = dict(
        note="SYNTHETIC mesh: one jittered grid sheet in grid order plus detached strips of 5 to 100 triangles, float32 vertices, three float32 "
             "attribute columns.  stage_ms: device events around one stage of the call (its sorts, scans and allocations included), whole_call_ms: "
             "wall clock around the public call, synchronised, host reads included; medians of the listed runs after two untimed ones.  The host "
             "figure is tests/simplify_restatement.py (NumPy, vectorised) on this box's CPU for the whole quadric call; Open3D and MeshLab are not "
             "installed here and were not timed.",
        device=torch.cuda.get_device_name(0), host_cpus_available=len(os.sched_getaffinity(0)),
        input=dict(vertices=int(v.shape[0]), faces=int(f.shape[0]), corner_records=int(3 * f.shape[0]), floaters=args.floaters), sizes=sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
