"""Times the five public functions of mesh_clean on the GPU and, on the same box's host, scipy.sparse.csgraph.connected_components over the
same adjacency: the disclosed comparison for the clustering step (Open3D and trimesh, which upstream calls, are not on this box).

    python scripts/gpu_meshclean_bench.py [--out profiles/meshclean_bench.json] [--faces 4000000] [--floaters 2000] [--repeats 5]

The mesh is SYNTHETIC: one jittered grid sheet of about `faces` triangles in grid order plus `floaters` detached strips of 5 to 100
triangles, float32 vertices -- the shape of a TSDF or marching-tetrahedra mesh before its floater filter, not one.  Every function is timed
as a caller sees it, wall clock around the call with a device synchronisation either side, its host reads and its allocations included: the
median of `repeats` calls after one untimed call.  There is no threshold: the numbers are recorded."""
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


def make_mesh(n_faces, n_floaters, seed=0):
    rng = np.random.default_rng(seed)
    n = max(2, int(np.sqrt(n_faces / 2)))
    gx, gy = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="xy")
    verts = [np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros(gx.size)], 1).astype(np.float64)]
    q = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    faces = [np.concatenate([np.stack([q, q + 1, q + n + 2], 1), np.stack([q, q + n + 2, q + n + 1], 1)])]
    base = verts[0].shape[0]
    for k, m in enumerate(rng.integers(5, 101, n_floaters)):
        i = np.arange(m + 2)
        verts.append(np.stack([i // 2 + 3.0 * (k % 1000), i % 2 + 3.0 * (k // 1000), np.full(m + 2, 5.0)], 1).astype(np.float64))
        t = np.arange(m) + base
        faces.append(np.stack([t, t + 1, t + 2], 1))
        base += m + 2
    verts = np.concatenate(verts)
    verts += rng.uniform(-0.2, 0.2, verts.shape)
    return verts.astype(np.float32), np.concatenate(faces).astype(np.int64)


def host_components(faces):
    """(seconds to build the adjacency, seconds in connected_components, labels): the triangles of equal neighbours among the sorted edge
    records are joined, the rule of adjacency "edge" """
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    F = faces.shape[0]
    a, b = faces.reshape(-1), np.roll(faces, -1, axis=1).reshape(-1)
    key = (np.minimum(a, b).astype(np.uint64) << np.uint64(32)) | np.maximum(a, b).astype(np.uint64)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    same = (ks[1:] == ks[:-1]) & (a[order][1:] != b[order][1:])
    rows, cols = order[:-1][same] // 3, order[1:][same] // 3
    graph = sp.coo_matrix((np.ones(rows.shape[0], np.int8), (rows, cols)), shape=(F, F)).tocsr()
    t1 = time.perf_counter()
    n, labels = connected_components(graph, directed=False)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, n, labels


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshclean_bench.json"))
    ap.add_argument("--faces", type=int, default=4_000_000)
    ap.add_argument("--floaters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_meshclean_bench: no GPU -- nothing is measured without one")
    import mesh_clean as mcl
    dev = "cuda:0"
    verts, faces = make_mesh(args.faces, args.floaters)
    v, f = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    remove = torch.from_numpy(np.random.default_rng(1).random(faces.shape[0]) < 0.1).to(dev)
    calls = dict(
        cluster_connected_triangles=lambda: mcl.cluster_connected_triangles(f, v),
        cluster_connected_triangles_without_areas=lambda: mcl.cluster_connected_triangles(f),
        cluster_connected_triangles_manifold_edge=lambda: mcl.cluster_connected_triangles(f, v, "manifold_edge"),
        remove_triangles_by_mask=lambda: mcl.remove_triangles_by_mask(v, f, remove),
        remove_unreferenced_vertices=lambda: mcl.remove_unreferenced_vertices(v, f),
        remove_degenerate_triangles=lambda: mcl.remove_degenerate_triangles(f),
        post_process_mesh=lambda: mcl.post_process_mesh(v, f),
        get_connected_mesh=lambda: mcl.get_connected_mesh(v, f, False, 0.2),
        compute_vertex_normals=lambda: mcl.compute_vertex_normals(v, f))
    ms, runs = {}, {}
    for name, fn in calls.items():
        ms[name], runs[name] = timed(fn, args.repeats)
    labels, counts, _ = mcl.cluster_connected_triangles(f, v)
    v1, f1, _ = mcl.post_process_mesh(v, f)
    build_s, cc_s, n_host, host_labels = host_components(faces)
    _, first, inverse = np.unique(host_labels, return_index=True, return_inverse=True)
    same_partition = bool(np.array_equal(np.argsort(np.argsort(first))[inverse], labels.cpu().numpy()))
    result = dict(
        note="SYNTHETIC mesh: one jittered grid sheet in grid order plus detached strips of 5 to 100 triangles, float32 vertices.  GPU times are wall "
             "clock around the public call, synchronised, host reads and allocations included; median of the listed runs after one untimed call.  "
             "The host figure is scipy.sparse.csgraph.connected_components on this box's CPU over the same adjacency, with the NumPy time to "
             "build that adjacency listed apart; Open3D and trimesh are not installed here and were not timed.",
        device=torch.cuda.get_device_name(0), host_cpus_available=len(os.sched_getaffinity(0)),
        sizes=dict(vertices=int(v.shape[0]), faces=int(f.shape[0]), clusters=int(counts.shape[0]), floaters=args.floaters,
                   faces_after_post_process_mesh=int(f1.shape[0]), vertices_after_post_process_mesh=int(v1.shape[0])),
        gpu_ms=ms, gpu_ms_runs=runs,
        host_scipy=dict(build_adjacency_ms=build_s * 1e3, connected_components_ms=cc_s * 1e3, clusters=int(n_host),
                        same_partition_as_gpu=same_partition),
        ratio_host_connected_components_over_gpu_cluster_without_areas=cc_s * 1e3 / ms["cluster_connected_triangles_without_areas"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
