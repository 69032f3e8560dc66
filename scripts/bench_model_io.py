"""Times the model state I/O on the GPU, step by step, and on the same box's host the restatement of upstream's path.

    python scripts/bench_model_io.py [--out profiles/modelio_bench.json] [--rows 1000000 5000000] [--host-rows 1000000] [--repeats 5] [--dir DIR]

For every row count, at SH degree 3 with the filter (63 floats = 252 B a record; the model itself is 60 floats = 240 B a row):
  pack / unpack kernel   device events around the launch alone, median of `repeats` after one untimed launch; bytes = rows x (240 + 252), the
                         bytes the algorithm must move, over that time, against the 6.3 TB/s a streaming kernel reaches on HBM
  device -> pinned, pinned -> device      the host-link copy of the whole payload, device events
  file write, file read  wall clock of writing the pinned payload to `--dir` and of reading it back into host memory; the file system is
                         whatever `--dir` is on and the page cache is warm: a property of this box, stated with the figure
  save_ply, load_ply     wall clock around the public call, synchronised: what a caller waits for
The host figures are the NumPy restatement of upstream's own statements at `--host-rows`: save_ply's `elements[:] = list(map(tuple,
attributes))` into the structured array and PlyData's write of it, and load_ply's per-column float64 copies followed by torch.tensor(...,
dtype=float) and the transposes (without the upload).  plyfile itself is not installed here and was not timed.  No threshold: recorded."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rade-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
HBM_STREAM_GBS = 6300.0


def events_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), [round(x, 4) for x in out]


def wall_ms(fn, repeats, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(x, 3) for x in out]


def gpu_side(P, folder, repeats, mio):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(P)
    K = 15
    t = [torch.randn(s, generator=g, device=dev) for s in ((P, 3), (P, 1, 3), (P, K, 3), (P, 1), (P, 3), (P, 4), (P, 1))]
    C, path = 63, os.path.join(folder, f"bench_{P}.ply")
    out = torch.empty((P, C), dtype=torch.float32, device=dev)
    pinned = torch.empty((P, C), dtype=torch.float32, pin_memory=True)
    res = dict(rows=P, payload_bytes=P * C * 4)
    moved = P * (240 + 252)

    def rate(ms):
        gbs = moved / ms / 1e6
        return dict(ms=ms, GB_per_s=gbs, share_of_6300_GB_per_s_streaming_HBM=gbs / HBM_STREAM_GBS)
    ms, runs = events_ms(lambda: mio._pack(t, P, K, 0, P, out, dev), repeats)
    res["pack_kernel"] = dict(rate(ms), runs_ms=runs)
    ms, runs = events_ms(lambda: pinned.copy_(out, non_blocking=True), repeats)
    res["device_to_pinned"] = dict(ms=ms, GB_per_s=P * C * 4 / ms / 1e6, runs_ms=runs)

    def write():
        with open(path, "wb") as f:
            f.write(pinned.numpy())
    ms, runs = wall_ms(write, repeats)
    res["file_write"] = dict(ms=ms, GB_per_s=P * C * 4 / ms / 1e6, runs_ms=runs)
    ms, runs = wall_ms(lambda: mio.save_ply(path, *t), repeats)
    res["save_ply"] = dict(ms=ms, runs_ms=runs)
    # ---- the way back ----
    header = mio.read_ply_header(path)
    ms, runs = wall_ms(lambda: mio._read_records(path, header), repeats)
    res["file_read"] = dict(ms=ms, GB_per_s=P * C * 4 / ms / 1e6, runs_ms=runs)
    buf, _, S, layout = mio._read_records(path, header)
    pinned_u8 = buf if buf.is_pinned() else buf.pin_memory()
    records = torch.empty(buf.shape[0], dtype=torch.uint8, device=dev)
    ms, runs = events_ms(lambda: records.copy_(pinned_u8, non_blocking=True), repeats)
    res["pinned_to_device"] = dict(ms=ms, GB_per_s=P * C * 4 / ms / 1e6, runs_ms=runs)
    back = [torch.empty_like(x) for x in t]
    names = mio.attribute_names(3 * K)
    dst = {"x": (0, 0), "y": (0, 1), "z": (0, 2), "opacity": (3, 0), "filter_3D": (6, 0)}
    dst.update({f"f_dc_{j}": (1, j) for j in range(3)}, **{f"scale_{j}": (4, j) for j in range(3)}, **{f"rot_{j}": (5, j) for j in range(4)})
    dst.update({f"f_rest_{j}": (2, (j % K) * 3 + j // K) for j in range(3 * K)})
    cols = [(back[dst[n][0]], dst[n][1]) + layout[n] + (False,) for n in names if n in dst]
    table = mio._column_table(S, cols, dev)
    ms, runs = events_ms(lambda: mio._launch_unpack(records, P, S, len(cols), table, dev), repeats)
    res["unpack_kernel"] = dict(rate(ms), runs_ms=runs)
    res["unpack_equals_the_packed_tensors"] = bool(all(torch.equal(a, b) for a, b in zip(back, t)))
    ms, runs = wall_ms(lambda: mio.load_ply(path, max_sh_degree=3), repeats)
    res["load_ply"] = dict(ms=ms, runs_ms=runs)
    st = mio.load_ply(path, max_sh_degree=3)
    res["load_equals_the_saved_tensors"] = bool(all(torch.equal(a, b) for a, b in zip(st, t)))
    os.remove(path)
    return res


def host_side(P, folder):
    """upstream's statements, restated (gaussian_model.py:382-397 and 516-557), on P rows at SH degree 3"""
    import model_io_restatement as mr
    rng = np.random.default_rng(0)
    K = 15
    arrays = [rng.standard_normal(s).astype(np.float32) for s in ((P, 3), (P, 1, 3), (P, K, 3), (P, 1), (P, 3), (P, 4), (P, 1))]
    names = mr.attribute_names(3 * K)
    path = os.path.join(folder, f"host_{P}.ply")
    t0 = time.perf_counter()
    attributes = mr.model_columns(*arrays)
    elements = np.empty(P, dtype=[(n, "f4") for n in names])
    t1 = time.perf_counter()
    elements[:] = list(map(tuple, attributes))
    t2 = time.perf_counter()
    with open(path, "wb") as f:
        f.write(mr.write_header(P, [(n, "f4") for n in names]))
        f.write(elements.tobytes())
    t3 = time.perf_counter()
    rec, _ = mr.read_vertex(open(path, "rb").read())
    t4 = time.perf_counter()
    xyz = np.stack((np.asarray(rec["x"]), np.asarray(rec["y"]), np.asarray(rec["z"])), axis=1)
    extra = np.zeros((P, 3 * K))
    for idx in range(3 * K):
        extra[:, idx] = np.asarray(rec[f"f_rest_{idx}"])
    extra = extra.reshape((P, 3, K))
    dc = np.zeros((P, 3, 1))
    for j in range(3):
        dc[:, j, 0] = np.asarray(rec[f"f_dc_{j}"])
    small = {}
    for key, ns in (("scale", [f"scale_{j}" for j in range(3)]), ("rot", [f"rot_{j}" for j in range(4)]), ("opacity", ["opacity"]), ("filter", ["filter_3D"])):
        small[key] = np.zeros((P, len(ns)))
        for j, n in enumerate(ns):
            small[key][:, j] = np.asarray(rec[n])
    tensors = [torch.tensor(xyz, dtype=torch.float), torch.tensor(dc, dtype=torch.float).transpose(1, 2).contiguous(),
               torch.tensor(extra, dtype=torch.float).transpose(1, 2).contiguous()] + [torch.tensor(v, dtype=torch.float) for v in small.values()]
    t5 = time.perf_counter()
    same = bool(np.array_equal(tensors[2].numpy(), arrays[2]) and np.array_equal(tensors[0].numpy(), arrays[0]))
    os.remove(path)
    return dict(rows=P, save=dict(concatenate_ms=(t1 - t0) * 1e3, list_map_tuple_into_structured_array_ms=(t2 - t1) * 1e3, write_ms=(t3 - t2) * 1e3,
                                  total_ms=(t3 - t0) * 1e3),
                load=dict(read_ms=(t4 - t3) * 1e3, per_column_float64_and_torch_tensor_ms=(t5 - t4) * 1e3, total_without_upload_ms=(t5 - t3) * 1e3),
                host_load_equals_what_was_saved=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modelio_bench.json"))
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--host-rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_model_io: no GPU -- nothing is measured without one")
    import model_io as mio
    with tempfile.TemporaryDirectory(dir=args.dir) as folder:
        gpu = [gpu_side(P, folder, args.repeats, mio) for P in args.rows]
        host = host_side(args.host_rows, folder) if args.host_rows else None
        fs = os.statvfs(folder)
    result = dict(
        note="SH degree 3 with the filter: 252-byte records.  Kernel and copy times are device events around the launch alone, median of the listed "
             "runs after one untimed launch; kernel GB/s counts rows x (240 + 252) bytes.  File and end-to-end times are wall clock, synchronised, "
             "page cache warm, on the temporary directory of this box.  The host figures restate upstream's own statements in NumPy on this box's "
             "CPU; plyfile is not installed here and was not timed.",
        device=torch.cuda.get_device_name(0), host_cpus_available=len(os.sched_getaffinity(0)), file_system_block_size=int(fs.f_bsize),
        gpu=gpu, host_restatement_of_upstream=host)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
