"""Times evaluation from files on the GPU.

    python scripts/gpu_evalio_bench.py [--out profiles/evalio_bench.json] [--pairs 300] [--hypotheses 100000] [--points 20000000] [--repeats 5]

Run without `--step` it is a driver: each step below runs in a child process of its own under its own time limit, and the first one that
fails, faults or runs out of time ends the run (nothing more is started on the device).  Nothing is read from any file the script did not
write itself from a seed.
  ransac  tnt_eval.ransac_correspondence on `--pairs` noisy pairs with 22 % outliers, `--hypotheses` hypotheses: device events around the
          call's two kernels (radegs_evalio_ransac) and a host clock around the whole call with its one host read, median of `--repeats`
          after one untimed call; then the NumPy restatement (tests/evalio_restatement.py) of the same search on the same box, once, and the
          two results compared (hypothesis and count must be equal).  Work: hypotheses x pairs pair evaluations of about 30 fp64 operations
          and one sqrt; the pairs are read from LDS, so no memory bound is stated.
  ply     eval_io.read_ply_points on a synthetic cloud of `--points` points in the layout of the benchmarks' ground truth (float x y z,
          float normals, uchar colours: 27 bytes a record), split as N15 reports its own reader: file read into pinned memory (host clock;
          the file was just written, so it comes from the page cache), upload (device events), kernel (device events, median of
          `--repeats`).  Traffic of the kernel: 27 B read and 24 B written per point.
No threshold: the figures are recorded."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rade-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
STEP_LIMIT_S = {"ransac": 300, "ply": 420}


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def step_ransac(args):
    import torch

    import evalio_restatement as er
    import geom_host as gh
    import tnt_eval as te
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda:0")
    N, K = args.pairs, args.hypotheses
    src, tgt, known = er.noisy_pairs(N, seed=300)
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    first = te.ransac_correspondence(s, t, 0.2, 6, K)                      # untimed: code objects, allocator
    counts, sumsq = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.float64, device=dev)
    out = torch.empty(15, dtype=torch.float64, device=dev)
    L = gh.bind(te._SIGNATURES)

    def kernels():
        gh.check(L.radegs_evalio_ransac(N, _C._ptr(s), _C._ptr(t), 0.2, 6, K, 0, _C._ptr(counts), _C._ptr(sumsq), _C._ptr(out), _C._stream(dev)), "ransac")
    kernel_ms, call_s = [], []
    for _ in range(args.repeats):
        kernel_ms.append(event_ms(kernels)[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = te.ransac_correspondence(s, t, 0.2, 6, K)
        call_s.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    exp = er.ransac(src, tgt, 0.2, 6, K, 0, check=False)
    numpy_s = time.perf_counter() - t0
    same = got["hypothesis"] == exp["hypothesis"] == first["hypothesis"] and got["count"] == exp["count"]
    k_ms = statistics.median(kernel_ms)
    res = {"pairs": N, "hypotheses": K, "kernel_ms": kernel_ms, "kernel_ms_median": k_ms, "call_s": call_s, "call_s_median": statistics.median(call_s),
           "pair_evaluations_per_s": N * K / (k_ms * 1e-3), "numpy_restatement_s": numpy_s, "numpy_over_call": numpy_s / statistics.median(call_s),
           "hypothesis": got["hypothesis"], "count": got["count"], "inlier_rmse": got["inlier_rmse"], "same_as_restatement": bool(same),
           "error_to_known": float(np.abs(got["transformation"] - known).max())}
    print("ransac", res, flush=True)
    return res if same else None


def step_ply(args):
    import torch

    import eval_io
    dev = torch.device("cuda:0")
    P = args.points
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rng = np.random.default_rng(20)
    rec = np.zeros(P, np.dtype(fields))
    for n in "xyz":
        rec[n] = rng.standard_normal(P, dtype=np.float32)
    spell = {"<f4": "float", "u1": "uchar"}
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n%send_header\n" % (P, "".join(f"property {spell[t]} {n}\n" for n, t in fields))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.ply")
        with open(path, "wb") as fh:
            fh.write(head.encode("ascii"))
            rec.tofile(fh)
        small = eval_io.read_ply_points(path, dev)                          # untimed: code objects, allocator, the page cache
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        whole = eval_io.read_ply_points(path, dev)
        torch.cuda.synchronize()
        whole_s = time.perf_counter() - t0
        header = eval_io._header(path)
        kv, xyz, S = eval_io._vertex_layout(path, header)
        t0 = time.perf_counter()
        buf = eval_io._read_bytes(path, header.data_offset, P * S)
        read_s = time.perf_counter() - t0
    upload_ms, on_dev = event_ms(lambda: buf.to(dev, non_blocking=True))
    cols = [xyz[n] for n in "xyz"]
    kernel_ms = [event_ms(lambda: eval_io.unpack_points(on_dev, 0, P, S, cols))[0] for _ in range(args.repeats)]
    k_ms = statistics.median(kernel_ms)
    exact = bool(torch.equal(whole, small)) and bool(np.array_equal(whole[:1000].cpu().numpy(), np.stack([rec[n][:1000].astype(np.float64) for n in "xyz"], 1)))
    res = {"points": P, "record_bytes": S, "file_bytes": P * S, "whole_call_s": whole_s, "file_read_s": read_s, "file_read_GBps": P * S / read_s / 1e9,
           "upload_ms": upload_ms, "upload_GBps": P * S / (upload_ms * 1e-3) / 1e9, "kernel_ms": kernel_ms, "kernel_ms_median": k_ms,
           "kernel_GBps_read_plus_written": P * (S + 24) / (k_ms * 1e-3) / 1e9, "exact": exact}
    print("ply", res, flush=True)
    return res if exact else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evalio_bench.json"))
    ap.add_argument("--pairs", type=int, default=300)
    ap.add_argument("--hypotheses", type=int, default=100000)
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step", choices=("ransac", "ply"))
    args = ap.parse_args()
    if args.step:
        res = {"ransac": step_ransac, "ply": step_ply}[args.step](args)
        if res is None:
            return 2
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    result = {"device": "MI355X (gfx950)", "command": " ".join(sys.argv)}
    for step in ("ransac", "ply"):
        part = args.out + "." + step
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--out", part, "--pairs", str(args.pairs), "--hypotheses", str(args.hypotheses),
               "--points", str(args.points), "--repeats", str(args.repeats)]
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
