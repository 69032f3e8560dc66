"""Times scene ingestion per image on the GPU, step by step, and on the same box's host a restatement of upstream's path.

    python scripts/gpu_sceneio_bench.py [--out profiles/sceneio_bench.json] [--images 3] [--repeats 5] [--dir DIR]

`--images` synthetic photographs (a smooth field under noise) per kind are written to a temporary directory as JPEG (quality 92) and PNG
(compress level 1), 4946x3286 and 1600x1200, and loaded at `-r -1`: the large ones are rescaled to 1600x1063, the small ones keep their size.
Per kind, over the images and `repeats` rounds after one untimed round, medians with the spread (min, max):
  decode            Pillow's open + np.asarray on one thread, wall clock: the host's, and the same call upstream makes
  upload            the 8-bit pixels host -> device (pageable memory, as np.asarray leaves them), device events
  resize (A + B)    both kernels of radegs_sceneio_resize as load_image launches them, device events; bytes = source rows read + the
                    intermediate written and read + the float planes written, over that time against the 6.3 TB/s a streaming kernel
                    reaches on HBM.  `horizontal (A + copy)` is passes="h" with 8-bit output: kernel A over all rows plus a byte copy
  edge (D)          radegs_sceneio_edge, device events, bytes = 3 planes read + 1 written
  load_camera       wall clock around scene_io.load_camera on decoded pixels, synchronised: upload + kernels + the host's matrix work;
                    `upload_and_plumbing` = load_camera - resize - edge (the upload inside load_camera is asynchronous and overlaps the
                    host's work, so the upload timed alone is not subtracted)
  pool              wall clock of load_cameras over all images of the kind with the default thread pool: what a caller waits for, per image
The host figures restate upstream's own statements on this box's CPU, one thread as upstream runs them: Image.resize, np.array, / 255,
permute, clamp (utils/general_utils.py PILtoTorch, scene/cameras.py:39) and the edge map's eager torch statements (cameras.py:59-68) on the
CPU; upstream runs that last part on the GPU after uploading the float image, so the host edge figure is listed apart and left out of
`host_total`.  No threshold: recorded."""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rade-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
HBM_STREAM_GBS = 6300.0


def stats(xs):
    return {"median_ms": round(float(np.median(xs)), 4), "min_ms": round(float(np.min(xs)), 4), "max_ms": round(float(np.max(xs)), 4), "n": len(xs)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def photograph(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    planes = [127 + 90 * np.sin(x / (37.0 + 11 * c) + seed) * np.cos(y / (53.0 - 7 * c)) for c in range(3)]
    img = np.stack(planes, axis=-1) + rng.normal(0, 6, (h, w, 3)).astype(np.float32)
    return np.clip(img, 0, 255).astype(np.uint8)


def host_path(Image, path, resolution):
    """upstream's statements on the host, timed apart"""
    t0 = time.perf_counter()
    im = Image.open(path)
    im.load()
    t1 = time.perf_counter()
    resized = torch.from_numpy(np.array(im.resize(resolution))) / 255.0
    image = resized.permute(2, 0, 1).clamp(0.0, 1.0)
    t2 = time.perf_counter()
    c = image[:, 1:-1, 1:-1]
    grads = [torch.mean(torch.abs(c - n), 0) for n in (image[:, 1:-1, :-2], image[:, 1:-1, 2:], image[:, :-2, 1:-1], image[:, 2:, 1:-1])]
    edge = torch.nn.functional.pad(torch.exp(-torch.max(torch.stack(grads, dim=-1), dim=-1)[0]), (1, 1, 1, 1), mode="constant", value=0)
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, image, edge


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sceneio_bench.json"))
    ap.add_argument("--images", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    from PIL import Image

    import scene_io as sio
    dev = torch.device("cuda:0")
    args = types.SimpleNamespace(resolution=-1, data_device="cuda")
    result = {"note": "Per image.  Kernel and upload times are device events around the call alone; decode, load_camera, pool and host times are wall "
                      "clock, synchronised.  Medians over images x repeats after one untimed round, with min and max.  Kernel GB/s counts the bytes the "
                      "passes must move (see the script's docstring) against 6300 GB/s streaming HBM.  The host figures restate upstream's statements "
                      "on this box's CPU on one thread.",
              "device": torch.cuda.get_device_name(0), "host_cpus_available": len(os.sched_getaffinity(0)), "pool_threads": sio.default_workers(),
              "pillow": Image.__version__ if hasattr(Image, "__version__") else __import__("PIL").__version__, "kinds": []}
    with tempfile.TemporaryDirectory(dir=a.dir) as folder:
        for (w, h) in ((4946, 3286), (1600, 1200)):
            for ext, kw in (("jpg", {"quality": 92}), ("png", {"compress_level": 1})):
                paths = []
                for i in range(a.images):
                    paths.append(os.path.join(folder, f"im_{w}_{i}.{ext}"))
                    Image.fromarray(photograph(w, h, i), "RGB").save(paths[-1], **kw)
                res = sio.target_resolution(w, h, -1, 1.0)
                infos = [sio.CameraInfo(uid=i, R=np.eye(3), T=np.array([0.0, 0.0, 4.0]), FovY=0.8, FovX=1.1, image_path=p, image_name=f"im_{i}", width=w,
                                        height=h) for i, p in enumerate(paths)]
                t = {k: [] for k in ("decode", "upload", "resize", "horizontal", "edge", "load_camera", "host_decode", "host_resize_to_float", "host_edge_cpu")}
                pool = []
                same = True
                for r in range(a.repeats + 1):
                    for info in infos:
                        ms_dec, px = wall_ms(lambda: sio.read_image(info.image_path))
                        ms_up, src = event_ms(lambda: torch.from_numpy(np.ascontiguousarray(px)).to(dev))
                        ms_rs, (image, _) = event_ms(lambda: sio.load_image(src, res, dev))
                        ms_h, _ = event_ms(lambda: sio.resize_u8(src, res, passes="h"))
                        ms_e, edge = event_ms(lambda: sio.edge_map(image))
                        ms_cam, cam = wall_ms(lambda: sio.load_camera(args, 0, info, 1.0, px, dev))
                        hd, hr, he, himage, hedge = host_path(Image, info.image_path, res)
                        if r == 0:
                            same = same and torch.equal(image.cpu(), himage) and torch.equal(cam.original_image.cpu(), himage)
                            same = same and float((edge.cpu() - hedge).abs().max()) < 1e-6
                            continue
                        for k, v in zip(t, (ms_dec, ms_up, ms_rs, ms_h, ms_e, ms_cam, hd, hr, he)):
                            t[k].append(v)
                    ms_pool, cams = wall_ms(lambda: sio.load_cameras(infos, 1.0, args))
                    if r:
                        pool.append(ms_pool / len(infos))
                bounds_first, bounds_last = (0, h) if res[1] == h else (lambda b: (int(b[0, 0]), int(b[-1, 0] + b[-1, 1])))(sio.resample_table(h, res[1])[0])
                rows = bounds_last - bounds_first
                resize_bytes = (rows * w * 3 + 2 * rows * res[0] * 3 if res[0] != w else h * w * 3) + 12 * res[0] * res[1]
                edge_bytes = 16 * res[0] * res[1]
                entry = {"source": [w, h], "format": ext, "file_bytes": int(np.mean([os.path.getsize(p) for p in paths])), "target": list(res),
                         "images": a.images, "repeats": a.repeats, "device_image_equals_host_image_bit_for_bit": bool(same)}
                entry.update({k: stats(v) for k, v in t.items()})
                entry["pool_per_image"] = stats(pool)
                med = {k: entry[k]["median_ms"] for k in t}
                entry["resize"]["GB_per_s"] = round(resize_bytes / med["resize"] / 1e6, 1)
                entry["resize"]["share_of_6300_GB_per_s_streaming_HBM"] = round(resize_bytes / med["resize"] / 1e6 / HBM_STREAM_GBS, 4)
                entry["edge"]["GB_per_s"] = round(edge_bytes / med["edge"] / 1e6, 1)
                entry["edge"]["share_of_6300_GB_per_s_streaming_HBM"] = round(edge_bytes / med["edge"] / 1e6 / HBM_STREAM_GBS, 4)
                entry["upload_and_plumbing_ms"] = round(med["load_camera"] - med["resize"] - med["edge"], 4)
                entry["device_total_after_decode_ms"] = med["load_camera"]
                entry["host_total_after_decode_ms"] = med["host_resize_to_float"]
                entry["decode_share_of_decode_plus_load_camera"] = round(med["decode"] / (med["decode"] + med["load_camera"]), 4)
                result["kinds"].append(entry)
                print(json.dumps({k: entry[k] for k in ("source", "format", "target", "decode", "upload", "resize", "edge", "load_camera", "pool_per_image",
                                                         "host_resize_to_float", "device_image_equals_host_image_bit_for_bit")}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
