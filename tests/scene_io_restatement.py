"""NumPy restatement of scene ingestion: Pillow's 8-bit `resize` with its default filter, the / 255 table, the Blender
composite, the edge map in float64, the resolution rule of loadCam and the COLMAP model records (binary and text, both directions: the
golden generator writes its fixture dataset with the writers here and reads it back with the reference's readers).

The resize is written from memory of Pillow's resampling (bicubic, a = -0.5, antialiased, 22 fractional bits, horizontal pass first over
the rows the vertical pass reads) and is checked against Pillow itself in tests/test_scene_io_restatement.py; nothing here imports Pillow.
The arithmetic is per output index, in plain loops, on purpose: rade-gs_amd/scene_io.py builds the same tables vectorised, and the two must
agree (tests/test_scene_io_api.py)."""
import hashlib
import math
import struct

import numpy as np

PRECISION_BITS = 22
A = -0.5


def bicubic(t):
    t = abs(t)
    if t < 1.0:
        return ((A + 2.0) * t - (A + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * A
    return 0.0


def coefficients(in_size, out_size):
    """(bounds int32 [out, 2] = (xmin, n), kk int32 [out, ksize]) of one axis"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - c + 0.5) * ss) for x in range(n)]
        total = 0.0
        for v in w:
            total += v
        for x in range(n):
            v = w[x] / total if total != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, n)
    return bounds, kk


def _pass(src, bounds, kk, axis):
    """one pass along `axis` (0 or 1) of uint8 [H, W, C]"""
    src = np.moveaxis(src, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
    for i, (lo, n) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[i, :n].astype(np.int64), src[lo:lo + n], axes=(0, 0))
        assert np.all(np.abs(acc) < 2 ** 31)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(image, size, passes="hv"):
    """uint8 [H, W, C] (or [H, W]) -> [h, w, C]: every channel on its own, the horizontal pass first, an unchanged axis skipped.
    passes="h": the horizontal pass alone, over all rows."""
    a = np.asarray(image)
    flat = a.ndim == 2
    a = a[:, :, None] if flat else a
    assert a.dtype == np.uint8
    w, h = size
    H, W = a.shape[:2]
    if W != w:
        a = _pass(a, *coefficients(W, w), axis=1)
    if "v" in passes and H != h:
        a = _pass(a, *coefficients(H, h), axis=0)
    a = np.ascontiguousarray(a)
    return a[:, :, 0] if flat else a


def lut():
    """float32 [256]: torch.from_numpy(uint8) / 255.0 divides in float32, correctly rounded"""
    return (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)


def pil_to_torch(image, size):
    """PILtoTorch (utils/general_utils.py): float32 [C, h, w] of uint8 [H, W, C] or [H, W]"""
    r = resize(image, size)
    r = r[:, :, None] if r.ndim == 2 else r
    return np.ascontiguousarray(lut()[r].transpose(2, 0, 1))


def composite(rgba, white_background):
    """dataset_readers.py:270-276: uint8 [..., 4] -> uint8 [..., 3]; the cast to np.byte is spelled as trunc and & 0xFF"""
    norm = rgba.astype(np.float64) / 255.0
    bg = 1.0 if white_background else 0.0
    arr = norm[..., :3] * norm[..., 3:4] + bg * (1 - norm[..., 3:4])
    return (np.trunc(arr * 255.0).astype(np.int64) & 0xFF).astype(np.uint8)


def edge_map64(image):
    """cameras.py:59-68 in float64 on float32 [C, H, W]"""
    x = image.astype(np.float64)
    c = x[:, 1:-1, 1:-1]
    grads = [np.mean(np.abs(c - n), axis=0) for n in (x[:, 1:-1, :-2], x[:, 1:-1, 2:], x[:, :-2, 1:-1], x[:, 2:, 1:-1])]
    out = np.zeros(x.shape[1:], dtype=np.float64)
    out[1:-1, 1:-1] = np.exp(-np.max(np.stack(grads, axis=-1), axis=-1))
    return out


def target_resolution(orig_w, orig_h, resolution, resolution_scale):
    """camera_utils.py:23-40"""
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


# ---------------------------------------------------------------- test contents ----------------------------------------------------------------
def random_bytes(n, seed):
    """n bytes of a fixed stream: a 64-bit multiply-xorshift hash of the index, independent of any library's generator"""
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)) * np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(31)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(29)
    return (x >> np.uint64(56)).astype(np.uint8)


CONTENTS = ("uniform", "binary", "rows")
# (H, W, C) -> (h, w)
RESIZE_SHAPES = (((37, 53, 3), (14, 20)), ((37, 53, 3), (14, 53)), ((37, 53, 3), (80, 106)), ((64, 97, 1), (64, 31)), ((120, 200, 3), (9, 17)),
                 ((9, 7, 3), (33, 40)), ((5, 5, 1), (1, 1)), ((33, 65, 3), (33, 64)), ((2, 3, 3), (5, 7)), ((53, 37, 4), (20, 14)),
                 ((6, 300, 3), (4, 63)), ((6, 300, 3), (4, 64)), ((6, 300, 3), (4, 65)), ((6, 300, 3), (4, 257)), ((37, 53, 3), (37, 53)))


def content(shape, kind, seed=0):
    H, W, C = shape
    n = H * W * C
    if kind == "uniform":
        return random_bytes(n, 11 + seed).reshape(shape)
    if kind == "binary":
        return ((random_bytes(n, 23 + seed) >> 7) * np.uint8(255)).reshape(shape)
    if kind == "rows":
        return np.ascontiguousarray(np.broadcast_to(((np.arange(H) & 1) * 255).astype(np.uint8)[:, None, None], shape))
    raise ValueError(kind)


def all_pairs_rgba():
    """uint8 [256, 256, 4]: red runs over the columns and alpha over the rows, so every (colour, alpha) pair occurs once in the red channel"""
    x, y = np.meshgrid(np.arange(256), np.arange(256))
    return np.stack([x, 255 - x, (x + y) & 255, y], axis=-1).astype(np.uint8)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_key(shape, size, kind):
    return "resize_%dx%dx%d_%dx%d_%s" % (shape + size + (kind,))


# ---------------------------------------------------------------- COLMAP records ----------------------------------------------------------------
# The public layout (COLMAP's documentation of its output format): little-endian; cameras.bin = u64 count, then per camera i32 id,
# i32 model id, u64 width, u64 height, f64 params; images.bin = u64 count, then per image i32 id, f64 qw qx qy qz, f64 tx ty tz,
# i32 camera id, the name up to a 0 byte, u64 count of 2D points, then per point f64 x, f64 y, i64 point3D id; points3D.bin = u64 count,
# then per point u64 id, f64 xyz, u8 rgb, f64 error, u64 track length, then per track element i32 image id, i32 point2D index.
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8),
                 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
MODEL_IDS = {name: (i, n) for i, (name, n) in CAMERA_MODELS.items()}


def write_cameras_bin(path, cameras):
    """cameras: [(id, model name, width, height, params)]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cameras)))
        for cid, model, w, h, params in cameras:
            f.write(struct.pack("<iiQQ", cid, MODEL_IDS[model][0], w, h) + struct.pack("<%dd" % len(params), *params))


def write_cameras_txt(path, cameras):
    with open(path, "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n# Number of cameras: %d\n" % len(cameras))
        for cid, model, w, h, params in cameras:
            f.write(" ".join([str(cid), model, str(w), str(h)] + [repr(float(p)) for p in params]) + "\n")


def write_images_bin(path, images):
    """images: [(id, qvec[4], tvec[3], camera id, name, xys [n,2], point3D ids [n])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(images)))
        for iid, q, t, cid, name, xys, pids in images:
            f.write(struct.pack("<i7di", iid, *q, *t, cid) + name.encode() + b"\0" + struct.pack("<Q", len(pids)))
            for (x, y), p in zip(xys, pids):
                f.write(struct.pack("<ddq", x, y, p))


def write_images_txt(path, images):
    with open(path, "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for iid, q, t, cid, name, xys, pids in images:
            f.write(" ".join([str(iid)] + [repr(float(v)) for v in list(q) + list(t)] + [str(cid), name]) + "\n")
            f.write(" ".join("%r %r %d" % (float(x), float(y), p) for (x, y), p in zip(xys, pids)) + "\n")


def write_points3d_bin(path, points):
    """points: [(id, xyz[3], rgb[3], error, [(image id, point2D index)])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(points)))
        for pid, xyz, rgb, err, track in points:
            f.write(struct.pack("<Q3d3BdQ", pid, *xyz, *rgb, err, len(track)))
            for i, j in track:
                f.write(struct.pack("<ii", i, j))


def write_points3d_txt(path, points):
    with open(path, "w") as f:
        f.write("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for pid, xyz, rgb, err, track in points:
            f.write(" ".join([str(pid)] + [repr(float(v)) for v in xyz] + [str(int(v)) for v in rgb] + [repr(float(err))]
                             + ["%d %d" % (i, j) for i, j in track]) + "\n")


def qvec2rotmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])
