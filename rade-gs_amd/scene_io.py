"""HIP-backed scene ingestion: a dataset folder becomes cameras and ground-truth images -- scene/__init__.py Scene,
scene/dataset_readers.py readColmapSceneInfo / readNerfSyntheticInfo, scene/colmap_loader.py, utils/camera_utils.py loadCam / camera_to_JSON,
utils/general_utils.py PILtoTorch and scene/cameras.py Camera -- without open3d, plyfile or trimesh.  The readers are host code of this
project's own (COLMAP's public record layout restated with `struct`).  After the decode, which stays Pillow's on a thread pool, the 8-bit
pixels are uploaded once and everything runs in csrc/radegs_sceneio.hip: Pillow's antialiased bicubic resize (bit for bit), / 255 through a
table, the Blender composite and the edge map.  include/radegs.h, "Scene ingestion", is the specification of the kernels and
tests/scene_io_restatement.py restates them in NumPy.  The resize is restated from memory of Pillow's resampling and checked against
Pillow 12.2 (DESIGN 11 N16 marks it).  Pillow is imported lazily, by the default image reader only."""
import collections
import concurrent.futures
import ctypes
import json
import math
import os
import struct
import sys
import threading

import numpy as np
import torch

import geom_host as gh
import model_io
from diff_gaussian_rasterization import _C
from geom_host import i32, ll, vp

PRECISION_BITS = 22       # RADEGS_SCENEIO_PRECISION_BITS
_A = -0.5                 # Pillow's bicubic


class _Table(ctypes.Structure):      # RadegsSceneioTable
    _fields_ = [("bounds", vp), ("kk", vp), ("in_size", i32), ("out_size", i32), ("ksize", i32), ("max_span", i32), ("first", i32), ("last", i32)]


_TP = ctypes.POINTER(_Table)
SIGNATURES = {
    "radegs_sceneio_resize": (i32, [i32] * 5 + [vp, _TP, _TP, i32, i32] + [vp] * 6),
    "radegs_sceneio_composite": (i32, [ll, vp, i32, vp, vp]),
    "radegs_sceneio_edge": (i32, [i32, i32, i32, vp, vp, vp]),
}
_SIGNATURES = SIGNATURES
MODES = ("L", "RGB", "RGBA")

CameraInfo = collections.namedtuple("CameraInfo", "uid R T FovY FovX image_path image_name width height white_background", defaults=(None,))
SceneInfo = collections.namedtuple("SceneInfo", "point_cloud train_cameras test_cameras nerf_normalization ply_path")
ColmapCamera = collections.namedtuple("ColmapCamera", "id model width height params")
ColmapImage = collections.namedtuple("ColmapImage", "id qvec tvec camera_id name xys point3D_ids")

# COLMAP's camera models: id -> (name, number of parameters)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8), 5: ("OPENCV_FISHEYE", 8),
                 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
UNHANDLED_MODEL = "Colmap camera model not handled: only undistorted datasets (PINHOLE or SIMPLE_PINHOLE cameras) supported!"


def _lib():
    return gh.bind(_SIGNATURES)


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"scene_io's kernels run on the GPU only, got device `{device}`")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


# ----------------------------------------------------------------------------- COLMAP -----------------------------------------------------------------------------
def qvec2rotmat(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


class _Bytes:
    def __init__(self, path):
        with open(path, "rb") as f:
            self.data, self.pos, self.path = f.read(), 0, path

    def take(self, fmt):
        size = struct.calcsize(fmt)
        if self.pos + size > len(self.data):
            raise RuntimeError(f"{self.path}: the file ends inside a record")
        out = struct.unpack_from(fmt, self.data, self.pos)
        self.pos += size
        return out

    def name(self):
        end = self.data.index(b"\0", self.pos)
        out = self.data[self.pos:end].decode("utf-8")
        self.pos = end + 1
        return out


def _lines(path):
    with open(path, "r") as f:
        for line in f:
            line = line.strip()
            if line and not line.startswith("#"):
                yield line


def read_cameras_binary(path):
    b, out = _Bytes(path), {}
    for _ in range(b.take("<Q")[0]):
        cid, model, w, h = b.take("<iiQQ")
        if model not in CAMERA_MODELS:
            raise RuntimeError(f"{path}: camera {cid} has the unknown model id {model}")
        name, n = CAMERA_MODELS[model]
        out[cid] = ColmapCamera(cid, name, w, h, np.array(b.take("<%dd" % n)))
    return out


def read_cameras_text(path):
    out = {}
    for line in _lines(path):
        e = line.split()
        out[int(e[0])] = ColmapCamera(int(e[0]), e[1], int(e[2]), int(e[3]), np.array([float(v) for v in e[4:]]))
    return out


def read_images_binary(path):
    b, out = _Bytes(path), {}
    for _ in range(b.take("<Q")[0]):
        v = b.take("<i7di")
        name = b.name()
        n = b.take("<Q")[0]
        pts = np.frombuffer(b.data, dtype=np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")]), count=n, offset=b.pos)
        b.pos += 24 * n
        out[v[0]] = ColmapImage(v[0], np.array(v[1:5]), np.array(v[5:8]), v[8], name, np.stack([pts["x"], pts["y"]], axis=1), pts["id"].copy())
    return out


def read_images_text(path):
    out, it = {}, None
    with open(path, "r") as f:                    # two lines per image; the second may be empty, so blank lines are not skipped after a first
        lines = [line.strip() for line in f]
    k = 0
    while k < len(lines):
        line = lines[k]
        k += 1
        if not line or line.startswith("#"):
            continue
        e = line.split()
        it = [float(v) for v in (lines[k].split() if k < len(lines) else [])]
        k += 1
        out[int(e[0])] = ColmapImage(int(e[0]), np.array([float(v) for v in e[1:5]]), np.array([float(v) for v in e[5:8]]), int(e[8]), e[9],
                                     np.array(list(zip(it[0::3], it[1::3]))).reshape(-1, 2), np.array([int(v) for v in it[2::3]], dtype=np.int64))
    return out


def read_colmap_model(sparse_dir):
    """(cameras {id: ColmapCamera}, images {id: ColmapImage}) of a COLMAP model folder: the .bin pair, or the .txt pair when the .bin pair
    cannot be read (dataset_readers.py:192-201)."""
    try:
        images = read_images_binary(os.path.join(sparse_dir, "images.bin"))
        cameras = read_cameras_binary(os.path.join(sparse_dir, "cameras.bin"))
    except Exception:
        images = read_images_text(os.path.join(sparse_dir, "images.txt"))
        cameras = read_cameras_text(os.path.join(sparse_dir, "cameras.txt"))
    return cameras, images


def read_points3d(sparse_dir):
    """(xyz float64 [N,3], rgb uint8 [N,3], error float64 [N]) from points3D.bin, or points3D.txt when the .bin cannot be read"""
    try:
        b = _Bytes(os.path.join(sparse_dir, "points3D.bin"))
        xyz, rgb, err = [], [], []
        for _ in range(b.take("<Q")[0]):
            v = b.take("<Q3d3BdQ")
            xyz.append(v[1:4]), rgb.append(v[4:7]), err.append(v[7])
            b.take("<%di" % (2 * v[8]))
    except Exception:
        xyz, rgb, err = [], [], []
        for line in _lines(os.path.join(sparse_dir, "points3D.txt")):
            e = line.split()
            xyz.append([float(v) for v in e[1:4]]), rgb.append([int(v) for v in e[4:7]]), err.append(float(e[7]))
    return np.array(xyz, dtype=np.float64).reshape(-1, 3), np.array(rgb, dtype=np.uint8).reshape(-1, 3), np.array(err, dtype=np.float64)


# ------------------------------------------------------------------------- camera geometry -------------------------------------------------------------------------
def focal2fov(focal, pixels):
    return 2 * math.atan(pixels / (2 * focal))


def fov2focal(fov, pixels):
    return pixels / (2 * math.tan(fov / 2))


def world_to_view(R, t, translate=np.array([0.0, 0.0, 0.0]), scale=1.0):
    """getWorld2View2 in float64 (the caller rounds): R is stored transposed, the camera centre is moved by `translate` and `scale`"""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = np.asarray(R).transpose()
    Rt[:3, 3] = t
    Rt[3, 3] = 1.0
    C2W = np.linalg.inv(Rt)
    C2W[:3, 3] = (C2W[:3, 3] + translate) * scale
    return np.linalg.inv(C2W)


def projection(znear, zfar, fovX, fovY):
    """getProjectionMatrix in float64 (the caller rounds)"""
    top, right = math.tan(fovY / 2) * znear, math.tan(fovX / 2) * znear
    P = np.zeros((4, 4))
    P[0, 0] = 2.0 * znear / (right + right)
    P[1, 1] = 2.0 * znear / (top + top)
    P[0, 2] = (right - right) / (right + right)
    P[1, 2] = (top - top) / (top + top)
    P[3, 2] = 1.0
    P[2, 2] = zfar / (zfar - znear)
    P[2, 3] = -(zfar * znear) / (zfar - znear)
    return P


def nerfpp_norm(cam_infos):
    """getNerfppNorm: translate = -(mean camera centre), radius = 1.1 max distance to it"""
    centers = np.hstack([np.linalg.inv(np.float32(world_to_view(c.R, c.T)))[:3, 3:4] for c in cam_infos])
    center = np.mean(centers, axis=1, keepdims=True)
    diagonal = np.max(np.linalg.norm(centers - center, axis=0, keepdims=True))
    return {"translate": -center.flatten(), "radius": diagonal * 1.1}


def camera_to_JSON(id, camera):
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = camera.R.transpose()
    Rt[:3, 3] = camera.T
    Rt[3, 3] = 1.0
    W2C = np.linalg.inv(Rt)
    return {"id": id, "img_name": camera.image_name, "width": camera.width, "height": camera.height, "position": W2C[:3, 3].tolist(),
            "rotation": [x.tolist() for x in W2C[:3, :3]], "fy": fov2focal(camera.FovY, camera.height), "fx": fov2focal(camera.FovX, camera.width)}


# ----------------------------------------------------------------------------- readers -----------------------------------------------------------------------------
def read_colmap_scene(path, images=None, eval=False, llffhold=8, device="cuda"):
    """readColmapSceneInfo: SceneInfo of <path>/sparse/0 and <path>/<images or "images">.  The images are not opened here: a CameraInfo
    carries the path, load_cameras decodes."""
    sparse = os.path.join(path, "sparse/0")
    cameras, extrinsics = read_colmap_model(sparse)
    folder = os.path.join(path, "images" if images is None else images)
    infos = []
    for key in extrinsics:
        extr = extrinsics[key]
        intr = cameras[extr.camera_id]
        if intr.model == "SIMPLE_PINHOLE":
            fy = fx = intr.params[0]
        elif intr.model == "PINHOLE":
            fx, fy = intr.params[0], intr.params[1]
        else:
            raise AssertionError(UNHANDLED_MODEL)
        image_path = os.path.join(folder, os.path.basename(extr.name))
        infos.append(CameraInfo(uid=intr.id, R=np.transpose(qvec2rotmat(extr.qvec)), T=np.array(extr.tvec), FovY=focal2fov(fy, intr.height),
                                FovX=focal2fov(fx, intr.width), image_path=image_path, image_name=os.path.basename(image_path).split(".")[0],
                                width=intr.width, height=intr.height))
    infos = sorted(infos, key=lambda c: c.image_name)
    train = [c for idx, c in enumerate(infos) if idx % llffhold != 0] if eval else infos
    test = [c for idx, c in enumerate(infos) if idx % llffhold == 0] if eval else []
    norm = nerfpp_norm(train)
    print(f'cameras extent: {norm["radius"]}')
    ply_path = os.path.join(path, "sparse/0/points3D.ply")
    if not os.path.exists(ply_path):
        print("Converting point3d.bin to .ply, will happen only the first time you open the scene.")
        xyz, rgb, _ = read_points3d(sparse)
        model_io.store_ply(ply_path, xyz, rgb)
    return SceneInfo(model_io.fetch_ply(ply_path, device=device), train, test, norm, ply_path)


def _image_size(path, image_reader):
    if image_reader is not None:
        a = image_reader(path)
        return a.shape[1], a.shape[0]
    with _pil().open(path) as im:
        return im.size


def read_transforms(path, transformsfile, white_background, extension=".png", image_reader=None):
    """readCamerasFromTransforms: the composite over the background is left to load_cameras (white_background rides on the CameraInfo)"""
    with open(os.path.join(path, transformsfile)) as f:
        contents = json.load(f)
    fovx, infos = contents["camera_angle_x"], []
    for idx, frame in enumerate(contents["frames"]):
        image_path = os.path.join(path, frame["file_path"] + extension)
        c2w = np.array(frame["transform_matrix"])
        c2w[:3, 1:3] *= -1                                  # OpenGL / Blender axes (Y up, Z back) -> COLMAP (Y down, Z forward)
        w2c = np.linalg.inv(c2w)
        w, h = _image_size(image_path, image_reader)
        infos.append(CameraInfo(uid=idx, R=np.transpose(w2c[:3, :3]), T=w2c[:3, 3], FovY=focal2fov(fov2focal(fovx, w), h), FovX=fovx, image_path=image_path,
                                image_name=os.path.splitext(os.path.basename(image_path))[0], width=w, height=h, white_background=bool(white_background)))
    return infos


def sh2rgb(sh):
    return sh * 0.28209479177387814 + 0.5


def read_blender_scene(path, white_background, eval, extension=".png", image_reader=None, device="cuda"):
    """readNerfSyntheticInfo.  Without points3d.ply the initial cloud is drawn with upstream's NumPy calls in upstream's order (the global
    np.random state: seed it for a repeatable cloud)."""
    print("Reading Training Transforms")
    train = read_transforms(path, "transforms_train.json", white_background, extension, image_reader)
    print("Reading Test Transforms")
    test = read_transforms(path, "transforms_test.json", white_background, extension, image_reader)
    print("train num:", len(train))
    norm = nerfpp_norm(train)
    ply_path = os.path.join(path, "points3d.ply")
    if not os.path.exists(ply_path):
        num_pts = 100_000
        print(f"Generating random point cloud ({num_pts})...")
        xyz = np.random.random((num_pts, 3)) * 2.6 - 1.3
        shs = np.random.random((num_pts, 3)) / 255.0
        model_io.store_ply(ply_path, xyz, sh2rgb(shs) * 255)
    return SceneInfo(model_io.fetch_ply(ply_path, device=device), train, test, norm, ply_path)


_WARNED = False


def target_resolution(orig_w, orig_h, resolution, resolution_scale):
    """camera_utils.py:23-40: (w, h) of the training image.  1, 2, 4, 8 divide and `round`; anything else is a target width (-1: the width
    itself, capped at 1600 with a warning printed once) and truncates."""
    global _WARNED
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        if orig_w > 1600:
            if not _WARNED:
                print("[ INFO ] Encountered quite large input images (>1.6K pixels width), rescaling to 1.6K.\n "
                      "If this is not desired, please explicitly specify '--resolution/-r' as 1")
                _WARNED = True
            global_down = orig_w / 1600
        else:
            global_down = 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


# ------------------------------------------------------------------------ coefficient tables ------------------------------------------------------------------------
def resample_table(in_size, out_size):
    """(bounds int32 [out, 2] = (first source index, taps), kk int32 [out, ksize]): Pillow's bicubic coefficients of one axis in fixed point,
    computed in float64 -- the weights of an output index summed left to right, each divided by the sum, rounded half away from zero at 22
    fractional bits.  Raises unless 255 sum|k| + 2^21 < 2^31 for every output index: the kernels' int32 sums cannot wrap."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise RuntimeError("image sizes must be positive")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    c = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(c - support + 0.5).astype(np.int64), 0)
    n = np.minimum(np.trunc(c + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs(((x + xmin[:, None]) - c[:, None] + 0.5) * ss)
    w = np.where(t < 1.0, ((_A + 2.0) * t - (_A + 3.0)) * t * t + 1, np.where(t < 2.0, (((t - 5) * t + 8) * t - 4) * _A, 0.0))
    w = np.where(x < n[:, None], w, 0.0)
    total = np.add.accumulate(w, axis=1)[:, -1:]           # left to right; the zeros past n leave the sum as it is
    w = np.where(total != 0.0, w / np.where(total != 0.0, total, 1.0), w)
    kk = np.where(w < 0, np.trunc(-0.5 + w * (1 << PRECISION_BITS)), np.trunc(0.5 + w * (1 << PRECISION_BITS))).astype(np.int64)
    if int(np.max(255 * np.abs(kk).sum(axis=1))) + (1 << (PRECISION_BITS - 1)) >= 1 << 31:
        raise RuntimeError(f"resize {in_size} -> {out_size}: 255 sum|k| + 2^21 reaches 2^31, the int32 pass would wrap")
    if np.any(n < 1) or np.any(n > ksize) or np.any(np.diff(xmin) < 0) or np.any(np.diff(xmin + n) < 0) or int((xmin + n).max()) > in_size:
        raise RuntimeError(f"resize {in_size} -> {out_size}: the tap ranges are not what the kernels assume")
    return np.stack([xmin, n], axis=1).astype(np.int32), kk.astype(np.int32)


_TABLES, _LUTS, _CACHE_LOCK = {}, {}, threading.Lock()


def _table(in_size, out_size, horizontal, dev):
    """the RadegsSceneioTable of one (in, out) pair on `dev`, built once (the tensors ride along: the structure holds their addresses)"""
    key = (dev, in_size, out_size, horizontal)
    with _CACHE_LOCK:
        if key not in _TABLES:
            bounds, kk = resample_table(in_size, out_size)
            lo, hi = bounds[:, 0].astype(np.int64), bounds[:, 0].astype(np.int64) + bounds[:, 1]
            starts = np.arange(0, out_size, 64)
            span = int(np.max(hi[np.minimum(starts + 63, out_size - 1)] - lo[starts]))
            b = torch.from_numpy(bounds).to(dev)
            k = torch.from_numpy(np.ascontiguousarray(kk.T) if horizontal else kk).to(dev)
            _TABLES[key] = (_Table(b.data_ptr(), k.data_ptr(), in_size, out_size, kk.shape[1], span, int(lo[0]), int(hi[-1])), b, k)
        return _TABLES[key][0]


def _lut(dev):
    with _CACHE_LOCK:
        if dev not in _LUTS:
            _LUTS[dev] = (torch.arange(256, dtype=torch.uint8) / 255.0).to(dev)      # torch's own division: bit-exact by construction
        return _LUTS[dev]


# ----------------------------------------------------------------------------- kernels -----------------------------------------------------------------------------
def _checked(pixels):
    """uint8 [H, W, C], C in {1, 3, 4}, where it is, from a Pillow image, a NumPy array or a tensor; anything else is refused by name"""
    mode = getattr(pixels, "mode", None)
    if mode is not None and not isinstance(pixels, (np.ndarray, torch.Tensor)):
        if mode not in MODES:
            raise NotImplementedError(f"image mode `{mode}`: scene_io takes {', '.join(MODES)} (8 bits per channel); convert the image first")
        pixels = np.asarray(pixels)
    t = pixels if isinstance(pixels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pixels))
    if t.dtype != torch.uint8:
        raise NotImplementedError(f"pixels of type {str(t.dtype).replace('torch.', '')}: scene_io takes {', '.join(MODES)} (8 bits per channel)")
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    if t.dim() != 3 or t.shape[2] not in (1, 3, 4) or t.shape[0] < 1 or t.shape[1] < 1:
        raise NotImplementedError(f"pixels of shape {tuple(t.shape)}: scene_io takes [H, W], [H, W, 1], [H, W, 3] or [H, W, 4]")
    return t


def _pixels(pixels, dev=None):
    """_checked(pixels) on the device (dev None: it must be there already), contiguous and 16-byte aligned"""
    t = _checked(pixels)
    if dev is None:
        _C._require_gpu(t, "image_u8")
        dev = t.device
    t = t.to(dev, non_blocking=True).contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t, dev


@torch.no_grad()
def _resize(src, size, passes, want_u8, want_float):
    dev = src.device
    H, W, C = src.shape
    w, h = int(size[0]), int(size[1])
    if w < 1 or h < 1:
        raise RuntimeError(f"the target size {size} must be positive")
    if passes not in ("hv", "h"):
        raise RuntimeError("`passes` must be 'hv' or 'h'")
    if passes == "h":
        h = H
    th = _table(W, w, True, dev) if W != w else None
    tv = _table(H, h, False, dev) if H != h else None
    first, rows = (tv.first, tv.last - tv.first) if tv is not None else (0, H)
    mid = torch.empty((rows, w, C), dtype=torch.uint8, device=dev) if th is not None else None
    out = torch.empty((h, w, C), dtype=torch.uint8, device=dev) if want_u8 else None
    image = torch.empty((min(C, 3), h, w), dtype=torch.float32, device=dev) if want_float else None
    mask = torch.empty((1, h, w), dtype=torch.float32, device=dev) if want_float and C == 4 else None
    gh.call(_SIGNATURES, "radegs_sceneio_resize", dev, H, W, C, h, w, src, ctypes.byref(th) if th is not None else None,
            ctypes.byref(tv) if tv is not None else None, first, rows, mid, _lut(dev) if want_float else None, out, image, mask)
    return out, image, mask


def resize_u8(image_u8, size, passes="hv"):
    """PIL.Image.resize(size) with the default filter on a device uint8 [H, W, C] (or [H, W]): uint8 [h, w, C], size = (w, h), every channel
    on its own.  passes="h": the horizontal pass alone, [H, w, C]."""
    flat = isinstance(image_u8, torch.Tensor) and image_u8.dim() == 2
    src, _ = _pixels(image_u8)
    out = _resize(src, size, passes, True, False)[0]
    return out[:, :, 0] if flat else out


def load_image(pixels_u8, resolution, device="cuda"):
    """PILtoTorch per plane, as loadCam calls it: (image float32 [3, h, w] ([1, h, w] for mode L), mask float32 [1, h, w] or None) on the device,
    resolution = (w, h).  The values are i / 255 for an integer i, so upstream's clamp(0, 1) is the identity."""
    src, _ = _pixels(_checked(pixels_u8), _device(device))
    _, image, mask = _resize(src, resolution, "hv", False, True)
    return image, mask


@torch.no_grad()
def composite_rgba(pixels_u8, white_background):
    """dataset_readers.py:270-276 on the device: uint8 [..., 4] -> uint8 [..., 3] over a white or black background"""
    t = pixels_u8 if isinstance(pixels_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pixels_u8)).cuda()
    _C._require_gpu(t, "pixels_u8")
    if t.dtype != torch.uint8 or t.dim() < 1 or t.shape[-1] != 4:
        raise RuntimeError("`pixels_u8` must be uint8 of shape [..., 4]")
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    out = torch.empty(t.shape[:-1] + (3,), dtype=torch.uint8, device=t.device)
    gh.call(_SIGNATURES, "radegs_sceneio_composite", t.device, t.numel() // 4, t, int(bool(white_background)), out)
    return out


@torch.no_grad()
def edge_map(image):
    """cameras.py:59-68: float32 [H, W] of a float32 [C, H, W] device image, C in {1, 3}"""
    _C._require_gpu(image, "image")
    if image.dtype != torch.float32 or image.dim() != 3 or image.shape[0] not in (1, 3) or image.shape[1] < 1 or image.shape[2] < 1:
        raise RuntimeError("`image` must be float32 of shape [1, H, W] or [3, H, W]")
    x = image.contiguous()
    out = torch.empty(x.shape[1:], dtype=torch.float32, device=x.device)
    gh.call(_SIGNATURES, "radegs_sceneio_edge", x.device, x.shape[0], x.shape[1], x.shape[2], x, out)
    return out


# ----------------------------------------------------------------------------- cameras -----------------------------------------------------------------------------
class Camera:
    """scene/cameras.py Camera: upstream's attribute names.  `image` [C, h, w] and `gt_alpha_mask` are device tensors; they and the edge map
    move to `data_device`, the matrices stay on the GPU as upstream's do.  The matrices are computed on the host in float64 from the float32
    world-view and projection matrices and rounded once."""

    def __init__(self, colmap_id, R, T, FoVx, FoVy, image, gt_alpha_mask, image_name, uid, trans=np.array([0.0, 0.0, 0.0]), scale=1.0, data_device="cuda"):
        self.uid, self.colmap_id, self.R, self.T, self.FoVx, self.FoVy, self.image_name = uid, colmap_id, R, T, FoVx, FoVy, image_name
        try:
            self.data_device = torch.device(data_device)
        except Exception as e:
            print(e)
            print(f"[Warning] Custom device {data_device} failed, fallback to default cuda device")
            self.data_device = torch.device("cuda")
        dev = image.device
        edge = edge_map(image)
        self.original_image = image.to(self.data_device)         # clamp(0, 1) is the identity on i / 255
        self.image_width, self.image_height = self.original_image.shape[2], self.original_image.shape[1]
        self.gt_mask = gt_alpha_mask.to(self.data_device) if gt_alpha_mask is not None else None
        self.edge = edge.to(self.data_device)
        self.zfar, self.znear, self.trans, self.scale = 100.0, 0.01, trans, scale
        view = np.float32(world_to_view(R, T, trans, scale)).T
        proj = np.float32(projection(self.znear, self.zfar, FoVx, FoVy)).T
        full = np.float32(view.astype(np.float64) @ proj.astype(np.float64))
        center = np.float32(np.linalg.inv(view.astype(np.float64))[3, :3])
        self.world_view_transform = torch.from_numpy(np.ascontiguousarray(view)).to(dev)
        self.projection_matrix = torch.from_numpy(np.ascontiguousarray(proj)).to(dev)
        self.full_proj_transform = torch.from_numpy(full).to(dev)
        self.camera_center = torch.from_numpy(center).to(dev)


def _pil():
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError("scene_io's default image reader decodes with Pillow, which is not installed: pass `image_reader`") from None
    return Image


def read_image(path):
    """the default image_reader: Pillow's decode, uint8 [H, W] or [H, W, C]; a mode other than L, RGB, RGBA is refused by name"""
    with _pil().open(path) as im:
        if im.mode not in MODES:
            raise NotImplementedError(f"{path}: image mode `{im.mode}`: scene_io takes {', '.join(MODES)} (8 bits per channel); convert the image first")
        return np.array(im)                                # upstream's own call; a writable copy, unlike np.asarray's view of the decoder's buffer


def default_workers():
    return min(16, len(os.sched_getaffinity(0)))


def load_camera(args, id, cam_info, resolution_scale, pixels, device="cuda"):
    """loadCam on decoded pixels: composite (Blender), resize, / 255, planes, edge map"""
    dev = _device(device)
    src, _ = _pixels(pixels, dev)
    if cam_info.white_background is not None:
        H, W, C = src.shape
        if C != 4:                                        # upstream's convert("RGBA"): grey to three channels, alpha 255
            src = torch.cat([src.expand(H, W, 3) if C == 1 else src, torch.full((H, W, 1), 255, dtype=torch.uint8, device=dev)], dim=2).contiguous()
        src = composite_rgba(src, cam_info.white_background)
    resolution = target_resolution(src.shape[1], src.shape[0], args.resolution, resolution_scale)
    _, image, mask = _resize(src, resolution, "hv", False, True)
    return Camera(colmap_id=cam_info.uid, R=cam_info.R, T=cam_info.T, FoVx=cam_info.FovX, FoVy=cam_info.FovY, image=image, gt_alpha_mask=mask,
                  image_name=cam_info.image_name, uid=id, data_device=getattr(args, "data_device", "cuda"))


def load_cameras(cam_infos, resolution_scale, args, image_reader=None, workers=None, device="cuda"):
    """cameraList_from_camInfos.  image_reader(path) -> uint8 pixels runs on a pool of threads (one process holds the GPU); the device work
    runs on the calling thread, camera by camera in input order whatever order the decodes finish in."""
    reader = read_image if image_reader is None else image_reader
    workers = default_workers() if workers is None else int(workers)
    if workers < 1:
        raise RuntimeError("`workers` must be at least 1")
    cam_infos = list(cam_infos)
    if not cam_infos:
        return []
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        decoded = pool.map(reader, [c.image_path for c in cam_infos])
        return [load_camera(args, id, c, resolution_scale, pixels, device) for id, (c, pixels) in enumerate(zip(cam_infos, decoded))]


# ------------------------------------------------------------------------------ Scene ------------------------------------------------------------------------------
def newest_iteration(folder):
    return max(int(name.split("_")[-1]) for name in os.listdir(folder))


class Scene:
    """scene/__init__.py Scene.  `gaussians` is a GaussianModel; its state is read and made through model_io (load_model_ply,
    create_from_pcd, save_model_ply), the path gaussian_model_ops.patch_gaussian_model_io installs as its methods."""

    def __init__(self, args, gaussians, load_iteration=None, shuffle=True, resolution_scales=[1.0], image_reader=None, workers=None):
        self.model_path, self.loaded_iter, self.gaussians = args.model_path, None, gaussians
        if load_iteration:
            self.loaded_iter = newest_iteration(os.path.join(self.model_path, "point_cloud")) if load_iteration == -1 else load_iteration
            print("Loading trained model at iteration {}".format(self.loaded_iter))
        self.train_cameras, self.test_cameras = {}, {}
        if os.path.exists(os.path.join(args.source_path, "sparse")):
            scene_info = read_colmap_scene(args.source_path, args.images, args.eval)
        elif os.path.exists(os.path.join(args.source_path, "transforms_train.json")):
            print("Found transforms_train.json file, assuming Blender data set!")
            scene_info = read_blender_scene(args.source_path, args.white_background, args.eval, image_reader=image_reader)
        else:
            raise RuntimeError(f"{args.source_path}: neither a `sparse` folder nor a transforms_train.json")
        if not self.loaded_iter:
            os.makedirs(self.model_path, exist_ok=True)
            with open(scene_info.ply_path, "rb") as src, open(os.path.join(self.model_path, "input.ply"), "wb") as dst:
                dst.write(src.read())
            camlist = list(scene_info.test_cameras) + list(scene_info.train_cameras)
            with open(os.path.join(self.model_path, "cameras.json"), "w") as f:
                json.dump([camera_to_JSON(id, cam) for id, cam in enumerate(camlist)], f)
        self.cameras_extent = scene_info.nerf_normalization["radius"]
        for s in resolution_scales:
            self.train_cameras[s] = load_cameras(scene_info.train_cameras, s, args, image_reader, workers)
            print(f"Loading Training Cameras: {len(self.train_cameras[s])} .")
            self.test_cameras[s] = load_cameras(scene_info.test_cameras, s, args, image_reader, workers)
            print(f"Loading Test Cameras: {len(self.test_cameras[s])} .")
        if self.loaded_iter:
            model_io.load_model_ply(gaussians, os.path.join(self.model_path, "point_cloud", "iteration_" + str(self.loaded_iter), "point_cloud.ply"))
        else:
            model_io.create_from_pcd(gaussians, scene_info.point_cloud, self.cameras_extent)

    def save(self, iteration):
        model_io.save_model_ply(self.gaussians, os.path.join(self.model_path, "point_cloud/iteration_{}".format(iteration), "point_cloud.ply"))

    def getTrainCameras(self, scale=1.0):
        return self.train_cameras[scale]

    def getTestCameras(self, scale=1.0):
        return self.test_cameras[scale]


def __getattr__(name):
    """`GaussianModel`, imported on first use: `from scene import Scene, GaussianModel` works after install() as it does upstream"""
    if name == "GaussianModel":
        from gaussian_model import GaussianModel
        return GaussianModel
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def install():
    """Registers this module as `scene`, so that upstream's `from scene import Scene` resolves to it (as lpipsPyTorch/ and tetranerf/ shadow
    upstream's names).  Opt-in: nothing calls it."""
    sys.modules["scene"] = sys.modules[__name__]
    return sys.modules[__name__]
