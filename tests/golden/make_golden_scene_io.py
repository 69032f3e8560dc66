"""Generates tests/golden/g_scene_io.npz and the two fixture datasets tests/golden/scene_colmap/ and tests/golden/scene_blender/ from the
REFERENCE's own code run on the CPU (/root/reference): utils/general_utils.py PILtoTorch, utils/camera_utils.py loadCam and camera_to_JSON,
scene/cameras.py Camera, scene/dataset_readers.py readColmapSceneInfo (with readColmapCameras and getNerfppNorm inside it) and
readCamerasFromTransforms, scene/colmap_loader.py read_*_binary / read_*_text.  Build container only.

open3d, plyfile, trimesh, cv2 and simple_knn are stubbed, scene/__init__.py is kept from running, `cuda` is routed to the CPU as
make_golden_model_io.py does; fetchPly / storePly (plyfile) are replaced by no-ops, the point cloud is model_io's business.  The datasets are
written with tests/scene_io_restatement.py's writers and read back by the reference's readers.

Image.fromarray(<int8 array>, "RGB") (dataset_readers.py:276) is refused by this Pillow (12.2): the generator hands the same memory over as
uint8, which is what the Pillow releases that accepted the call did with it.  The cast to np.byte itself is upstream's and runs.

edge_K and cam_K are the reference's own float32 errors against float64, in units of 2^-24 (edge) and 2^-24 max(1, max|M|) (matrices): the GPU
tests allow twice that.  The resize cases record a SHA-256 of Pillow's own bytes, full and horizontal-only, and the bytes too where few."""
import hashlib
import json
import os
import shutil
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import scene_io_restatement as sr  # noqa: E402

for name, attrs in {"plyfile": ("PlyData", "PlyElement"), "simple_knn": (), "simple_knn._C": ("distCUDA2",), "trimesh": (), "cv2": (), "open3d": ()}.items():
    m = types.ModuleType(name)
    for a in attrs:
        setattr(m, a, None)
    sys.modules.setdefault(name, m)
sys.path.insert(0, "/root/reference")
pkg = types.ModuleType("scene")            # keep scene/__init__.py from running
pkg.__path__ = ["/root/reference/scene"]
sys.modules["scene"] = pkg
for fn in ("zeros", "ones", "empty", "full", "tensor", "rand", "randn"):   # device="cuda" -> CPU
    def _route(*a, __f=getattr(torch, fn), **k):
        if str(k.get("device", "")).startswith("cuda"):
            k.pop("device")
        return __f(*a, **k)
    setattr(torch, fn, _route)
torch.Tensor.cuda = lambda self, *a, **k: self

from PIL import Image  # noqa: E402
import scene.colmap_loader as cl  # noqa: E402
import scene.dataset_readers as dr  # noqa: E402
import utils.camera_utils as cu  # noqa: E402
from utils.general_utils import PILtoTorch  # noqa: E402

dr.fetchPly = lambda path: None
dr.storePly = lambda path, xyz, rgb: None
_fromarray = Image.fromarray
Image.fromarray = lambda a, mode=None: _fromarray(a.view(np.uint8) if a.dtype == np.int8 else a, mode)

data = {}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


rng = np.random.default_rng(16)

# ---------------------------------------------------------------- the COLMAP dataset ----------------------------------------------------------------
W, H = 53, 37
colmap = os.path.join(HERE, "scene_colmap")
shutil.rmtree(colmap, ignore_errors=True)
os.makedirs(os.path.join(colmap, "sparse", "0"))
os.makedirs(os.path.join(colmap, "images"))
cameras = [(1, "SIMPLE_PINHOLE", W, H, [48.5, 26.5, 18.5]), (2, "PINHOLE", W, H, [51.25, 47.75, 26.0, 19.0])]
names = ["view_d.png", "view_a.png", "view_f.png", "view_c.png", "view_b.png", "view_e.png"]        # not in name order
images = []
for i, name in enumerate(names):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    t = rng.standard_normal(3) * 2.0 + [0.0, 0.0, 4.0]
    n2d = int(rng.integers(0, 4))
    images.append((i + 1, q.tolist(), t.tolist(), 1 + i % 2, name, rng.random((n2d, 2)).tolist(), [int(v) for v in rng.integers(-1, 40, n2d)]))
    rgba = name == "view_c.png"
    px = sr.content((H, W, 4 if rgba else 3), "uniform", seed=100 + i)
    px = (px.astype(np.int32) // 3 + (np.arange(W)[None, :, None] * 3 + np.arange(H)[:, None, None] * 2)).clip(0, 255).astype(np.uint8)   # a ramp under the noise
    Image.fromarray(px, "RGBA" if rgba else "RGB").save(os.path.join(colmap, "images", name))
points = [(j + 1, (rng.standard_normal(3) * 1.5).tolist(), [int(v) for v in rng.integers(0, 256, 3)], float(rng.random()),
           [(int(rng.integers(1, 7)), int(rng.integers(0, 3))) for _ in range(int(rng.integers(2, 5)))]) for j in range(40)]
sparse = os.path.join(colmap, "sparse", "0")
sr.write_cameras_bin(os.path.join(sparse, "cameras.bin"), cameras)
sr.write_cameras_txt(os.path.join(sparse, "cameras.txt"), cameras)
sr.write_images_bin(os.path.join(sparse, "images.bin"), images)
sr.write_images_txt(os.path.join(sparse, "images.txt"), images)
sr.write_points3d_bin(os.path.join(sparse, "points3D.bin"), points)
sr.write_points3d_txt(os.path.join(sparse, "points3D.txt"), points)

# the reference's readers on both encodings
for kind, ri, rp in (("bin", cl.read_extrinsics_binary, cl.read_points3D_binary), ("txt", cl.read_extrinsics_text, cl.read_points3D_text)):
    # the reference's text reader of cameras asserts PINHOLE (colmap_loader.py:159): the SIMPLE_PINHOLE line is read from the .bin in both rounds
    cams, ims = cl.read_intrinsics_binary(os.path.join(sparse, "cameras.bin")), ri(os.path.join(sparse, "images." + kind))
    xyz, rgb, err = rp(os.path.join(sparse, "points3D." + kind))
    data.update({f"colmap_{kind}_cam_ids": np.array(sorted(cams)), f"colmap_{kind}_cam_models": np.array([cams[k].model for k in sorted(cams)]),
                 f"colmap_{kind}_cam_wh": np.array([[cams[k].width, cams[k].height] for k in sorted(cams)]),
                 f"colmap_{kind}_cam_params": np.concatenate([cams[k].params for k in sorted(cams)]),
                 f"colmap_{kind}_im_ids": np.array(list(ims)), f"colmap_{kind}_im_q": np.array([ims[k].qvec for k in ims]),
                 f"colmap_{kind}_im_t": np.array([ims[k].tvec for k in ims]), f"colmap_{kind}_im_cam": np.array([ims[k].camera_id for k in ims]),
                 f"colmap_{kind}_im_names": np.array([ims[k].name for k in ims]),
                 f"colmap_{kind}_im_xys": np.concatenate([np.asarray(ims[k].xys, dtype=np.float64).reshape(-1, 2) for k in ims]),
                 f"colmap_{kind}_im_p3d": np.concatenate([np.asarray(ims[k].point3D_ids, dtype=np.int64).reshape(-1) for k in ims]),
                 f"colmap_{kind}_xyz": xyz, f"colmap_{kind}_rgb": rgb, f"colmap_{kind}_err": np.asarray(err).reshape(-1)})
for k in [k for k in data if k.startswith("colmap_bin_")]:
    assert np.array_equal(data[k], data[k.replace("_bin_", "_txt_")]), k


def f64_matrices(R, T, fovx, fovy):
    Rt = np.zeros((4, 4))
    Rt[:3, :3], Rt[:3, 3], Rt[3, 3] = R.transpose(), T, 1.0
    view = np.linalg.inv(np.linalg.inv(Rt)).T
    top, right = np.tan(fovy / 2) * 0.01, np.tan(fovx / 2) * 0.01
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[3, 2], P[2, 2], P[2, 3] = 2 * 0.01 / (2 * right), 2 * 0.01 / (2 * top), 1.0, 100.0 / (100.0 - 0.01), -(100.0 * 0.01) / (100.0 - 0.01)
    proj = P.T
    return view, proj, view @ proj, np.linalg.inv(view)[3, :3]


cam_K = np.zeros(4)
edge_K = 0.0


def record(prefix, infos, cams):
    global edge_K
    data.update({prefix + "names": np.array([c.image_name for c in infos]), prefix + "uids": np.array([c.uid for c in infos]),
                 prefix + "R": np.array([c.R for c in infos]), prefix + "T": np.array([c.T for c in infos]),
                 prefix + "fov": np.array([[c.FovX, c.FovY] for c in infos]), prefix + "wh": np.array([[c.width, c.height] for c in infos])})
    mats = [[], [], [], []]
    for info, cam in zip(infos, cams):
        assert cam.image_name == info.image_name and cam.colmap_id == info.uid
        ref = (cam.world_view_transform, cam.projection_matrix, cam.full_proj_transform, cam.camera_center)
        for j, (r, m) in enumerate(zip(ref, f64_matrices(info.R, info.T, info.FovX, info.FovY))):
            assert r.dtype == torch.float32
            cam_K[j] = max(cam_K[j], float(np.max(np.abs(r.numpy().astype(np.float64) - m)) / (2.0 ** -24 * max(1.0, np.max(np.abs(m))))))
            mats[j].append(m)
        img = cam.original_image.numpy()
        edge_K = max(edge_K, float(np.max(np.abs(cam.edge.numpy().astype(np.float64) - sr.edge_map64(img))) / 2.0 ** -24))
        assert np.all(cam.edge.numpy()[0] == 0) and np.all(cam.edge.numpy()[:, -1] == 0)
        data[prefix + "image_" + cam.image_name] = img
        if cam.gt_mask is not None:
            data[prefix + "mask_" + cam.image_name] = cam.gt_mask.numpy()
    for j, n in enumerate(("view64", "proj64", "full64", "center64")):
        data[prefix + n] = np.array(mats[j])


class Args:
    resolution, data_device = 2, "cpu"


for ev in (False, True):
    info = dr.readColmapSceneInfo(colmap, None, ev, llffhold=4)
    p = "colmap_eval_" if ev else "colmap_"
    data.update({p + "train_names": np.array([c.image_name for c in info.train_cameras]), p + "test_names": np.array([c.image_name for c in info.test_cameras]),
                 p + "translate": info.nerf_normalization["translate"], p + "radius": np.asarray(info.nerf_normalization["radius"])})
    if not ev:
        cams = cu.cameraList_from_camInfos(info.train_cameras, 1.0, Args)
        record("colmap_cam_", info.train_cameras, cams)
        data["colmap_cam_uid_order"] = np.array([c.uid for c in cams])
        data["colmap_cameras_json"] = np.array(json.dumps([cu.camera_to_JSON(i, c) for i, c in enumerate(info.train_cameras)]))
        for c in info.train_cameras:
            data["pixels_" + c.image_name] = np.array(c.image)
assert os.listdir(sparse).count("points3D.ply") == 0

# load_image: PILtoTorch per plane as loadCam calls it, on a size that is no integer fraction, and one image at full size
for mode, name in (("RGB", "view_a"), ("RGBA", "view_c"), ("L", "view_b")):
    im = Image.open(os.path.join(colmap, "images", name + ".png"))
    im = im.convert("L") if mode == "L" else im
    assert im.mode == mode
    if mode == "L":                          # the other two are pixels_view_a and pixels_view_c
        data["load_pixels_L"] = np.array(im)
    for size in ((20, 14), (W, H)) if mode == "RGB" else ((20, 14),):
        planes = [PILtoTorch(p, size) for p in im.split()[:3]] if mode == "RGBA" else [PILtoTorch(im, size)]
        data["load_%s_%dx%d" % ((mode,) + size)] = torch.cat(planes, dim=0).numpy()
        if mode == "RGBA":
            data["load_RGBA_mask_%dx%d" % size] = PILtoTorch(im.split()[3], size).numpy()
data["lut"] = (torch.arange(256, dtype=torch.uint8) / 255.0).numpy()

# ---------------------------------------------------------------- the Blender dataset ----------------------------------------------------------------
blender = os.path.join(HERE, "scene_blender")
shutil.rmtree(blender, ignore_errors=True)
os.makedirs(os.path.join(blender, "train"))
pairs = sr.all_pairs_rgba()                                                     # red: every (colour, alpha) pair once
Image.fromarray(pairs, "RGBA").save(os.path.join(blender, "train", "r_0.png"))
small = sr.content((H, W, 4), "uniform", seed=200)
small[:, :10, 3], small[:, 10:20, 3] = 0, 255
Image.fromarray(small, "RGBA").save(os.path.join(blender, "train", "r_1.png"))


def pose(k):
    c2w = np.eye(4)
    a = 0.7 * k + 0.3
    c2w[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0, 0], [0, 0.6, -0.8], [0, 0.8, 0.6]])
    c2w[:3, 3] = [4.0 * np.sin(a), -4.0 * np.cos(a), 1.5 + k]
    return c2w.tolist()


for split, frames in (("train", ("train/r_0", "train/r_1")), ("test", ("train/r_1",))):
    with open(os.path.join(blender, f"transforms_{split}.json"), "w") as f:
        json.dump({"camera_angle_x": 0.6911112070083618, "frames": [{"file_path": p, "transform_matrix": pose(k)} for k, p in enumerate(frames)]}, f, indent=1)
pixels = {"r_0": pairs, "r_1": small}      # r_0 is a formula (scene_io_restatement.all_pairs_rgba): not recorded
data["blender_pixels_r_1"] = small


class Args8:
    resolution, data_device = 8, "cpu"


for white in (False, True):
    infos = dr.readCamerasFromTransforms(blender, "transforms_train.json", white)
    p = "blender_white_" if white else "blender_black_"
    for c in infos:
        comp = np.array(c.image)
        assert np.array_equal(comp, sr.composite(pixels[c.image_name], white)), "the restatement's composite is not upstream's"
        data[p + "composite_" + c.image_name + "_sha256"] = np.array(sha(comp))
        if comp.size < 8192:
            data[p + "composite_" + c.image_name] = comp
    record(p, infos, cu.cameraList_from_camInfos(infos, 1.0, Args8))
    norm = dr.getNerfppNorm(infos)
    data.update({p + "translate": norm["translate"], p + "radius": np.asarray(norm["radius"])})
data["blender_test_names"] = np.array([c.image_name for c in dr.readCamerasFromTransforms(blender, "transforms_test.json", True)])

# the random initial cloud: upstream's calls in upstream's order (dataset_readers.py:307-308) under a seed
np.random.seed(7)
xyz = np.random.random((100_000, 3)) * 2.6 - 1.3
shs = np.random.random((100_000, 3)) / 255.0
data.update(cloud_seed=np.asarray(7), cloud_xyz_head=xyz[:16], cloud_xyz_sum=np.asarray(xyz.sum()), cloud_rgb_head=(dr.SH2RGB(shs) * 255)[:16])

# ---------------------------------------------------------------- resize ----------------------------------------------------------------
for shape, (h, w) in sr.RESIZE_SHAPES:
    for kind in sr.CONTENTS:
        a = sr.content(shape, kind)
        full = np.stack([np.asarray(Image.fromarray(a[:, :, c]).resize((w, h))) for c in range(shape[2])], axis=-1)
        hor = np.stack([np.asarray(Image.fromarray(a[:, :, c]).resize((w, shape[0]))) for c in range(shape[2])], axis=-1)
        if shape[2] == 3:
            assert np.array_equal(full, np.asarray(Image.fromarray(a, "RGB").resize((w, h))))
        assert np.array_equal(full, sr.resize(a, (w, h))) and np.array_equal(hor, sr.resize(a, (w, h), passes="h"))
        if full.size < 8192:                 # the bytes themselves where they are few, for a failing test to show; the digests decide
            data[sr.case_key(shape, (h, w), kind)] = full
        data[sr.case_key(shape, (h, w), kind) + "_sha256"] = np.array(sha(full))
        data[sr.case_key(shape, (h, w), kind) + "_h_sha256"] = np.array(sha(hor))
    print(shape, (h, w), "min/max", int(full.min()), int(full.max()))

data.update(edge_K=np.asarray(edge_K), cam_K=cam_K, pillow_version=np.array(Image.__version__ if hasattr(Image, "__version__") else ""))
print("edge_K", edge_K, "cam_K", cam_K)
path = os.path.join(HERE, "g_scene_io.npz")
np.savez_compressed(path, **data)
total = os.path.getsize(path) + sum(os.path.getsize(os.path.join(d, f)) for top in (colmap, blender) for d, _, fs in os.walk(top) for f in fs)
print(os.path.basename(path), os.path.getsize(path), "bytes; with the datasets", total)
assert total < 330_000
