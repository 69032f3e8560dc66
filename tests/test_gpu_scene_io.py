"""GPU tier of scene ingestion: rade-gs_amd/scene_io.py and the four kernels of csrc/radegs_sceneio.hip against
tests/golden/g_scene_io.npz (the reference's own code and Pillow itself, run on the CPU by tests/golden/make_golden_scene_io.py) and
tests/scene_io_restatement.py.  Nothing here imports Pillow: `image_reader` serves the decoded pixels the generator recorded.

Resize, / 255 and the composite are integer and table work: bytes and float bits are compared for equality (the golden holds a SHA-256 of
Pillow's bytes for every case, and the bytes themselves where they are few).  Edge map: |got - f64| <= 2 edge_K 2^-24, edge_K the
reference's own float32 error against the float64 restatement (0.55 on the fixtures); the kernel computes in float64 and rounds once, and the
test prints what the device reaches (0.500; DESIGN 11 N16 records it).  Camera
matrices: |got - f64| <= 2 cam_K 2^-24 max(1, max|M|) per matrix kind, cam_K measured the same way (0.86, 0.57, 1.29, 2.74)."""
import json
import os
import shutil
import types

import numpy as np
import pytest
import torch

import model_io as mio
import scene_io as sio
import scene_io_restatement as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD = np.load(os.path.join(GOLDEN, "g_scene_io.npz"))
_INPUTS = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def source(shape, kind):
    if (shape, kind) not in _INPUTS:
        _INPUTS[(shape, kind)] = dev(sr.content(shape, kind))
    return _INPUTS[(shape, kind)]


def reader(path):
    """the decoded pixels of a fixture image, from the npz"""
    name = os.path.splitext(os.path.basename(path))[0]
    if name == "r_0":
        return sr.all_pairs_rgba()
    return GOLD["blender_pixels_" + name] if name.startswith("r_") else GOLD["pixels_" + name]


def args(source_path, model_path="", resolution=2, white_background=False, data_device="cuda", eval=False):
    return types.SimpleNamespace(source_path=source_path, model_path=model_path, images=None, eval=eval, white_background=white_background,
                                 resolution=resolution, data_device=data_device)


@pytest.fixture
def colmap(tmp_path):
    """a copy of the fixture dataset: points3D.ply is written on first use, next to the model"""
    return shutil.copytree(os.path.join(GOLDEN, "scene_colmap"), str(tmp_path / "scene_colmap"))


# ----------------------------------------------------------------------------- resize -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sr.CONTENTS)
@pytest.mark.parametrize("shape,size", sr.RESIZE_SHAPES, ids=["%dx%dx%d-%dx%d" % (s + z) for s, z in sr.RESIZE_SHAPES])
def test_resize_gives_pillows_bytes_after_the_horizontal_pass_and_after_both(shape, size, kind):
    h, w = size
    key = sr.case_key(shape, size, kind)
    src = source(shape, kind)
    hor = host(sio.resize_u8(src, (w, h), passes="h"))
    assert hor.shape == (shape[0], w, shape[2]) and hor.dtype == np.uint8
    assert sr.sha256(hor) == str(GOLD[key + "_h_sha256"]), ("horizontal pass", int(np.abs(hor.astype(int) - sr.resize(host(src), (w, h), passes="h")).max()))
    full = host(sio.resize_u8(src, (w, h)))
    assert full.shape == (h, w, shape[2]) and full.dtype == np.uint8
    if key in GOLD.files:
        assert np.array_equal(full, GOLD[key]), int(np.abs(full.astype(int) - GOLD[key]).max())
    assert sr.sha256(full) == str(GOLD[key + "_sha256"]), ("both passes", int(np.abs(full.astype(int) - sr.resize(host(src), (w, h))).max()))


def test_equal_sizes_give_a_copy_and_a_two_dimensional_image_stays_two_dimensional():
    src = source((37, 53, 3), "uniform")
    out = sio.resize_u8(src, (53, 37))
    assert out.data_ptr() != src.data_ptr() and torch.equal(out, src)
    grey = source((64, 97, 1), "uniform")[:, :, 0].contiguous()
    out = sio.resize_u8(grey, (31, 64))
    assert tuple(out.shape) == (64, 31) and sr.sha256(host(out)) == str(GOLD[sr.case_key((64, 97, 1), (64, 31), "uniform") + "_sha256"])


def test_both_ends_of_the_clip_are_reached():
    """bicubic overshoots on 0 / 255 content: without the clip the byte would wrap"""
    out = host(sio.resize_u8(source((37, 53, 3), "binary"), (106, 80)))
    assert out.min() == 0 and out.max() == 255
    bounds, kk = sio.resample_table(37, 80)
    acc = (kk.astype(np.int64) * 255 * (kk > 0)).sum(axis=1) + (1 << 21)
    assert (acc >> 22).max() > 255                                      # a sum the clip has to bring back does occur in this table


# --------------------------------------------------------------------------- load_image ---------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_load_image_gives_piltotorchs_floats(where):
    put = dev if where == "device" else (lambda a: a)
    image, mask = sio.load_image(put(GOLD["pixels_view_a"]), (20, 14), DEV)
    assert mask is None and same_bits(host(image), GOLD["load_RGB_20x14"])
    image, mask = sio.load_image(put(GOLD["pixels_view_a"]), (53, 37), DEV)                     # equal sizes: the table alone
    assert mask is None and same_bits(host(image), GOLD["load_RGB_53x37"])
    image, mask = sio.load_image(put(GOLD["pixels_view_c"]), (20, 14), DEV)
    assert same_bits(host(image), GOLD["load_RGBA_20x14"]) and same_bits(host(mask), GOLD["load_RGBA_mask_20x14"])
    image, mask = sio.load_image(put(GOLD["load_pixels_L"]), (20, 14), DEV)
    assert mask is None and same_bits(host(image), GOLD["load_L_20x14"])
    assert image.is_contiguous() and image.device == torch.device(DEV) and float(image.min()) >= 0.0 and float(image.max()) <= 1.0


def test_the_table_is_torchs_own_division():
    assert same_bits(host(sio._lut(torch.device(DEV))), GOLD["lut"]) and same_bits(sr.lut(), GOLD["lut"])


# ---------------------------------------------------------------------------- composite ----------------------------------------------------------------------------
@pytest.mark.parametrize("white", [False, True])
def test_composite_of_every_colour_alpha_pair(white):
    pairs = sr.all_pairs_rgba()
    p = "blender_white_" if white else "blender_black_"
    got = host(sio.composite_rgba(dev(pairs), white))
    assert got.shape == (256, 256, 3) and np.array_equal(got, sr.composite(pairs, white))
    assert sr.sha256(got) == str(GOLD[p + "composite_r_0_sha256"])
    small = GOLD["blender_pixels_r_1"]
    assert np.array_equal(host(sio.composite_rgba(dev(small), white)), GOLD[p + "composite_r_1"])
    for n in (1, 2, 3, 5, 1023):                                          # counts that are no multiple of the four pixels a thread takes
        flat = pairs.reshape(-1, 4)[7:7 + n]
        assert np.array_equal(host(sio.composite_rgba(dev(flat), white)), sr.composite(flat, white)), n


# ----------------------------------------------------------------------------- edge map -----------------------------------------------------------------------------
def test_edge_map_is_within_twice_the_references_own_error_and_zero_on_the_border(capsys):
    bound = 2.0 * float(GOLD["edge_K"]) * 2.0 ** -24
    worst = 0.0
    images = [GOLD["load_RGB_53x37"], GOLD["load_RGB_20x14"], GOLD["load_L_20x14"], GOLD["blender_white_image_r_0"]]
    rng = np.random.default_rng(3)
    images += [rng.random((3, 70, 131), dtype=np.float32), rng.random((3, 2, 5), dtype=np.float32), rng.random((3, 3, 3), dtype=np.float32),
               rng.random((1, 17, 65), dtype=np.float32)]                          # more than one tile each way; no interior; one interior pixel
    for img in images:
        got = host(sio.edge_map(dev(img))).astype(np.float64)
        assert got.shape == img.shape[1:]
        assert np.all(got[0] == 0) and np.all(got[-1] == 0) and np.all(got[:, 0] == 0) and np.all(got[:, -1] == 0)
        worst = max(worst, float(np.abs(got - sr.edge_map64(img)).max()))
    with capsys.disabled():
        print(f"\nedge map: device reaches {worst / 2.0 ** -24:.3f} x 2^-24, allowed {2.0 * float(GOLD['edge_K']):.3f} x 2^-24")
    assert worst <= bound


# ------------------------------------------------------------------------------ scene ------------------------------------------------------------------------------
def close(got, want, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= rel * np.maximum(np.abs(want), 1e-300)))


def assert_cameras(cams, infos, prefix):
    assert [c.image_name for c in cams] == list(GOLD[prefix + "names"]) and [c.colmap_id for c in cams] == list(GOLD[prefix + "uids"])
    assert [c.uid for c in cams] == list(range(len(cams)))
    K = GOLD["cam_K"]
    for i, (cam, info) in enumerate(zip(cams, infos)):
        assert close(cam.R, GOLD[prefix + "R"][i]) and close(cam.T, GOLD[prefix + "T"][i]) and close([cam.FoVx, cam.FoVy], GOLD[prefix + "fov"][i])
        assert [info.width, info.height] == list(GOLD[prefix + "wh"][i])
        for j, (name, attr) in enumerate((("view64", "world_view_transform"), ("proj64", "projection_matrix"), ("full64", "full_proj_transform"),
                                          ("center64", "camera_center"))):
            got, want = getattr(cam, attr), GOLD[prefix + name][i]
            assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == want.shape
            err = np.abs(host(got).astype(np.float64) - want).max() / (2.0 ** -24 * max(1.0, np.abs(want).max()))
            assert err <= 2.0 * K[j], (attr, err, K[j])
        want = GOLD[prefix + "image_" + cam.image_name]
        assert same_bits(host(cam.original_image), want) and (cam.image_height, cam.image_width) == want.shape[1:]
        if prefix + "mask_" + cam.image_name in GOLD.files:
            assert same_bits(host(cam.gt_mask), GOLD[prefix + "mask_" + cam.image_name])
        else:
            assert cam.gt_mask is None
        edge = host(cam.edge).astype(np.float64)
        assert np.abs(edge - sr.edge_map64(want)).max() <= 2.0 * float(GOLD["edge_K"]) * 2.0 ** -24
        assert (cam.znear, cam.zfar, cam.scale) == (0.01, 100.0, 1.0) and np.array_equal(cam.trans, [0.0, 0.0, 0.0])


def test_colmap_scene_names_order_split_and_host_numbers(colmap):
    info = sio.read_colmap_scene(colmap, device=DEV)
    assert [c.image_name for c in info.train_cameras] == list(GOLD["colmap_train_names"]) and info.test_cameras == []
    assert close(info.nerf_normalization["translate"], GOLD["colmap_translate"]) and close(info.nerf_normalization["radius"], GOLD["colmap_radius"])
    ev = sio.read_colmap_scene(colmap, eval=True, llffhold=4, device=DEV)
    assert [c.image_name for c in ev.train_cameras] == list(GOLD["colmap_eval_train_names"])
    assert [c.image_name for c in ev.test_cameras] == list(GOLD["colmap_eval_test_names"])
    assert close(ev.nerf_normalization["translate"], GOLD["colmap_eval_translate"]) and close(ev.nerf_normalization["radius"], GOLD["colmap_eval_radius"])
    want = json.loads(str(GOLD["colmap_cameras_json"]))
    got = [sio.camera_to_JSON(i, c) for i, c in enumerate(info.train_cameras)]
    for g, w in zip(got, want):
        assert g.keys() == w.keys() and (g["id"], g["img_name"], g["width"], g["height"]) == (w["id"], w["img_name"], w["width"], w["height"])
        assert close(g["position"], w["position"]) and close(g["rotation"], w["rotation"]) and close([g["fx"], g["fy"]], [w["fx"], w["fy"]])
    # the cloud: points3D.ply was written by store_ply and read by fetch_ply
    assert os.path.exists(info.ply_path)
    assert np.array_equal(host(info.point_cloud.points), GOLD["colmap_bin_xyz"].astype(np.float32))
    assert np.array_equal(host(info.point_cloud.colors), (GOLD["colmap_bin_rgb"] / 255.0).astype(np.float32))


def test_colmap_cameras_equal_the_references(colmap):
    info = sio.read_colmap_scene(colmap, device=DEV)
    cams = sio.load_cameras(info.train_cameras, 1.0, args(colmap), image_reader=reader, workers=3)
    assert_cameras(cams, info.train_cameras, "colmap_cam_")
    on_host = sio.load_cameras(info.train_cameras[:2], 1.0, args(colmap, data_device="cpu"), image_reader=reader)
    for a, b in zip(on_host, cams):
        assert a.original_image.device.type == "cpu" and a.edge.device.type == "cpu" and a.world_view_transform.is_cuda
        assert same_bits(host(a.original_image), host(b.original_image)) and same_bits(host(a.edge), host(b.edge))


@pytest.mark.parametrize("white", [False, True])
def test_blender_cameras_equal_the_references(white):
    path = os.path.join(GOLDEN, "scene_blender")
    p = "blender_white_" if white else "blender_black_"
    infos = sio.read_transforms(path, "transforms_train.json", white, image_reader=reader)
    norm = sio.nerfpp_norm(infos)
    assert close(norm["translate"], GOLD[p + "translate"]) and close(norm["radius"], GOLD[p + "radius"])
    cams = sio.load_cameras(infos, 1.0, args(path, resolution=8, white_background=white), image_reader=reader)
    assert_cameras(cams, infos, p)
    test = sio.read_transforms(path, "transforms_test.json", white, image_reader=reader)
    assert [c.image_name for c in test] == list(GOLD["blender_test_names"])


def test_blender_scene_draws_upstreams_cloud_under_a_seed(tmp_path):
    path = shutil.copytree(os.path.join(GOLDEN, "scene_blender"), str(tmp_path / "scene_blender"))
    np.random.seed(int(GOLD["cloud_seed"]))
    info = sio.read_blender_scene(path, True, False, image_reader=reader, device=DEV)
    pts = host(info.point_cloud.points)
    assert pts.shape == (100_000, 3) and np.array_equal(pts[:16], GOLD["cloud_xyz_head"].astype(np.float32))
    assert np.array_equal(host(info.point_cloud.colors)[:16], (GOLD["cloud_rgb_head"].astype(np.uint8) / 255.0).astype(np.float32))
    assert len(info.train_cameras) == 2 and len(info.test_cameras) == 1 and info.ply_path == os.path.join(path, "points3d.ply")


def model():
    return types.SimpleNamespace(max_sh_degree=3, active_sh_degree=0)


def test_scene_writes_its_files_and_makes_the_model_model_io_makes(colmap, tmp_path):
    out = str(tmp_path / "model")
    g = model()
    scene = sio.Scene(args(colmap, out), g, image_reader=reader)
    assert open(os.path.join(out, "input.ply"), "rb").read() == open(os.path.join(colmap, "sparse/0/points3D.ply"), "rb").read()
    want = json.loads(str(GOLD["colmap_cameras_json"]))
    got = json.load(open(os.path.join(out, "cameras.json")))
    assert [c["img_name"] for c in got] == [c["img_name"] for c in want] and close([c["fx"] for c in got], [c["fx"] for c in want])
    assert close(scene.cameras_extent, GOLD["colmap_radius"]) and scene.getTestCameras() == [] and len(scene.getTrainCameras()) == 6
    ref = model()
    mio.create_from_pcd(ref, mio.fetch_ply(os.path.join(out, "input.ply"), device=DEV), scene.cameras_extent)
    for attr in mio._PARAMS + ("max_radii2D",):
        assert same_bits(host(getattr(g, attr)), host(getattr(ref, attr))), attr
    assert g.spatial_lr_scale == scene.cameras_extent
    # save, then the newest iteration is what load_iteration=-1 reads
    g.filter_3D = torch.full((g._xyz.shape[0], 1), 0.25, device=DEV)
    scene.save(30)
    scene.save(7)
    again = model()
    loaded = sio.Scene(args(colmap, out), again, load_iteration=-1, image_reader=reader)
    assert loaded.loaded_iter == 30 and same_bits(host(again._xyz), host(g._xyz)) and same_bits(host(again._scaling), host(g._scaling))


def test_two_runs_are_bit_identical(colmap):
    def run():
        out = []
        for shape, (h, w) in sr.RESIZE_SHAPES[:6]:
            out.append(host(sio.resize_u8(source(shape, "binary"), (w, h))))
        out.append(host(sio.composite_rgba(dev(sr.all_pairs_rgba()), True)))
        info = sio.read_colmap_scene(colmap, device=DEV)
        for cam in sio.load_cameras(info.train_cameras, 1.0, args(colmap), image_reader=reader):
            out += [host(cam.original_image), host(cam.edge), host(cam.full_proj_transform), host(cam.camera_center)]
            out += [host(cam.gt_mask)] if cam.gt_mask is not None else []
        return out
    a, b = run(), run()
    assert len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def test_the_scene_renders(colmap, tmp_path):
    """Scene's cameras and model go into the rasterizer the way upstream's gaussian_renderer.render hands them over"""
    import math

    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    g = model()
    scene = sio.Scene(args(colmap, str(tmp_path / "model")), g, image_reader=reader)
    cam = scene.getTrainCameras()[0]
    settings = GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        kernel_size=0.0, bg=torch.zeros(3, device=DEV), scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
        sh_degree=g.active_sh_degree, campos=cam.camera_center, prefiltered=False, require_depth=True, require_coord=False, debug=False)
    shs = torch.cat((g._features_dc, g._features_rest), dim=1).contiguous()
    with torch.no_grad():
        out = GaussianRasterizer(raster_settings=settings)(means3D=g._xyz, means2D=torch.zeros_like(g._xyz), shs=shs, colors_precomp=None,
                                                           opacities=torch.sigmoid(g._opacity), scales=torch.exp(g._scaling),
                                                           rotations=torch.nn.functional.normalize(g._rotation), cov3D_precomp=None)
    image = out[0]
    assert tuple(image.shape) == tuple(cam.original_image.shape) and bool(torch.isfinite(image).all())
