"""tests/scene_io_restatement.py against Pillow itself (this file alone imports it, and skips where it is absent) and against
tests/golden/g_scene_io.npz, which holds what the reference's own code and Pillow 12.2 gave (tests/golden/make_golden_scene_io.py).  The
GPU tier compares the kernels with the golden file and with this restatement; this tier is what ties the restatement to its sources."""
import os

import numpy as np
import pytest

import scene_io_restatement as sr

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_scene_io.npz"))
IDS = ["%dx%dx%d-%dx%d" % (s + z) for s, z in sr.RESIZE_SHAPES]


def pillow(a, size):
    """every plane on its own, as loadCam resizes an image with an alpha channel"""
    Image = pytest.importorskip("PIL.Image")
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(a[:, :, c])).resize(size)) for c in range(a.shape[2])], axis=-1)


@pytest.mark.parametrize("kind", sr.CONTENTS)
@pytest.mark.parametrize("shape,size", sr.RESIZE_SHAPES, ids=IDS)
def test_the_restatement_gives_the_recorded_bytes(shape, size, kind):
    h, w = size
    key = sr.case_key(shape, size, kind)
    a = sr.content(shape, kind)
    full, hor = sr.resize(a, (w, h)), sr.resize(a, (w, h), passes="h")
    assert full.shape == (h, w, shape[2]) and hor.shape == (shape[0], w, shape[2])
    assert sr.sha256(full) == str(GOLD[key + "_sha256"]) and sr.sha256(hor) == str(GOLD[key + "_h_sha256"])
    if key in GOLD.files:
        assert np.array_equal(full, GOLD[key])


@pytest.mark.parametrize("kind", sr.CONTENTS)
@pytest.mark.parametrize("shape,size", sr.RESIZE_SHAPES, ids=IDS)
def test_the_restatement_gives_pillows_bytes(shape, size, kind):
    h, w = size
    a = sr.content(shape, kind)
    assert np.array_equal(sr.resize(a, (w, h)), pillow(a, (w, h)))
    assert np.array_equal(sr.resize(a, (w, h), passes="h"), pillow(a, (w, shape[0])))


def test_an_rgb_image_resized_whole_equals_its_planes_resized_apart():
    Image = pytest.importorskip("PIL.Image")
    a = sr.content((37, 53, 3), "uniform")
    assert np.array_equal(np.asarray(Image.fromarray(a, "RGB").resize((20, 14))), sr.resize(a, (20, 14)))
    grey = sr.content((64, 97, 1), "binary")[:, :, 0]
    assert np.array_equal(np.asarray(Image.fromarray(grey).resize((31, 40))), sr.resize(grey, (31, 40)))


def test_the_contents_reach_both_ends_of_the_clip():
    for kind in ("binary", "rows"):
        out = sr.resize(sr.content((37, 53, 3), kind), (106, 80))
        assert out.min() == 0 and out.max() == 255


def test_piltotorch_and_the_table():
    assert np.array_equal(sr.lut().view(np.uint32), GOLD["lut"].view(np.uint32))
    assert np.array_equal(sr.pil_to_torch(GOLD["pixels_view_a"], (20, 14)).view(np.uint32), GOLD["load_RGB_20x14"].view(np.uint32))
    assert np.array_equal(sr.pil_to_torch(GOLD["load_pixels_L"], (20, 14)).view(np.uint32), GOLD["load_L_20x14"].view(np.uint32))
    rgba = sr.pil_to_torch(GOLD["pixels_view_c"], (20, 14))
    assert np.array_equal(rgba[:3].view(np.uint32), GOLD["load_RGBA_20x14"].view(np.uint32))
    assert np.array_equal(rgba[3:].view(np.uint32), GOLD["load_RGBA_mask_20x14"].view(np.uint32))
    assert sr.lut().min() == 0.0 and sr.lut().max() == 1.0               # clamp(0, 1) is the identity


def test_the_cameras_images_are_the_restatements():
    for name in GOLD["colmap_cam_names"]:
        px = GOLD["pixels_" + name]
        got = sr.pil_to_torch(px, sr.target_resolution(px.shape[1], px.shape[0], 2, 1.0))
        assert np.array_equal(got[:3].view(np.uint32), GOLD["colmap_cam_image_" + name].view(np.uint32))
        if px.shape[2] == 4:
            assert np.array_equal(got[3:].view(np.uint32), GOLD["colmap_cam_mask_" + name].view(np.uint32))


@pytest.mark.parametrize("white", [False, True])
def test_the_composite(white):
    p = "blender_white_" if white else "blender_black_"
    pairs = sr.all_pairs_rgba()
    red = {(int(c), int(a)) for c, a in zip(pairs[:, :, 0].reshape(-1), pairs[:, :, 3].reshape(-1))}
    assert len(red) == 65536
    assert sr.sha256(sr.composite(pairs, white)) == str(GOLD[p + "composite_r_0_sha256"])
    assert np.array_equal(sr.composite(GOLD["blender_pixels_r_1"], white), GOLD[p + "composite_r_1"])
    # full alpha gives the colour back ((c / 255.0) * 255.0 is c for every byte), no alpha gives the background
    assert np.array_equal(sr.composite(pairs[255:256], white)[0, :, 0], np.arange(256)) and np.all(sr.composite(pairs[0:1], white) == (255 if white else 0))
    got = sr.pil_to_torch(sr.composite(pairs, white), (32, 32))
    assert np.array_equal(got.view(np.uint32), GOLD[p + "image_r_0"].view(np.uint32))


def test_the_edge_map_in_float64_is_within_the_recorded_error_of_the_references():
    img = GOLD["load_RGB_53x37"]
    e = sr.edge_map64(img)
    assert e.shape == (37, 53) and not e[0].any() and not e[-1].any() and not e[:, 0].any() and not e[:, -1].any()
    c = img.astype(np.float64)
    y, x = 5, 7
    want = np.exp(-max(np.mean(np.abs(c[:, y, x] - c[:, y, x - 1])), np.mean(np.abs(c[:, y, x] - c[:, y, x + 1])),
                       np.mean(np.abs(c[:, y, x] - c[:, y - 1, x])), np.mean(np.abs(c[:, y, x] - c[:, y + 1, x]))))
    assert e[y, x] == want and 0.0 < float(GOLD["edge_K"]) < 4.0


def test_the_colmap_writers_and_the_records(tmp_path):
    import struct
    cams = [(7, "PINHOLE", 640, 480, [500.0, 501.0, 320.0, 240.0])]
    sr.write_cameras_bin(str(tmp_path / "cameras.bin"), cams)
    raw = open(str(tmp_path / "cameras.bin"), "rb").read()
    assert len(raw) == 8 + 24 + 32 and struct.unpack_from("<QiiQQ", raw) == (1, 7, 1, 640, 480)
    sr.write_points3d_bin(str(tmp_path / "points3D.bin"), [(3, [1.0, 2.0, 3.0], [4, 5, 6], 0.5, [(1, 2), (3, 4)])])
    assert len(open(str(tmp_path / "points3D.bin"), "rb").read()) == 8 + 43 + 8 + 16
    sr.write_images_bin(str(tmp_path / "images.bin"), [(2, [1.0, 0, 0, 0], [0.0, 0, 0], 7, "ab.png", [[1.0, 2.0]], [9])])
    assert len(open(str(tmp_path / "images.bin"), "rb").read()) == 8 + 64 + 7 + 8 + 24
