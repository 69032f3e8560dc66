"""CPU tier of scene ingestion: what rade-gs_amd/scene_io.py does on the host -- the resolution rule, the COLMAP readers and
their fallbacks, the refusals, the coefficient tables, the decode pool's order and install().  No kernel runs here; the GPU tier is
tests/test_gpu_scene_io.py.  Only the two checks of the default Pillow reader may skip (Pillow absent)."""
import os
import shutil
import sys
import threading
import types

import numpy as np
import pytest

import scene_io as sio
import scene_io_restatement as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD = np.load(os.path.join(GOLDEN, "g_scene_io.npz"))
SPARSE = os.path.join(GOLDEN, "scene_colmap", "sparse", "0")


# --------------------------------------------------------------------------- resolution ---------------------------------------------------------------------------
def test_the_listed_divisors_round_half_to_even():
    assert sio.target_resolution(53, 37, 2, 1.0) == (26, 18)              # 26.5 -> 26, 18.5 -> 18: Python's round
    assert sio.target_resolution(54, 38, 4, 1.0) == (14, 10)              # 13.5 -> 14, 9.5 -> 10
    assert sio.target_resolution(53, 37, 1, 1.0) == (53, 37) and sio.target_resolution(1000, 600, 8, 2.0) == (62, 38)      # 62.5 -> 62, 37.5 -> 38
    assert sio.target_resolution(4946, 3286, 1, 1.0) == (4946, 3286)      # a listed divisor never meets the 1600 rule


def test_any_other_value_is_a_target_width_and_truncates():
    assert sio.target_resolution(53, 37, 20, 1.0) == (20, 13)             # 37 / 2.65 = 13.96 -> 13: int, not round
    assert sio.target_resolution(53, 37, 3, 1.0) == (3, 2) and sio.target_resolution(1000, 600, 500, 2.0) == (250, 150)
    for a in ((53, 37, 2, 1.0), (53, 37, 20, 1.0), (4946, 3286, -1, 1.0), (1600, 1200, -1, 2.0), (999, 777, 8, 1.0), (999, 777, 640, 1.0)):
        assert sio.target_resolution(*a) == sr.target_resolution(*a)


def test_the_1600_rule_and_its_one_warning(capsys, monkeypatch):
    monkeypatch.setattr(sio, "_WARNED", False)
    assert sio.target_resolution(4946, 3286, -1, 1.0) == (1600, 1063)
    assert "rescaling to 1.6K" in capsys.readouterr().out
    assert sio.target_resolution(4946, 3286, -1, 2.0) == (800, 531)
    assert capsys.readouterr().out == ""                                  # once
    assert sio.target_resolution(1600, 1200, -1, 1.0) == (1600, 1200)
    # 1601 / (1601 / 1600) is 1599.99..., and int() truncates: upstream's rule gives 1599 here, and so does this one
    assert sio.target_resolution(1601, 1200, -1, 1.0) == sr.target_resolution(1601, 1200, -1, 1.0) == (int(1601 / (1601 / 1600)), int(1200 / (1601 / 1600)))


# ----------------------------------------------------------------------------- readers -----------------------------------------------------------------------------
def check_model(cameras, images, cams_too=True):
    assert list(images) == list(GOLD["colmap_bin_im_ids"]) and [images[k].name for k in images] == list(GOLD["colmap_bin_im_names"])
    assert np.array_equal(np.array([images[k].qvec for k in images]), GOLD["colmap_bin_im_q"])
    assert np.array_equal(np.array([images[k].tvec for k in images]), GOLD["colmap_bin_im_t"])
    assert [images[k].camera_id for k in images] == list(GOLD["colmap_bin_im_cam"])
    assert np.array_equal(np.concatenate([images[k].xys.reshape(-1, 2) for k in images]), GOLD["colmap_bin_im_xys"])
    assert np.array_equal(np.concatenate([images[k].point3D_ids for k in images]), GOLD["colmap_bin_im_p3d"])
    assert sorted(cameras) == list(GOLD["colmap_bin_cam_ids"]) and [cameras[k].model for k in sorted(cameras)] == list(GOLD["colmap_bin_cam_models"])
    assert np.array_equal(np.array([[cameras[k].width, cameras[k].height] for k in sorted(cameras)]), GOLD["colmap_bin_cam_wh"])
    assert np.array_equal(np.concatenate([cameras[k].params for k in sorted(cameras)]), GOLD["colmap_bin_cam_params"])


def test_the_binary_model_is_what_the_references_reader_reads():
    check_model(*sio.read_colmap_model(SPARSE))
    xyz, rgb, err = sio.read_points3d(SPARSE)
    assert np.array_equal(xyz, GOLD["colmap_bin_xyz"]) and np.array_equal(rgb, GOLD["colmap_bin_rgb"]) and np.array_equal(err, GOLD["colmap_bin_err"])
    assert rgb.dtype == np.uint8 and xyz.dtype == np.float64


def test_the_text_files_are_the_fallback(tmp_path):
    d = str(tmp_path / "0")
    os.makedirs(d)
    for name in ("cameras.txt", "images.txt", "points3D.txt"):
        shutil.copy(os.path.join(SPARSE, name), d)
    check_model(*sio.read_colmap_model(d))
    xyz, rgb, err = sio.read_points3d(d)
    assert np.array_equal(xyz, GOLD["colmap_bin_xyz"]) and np.array_equal(rgb, GOLD["colmap_bin_rgb"]) and np.array_equal(err, GOLD["colmap_bin_err"])
    shutil.copy(os.path.join(SPARSE, "images.bin"), d)                    # images.bin alone, cameras.bin missing: the .txt pair, as upstream's try does
    with open(os.path.join(d, "cameras.bin"), "wb") as f:
        f.write(b"\x02\0\0\0\0\0\0\0\x01\0")                               # ends inside a record
    check_model(*sio.read_colmap_model(d))


def test_a_distorted_camera_model_is_refused_with_upstreams_message(tmp_path):
    root = str(tmp_path / "scene")
    d = os.path.join(root, "sparse", "0")
    os.makedirs(d)
    sr.write_cameras_bin(os.path.join(d, "cameras.bin"), [(1, "OPENCV", 53, 37, [50.0, 50.0, 26.5, 18.5, 0.1, 0.0, 0.0, 0.0])])
    sr.write_images_bin(os.path.join(d, "images.bin"), [(1, [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0], 1, "a.png", [], [])])
    with pytest.raises(AssertionError, match="Colmap camera model not handled: only undistorted datasets"):
        sio.read_colmap_scene(root)


def test_qvec2rotmat_is_a_rotation_and_matches_the_restatement():
    q = np.array([0.5, -0.5, 0.5, 0.5])
    R = sio.qvec2rotmat(q)
    assert np.allclose(R @ R.T, np.eye(3)) and np.isclose(np.linalg.det(R), 1.0) and np.array_equal(R, sr.qvec2rotmat(q))


# ----------------------------------------------------------------------------- refusals -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["P", "I;16", "CMYK", "1", "LA"])
def test_an_image_mode_outside_l_rgb_rgba_is_refused_by_name(mode):
    fake = types.SimpleNamespace(mode=mode, size=(4, 4))
    with pytest.raises(NotImplementedError, match="image mode `%s`" % mode.replace(";", ".")):
        sio.load_image(fake, (2, 2))


def test_pixels_that_are_not_eight_bit_or_not_an_image_are_refused():
    with pytest.raises(NotImplementedError, match="uint16"):
        sio.load_image(np.zeros((4, 4), dtype=np.uint16), (2, 2))
    with pytest.raises(NotImplementedError, match="shape"):
        sio.load_image(np.zeros((4, 4, 2), dtype=np.uint8), (2, 2))


def test_the_default_reader_refuses_a_palette_image(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    path = str(tmp_path / "p.png")
    Image.fromarray(np.arange(16, dtype=np.uint8).reshape(4, 4), "L").convert("P").save(path)
    with pytest.raises(NotImplementedError, match="image mode `P`"):
        sio.read_image(path)


def test_the_default_reader_returns_the_recorded_pixels():
    pytest.importorskip("PIL.Image")
    for name in ("view_a", "view_b", "view_c", "view_d", "view_e", "view_f"):
        got = sio.read_image(os.path.join(GOLDEN, "scene_colmap", "images", name + ".png"))
        assert got.dtype == np.uint8 and np.array_equal(got, GOLD["pixels_" + name])
    assert GOLD["pixels_view_c"].shape == (37, 53, 4)
    assert np.array_equal(sio.read_image(os.path.join(GOLDEN, "scene_blender", "train", "r_0.png")), sr.all_pairs_rgba())
    assert np.array_equal(sio.read_image(os.path.join(GOLDEN, "scene_blender", "train", "r_1.png")), GOLD["blender_pixels_r_1"])


# ------------------------------------------------------------------------------ tables ------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(53, 20), (37, 14), (37, 80), (200, 17), (120, 9), (7, 40), (5, 1), (65, 64), (3, 7), (300, 257), (4946, 1600), (3286, 1063)])
def test_the_vectorised_table_is_the_restatements(sizes):
    bounds, kk = sio.resample_table(*sizes)
    want_bounds, want_kk = sr.coefficients(*sizes)
    assert bounds.dtype == np.int32 and kk.dtype == np.int32 and np.array_equal(bounds, want_bounds) and np.array_equal(kk, want_kk)
    assert 255 * int(np.abs(kk.astype(np.int64)).sum(axis=1).max()) + (1 << 21) < 1 << 31
    for i, (lo, n) in enumerate(bounds):
        assert not kk[i, n:].any()


def test_a_table_whose_sum_could_wrap_is_refused(monkeypatch):
    monkeypatch.setattr(sio, "PRECISION_BITS", 24)                        # 255 * 1.2 * 2^24 passes 2^31
    with pytest.raises(RuntimeError, match="would wrap"):
        sio.resample_table(53, 20)


# ------------------------------------------------------------------------- the decode pool -------------------------------------------------------------------------
def test_cameras_come_back_in_input_order_whatever_order_the_decodes_finish_in(monkeypatch):
    infos = [sio.CameraInfo(uid=i, R=np.eye(3), T=np.zeros(3), FovY=1.0, FovX=1.0, image_path="img_%d" % i, image_name="img_%d" % i, width=4, height=4)
             for i in range(6)]
    finished, last_done, lock = [], threading.Event(), threading.Lock()

    def reader(path):
        i = int(path.split("_")[1])
        if i < 3:
            assert last_done.wait(60), "the later decodes never ran: the pool is not concurrent"       # the first three finish after the last
        with lock:
            finished.append(i)
        if i == 5:
            last_done.set()
        return np.full((4, 4, 3), i, dtype=np.uint8)

    seen = []
    monkeypatch.setattr(sio, "load_camera", lambda args, id, info, scale, pixels, device="cuda": seen.append((id, info.uid, int(pixels[0, 0, 0]))) or id)
    out = sio.load_cameras(infos, 1.0, types.SimpleNamespace(resolution=1, data_device="cpu"), image_reader=reader, workers=4)
    assert out == list(range(6)) and seen == [(i, i, i) for i in range(6)]
    assert sorted(finished) == list(range(6)) and finished.index(5) < min(finished.index(i) for i in range(3))
    assert sio.load_cameras([], 1.0, None) == [] and 1 <= sio.default_workers() <= 16


def test_install_registers_the_module_as_scene(monkeypatch):
    monkeypatch.delitem(sys.modules, "scene", raising=False)
    assert "scene" not in sys.modules                                      # opt-in: importing scene_io registered nothing
    assert sio.install() is sio
    from scene import Scene
    assert Scene is sio.Scene and set(("save", "getTrainCameras", "getTestCameras")) <= set(dir(Scene))
