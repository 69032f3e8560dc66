"""GPU tier of evaluation from files, from paths to tensors and numbers: eval_io.read_ply_points / read_ply_mesh against the
NumPy structured-dtype reader of tests/evalio_restatement.py on every layout and format (values exactly), against tetmesh.read_ply, and on the
files this project's own writers write; merge_vertices against the restatement; the three drivers against the composition of their parts by
hand (bit for bit: the same kernels on the same inputs) and against the fixtures their synthetic directories are built from."""
import json
import os

import numpy as np
import pytest
import torch

import evalio_restatement as er
import tnteval_restatement as tr
from test_mesheval_golden import cull_cameras, load

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMATS = ("binary_little_endian", "binary_big_endian", "ascii")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def same_bits(t, a):
    got = host(t)
    return got.dtype == a.dtype and got.shape == a.shape and got.tobytes() == np.ascontiguousarray(a).tobytes()


# --------------------------------------------------------------------------- readers ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("layout", sorted(er.LAYOUTS))
def test_readers_equal_the_restatement_on_every_layout(tmp_path, layout, fmt):
    import eval_io
    for V, F in ((37, 50), (4097, 4099), (1, 0)):                    # more than one tile of records; a single vertex without a face
        v, f = er.mesh_data(V, F, seed=V)
        elements, exp_v, exp_f = er.LAYOUTS[layout](v, f)
        path = str(tmp_path / f"{layout}_{V}.ply")
        er.write_ply(path, elements, fmt)
        got = eval_io.read_ply_points(path, DEV)
        assert same_bits(got, er.ply_points(path)) and same_bits(got, exp_v)
        if exp_f is not None:
            gv, gf = eval_io.read_ply_mesh(path, DEV)
            rv, rf = er.ply_mesh(path)
            assert same_bits(gv, rv) and same_bits(gf, rf) and np.array_equal(rf, exp_f.reshape(-1, 3))


def test_read_ply_mesh_equals_tetmesh_read_ply_and_reads_the_projects_writers(tmp_path):
    import eval_io
    import tetmesh
    import tsdf
    v, f = er.mesh_data(301, 517, seed=9)
    v32 = v.astype(np.float32)
    path = str(tmp_path / "tet.ply")
    tetmesh.write_ply(path, v32, f)
    gv, gf = eval_io.read_ply_mesh(path, DEV)
    rv, rf = tetmesh.read_ply(path)
    assert same_bits(gv, rv.astype(np.float64)) and same_bits(gf, rf)
    colors, normals = np.abs(np.sin(v32)), np.cos(v32)
    for kw in (dict(colors=dev(colors)), dict(normals=dev(normals)), dict(colors=dev(colors), normals=dev(normals))):   # tsdf, mesh_clean, unbounded_mesh
        path = str(tmp_path / ("_".join(sorted(kw)) + ".ply"))
        tsdf.write_ply(path, dev(v32), dev(f), **kw)
        gv, gf = eval_io.read_ply_mesh(path, DEV)
        assert same_bits(gv, v32.astype(np.float64)) and same_bits(gf, f) and same_bits(eval_io.read_ply_points(path, DEV), v32.astype(np.float64))


def test_a_quad_or_an_index_out_of_range_anywhere_is_refused(tmp_path):
    import eval_io
    v, f = er.mesh_data(100, 4097, seed=2)
    xyz, cols = er._xyz(v, "f8")
    for where, row, reason in ((4000, [1, 2, 100], "index"), (64, [5, 6, -1], "index")):
        bad = [list(r) for r in f]
        bad[where] = row
        for fmt in FORMATS:
            path = str(tmp_path / f"bad_{fmt}.ply")
            er.write_ply(path, [("vertex", xyz, cols), ("face", [("vertex_indices", ("list", "u1", "i4"))], [bad])], fmt)
            with pytest.raises(RuntimeError, match=r"1 of the 4097 `face` records are not a triangle of indices in \[0, 100\)"):
                eval_io.read_ply_mesh(path, DEV)
    # a quad and a line that keep the element's size: only the kernel can see them
    bad = [list(r) for r in f]
    bad[10], bad[2000] = [1, 2, 3, 4], [7, 8]
    path = str(tmp_path / "quad.ply")
    er.write_ply(path, [("vertex", xyz, cols), ("face", [("vertex_indices", ("list", "u1", "i4"))], [bad])])
    with pytest.raises(RuntimeError, match="`face` records are not a triangle"):
        eval_io.read_ply_mesh(path, DEV)


def test_merge_vertices_equals_the_restatement():
    import eval_io
    rng = np.random.default_rng(0)
    base = rng.uniform(-1, 1, (300, 3))
    pick = rng.integers(0, 300, 2000)
    v = base[pick] + rng.integers(0, 2, (2000, 1)) * 3e-9            # some copies 3e-9 off: welded at eight digits, apart at nine
    v[::97] = np.nan
    v[5, 1] = np.inf
    f = rng.integers(0, 2000, (1500, 3))
    for digits in (8, 9, 2):
        mv, mf = eval_io.merge_vertices(dev(v), dev(f), digits)
        ev, ef = er.merge_vertices(v, f, digits)
        assert same_bits(mv, ev) and same_bits(mf, ef)
    mv, mf = eval_io.merge_vertices(dev(v), dev(f[:0]))
    assert tuple(mv.shape) == (0, 3) and tuple(mf.shape) == (0, 3) and mf.dtype == torch.int64
    mv, mf = eval_io.merge_vertices(dev(v), dev(f).int())            # int32 faces are taken, as everywhere
    assert same_bits(mf, er.merge_vertices(v, f)[1])


# --------------------------------------------------------------------------- Tanks and Temples ---------------------------------------------------------------------------
def write_log(path, poses):
    with open(path, "w") as fh:
        for k, p in enumerate(poses):
            fh.write(f"{k} {k} 0\n")
            fh.write("\n".join(" ".join(repr(float(x)) for x in row) for row in p) + "\n")


@pytest.fixture(scope="module")
def tnt_scene(tmp_path_factory):
    """a scene directory `Church` built from tests/golden/tnteval_pipeline.npz: the mesh in trimesh's layout, the ground truth as a cloud with
    normals and colours, the crop file, a _trans.txt, and 40 cameras whose estimated centres are the reference ones moved by the inverse of
    the fixture's known similarity (mesh frame -> world)"""
    fx = load("tnteval_pipeline.npz")
    root = tmp_path_factory.mktemp("tnt")
    scene = root / "Church"
    os.makedirs(scene)
    v, f, gt = fx["vertices"].astype(np.float64), fx["faces"].astype(np.int64), fx["gt"].astype(np.float64)
    ply = str(root / "recon.ply")
    er.write_ply(ply, er.LAYOUTS["tetmesh"](v, f)[0])
    er.write_ply(str(scene / "Church.ply"), er.LAYOUTS["cloud"](gt, None)[0])
    vol = tr.volume_of(fx)
    with open(scene / "Church.json", "w") as fh:
        json.dump(dict(class_name="SelectionPolygonVolume", orthogonal_axis=vol["orthogonal_axis"], axis_min=vol["axis_min"], axis_max=vol["axis_max"],
                       bounding_polygon=vol["bounding_polygon"].tolist(), version_major=1, version_minor=0), fh)
    rng = np.random.default_rng(40)
    gt_trans = er.similarity(rng, scale=1.0)
    np.savetxt(scene / "Church_trans.txt", gt_trans)
    world = np.tile(np.eye(4), (40, 1, 1))
    world[:, :3, 3] = np.array([3.0, -2.0, 5.0]) + rng.uniform(-3, 3, (40, 3))               # camera centres around the fixture's object
    colmap, est = world.copy(), world.copy()
    colmap[:, :3, 3] = tr.transform(world[:, :3, 3], np.linalg.inv(gt_trans))
    est[:, :3, 3] = tr.transform(world[:, :3, 3], np.linalg.inv(fx["known"]))
    write_log(scene / "Church_COLMAP_SfM.log", colmap)
    write_log(root / "est.log", est)
    np.save(root / "est.npy", est)
    return dict(fx=fx, dataset=str(scene), ply=ply, log=str(root / "est.log"), npy=str(root / "est.npy"), out=str(root / "out"))


def test_run_evaluation_equals_the_composition_by_hand(tnt_scene, capsys):
    import eval_io
    import tnt_eval as te
    sc, fx = tnt_scene, tnt_scene["fx"]
    res = te.run_evaluation(sc["dataset"] + "/", sc["log"], sc["ply"], out_dir=sc["out"])
    report = capsys.readouterr().out
    # by hand
    v, f = eval_io.read_ply_mesh(sc["ply"], DEV)
    gt = eval_io.read_ply_points(os.path.join(sc["dataset"], "Church.ply"), DEV)
    assert same_bits(v, fx["vertices"].astype(np.float64)) and same_bits(f, fx["faces"].astype(np.int64)) and same_bits(gt, fx["gt"].astype(np.float64))
    init = te.trajectory_alignment(None, eval_io.read_trajectory(sc["log"])[0], eval_io.read_trajectory(os.path.join(sc["dataset"], "Church_COLMAP_SfM.log"))[0],
                                   eval_io.load_transform(os.path.join(sc["dataset"], "Church_trans.txt")))
    hand = te.evaluate(v, f, gt, init, te.CropVolume.from_json(os.path.join(sc["dataset"], "Church.json")), te.SCENES_TAU["Church"])
    assert res["scene"] == "Church" and res["tau"] == 0.025 and res["init_transform"].tobytes() == init.tobytes()
    for k in ("precision", "recall", "fscore"):
        assert res[k] == hand[k] and 0 < res[k] < 1
    for k in ("cum_source", "cum_target", "edges_source", "transformation"):
        assert res[k].tobytes() == hand[k].tobytes()
    for k in ("s", "t", "dist1", "dist2", "idx1", "idx2"):
        assert torch.equal(res[k], hand[k])
    # the coarse alignment: exact camera centres, so the known similarity comes back far inside the error the fixture records for the restatement
    assert np.abs(init - fx["known"]).max() <= float(fx["recovery_error"]) and np.abs(init - fx["known"]).max() < 1e-9
    assert "Evaluating Church" in report and "distance tau : 0.025" in report and "f-score : %.4f" % res["fscore"] in report
    assert np.array_equal(np.loadtxt(os.path.join(sc["out"], "Church.recall.txt")), np.loadtxt(_saved(sc["out"], res["cum_target"])))
    assert np.array_equal(np.loadtxt(os.path.join(sc["out"], "Church.precision.txt")), np.loadtxt(_saved(sc["out"], res["cum_source"])))
    assert np.array_equal(np.loadtxt(os.path.join(sc["out"], "Church.prf_tau_plotstr.txt")),
                          np.loadtxt(_saved(sc["out"], np.array([res["precision"], res["recall"], res["fscore"], 0.025, 5]))))
    again = te.run_evaluation(sc["dataset"], sc["npy"], sc["ply"])                           # the .npy branch; no out_dir: nothing written
    assert again["fscore"] == res["fscore"] and again["init_transform"].tobytes() == init.tobytes()


def _saved(folder, array):
    path = os.path.join(folder, "expected.txt")
    np.savetxt(path, array)
    return path


def test_trajectory_alignment_takes_the_sparse_trajectory_above_1600_poses(tmp_path):
    import tnt_eval as te
    rng = np.random.default_rng(3)
    known = er.similarity(rng)
    ref = np.tile(np.eye(4), (30, 1, 1))
    ref[:, :3, 3] = rng.uniform(-3, 3, (30, 3))
    full = np.tile(np.eye(4), (1700, 1, 1))
    full[:, :3, 3] = rng.uniform(-3, 3, (1700, 3))                                          # frames the mapping does not name: unrelated
    frames = np.sort(rng.permutation(1700)[:30]) + 1
    full[frames - 1, :3, 3] = tr.transform(ref[:, :3, 3], np.linalg.inv(known))
    with open(tmp_path / "map.txt", "w") as fh:
        fh.write("30\n1700\n" + "".join(f"{a} {b}\n" for a, b in enumerate(frames)))
    T = te.trajectory_alignment(str(tmp_path / "map.txt"), full, ref, None)
    assert np.abs(T - known).max() < 1e-9
    with pytest.raises(RuntimeError, match="1700 poses to register against 30"):
        te.trajectory_alignment(None, full, ref, None)


def test_cull_mesh_file_equals_the_composition_by_hand(tmp_path):
    import eval_io
    import tetmesh
    import tnt_cull
    import tntcull_cases as cs
    v, f, _ = cs.box_scene()
    v = np.concatenate([v, v[:7]]).astype(np.float32)                                        # seven vertices twice: merge_vertices welds them
    f = np.concatenate([f, [[len(v) - 7, len(v) - 6, len(v) - 5]]]).astype(np.int64)
    mesh, traj = str(tmp_path / "recon.ply"), str(tmp_path / "traj.npy")
    er.write_ply(mesh, er.LAYOUTS["tetmesh"](v.astype(np.float64), f)[0])
    np.save(traj, np.array(cs.ring_cameras(), dtype=np.float64))
    H, W = cs.CULL_SIZE
    fx, fy, cx, cy = cs.CULL_K
    kw = dict(H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, eps=0.1, pose="opencv")
    kv, kf, out = tnt_cull.cull_mesh_file(mesh, traj, **kw)
    assert out == str(tmp_path / "recon_cull.ply") and os.path.isfile(out)
    mv, mf = eval_io.merge_vertices(*eval_io.read_ply_mesh(mesh, DEV))
    ev, ef = er.merge_vertices(v.astype(np.float64), f)
    assert mv.shape[0] <= len(v) - 7 and same_bits(mv, ev) and same_bits(mf, ef)
    hv, hf = tnt_cull.cull_mesh(mv, mf, eval_io.get_traj(traj), **kw)
    assert torch.equal(kv, hv) and torch.equal(kf, hf) and 0 < kv.shape[0] < mv.shape[0] and kv.dtype == torch.float64
    rv, rf = tetmesh.read_ply(out)
    assert np.array_equal(rv, host(kv).astype(np.float32)) and np.array_equal(rf, host(kf))
    other = str(tmp_path / "elsewhere.ply")
    assert tnt_cull.cull_mesh_file(mesh, traj, out_path=other, **kw)[2] == other and os.path.isfile(other)


# ------------------------------------------------------------------------------- DTU -------------------------------------------------------------------------------
def test_evaluate_dtu_mesh_equals_the_composition_by_hand(tmp_path):
    """A DTU directory built around tests/golden/mesheval_cull.npz (the mesh and four masked cameras, extended to eight by four cameras with
    full masks) and mesheval_chamfer.npz (the scan, ObsMask, plane): the calibration files hold K R [I | -C] with C the training cameras'
    centres under a known similarity that puts the culled mesh where the scan is."""
    import eval_io
    import mesh_eval
    from scipy.io import savemat
    cull_fx, ch = load("mesheval_cull.npz"), load("mesheval_chamfer.npz")
    cams = [(w2c, fx, fy, W, H, dev(mask)) for w2c, fx, fy, W, H, mask in cull_cameras(cull_fx)]
    rng = np.random.default_rng(8)
    for k in range(4):                                                                       # four more: they see everything
        w2c = cams[k][0].copy()
        w2c[:3, 3] += rng.uniform(-1, 1, 3).astype(np.float32)
        cams.append((w2c, cams[k][1], cams[k][2], cams[k][3], cams[k][4], torch.ones_like(cams[k][5])))
    centres = np.array([np.linalg.inv(c[0].astype(np.float64))[:3, 3] for c in cams])
    R = er.similarity(rng, scale=1.0)[:3, :3]
    shift = ch["vertices"].astype(np.float64).mean(0) - 6.0 * (R @ cull_fx["out_vertices"].astype(np.float64).mean(0))
    root = tmp_path / "dtu"
    os.makedirs(root / "Calibration" / "cal18")
    os.makedirs(root / "ObsMask")
    os.makedirs(root / "Points" / "stl")
    K = np.array([[2892.33, 0.0, 823.205], [0.0, 2883.18, 619.071], [0.0, 0.0, 1.0]])
    for i, c in enumerate(centres):
        C, Rc = 6.0 * (R @ c) + shift, er.similarity(rng, scale=1.0)[:3, :3]
        np.savetxt(root / "Calibration" / "cal18" / f"pos_{i + 1:03d}.txt", K @ np.concatenate([Rc, -(Rc @ C)[:, None]], 1), fmt="%.6f")
    savemat(root / "ObsMask" / "ObsMask24_10.mat", dict(ObsMask=ch["obs_mask"], BB=ch["BB"], Res=ch["Res"]))
    savemat(root / "ObsMask" / "Plane24.mat", dict(P=ch["plane"]))
    er.write_ply(str(root / "Points" / "stl" / "stl024_total.ply"), er.LAYOUTS["cloud"](ch["stl"].astype(np.float64), None)[0])
    mesh = str(tmp_path / "recon.ply")
    er.write_ply(mesh, er.LAYOUTS["tetmesh"](cull_fx["vertices"].astype(np.float64), cull_fx["faces"].astype(np.int64))[0])
    # by hand
    v, f = mesh_eval.cull_mesh(*eval_io.read_ply_mesh(mesh, DEV), cams)
    assert same_bits(v, cull_fx["out_vertices"].astype(np.float64)) and same_bits(f, cull_fx["out_faces"])          # the fixture's culled mesh
    points = np.array([torch.as_tensor(c[0]).float().inverse()[:3, 3].numpy() for c in cams])
    scale_gt, scale, r, t = eval_io.dtu_alignment(points, eval_io.dtu_camera_centres(str(root / "Calibration" / "cal18"), n=8))
    assert abs(float(scale_gt) / float(scale) - 6.0) < 1e-3 and np.abs(r - R).max() < 1e-4                          # float32 centres
    va = ((v * float(scale_gt) / float(scale)) @ dev(r.T.astype(np.float64)) + dev(t.astype(np.float64))).contiguous()
    stl = eval_io.read_ply_points(str(root / "Points" / "stl" / "stl024_total.ply"), DEV)
    assert same_bits(stl, ch["stl"].astype(np.float64))
    hand = mesh_eval.dtu_chamfer(va, f, stl, *eval_io.load_dtu_masks(str(root), 24), generator=torch.Generator(device=DEV).manual_seed(5))
    out = str(tmp_path / "vis")
    res = mesh_eval.evaluate_dtu_mesh(mesh, cams, str(root), 24, out_dir=out, perm=hand["perm"])
    for k in ("mean_d2s", "mean_s2d", "overall"):
        assert res[k] == hand[k] and np.isfinite(res[k])
    assert torch.equal(res["vertices"], va) and torch.equal(res["faces"], f) and torch.equal(res["dist_d2s"], hand["dist_d2s"])
    assert json.load(open(os.path.join(out, "results.json"))) == {k: res[k] for k in ("mean_d2s", "mean_s2d", "overall")}
    cv, cf = eval_io.read_ply_mesh(os.path.join(out, "recon_culled.ply"), DEV)
    av, af = eval_io.read_ply_mesh(os.path.join(out, "recon_aligned.ply"), DEV)
    assert same_bits(cv, cull_fx["out_vertices"].astype(np.float64)) and torch.equal(cf, f) and torch.equal(af, f)
    assert same_bits(av, host(va).astype(np.float32).astype(np.float64))
