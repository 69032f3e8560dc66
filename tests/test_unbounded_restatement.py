"""CPU tier of unbounded mesh extraction: tests/unbounded_restatement.py -- the NumPy float32 restatement of include/radegs.h,
"Unbounded mesh extraction", which the kernels are held to bit for bit -- against the reference's own extract_mesh_unbounded
(tests/golden/unbounded_*.npz, written by tests/golden/make_golden_unbounded.py) and against properties that do not depend on it.

The band.  Each fixture holds the reference's float32 run and the same code fed with float64 samples, maps and matrices.  The restatement
must lie within 2 x the largest |float32 run - float64 run| of the reference itself on that fixture, against the float64 run: two valid
float32 evaluation orders may each miss the float64 value by that much (the CPU BLAS order of `points @ full_proj_transform` is not the
restatement's).  The band is measured by the generator and stored, not chosen here: 3.2e-6 (sphere) and 4.2e-6 (wide) for the tsdf,
7.1e-7 and 9.0e-7 for the colours.  Samples that sit on a decision of some view in float64 (|px|, |py| within 1e-4 of 1, |z| < 1e-4,
|sdf + trunc| < 1e-4 trunc) are left out, 0.058 % and 0.083 % of the two fixtures; the generator refuses more than 1 %."""
import os

import numpy as np
import pytest

import unbounded_restatement as ur

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("sphere", "wide")


@pytest.fixture(scope="module", params=FIXTURES)
def golden(request):
    g = dict(np.load(os.path.join(GOLDEN, f"unbounded_{request.param}.npz")))
    H, W = g["depth"].shape[1:]
    g["views"] = [(g["full_proj"][v], g["depth"][v], ur.pattern_colour(v, W, H)) for v in range(len(g["depth"]))]
    g["name"] = request.param
    return g


def test_fixture_leaves_out_at_most_one_percent(golden):
    assert golden["left_out"].mean() <= 0.01 and golden["left_out_colour"].mean() <= 0.01
    assert golden["band"] > 0 and golden["band_colour"] > 0
    assert (golden["tsdf64"] != 1).mean() > 0.3                     # the fixture does integrate
    if golden["name"] == "wide":                                     # and reaches beyond the unit ball, and beyond a world norm of 1.9
        mag = np.linalg.norm(golden["samples"].astype(np.float64), axis=1)
        assert (mag > 1).mean() > 0.5 and mag.max() > 1.9 and ((mag > 1) & (golden["tsdf64"] != 1)).sum() > 500


def test_tsdf_within_twice_the_references_own_float32_error(golden):
    got = ur.fuse(golden["samples"], golden["views"], float(golden["voxel_size"]), golden["center"], float(golden["radius"]), contract=True)
    keep = ~golden["left_out"] & ~np.isnan(golden["tsdf64"])
    assert np.array_equal(np.isnan(got), np.isnan(golden["tsdf64"]))
    err = np.abs(got[keep].astype(np.float64) - golden["tsdf64"][keep]).max()
    ref = np.abs(golden["tsdf32"][keep].astype(np.float64) - golden["tsdf64"][keep]).max()
    print(f"{golden['name']}: restatement {err:.3e}, reference float32 {ref:.3e}, band {float(golden['band']):.3e}, left out {golden['left_out'].mean():.5f}")
    assert ref == float(golden["band"])
    assert err <= 2 * float(golden["band"])


def test_colours_within_twice_the_references_own_float32_error(golden):
    _, got = ur.fuse(golden["colour_points"], golden["views"], float(golden["voxel_size"]), golden["center"], float(golden["radius"]), contract=False,
                     return_rgb=True)
    keep = ~golden["left_out_colour"]
    err = np.abs(got[keep].astype(np.float64) - golden["colour64"][keep]).max()
    print(f"{golden['name']}: colour restatement {err:.3e}, band {float(golden['band_colour']):.3e}")
    assert (golden["colour64"][keep] > 0).mean() > 0.9
    assert err <= 2 * float(golden["band_colour"])


def test_host_helpers_equal_the_references(golden):
    """center, radius, R and voxel_size: float64 host arithmetic in upstream's order -- equality, no ulp needed"""
    import unbounded_mesh as um
    for mod in (um, ur):
        center, radius = mod.scene_normalisation(list(golden["world_view"]))
        assert np.array_equal(center, golden["center"]) and radius == float(golden["radius"])
        assert mod.contracted_bound(golden["xyz"], center, radius) == float(golden["R"])
        assert radius * 2 / int(golden["resolution"]) == float(golden["voxel_size"])


def test_contract_and_uncontract_are_inverse():
    import unbounded_mesh as um
    rng = np.random.default_rng(3)
    x = rng.standard_normal((200, 3)) * np.array([0.3, 2.0, 30.0])[rng.integers(0, 3, 200), None]
    y = um.contract(x)
    assert (np.linalg.norm(y, axis=1) < 2).all() and np.array_equal(y[np.linalg.norm(x, axis=1) < 1], x[np.linalg.norm(x, axis=1) < 1])
    assert np.allclose(um.uncontract(y), x, rtol=1e-9, atol=1e-9)
    assert np.allclose(ur.contract_f32(x), y, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------- dense marching cubes -------------------------------------------------------------------
def test_all_256_cases_on_one_cell():
    T = ur.tables()
    ax, ay, az = np.array([0.5, 1.75], np.float32), np.array([-2.0, -1.0], np.float32), np.array([3.0, 3.5], np.float32)
    lo, hi = np.array([0.5, -2.0, 3.0]), np.array([1.75, -1.0, 3.5])
    for case in range(256):
        neg = np.array([(case >> i) & 1 for i in range(8)], bool)
        mag = np.float32(0.25) + np.float32(0.125) * np.arange(8, dtype=np.float32)
        corner = np.where(neg, -mag, mag).astype(np.float32)
        values = np.zeros((2, 2, 2), np.float32)
        for i in range(8):
            values[i & 1, (i >> 1) & 1, i >> 2] = corner[i]
        v, keys, f = ur.dense_marching_cubes(values, ax, ay, az)
        mask = int(T["edge_mask"][case])
        assert len(v) == bin(mask).count("1") and len(f) == int(T["ntri"][case]), case
        assert len(np.unique(keys)) == len(keys) and (np.diff(keys) > 0).all()
        # every vertex on its cut edge, at the ratio of the two corner values
        edges = [e for e in range(12) if mask >> e & 1]
        want = {}
        for e in edges:
            dx, dy, dz, axis = T["edge_info"][e]
            o = np.array([dx, dy, dz])
            far = o.copy()
            far[axis] += 1
            v_o, v_e = values[tuple(o)], values[tuple(far)]
            assert (v_o < 0) != (v_e < 0)
            t = np.float32(0 - v_o) / np.float32(v_e - v_o)
            p = np.where(o == 1, hi, lo).astype(np.float32)
            assert o[axis] == 0                                      # the owner is the edge's lower end
            p[axis] = p[axis] + t * (np.float32(hi[axis]) - p[axis])
            want[int(((o[0] * 2 + o[1]) * 2 + o[2]) * 3 + axis)] = p
        assert sorted(want) == keys.tolist(), case
        for k, row in zip(keys.tolist(), v):
            assert np.array_equal(row, want[k]), (case, k, row, want[k])
        # the faces are the table's edges, in table order
        tri = T["tri"][case][:3 * int(T["ntri"][case])].reshape(-1, 3)
        key_of_edge = {e: int(((T["edge_info"][e][0] * 2 + T["edge_info"][e][1]) * 2 + T["edge_info"][e][2]) * 3 + T["edge_info"][e][3]) for e in edges}
        assert np.array_equal(keys[f], np.array([[key_of_edge[int(e)] for e in row] for row in tri], np.int64).reshape(-1, 3)), case


def analytic_sphere(p):
    return (np.linalg.norm(p.astype(np.float64) - np.array([0.03, -0.02, 0.05]), axis=1) - 0.6).astype(np.float32)


def test_sphere_over_eight_crops_is_watertight_after_the_weld_and_not_before():
    parts = ur.cropped_marching_cubes(analytic_sphere, 1.0, 18, 9)
    assert len(parts) == 8 and all(len(p[0]) for p in parts)
    v, f = ur.weld(parts)
    rep = ur.mesh_report(v, f)
    assert rep["edges_in_two_faces"] and rep["directed_once"] and rep["no_collapsed_face"] and rep["all_vertices_used"]
    assert rep["volume"] > 0 and rep["euler"] == 2
    assert abs(rep["volume"] - 4 / 3 * np.pi * 0.6 ** 3) < 0.05
    keys = np.concatenate([p[1] for p in parts])
    assert len(np.unique(keys)) == len(v) < len(keys)               # vertices on the shared planes were emitted twice (or four times)
    # the duplicates carry the same bits: the weld picks any
    allv = np.concatenate([p[0] for p in parts])
    order = np.argsort(keys, kind="stable")
    same = keys[order][1:] == keys[order][:-1]
    assert same.sum() > 50 and np.array_equal(allv[order][1:][same].view(np.uint32), allv[order][:-1][same].view(np.uint32))
    # without the weld the seams are open
    v2, f2 = ur.concatenate(parts)
    rep2 = ur.mesh_report(v2, f2)
    assert not rep2["edges_in_two_faces"] and rep2["euler"] != 2


def test_all_positive_lattice_yields_nothing():
    ax = np.linspace(-1, 1, 5).astype(np.float32)
    for values in (np.ones((5, 5, 5), np.float32), np.zeros((5, 5, 5), np.float32), np.full((5, 5, 5), np.nan, np.float32)):
        v, k, f = ur.dense_marching_cubes(values, ax, ax, ax)
        assert v.shape == (0, 3) and k.shape == (0,) and f.shape == (0, 3)
    v, f = ur.weld([ur.dense_marching_cubes(np.ones((5, 5, 5), np.float32), ax, ax, ax)])
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_the_scene_mesh_is_closed_and_coloured():
    """the end-to-end scene of tests/test_gpu_unbounded.py, in the restatement: resolution 32, crops of 16"""
    v, f, c, info = ur.sphere_mesh()
    rep = ur.mesh_report(v, f)
    assert rep["edges_in_two_faces"] and rep["directed_once"] and rep["volume"] > 0 and rep["euler"] == 2 and len(f) > 1000
    d = np.abs(np.linalg.norm(v.astype(np.float64) - ur.SPHERE_CENTRE, axis=1) - ur.SPHERE_RADIUS)
    assert d.max() < 5 * info["voxel_size"]
    col = np.asarray(ur.COLOUR, np.float32)
    assert (c >= col / 2).all() and (c < col).all()
