"""tsdf.py's argument checks (no GPU needed: every refusal comes before the first device call) and its PLY writer."""
import numpy as np
import pytest
import torch

import tsdf

K = np.array([[100.0, 0, 8], [0, 100.0, 6], [0, 0, 1]])
E = np.eye(4)


def grid(**kw):
    return tsdf.VoxelBlockGrid(voxel_size=0.01, block_count=4, **kw)


def depth(h=12, w=16, dtype=torch.float32):
    return torch.ones((h, w), dtype=dtype)


def coords(n=2, dtype=torch.int32):
    return torch.zeros((n, 3), dtype=dtype)


def test_cpu_tensors_are_refused():
    g = grid()
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        g.compute_unique_block_coordinates(depth(), K, E)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        g.integrate(coords(), depth(), torch.zeros((12, 16, 3)), K, E)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        tsdf.unique_block_coordinates(coords())
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        tsdf.VoxelBlockGrid(device="cpu")

    class View:
        image_width, image_height, FoVx, FoVy = 16, 12, 0.5, 0.4
        world_view_transform = torch.eye(4)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        tsdf.fuse_views([View()], lambda v: dict(render=torch.zeros((3, 12, 16)), median_depth=torch.ones((1, 12, 16)), mask=torch.ones((1, 12, 16))))


def test_block_resolution_other_than_16_is_refused():
    for r in (8, 32, 15):
        with pytest.raises(RuntimeError, match="block_resolution"):
            tsdf.VoxelBlockGrid(block_resolution=r)
    assert grid(block_resolution=16).block_size == pytest.approx(0.16)


def test_grid_parameters_are_checked():
    for bad in (0, -0.01, float("nan"), float("inf"), "0.01"):
        with pytest.raises(RuntimeError, match="voxel_size"):
            tsdf.VoxelBlockGrid(voxel_size=bad)
    for bad in (0, -1, 2.5, 1 << 19):
        with pytest.raises(RuntimeError, match="block_count"):
            tsdf.VoxelBlockGrid(block_count=bad)


def test_color_must_match_with_color():
    with pytest.raises(RuntimeError, match="with_color"):
        grid(with_color=True).integrate(coords(), depth(), None, K, E)
    with pytest.raises(RuntimeError, match="with_color"):
        grid(with_color=False).integrate(coords(), depth(), torch.zeros((12, 16, 3)), K, E)


def test_bad_shapes_and_dtypes_are_refused_before_any_device_call():
    g = grid()
    colour = torch.zeros((12, 16, 3))
    for bad, what in ((torch.ones((1, 12, 16)), "depth"), (torch.ones(12), "depth"), (depth(dtype=torch.float64), "depth"), (torch.ones((0, 16)), "depth"),
                      (np.ones((12, 16), np.float32), "depth")):
        with pytest.raises(RuntimeError, match=what):
            g.compute_unique_block_coordinates(bad, K, E)
        with pytest.raises(RuntimeError, match=what):
            g.integrate(coords(), bad, colour, K, E)
    for bad in (torch.zeros((3, 12, 16)), torch.zeros((12, 16, 4)), torch.zeros((12, 16, 3), dtype=torch.uint8), torch.zeros((12, 8, 3))):
        with pytest.raises(RuntimeError, match="color"):
            g.integrate(coords(), depth(), bad, K, E)
    for bad in (torch.zeros((2, 4), dtype=torch.int32), torch.zeros(3, dtype=torch.int32), coords(dtype=torch.int64), coords(dtype=torch.float32)):
        with pytest.raises(RuntimeError, match="block_coords"):
            g.integrate(bad, depth(), colour, K, E)
        with pytest.raises(RuntimeError, match="coords"):
            tsdf.unique_block_coordinates(bad)
    for bad_K in (np.eye(4), np.full((3, 3), np.nan), [[1, 2], [3, 4]]):
        with pytest.raises(RuntimeError, match="intrinsic"):
            g.compute_unique_block_coordinates(depth(), bad_K, E)
    for bad_E in (np.eye(3), np.full((4, 4), np.inf)):
        with pytest.raises(RuntimeError, match="extrinsic"):
            g.integrate(coords(), depth(), colour, K, bad_E)
    for name in ("depth_scale", "depth_max", "trunc_voxel_multiplier"):
        with pytest.raises(RuntimeError, match=name):
            g.compute_unique_block_coordinates(depth(), K, E, **{name: 0.0})
        with pytest.raises(RuntimeError, match=name):
            g.integrate(coords(), depth(), colour, K, E, **{name: float("nan")})
    with pytest.raises(RuntimeError, match="weight_threshold"):
        g.extract_triangle_mesh(float("nan"))


def parse_ply(path):
    """a reader written for this test: header line by line, then the two record arrays"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").strip().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    elements, current = {}, None
    for line in lines[2:-1]:
        words = line.split()
        if words[0] == "element":
            current = words[1]
            elements[current] = dict(count=int(words[2]), properties=[])
        else:
            assert words[0] == "property"
            elements[current]["properties"].append(tuple(words[1:]))
    assert list(elements) == ["vertex", "face"]
    kinds = {"float": "<f4", "uchar": "u1"}
    vdtype = np.dtype([(p[1], kinds[p[0]]) for p in elements["vertex"]["properties"]])
    assert elements["face"]["properties"] == [("list", "uchar", "int", "vertex_indices")]
    nv, nf = elements["vertex"]["count"], elements["face"]["count"]
    v = np.frombuffer(data, vdtype, nv, end)
    f = np.frombuffer(data, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), nf, end + nv * vdtype.itemsize)
    assert end + nv * vdtype.itemsize + nf * 13 == len(data)
    return v, f


@pytest.mark.parametrize("as_tensor", [False, True])
def test_write_ply_round_trip(tmp_path, as_tensor):
    rng = np.random.default_rng(5)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    f = rng.integers(0, 7, (9, 3)).astype(np.int64)
    c = np.array([[0, 0.5, 1], [0.2, 0.4, 0.6], [1.5, -0.5, 0.999], [1 / 255, 2 / 255, 254.4 / 255], [0, 0, 0], [1, 1, 1], [0.3, 0.3, 0.3]], np.float32)
    wrap = (lambda a: torch.from_numpy(a)) if as_tensor else (lambda a: a)
    plain, coloured = str(tmp_path / "plain.ply"), str(tmp_path / "coloured.ply")
    tsdf.write_ply(plain, wrap(v), wrap(f))
    pv, pf = parse_ply(plain)
    assert pv.dtype.names == ("x", "y", "z")
    assert np.array_equal(np.stack([pv["x"], pv["y"], pv["z"]], 1), v) and (pf["n"] == 3).all() and np.array_equal(pf["v"], f)
    tsdf.write_ply(coloured, wrap(v), wrap(f), wrap(c))
    cv, cf = parse_ply(coloured)
    assert cv.dtype.names == ("x", "y", "z", "red", "green", "blue")
    assert np.array_equal(np.stack([cv["x"], cv["y"], cv["z"]], 1), v) and np.array_equal(cf["v"], f)
    want = np.rint(np.clip(c.astype(np.float64), 0, 1) * 255).astype(np.uint8)
    assert np.array_equal(np.stack([cv["red"], cv["green"], cv["blue"]], 1), want)
    assert want[2].tolist() == [255, 0, 255] and want[3].tolist() == [1, 2, 254]
    # the uncoloured file is what tetmesh.read_ply reads
    import tetmesh
    rv, rf = tetmesh.read_ply(plain)
    assert np.array_equal(rv, v) and np.array_equal(rf, f)


def test_write_ply_refuses_what_it_cannot_write(tmp_path):
    v = np.zeros((3, 3), np.float32)
    with pytest.raises(RuntimeError, match="face index"):
        tsdf.write_ply(str(tmp_path / "a.ply"), v, np.array([[0, 1, 3]]))
    with pytest.raises(RuntimeError, match="colors"):
        tsdf.write_ply(str(tmp_path / "b.ply"), v, np.array([[0, 1, 2]]), np.zeros((2, 3), np.float32))
    tsdf.write_ply(str(tmp_path / "c.ply"), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), np.zeros((0, 3), np.float32))
    cv, cf = parse_ply(str(tmp_path / "c.ply"))
    assert len(cv) == 0 and len(cf) == 0
