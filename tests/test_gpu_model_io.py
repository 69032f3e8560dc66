"""GPU tier of the model state I/O: rade-gs_amd/model_io.py and the four kernels of csrc/radegs_modelio.hip against
tests/model_io_restatement.py and tests/golden/g_model_io.npz (the reference's own code run on the CPU).

Pack and unpack move bits: files are compared byte for byte and tensors bit for bit.  Init: f_dc is one IEEE subtraction and one IEEE
division, bit-equal to the float32 restatement and within 1 ulp of torch's RGB2SH (its divisor is the double constant rounded by the
division's own path); scaling within 2^-22 max(1, |ref|) of float64 on the same dist2 (sqrt correctly rounded: 2^-24 relative = at most 2^-24
absolute after the log; logf a few ulp of the result; a factor of about 2 is left).  Reset: |got - f64| <= 2 reset_K 2^-24 (kappa + |f64|),
kappa = 1 / (1 - x), reset_K the reference's own measured error in those units (3.73): the device's expf / logf differ from the host's by an
error of the same size.  The test prints what the device reaches; DESIGN 11 N15 records it."""
import collections
import os

import numpy as np
import pytest
import torch

import gaussian_model_ops as gmo
import model_io as mio
import model_io_restatement as mr
from simple_knn._C import distCUDA2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_model_io.npz"))
SIZES, DEGREES = (0, 1, 63, 64, 65, 257), (0, 1, 3)
_CASES = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def case(P, degree, with_filter):
    """(host arrays, device tensors, the restatement's file) of a model whose every element has a value of its own, made once"""
    key = (P, degree, with_filter)
    if key not in _CASES:
        K = (degree + 1) ** 2 - 1
        shapes = ((P, 3), (P, 1, 3), (P, K, 3), (P, 1), (P, 3), (P, 4), (P, 1))
        arrays = [(np.arange(int(np.prod(s)), dtype=np.float32).reshape(s) + np.float32(100000 * (i + 1) + 0.5)) * np.float32(-1 if i % 2 else 1)
                  for i, s in enumerate(shapes)]
        if not with_filter:
            arrays[6] = None
        _CASES[key] = (arrays, [None if a is None else dev(a) for a in arrays], mr.model_file(*arrays))
    return _CASES[key]


def assert_state(st, arrays, what=""):
    assert isinstance(st, mio.GaussianState)
    for name, got, want in zip(st._fields, st, arrays):
        if want is None:
            assert got is None, (what, name)
            continue
        assert got.dtype == torch.float32 and got.is_contiguous() and got.device == torch.device(DEV), (what, name)
        assert tuple(got.shape) == want.shape, (what, name, tuple(got.shape), want.shape)
        assert same_bits(host(got), want), (what, name)


# ------------------------------------------------------------------------------ pack ------------------------------------------------------------------------------
@pytest.mark.parametrize("with_filter", [True, False])
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("P", SIZES)
def test_the_saved_file_equals_the_restatements_byte_for_byte(tmp_path, P, degree, with_filter):
    _, tensors, want = case(P, degree, with_filter)
    path = str(tmp_path / "deep" / "er" / "point_cloud.ply")          # the directory is made, as upstream's mkdir_p does
    mio.save_ply(path, *tensors)
    assert open(path, "rb").read() == want


@pytest.mark.parametrize("chunk_rows", [64, 100, 256, 257, 1000])
def test_chunks_on_and_off_the_tile_edge_write_the_same_file(tmp_path, chunk_rows):
    _, tensors, want = case(257, 3, True)
    path = str(tmp_path / "chunked.ply")
    mio.save_ply(path, *tensors, chunk_rows=chunk_rows)
    assert open(path, "rb").read() == want


def test_a_row_range_packs_those_rows():
    arrays, tensors, _ = case(257, 3, True)
    table = mr.model_columns(*arrays)
    for begin, end in ((0, 257), (0, 0), (100, 200), (64, 65), (193, 257), (1, 256)):
        got = mio.pack_records(*tensors, row_begin=begin, row_end=end)
        assert got.shape == (end - begin, 63) and same_bits(host(got), table[begin:end]), (begin, end)
    with pytest.raises(RuntimeError, match="outside the 257 rows"):
        mio.pack_records(*tensors, row_begin=0, row_end=258)


def test_wrong_dtype_shape_layout_and_device_are_refused(tmp_path):
    _, t, _ = case(65, 1, True)
    path = str(tmp_path / "never.ply")
    for k, bad, msg in ((0, t[0].double(), "`xyz` must be float32"), (1, t[1].reshape(65, 3), "`features_dc` must have shape"),
                        (4, t[4][:64], "`scaling` must have shape"), (5, t[5].t().contiguous().t(), "`rotation` must be contiguous"),
                        (3, t[3].cpu(), "`opacity` must be a GPU tensor"), (6, t[6].reshape(65), "`filter_3D` must have shape")):
        args = list(t)
        args[k] = bad
        with pytest.raises(RuntimeError, match=msg):
            mio.save_ply(path, *args)
    assert not os.path.exists(path)
    with pytest.raises(RuntimeError, match="chunk_rows"):
        mio.save_ply(path, *t, chunk_rows=0)


# ----------------------------------------------------------------------------- unpack -----------------------------------------------------------------------------
@pytest.mark.parametrize("with_filter", [True, False])
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("P", SIZES)
def test_load_returns_what_was_saved_bit_for_bit(tmp_path, P, degree, with_filter):
    arrays, tensors, _ = case(P, degree, with_filter)
    path = str(tmp_path / "m.ply")
    mio.save_ply(path, *tensors)
    assert_state(mio.load_ply(path, max_sh_degree=degree, require_filter=with_filter, device=DEV), arrays)
    assert_state(mio.load_ply(path, require_filter=False, device=DEV), arrays, "degree implied")


def test_special_bit_patterns_survive_the_round_trip(tmp_path):
    arrays = [a.copy() for a in case(65, 1, True)[0]]
    bits = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000], dtype=np.uint32).view(np.float32)
    for a in arrays:
        a.reshape(-1)[:8] = bits
        a.reshape(-1)[-8:] = bits[::-1]
    path = str(tmp_path / "bits.ply")
    mio.save_ply(path, *[dev(a) for a in arrays])
    assert open(path, "rb").read() == mr.model_file(*arrays)
    assert_state(mio.load_ply(path, device=DEV), arrays)


def foreign_file(arrays, fmt="binary_little_endian", types="f4", seed=1, extras=True):
    """a model file as another program might write it: the properties in a permuted order, optionally two unknown ones -- a uchar in front,
    so that every float sits at an odd address, and a short in the middle -- in the given format; returns (bytes, record size)"""
    table = mr.model_columns(*arrays)
    names = mr.attribute_names(3 * arrays[2].shape[1], arrays[6] is not None)
    rng = np.random.default_rng(seed)
    order = [int(j) for j in rng.permutation(len(names))]
    props = [(names[j], types) for j in order]
    if extras:
        props = [("flag", "u1")] + props[:7] + [("label", "i2")] + props[7:]
    rec = np.zeros(table.shape[0], dtype=mr.record_dtype(props, ">" if fmt == "binary_big_endian" else "<"))
    for j in order:
        rec[names[j]] = table[:, j]
    if extras:
        rec["flag"], rec["label"] = rng.integers(0, 256, table.shape[0]), rng.integers(-30000, 30000, table.shape[0])
    head = mr.write_header(table.shape[0], props, fmt=fmt, spelling=1, comments=("written by someone else",))
    if fmt == "ascii":
        body = "".join(" ".join(repr(v.item()) for v in row) + "\n" for row in rec).encode("ascii")
        return head + body, rec.dtype.itemsize
    return head + rec.tobytes(), rec.dtype.itemsize


@pytest.mark.parametrize("P", [1, 65, 257])
def test_permuted_properties_and_unknown_ones_at_odd_addresses(tmp_path, P):
    arrays, _, _ = case(P, 3, True)
    data, S = foreign_file(arrays)
    assert S == 255 and S % 4 == 3
    path = str(tmp_path / "foreign.ply")
    open(path, "wb").write(data)
    assert_state(mio.load_ply(path, max_sh_degree=3, device=DEV), arrays)
    got = mio.read_vertex_columns(path, ["label", "x", "flag"], device=DEV)             # by name, the other 62 are skipped
    rec, _ = mr.read_vertex(data)
    assert same_bits(host(got), np.stack([rec["label"].astype(np.float32), rec["x"], rec["flag"].astype(np.float32)], axis=1))


@pytest.mark.parametrize("fmt", ["binary_big_endian", "ascii"])
def test_big_endian_and_ascii_files_take_the_same_kernel(tmp_path, fmt):
    arrays, _, _ = case(65, 1, False)
    data, _ = foreign_file(arrays, fmt=fmt)
    path = str(tmp_path / "other.ply")
    open(path, "wb").write(data)
    assert_state(mio.load_ply(path, max_sh_degree=1, require_filter=False, device=DEV), arrays, fmt)


def test_double_properties_are_rounded_to_nearest_even_once(tmp_path):
    rng = np.random.default_rng(4)
    P = 65
    arrays64 = [rng.standard_normal(s) * 10.0 ** rng.integers(-3, 4, s) for s in ((P, 3), (P, 1, 3), (P, 3, 3), (P, 1), (P, 3), (P, 4), (P, 1))]
    ties = np.array([1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -(1 + 2.0 ** -24), 1 + 2.0 ** -24 + 2.0 ** -50, 1e-46, 3.5e38, 2.0 ** -149 * 0.5, 2.0 ** -149 * 1.5])
    arrays64[0].reshape(-1)[:8] = ties
    arrays64[2].reshape(-1)[:8] = ties
    names = mr.attribute_names(9)
    table = np.concatenate([arrays64[0], np.zeros((P, 3)), arrays64[1].transpose(0, 2, 1).reshape(P, -1), arrays64[2].transpose(0, 2, 1).reshape(P, -1)]
                           + arrays64[3:], axis=1)
    rec = np.zeros(P, dtype=mr.record_dtype([(n, "f8") for n in names]))
    for j, n in enumerate(names):
        rec[n] = table[:, j]
    data = mr.write_header(P, [(n, "f8") for n in names]) + rec.tobytes()
    path = str(tmp_path / "double.ply")
    open(path, "wb").write(data)
    with np.errstate(over="ignore"):
        want = mr.model_from_file(data)
        assert same_bits(want[0], arrays64[0].astype(np.float32)) and np.isinf(want[0].reshape(-1)[5]) and want[0].reshape(-1)[0] == 1.0
    assert_state(mio.load_ply(path, max_sh_degree=1, device=DEV), want)


@pytest.mark.parametrize("P", [1, 64, 65])
def test_fetch_ply_reads_the_27_byte_record(tmp_path, P):
    rng = np.random.default_rng(P)
    xyz, nrm = rng.standard_normal((P, 3)).astype(np.float32), rng.standard_normal((P, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (P, 3)).astype(np.uint8)
    rgb.reshape(-1)[:3] = [0, 255, 1]
    data = mr.points3d_file(xyz, rgb, nrm)
    assert (len(data) - len(mr.write_header(P, mr.POINTS3D))) == 27 * P
    path = str(tmp_path / "points3D.ply")
    open(path, "wb").write(data)
    got = mio.fetch_ply(path, device=DEV)
    want = mr.fetch_points3d(data)
    assert want[1].dtype == np.float32 and same_bits(want[0], xyz)
    for g, w, name in zip(got, want, got._fields):
        assert g.is_contiguous() and g.dtype == torch.float32 and same_bits(host(g), w), name
    mio.store_ply(path, xyz, rgb)                                                     # storePly's file: the same points and colours, zero normals
    back = mio.fetch_ply(path, device=DEV)
    assert same_bits(host(back.points), xyz) and same_bits(host(back.colors), want[1]) and not host(back.normals).any()


def test_a_payload_at_an_odd_file_offset(tmp_path):
    arrays, _, want = case(65, 3, True)
    props = [(n, "f4") for n in mr.attribute_names(45)]
    for pad in ("x", "xy"):
        head = mr.write_header(65, props, comments=(pad,))
        data = head + want[len(mr.write_header(65, props)):]
        path = str(tmp_path / f"odd_{pad}.ply")
        open(path, "wb").write(data)
        assert mio.read_ply_header(path).data_offset == len(head)
        assert_state(mio.load_ply(path, device=DEV), arrays, pad)
    assert {len(mr.write_header(65, props, comments=(p,))) % 2 for p in ("x", "xy")} == {0, 1}


# ------------------------------------------------------------------------------ init ------------------------------------------------------------------------------
def assert_init(st, points, colors, d2, degree):
    want = mr.init_state(points, colors, d2, degree)
    P, K = points.shape[0], (degree + 1) ** 2 - 1
    assert st.filter_3D is None and tuple(st.features_rest.shape) == (P, K, 3) and tuple(st.features_dc.shape) == (P, 1, 3)
    assert same_bits(host(st.xyz), want["xyz"]) and same_bits(host(st.features_dc), want["features_dc"])
    assert same_bits(host(st.features_rest), want["features_rest"]) and same_bits(host(st.rotation), want["rotation"])
    assert same_bits(host(st.opacity), want["opacity"]) and host(st.opacity)[0, 0] == np.float32(mio.initial_opacity())
    s = host(st.scaling)
    err = np.abs(s.astype(np.float64) - want["scaling64"]) / np.maximum(1.0, np.abs(want["scaling64"]))
    print("init P", P, "scaling: largest error in units of 2^-22 max(1, |ref|):", float(err.max() / 2.0 ** -22))
    assert s.shape == (P, 3) and (err <= 2.0 ** -22).all()
    assert np.array_equal(s[:, 0], s[:, 1]) and np.array_equal(s[:, 0], s[:, 2])
    return want


@pytest.mark.parametrize("P", [4, 65, 1000])
def test_init_from_points(P):
    rng = np.random.default_rng(100 + P)
    points, colors = rng.standard_normal((P, 3)).astype(np.float32), rng.random((P, 3)).astype(np.float32)
    colors.reshape(-1)[:3] = [0.0, 1.0, 0.5]
    p, c = dev(points), dev(colors)
    d2 = distCUDA2(p)
    for degree in (3, 0):
        assert_init(mio.init_from_points(p, c, degree), points, colors, host(d2), degree)          # the kNN step inside
        assert_init(mio.init_from_points(p, c, degree, dist2=d2), points, colors, host(d2), degree)


def test_init_against_the_references_own_run():
    pts, col, d2 = GOLD["pcd_points"], GOLD["pcd_colors"], GOLD["pcd_dist2"]
    st = mio.init_from_points(dev(pts), dev(col), 3, dist2=dev(d2))
    assert_init(st, pts, col, d2, 3)
    ulp = np.abs(host(st.features_dc).view(np.int32).astype(np.int64) - GOLD["pcd_features_dc"].view(np.int32).astype(np.int64))
    assert ulp.max() <= 1 and tuple(GOLD["pcd_features_rest_shape"]) == tuple(st.features_rest.shape)
    assert same_bits(host(st.opacity), GOLD["pcd_opacity"]) and same_bits(host(st.rotation), GOLD["pcd_rotation"])
    ref = GOLD["pcd_scaling"].astype(np.float64)
    assert (np.abs(host(st.scaling) - ref) <= 2 * 2.0 ** -22 * np.maximum(1, np.abs(ref))).all()      # both sides within 2^-22 of float64
    clamped = host(st.scaling)[d2 == 0]                                                              # four coincident points: the clamp at 1e-7
    assert clamped.shape == (4, 3) and (clamped == clamped[0, 0]).all() and abs(clamped[0, 0] - 0.5 * np.log(1e-7)) < 1e-5
    sh = host(mio.init_from_points(dev(np.zeros((512, 3), np.float32)), dev(GOLD["rgb"]), 0, dist2=dev(np.ones(512, np.float32))).features_dc)
    ulp = np.abs(sh.reshape(512, 3).view(np.int32).astype(np.int64) - GOLD["rgb2sh"].view(np.int32).astype(np.int64))
    print("RGB2SH against torch's: largest difference in ulps", int(ulp.max()))
    assert ulp.max() <= 1


# ------------------------------------------------------------------------------ reset ------------------------------------------------------------------------------
_RESET = {}


def reset_reference():
    """the recipe, its float64 value and the device's result, computed once and left unchanged"""
    if not _RESET:
        o, s, f = mr.reset_recipe()
        f64, x, kappa = mr.reset_opacity64(o, s, f)
        _RESET.update(o=o, s=s, f=f, f64=f64, kappa=kappa, got=host(mio.reset_opacity(dev(o), dev(s), dev(f))))
    return _RESET


def test_reset_opacity_on_the_recipe_is_within_twice_the_references_own_error():
    r = reset_reference()
    K = float(GOLD["reset_K"])
    assert r["got"].shape == (4096, 1) and r["got"].dtype == np.float32 and np.isfinite(r["got"]).all() and np.isfinite(r["f64"]).all()
    units = np.abs(r["got"].astype(np.float64) - r["f64"]) / (2.0 ** -24 * (r["kappa"] + np.abs(r["f64"])))
    print("reset_K (the reference's own error)", K, "; the device reaches", float(units.max()), "; differing from the reference's bits:",
          int((r["got"] != GOLD["reset_new"]).sum()), "of 4096")
    assert (units <= 2 * K).all()                      # every element: none is left out


def test_reset_opacity_edge_rows_by_class_then_by_the_bound():
    names, o, s, f = mr.reset_edges()
    got = host(mio.reset_opacity(dev(o), dev(s), dev(f)))[:, 0]
    ref = GOLD["edge_new"][:, 0]
    with np.errstate(all="ignore"):
        f64, _, kappa = (a[:, 0] for a in mr.reset_opacity64(o, s, f))
    K = float(GOLD["reset_K"])
    for i, n in enumerate(names):
        cls = lambda v: "nan" if np.isnan(v) else "+inf" if v == np.inf else "-inf" if v == -np.inf else "finite"   # noqa: E731
        assert cls(got[i]) == cls(ref[i]), (n, got[i], ref[i])
        if np.isfinite(ref[i]):
            assert abs(float(got[i]) - f64[i]) <= 2 * K * 2.0 ** -24 * (kappa[i] + abs(f64[i])), (n, got[i], f64[i])
    clamp = np.log(np.float32(0.01) / (np.float32(1.0) - np.float32(0.01)))
    assert abs(got[names.index("filter 0")] - clamp) <= 2 * K * 2.0 ** -24 * (1 / 0.99 + abs(clamp))      # coef exactly 1: the clamp's logit
    assert got[names.index("filter 0")] == got[names.index("scale e^8")]


@pytest.mark.parametrize("P", [1, 64, 65])
def test_reset_opacity_sizes_and_moments(P):
    r = reset_reference()
    o, s, f = (dev(r[k][:P]) for k in "osf")
    got, m, v = mio.reset_opacity(o, s, f, zero_moments=True)
    assert same_bits(host(got), r["got"][:P])                                       # a row's value does not depend on the launch's size
    for z in (m, v):
        assert z.shape == (P, 1) and z.dtype == torch.float32 and not host(z).any() and not np.signbit(host(z)).any()
    empty = mio.reset_opacity(o[:0], s[:0], f[:0])
    assert empty.shape == (0, 1)


class Model:
    """a stand-in with upstream's attribute names"""

    def __init__(self, sh_degree):
        self.active_sh_degree, self.max_sh_degree = 0, sh_degree


GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"))


def test_reset_through_the_model_moves_the_optimizer_state():
    r = reset_reference()
    P = 4096
    cls = gmo.patch_gaussian_model_io(gmo.patch_gaussian_model(type("Patched", (Model,), {})))
    m = cls(1)
    shapes = dict(_xyz=(P, 3), _features_dc=(P, 1, 3), _features_rest=(P, 3, 3), _rotation=(P, 4))
    for a, shape in shapes.items():
        setattr(m, a, torch.nn.Parameter(torch.zeros(shape, device=DEV)))
    m._opacity, m._scaling, m.filter_3D = torch.nn.Parameter(dev(r["o"])), torch.nn.Parameter(dev(r["s"])), dev(r["f"])
    m.optimizer = torch.optim.Adam([{"params": [getattr(m, a)], "lr": 0.0, "name": n} for n, a in GROUPS], lr=0.0, eps=1e-15)
    old, scaling = m._opacity, m._scaling
    state = {"step": torch.tensor(float(GOLD["reset_before_step"])), "exp_avg": dev(GOLD["reset_before_exp_avg"]),
             "exp_avg_sq": dev(GOLD["reset_before_exp_avg_sq"])}
    m.optimizer.state[old] = state
    m.reset_opacity()
    group = [g for g in m.optimizer.param_groups if g["name"] == "opacity"][0]
    new = group["params"][0]
    assert new is m._opacity and new is not old and isinstance(new, torch.nn.Parameter) and new.requires_grad and new.is_leaf
    assert old not in m.optimizer.state and m.optimizer.state[new] is state and len(group["params"]) == 1
    assert float(state["step"]) == float(GOLD["reset_after_step"])
    assert same_bits(host(state["exp_avg"]), GOLD["reset_after_exp_avg"]) and same_bits(host(state["exp_avg_sq"]), GOLD["reset_after_exp_avg_sq"])
    assert same_bits(host(new), r["got"]) and m._scaling is scaling
    assert [g["params"][0] for g in m.optimizer.param_groups if g["name"] == "scaling"][0] is scaling


# ---------------------------------------------------------------------------- lifecycle ----------------------------------------------------------------------------
def test_create_save_load_through_the_patched_class(tmp_path):
    cls = gmo.patch_gaussian_model_io(gmo.patch_gaussian_model(type("Patched", (Model,), {})))
    rng = np.random.default_rng(8)
    P = 300
    Pcd = collections.namedtuple("BasicPointCloud", "points colors normals")
    pcd = Pcd(rng.standard_normal((P, 3)), rng.random((P, 3)), np.zeros((P, 3)))           # float64, as fetchPly returns them
    a = cls(3)
    a.create_from_pcd(pcd, 1.5)
    assert a.spatial_lr_scale == 1.5 and a.active_sh_degree == 0
    assert a.max_radii2D.shape == (P,) and a.max_radii2D.is_cuda and not host(a.max_radii2D).any()
    for _, attr in GROUPS:
        p = getattr(a, attr)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf and p.is_cuda, attr
    assert tuple(a._features_rest.shape) == (P, 15, 3) and same_bits(host(a._xyz), pcd.points.astype(np.float32))
    want = mr.init_state(pcd.points.astype(np.float32), pcd.colors.astype(np.float32), host(distCUDA2(a._xyz.detach())), 3)
    assert same_bits(host(a._features_dc), want["features_dc"])
    with torch.no_grad():                                                                  # a model that has trained a little
        a._features_rest.copy_(dev(rng.standard_normal((P, 15, 3)).astype(np.float32)))
        a._rotation.copy_(dev(rng.standard_normal((P, 4)).astype(np.float32)))
    a.filter_3D = dev(rng.random((P, 1)).astype(np.float32))
    path = str(tmp_path / "point_cloud" / "iteration_7" / "point_cloud.ply")
    a.save_ply(path)
    b = cls(3)
    b.load_ply(path)
    assert b.active_sh_degree == 3
    for _, attr in GROUPS:
        p, q = getattr(a, attr), getattr(b, attr)
        assert isinstance(q, torch.nn.Parameter) and q.requires_grad and q.is_leaf and q.shape == p.shape and same_bits(host(q), host(p)), attr
    assert not isinstance(b.filter_3D, torch.nn.Parameter) and same_bits(host(b.filter_3D), host(a.filter_3D))
    with pytest.raises(RuntimeError, match="SH degree 2 needs 24"):
        cls(2).load_ply(path)


# --------------------------------------------------------------------------- determinism ---------------------------------------------------------------------------
def test_two_runs_return_the_same_bits(tmp_path):
    arrays, tensors, want = case(65, 3, True)
    assert same_bits(host(mio.pack_records(*tensors)), host(mio.pack_records(*tensors)))
    path = str(tmp_path / "m.ply")
    open(path, "wb").write(want)
    one, two = mio.load_ply(path, device=DEV), mio.load_ply(path, device=DEV)
    assert all(same_bits(host(x), host(y)) for x, y in zip(one, two))
    r = reset_reference()
    o, s, f = (dev(r[k][:65]) for k in "osf")
    assert same_bits(host(mio.reset_opacity(o, s, f)), host(mio.reset_opacity(o, s, f)))
    p, c, d2 = dev(GOLD["pcd_points"][:65]), dev(GOLD["pcd_colors"][:65]), dev(GOLD["pcd_dist2"][:65])
    one, two = mio.init_from_points(p, c, 3, dist2=d2), mio.init_from_points(p, c, 3, dist2=d2)
    assert all(same_bits(host(x), host(y)) for x, y in zip(one[:6], two[:6]))
