"""The deterministic backward (RADEGS_DETERMINISTIC=1 -> radegs_backward_ordered, include/radegs.h) on the MI355X: the same
criteria as the default path, bit-identical repeats, the summation order restated in numpy and compared bit for bit, exact agreement with
the atomic kernel where the order cannot matter, the edges, and a training loop whose end state has the same digest in two processes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from synth_scene import make_scene, upstream_grads
from test_gpu_parity import MODES, check_backward, check_forward
from util import ATOL, RTOL, close, cov3d_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRADS = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
# What preprocess_bwd_kernel does to a record it keeps (RadegsBwdArgs::keep_sums, AccRecord::store_sums): it stores float4 2 and 3 of it again, i.e.
# slots 8..15.  Slot 8, slot 11 (the abs-gradient sum, passed through) and slot 15 (the opacity sum) go back as they came; slots 9 and 10
# become the reference's mean2D sums (the moments times the conic, plus the plane terms) and slots 12..14 the raw second moments times
# -0.5f.  So LAST_ACC must equal the fixed-order sum BIT FOR BIT in every slot but 9, 10, 12, 13, 14 ...
REWRITTEN = (9, 10, 12, 13, 14)
# ... and of those, 12..14 are an exact function of the sum (a multiplication by -0.5f rounds nothing), so they are compared bit for bit as well
HALVED = (12, 13, 14)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X box"
    return "cuda:0"


def _small_scene(coord, depth, mu_px=3.0):
    """the scene of test_gpu_parity.test_small_scene_all_modes"""
    return make_scene(3000, 200, 136, sh_degree=3, mu_px=mu_px, seed=21, kernel_size=0.1, require_coord=coord, require_depth=depth,
                      pose="random", bg=(0.2, 0.5, 0.9))


def _backward(h, st, g, keep=False):
    """One direct call of _C.rasterize_gaussians_backward over the state `st` of h.forward_native(): ({name: numpy gradient}, LAST_ACC
    [P, REC] or None, LAST_PARTIALS [R, REC] or None).  The switches are re-read from the environment first, like HipRun.backward does."""
    C, rs, dev = h.C, h.rs, h.dev
    e = torch.Tensor([])
    gd = {k: v.to(dev) for k, v in g.items()}
    opt = lambda t: e if t is None else t.detach()
    C.reload_env()
    C.KEEP_ACC = keep
    try:
        out = C.rasterize_gaussians_backward(rs.bg, h.means3D.detach(), st[8], opt(h.colors), opt(h.scales), opt(h.rotations), rs.scale_modifier,
                                             opt(h.cov3D), rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.kernel_size, gd["color"],
                                             gd["coord"], gd["mcoord"], gd["depth"], gd["mdepth"], gd["alpha"], gd["normal"], st[5], opt(h.shs),
                                             rs.sh_degree, rs.campos, st[9], st[0], st[10], st[11], st[4], rs.require_coord, rs.require_depth, False)
        torch.cuda.synchronize(dev)
        rec = 32 if rs.require_coord else 16
        acc = C.LAST_ACC.cpu().numpy()[: h.P * rec].reshape(h.P, rec).copy() if keep else None
        part = None
        if keep and C.LAST_PARTIALS is not None:
            part, R = C.LAST_PARTIALS
            assert R == st[0] and tuple(part.shape) == (R, rec)
            part = part.cpu().numpy()
    finally:
        C.KEEP_ACC = False
        C.LAST_ACC = None
        C.LAST_PARTIALS = None
    return {k: (None if t is None else t.cpu().numpy()) for k, t in zip(GRADS, out)}, acc, part


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def restated_sums(point_list, part, P):
    """The order include/radegs.h specifies, in numpy: a stable argsort of point_list gives every Gaussian its positions in ascending
    order; its partial records are added in that order, one float32 add at a time, starting from 0.0."""
    order = np.argsort(point_list, kind="stable")
    gid = point_list[order]
    first = np.searchsorted(gid, np.arange(P), side="left")
    count = np.searchsorted(gid, np.arange(P), side="right") - first
    acc = np.zeros((P, part.shape[1]), np.float32)
    for k in range(int(count.max()) if P else 0):       # the k-th instance of every Gaussian that has one
        rows = np.nonzero(count > k)[0]
        acc[rows] = acc[rows] + part[order[first[rows] + k]]   # float32 + float32: one rounding, as the kernel's v_add_f32
    return acc, count


def check_against_restatement(s, monkeypatch, colors=None, cov3D=None, seed=0):
    """Ordered backward of `s` with the sums kept: LAST_ACC against the numpy restatement over LAST_PARTIALS and the exported point_list
    (exact outside REWRITTEN, exact times -0.5f in HALVED); slots 9 and 10 -- not a function of the restated record alone -- at ATOL / RTOL
    against the dL_dmeans2D the same launch returned.  Returns (ordered gradients, default gradients, instance counts)."""
    from gpu_util import HipRun
    g = upstream_grads(s, seed)
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    h = HipRun(s, _dev(), colors=colors, cov3D=cov3D)
    st = h.forward_native()
    R, P = st[0], h.P
    got, acc, part = _backward(h, st, g, keep=True)
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "0")
    ref, acc_default, none = _backward(h, st, g, keep=True)
    assert none is None                                   # the default path leaves no partial records
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    rec = 32 if s.require_coord else 16
    if R == 0:
        assert part.shape == (0, rec) and not acc.any()
        return got, ref, np.zeros(P, np.int64)
    pl = h.export("point_list", torch.int32, R).view(np.uint32).astype(np.int64)
    want, count = restated_sums(pl, part, P)
    exact = [c for c in range(rec) if c not in REWRITTEN]
    bad = np.nonzero((_bits(acc[:, exact]) != _bits(want[:, exact])).any(1))[0]
    assert bad.size == 0, f"{bad.size} records differ from the restated order; first: Gaussian {bad[0]} with {count[bad[0]]} instances"
    vis = st[8].cpu().numpy() > 0                         # the write-back touches visible Gaussians only; the others keep their zero sums
    halved = np.where(vis[:, None], np.float32(-0.5) * want[:, HALVED], want[:, HALVED]).astype(np.float32)
    assert np.array_equal(_bits(acc[:, HALVED]), _bits(halved)), "slots 12..14"
    # Slots 9 and 10 hold the mean2D sums in the reference's form: no function of the restated record alone (the conversion uses the conic and
    # the plane terms), and against any other summation order they carry that order's noise.  The one value they can be held against without
    # it is what the same launch returned: dL_dmean2D = these sums times W/2, H/2, one fp32 multiplication each (preprocess_bwd()).
    wh = np.array([0.5 * s.W, 0.5 * s.H], np.float32)
    a, b = acc[vis][:, 9:11] * wh, got["dL_dmeans2D"][vis][:, :2]
    d = acc_default[vis][:, 9:11]
    print(f"slots 9, 10 times W/2, H/2 against the returned dL_dmeans2D: {int((_bits(a) != _bits(b)).sum())} of {a.size} differ in bits; against the "
          f"default path's sums: max |diff| {float(np.abs(acc[vis][:, 9:11] - d).max()) if d.size else 0.0:.3e} at max |value| "
          f"{float(np.abs(d).max()) if d.size else 0.0:.3e}; longest segment {int(count.max())}")
    assert close(a, b, atol=ATOL, rtol=RTOL).all(), f"slots 9, 10: max abs diff {np.abs(a - b).max():.3e}"
    assert np.array_equal(_bits(acc[vis][:, 11]), _bits(got["dL_dmeans2D"][vis][:, 2]))
    return got, ref, count


def _within_band(got, ref):
    """ordered against default gradients: the band the project uses for sums that differ in summation order (smoke(), check_backward's
    accumulator check): ATOL + 1e-4 of the tensor's scale, 1e-3 relative"""
    for k in GRADS:
        if got[k] is None:
            assert ref[k] is None
            continue
        assert np.isfinite(got[k]).all(), k
        scale = float(np.abs(ref[k]).max()) + 1e-30
        assert close(got[k], ref[k], atol=ATOL + 1e-4 * scale, rtol=1e-3).all(), (k, float(np.abs(got[k] - ref[k]).max()), scale)


# ---- 1. the default path's criteria ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coord,depth", MODES)
def test_same_criteria_as_the_default_path(coord, depth, monkeypatch):
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    s = _small_scene(coord, depth)
    o, _ = check_forward(s)
    check_backward(s, o, seed=21)


# ---- 2. bit-identical repeats ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coord,depth", [(False, True), (True, True)])
def test_repeats_are_bit_identical(coord, depth, monkeypatch):
    from gpu_util import HipRun
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    s = _small_scene(coord, depth)
    g = upstream_grads(s, 21)
    h = HipRun(s, _dev())
    st = h.forward_native()
    torch.cuda.synchronize()
    first, acc1, _ = _backward(h, st, g, keep=True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                          # a non-default stream: its own cached scratch
        second, acc2, _ = _backward(h, st, g, keep=True)
    side.synchronize()
    # an unrelated backward in between: the cached scratch of the default stream now holds another scene's partial records
    other = make_scene(4000, 203, 131, sh_degree=1, mu_px=5.0, seed=64, kernel_size=0.1, require_coord=coord, require_depth=depth, pose="random")
    ho = HipRun(other, _dev())
    _backward(ho, ho.forward_native(), upstream_grads(other, 64))
    third, acc3, _ = _backward(h, st, g, keep=True)
    for name, (gr, acc) in (("side stream", (second, acc2)), ("after another scene", (third, acc3))):
        assert np.array_equal(_bits(acc), _bits(acc1)), f"LAST_ACC, {name}"
        for k in GRADS:
            if first[k] is None:
                assert gr[k] is None
            else:
                assert np.array_equal(_bits(gr[k]), _bits(first[k])), f"{k}, {name}"
    assert any(np.abs(first[k]).max() > 0 for k in GRADS if first[k] is not None)
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "0")
    default, _, _ = _backward(h, st, g)
    _within_band(first, default)


# ---- 3. the order is the specified one -------------------------------------------------------------------------------------------------
def test_order_is_the_specified_one_heavy_overdraw(monkeypatch):
    """test_gpu_parity.test_heavy_overdraw_and_ragged_image's scene: long segments, tail tiles, early termination, entries past wave_last"""
    s = make_scene(6000, 203, 117, sh_degree=2, mu_px=14.0, seed=33, kernel_size=0.0, require_coord=True, require_depth=True, pose="identity")
    got, ref, count = check_against_restatement(s, monkeypatch, seed=33)
    assert count.max() >= 16


def _whole_image_scene():
    """500 small Gaussians and one scaled to cover every one of the 13 x 8 tiles of a 203 x 117 image: a segment of 104 instances"""
    s = make_scene(501, 203, 117, sh_degree=1, mu_px=2.0, seed=7, kernel_size=0.0, require_coord=True, require_depth=True, pose="identity")
    m, sc, op = s.means3D.clone(), s.scales.clone(), s.opacities.clone()
    m[0] = torch.tensor([0.0, 0.0, float(s.means3D[:, 2].median())])
    sc[0] = 50.0
    op[0] = 0.3
    return s._replace(means3D=m, scales=sc, opacities=op)


def test_order_is_the_specified_one_segment_of_104(monkeypatch):
    s = _whole_image_scene()
    got, ref, count = check_against_restatement(s, monkeypatch, seed=7)
    assert count[0] == 104 and count[1:].max() < 104


# ---- 4. exact agreement with the atomic kernel where the order cannot matter -----------------------------------------------------------
def test_equals_the_atomic_kernel_where_order_cannot_matter(monkeypatch):
    """A Gaussian in at most two tiles has at most two partial records a, b: 0 + a + b is the same number in either order (fp32 addition is
    commutative), and the one-wave-per-tile atomic kernel computes a and b with the same instructions.  mu_px = 1.0 instead of the 3.0 of
    test 1's scene: at 3.0 only 16 % of the visible Gaussians touch at most two tiles (oracle's tiles_touched), at 1.0 60 %."""
    from gpu_util import HipRun
    monkeypatch.setenv("RADEGS_STREAMS", "0")
    monkeypatch.setenv("RADEGS_BWD_PPL", "4")
    s = _small_scene(True, True, mu_px=1.0)
    g = upstream_grads(s, 21)
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "0")
    h = HipRun(s, _dev())
    st = h.forward_native()
    _, atomic, _ = _backward(h, st, g, keep=True)
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    _, ordered, _ = _backward(h, st, g, keep=True)
    tt = h.export("tiles_touched", torch.int32, h.P)
    vis = st[8].cpu().numpy() > 0
    few = vis & (tt <= 2)
    share = few.sum() / max(int(vis.sum()), 1)
    print(f"{int(few.sum())} of {int(vis.sum())} visible Gaussians touch at most two tiles ({share:.3f})")
    assert share >= 0.5
    assert (ordered[few] != 0).any()
    same = (ordered[few] == atomic[few]).all(1)             # ==: -0 and +0 are the same number
    assert same.all(), f"{int((~same).sum())} records differ; first: Gaussian {np.nonzero(few)[0][np.argmin(same)]}"


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------------
def test_no_gaussians_and_all_culled(monkeypatch):
    from gpu_util import HipRun
    from test_oracle_kat import _single
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    s = _single(zs=[0.1], n=1)                              # behind the near plane: R == 0, the binning buffer is empty (NULL at the C ABI)
    h = HipRun(s, _dev())
    out = h.forward()
    got = h.backward(upstream_grads(s, 0))
    assert int((out[1] > 0).sum()) == 0
    for k, v in got.items():
        if v is not None:
            assert v.shape[0] == 1 and not v.any(), k
    got, _, count = check_against_restatement(s, monkeypatch)
    assert count.sum() == 0 and all(not v.any() for v in got.values() if v is not None)
    s0 = s._replace(means3D=torch.zeros(0, 3), shs=torch.zeros(0, 16, 3), rotations=torch.zeros(0, 4), scales=torch.zeros(0, 3),
                    opacities=torch.zeros(0, 1))            # P == 0: nothing is launched
    h = HipRun(s0, _dev())
    got, _, _ = _backward(h, h.forward_native(), upstream_grads(s0, 0))
    for k, v in got.items():
        assert v is None or v.size == 0, k


@pytest.mark.parametrize("n,zs", [(1, None), (2, [3.0, 4.0])])
def test_one_and_two_gaussians(n, zs, monkeypatch):
    """the sort runs over max(1, ceil(log2 P)) = 1 key bit"""
    from test_oracle_kat import _single
    s = _single(n=n, zs=zs)
    check_forward(s)
    got, ref, count = check_against_restatement(s, monkeypatch)
    assert (count > 0).all()
    _within_band(got, ref)


def test_image_narrower_than_one_tile(monkeypatch):
    s = make_scene(300, 12, 9, sh_degree=1, mu_px=2.0, seed=19, kernel_size=0.1, require_coord=True, require_depth=True, pose="random")
    check_forward(s)
    got, ref, count = check_against_restatement(s, monkeypatch, seed=19)
    assert count.max() == 1 and count.sum() > 10           # one tile: every visible Gaussian has exactly one partial record
    _within_band(got, ref)


def test_precomputed_colors_and_covariance(monkeypatch):
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    s = make_scene(2500, 160, 120, sh_degree=0, mu_px=2.5, seed=5, kernel_size=0.1, pose="random", require_coord=False, require_depth=True)
    cov, colors = cov3d_of(s), torch.rand(s.means3D.shape[0], 3, generator=torch.Generator().manual_seed(1))
    o, _ = check_forward(s, colors=colors, cov3D=cov)
    check_backward(s, o, colors=colors, cov3D=cov, seed=5)


def test_after_a_stream_forward(monkeypatch):
    """the ordered mode never replays entry streams: the tile-wide formulation is valid after either forward"""
    import diff_gaussian_rasterization._C as C
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    monkeypatch.setenv("RADEGS_STREAMS", "1")
    s = make_scene(6000, 203, 131, sh_degree=2, mu_px=2.0, seed=62, kernel_size=0.1, require_coord=False, require_depth=True, pose="random",
                   bg=(0.3, 0.1, 0.7))
    o, _ = check_forward(s)
    assert C.last_forward_used_streams() is True
    check_backward(s, o, seed=62)
    assert C.last_forward_used_streams() is True


# ---- 6. a training loop is reproducible ------------------------------------------------------------------------------------------------
def test_training_loop_is_reproducible():
    """tests/deterministic_train_worker.py twice, each a fresh process (the same history of forward calls), one after the other, never two at
    a time; the second only if the first succeeded"""
    worker = os.path.join(ROOT, "tests", "deterministic_train_worker.py")
    env = dict(os.environ, RADEGS_DETERMINISTIC="1")
    digests = []
    for run in range(2):
        r = subprocess.run([sys.executable, worker, "15"], env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, f"run {run}: exit {r.returncode}\n{r.stderr[-2000:]}"
        lines = [l for l in r.stdout.splitlines() if l.startswith("DIGEST ")]
        assert len(lines) == 1, r.stdout[-2000:]
        digests.append(lines[0].split()[1])
    assert digests[0] == digests[1], digests
