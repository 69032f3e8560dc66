"""What the sub-tile entry-stream stage produces, looked at directly (csrc/rg_streams.inc, csrc/rg_blend.h).

A  the DEVICE build of rg_blend.h's decision pieces (csrc/radegs_blend_check.hip -> libradegs_blend_check.so, built by rade-gs_amd/build.py
   with the product's flags): ellipse_block_mask and the emission's per-rectangle pattern with the approximate sqrt / rcp against the
   brute-force truth (the kernels' per-pixel rule at all 32 pixel centres of every block), exp_spec / exp_spec_floor / splat_power bit for
   bit against their np.float32 restatements, skip_threshold with the device's logf still conservative.
B  the lists a stream forward leaves in the image state (radegs_debug_export), exactly: stream_lists.check_stream_state.
C  the contribution words, blk_consumed and both planes of n_contrib against a float32 replay of every pixel: stream_lists.check_contributions.

The checker itself is proven on a host stand-in with nine corruptions by tests/test_stream_lists_standin.py, which also pins the numpy
restatements used here to the host build of the header (this machine needs no compiler)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stream_lists as sl
from test_block_masks import EDGE_MASKS, EDGE_RECORDS, EMISSION_RECT, EMISSION_SETS, FAMILIES, _conics, _emission_set, _family

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(HERE), "rade-gs_amd", "diff_gaussian_rasterization", "libradegs_blend_check.so")
DEV = "cuda:0"
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        assert os.path.exists(LIB_PATH), LIB_PATH + " is missing: build it with `python rade-gs_amd/build.py`"
        L = ctypes.CDLL(LIB_PATH)
        vp, ci, cf, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint32
        for name, args in (("block_masks", [ci, vp, cf, cf, vp, vp]), ("block_masks_rect", [ci, vp, vp, vp, vp, vp, vp]),
                           ("exp_spec_bits", [u32, u32, u32, vp, vp, vp]), ("skip_thresholds", [ci, vp, vp, vp]),
                           ("splat_powers", [ci, vp, vp, vp, vp, vp, vp, vp]), ("truth_masks", [ci, vp, ci, vp, vp, vp, vp, vp])):
            f = getattr(L, "blendcheck_" + name)
            f.restype, f.argtypes = ci, args
        _LIB = L
    return _LIB


def _up(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view({np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))).to(DEV)


def _out(n, dtype=torch.int32):
    return torch.full((max(int(n), 1),), -1, dtype=dtype, device=DEV)   # (-1: an element a kernel leaves unwritten shows)


def _call(name, *args):
    rc = getattr(_lib(), "blendcheck_" + name)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (name, rc)


def _u32(t, n):
    torch.cuda.synchronize()
    return t.cpu().numpy()[:n].view(np.uint32)


def dev_skip_thresholds(op):
    op_d, thr = _up(op, np.float32), _out(len(op), torch.float32)
    _call("skip_thresholds", len(op), op_d.data_ptr(), thr.data_ptr())
    torch.cuda.synchronize()
    return thr.cpu().numpy()[:len(op)]


def dev_block_masks(rec_thr, tx0, ty0):
    rec, mask = _up(rec_thr, np.float32), _out(len(rec_thr))
    _call("block_masks", len(rec_thr), rec.data_ptr(), float(tx0), float(ty0), mask.data_ptr())
    return _u32(mask, len(rec_thr))


def dev_block_masks_rect(rec_thr, rect):
    rect = np.ascontiguousarray(rect, np.int32)
    cnt = ((rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])).astype(np.int64)
    off = (np.cumsum(cnt) - cnt).astype(np.uint32)
    total = int(cnt.sum())
    rec, rect_d, off_d, mask, txy = _up(rec_thr, np.float32), _up(rect, np.int32), _up(off, np.uint32), _out(total), _out(total)
    _call("block_masks_rect", len(rec_thr), rec.data_ptr(), rect_d.data_ptr(), off_d.data_ptr(), mask.data_ptr(), txy.data_ptr())
    return _u32(mask, total), _u32(txy, total), cnt


def dev_truth(rec, gid, ox, oy):
    """stream_lists' truth_fn: records of rec.shape[1] floats (words 0..5 = mx, my, cx, cy, cz, op), pair i = record gid[i] (i when None)"""
    rec = np.ascontiguousarray(rec, np.float32)
    n = len(ox)
    assert len(oy) == n and (len(rec) >= n if gid is None else (len(gid) == n and (n == 0 or int(np.max(gid)) < len(rec)))), "pairs outside the records"
    rec_d, ox_d, oy_d, out = _up(rec, np.float32), _up(ox, np.float32), _up(oy, np.float32), _out(n)
    gid_d = None if gid is None else _up(np.asarray(gid).astype(np.uint32), np.uint32)
    _call("truth_masks", n, rec_d.data_ptr(), rec.shape[1], None if gid_d is None else gid_d.data_ptr(), ox_d.data_ptr(), oy_d.data_ptr(), out.data_ptr())
    return _u32(out, n)


def _host_compiled(fn, *args):
    """the host-compiled answer, for the report only, where this machine has the library"""
    try:
        from hostcheck import hostcheck as hc
        return getattr(hc, fn)(*args)
    except Exception:      # no compiler and no library here
        return None


# =================================================================================== A. the device's decision pieces
def _with_device_thr(mx, my, cx, cy, cz, op):
    return np.stack([mx, my, cx, cy, cz, dev_skip_thresholds(op)], 1).astype(np.float32), np.stack([mx, my, cx, cy, cz, op], 1).astype(np.float32)


@pytest.mark.parametrize("name", list(FAMILIES))
def test_device_block_mask_never_drops_a_reachable_block(name):
    mx, my, cx, cy, cz, op, tx0, ty0 = _family(name)
    rec_thr, rec_op = _with_device_thr(mx, my, cx, cy, cz, op)
    mask = dev_block_masks(rec_thr, tx0, ty0)
    truth = dev_truth(rec_op, None, np.full(len(mx), tx0, np.float32), np.full(len(mx), ty0, np.float32))
    kept, needed = sl.popcount(mask), sl.popcount(truth)
    host = _host_compiled("block_masks", rec_op, tx0, ty0)
    differ = "host library absent" if host is None else f"{int((host[0] != mask).sum())} of {len(mask)} records differ from the host-compiled mask"
    print(f"{name}: device blocks kept {kept}, reachable {needed}, ratio {kept / max(needed, 1):.4f}; {differ}")
    assert needed > 10000 and not (mask >> 8).any()
    missed = truth & ~mask
    assert not missed.any(), (name, int((missed != 0).sum()), rec_op[missed != 0][:5], mask[missed != 0][:5], truth[missed != 0][:5])
    if name in ("small", "large"):
        assert kept <= 1.25 * needed + 100


def test_device_block_mask_edge_cases():
    rec_thr, rec_op = _with_device_thr(*EDGE_RECORDS.T)
    mask = dev_block_masks(rec_thr, 0.0, 0.0)
    truth = dev_truth(rec_op, None, np.zeros(6, np.float32), np.zeros(6, np.float32))
    print("edge cases: device masks", list(mask), "truth", list(truth), "host-compiled", EDGE_MASKS)
    assert not (truth & ~mask).any()
    assert list(mask[:4]) == EDGE_MASKS[:4]     # thr > 0 and the irregular conics are decided by compares alone: no approximate arithmetic
    assert int(truth[5]) == 1 and int(truth[0]) == 0 and int(truth[4]) == 0


def _rect_truth(rec_op, rect, cnt, txy):
    g = np.repeat(np.arange(len(cnt)), cnt)
    tx, ty = (txy & 0xFFFF).astype(np.int64), (txy >> 16).astype(np.int64)
    return dev_truth(rec_op, g, ((rect[g, 0] + tx) * 16).astype(np.float32), ((rect[g, 1] + ty) * 16).astype(np.float32)), g


def _row_major(rect, cnt, txy):
    local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    w = np.repeat(rect[:, 2] - rect[:, 0], cnt).astype(np.int64)
    bad = np.flatnonzero(((txy & 0xFFFF) != local % w) | ((txy >> 16) != local // w))
    assert not len(bad), (f"{len(bad)} positions land in another tile; first: position {local[bad[0]]} of a rectangle {w[bad[0]]} wide -> "
                          f"tile ({txy[bad[0]] & 0xFFFF}, {txy[bad[0]] >> 16})")


@pytest.mark.parametrize("sig_lo,sig_hi,aspect_hi", EMISSION_SETS)
def test_device_masks_as_the_emission_asks(sig_lo, sig_hi, aspect_hi):
    rec_thr, rec_op = _with_device_thr(*_emission_set(sig_lo, sig_hi, aspect_hi))
    rect = np.tile(np.array(EMISSION_RECT, np.int32), (len(rec_thr), 1))
    mask, txy, cnt = dev_block_masks_rect(rec_thr, rect)
    _row_major(rect, cnt, txy)
    truth, _ = _rect_truth(rec_op, rect, cnt, txy)
    kept, needed = sl.popcount(mask), sl.popcount(truth)
    print(f"emission pattern ({sig_lo}, {sig_hi}, {aspect_hi}): device blocks kept {kept}, reachable {needed}")
    assert needed > 10000 and not (mask >> 8).any() and not (truth & ~mask).any(), int(((truth & ~mask) != 0).sum())
    assert kept <= 1.3 * needed + 100       # the CPU test's bound for this pattern


def test_device_masks_over_rectangles_that_stress_the_tile_recovery():
    """local -> (tx, ty) through the approximate reciprocal and one correction step: widths 1, 3, 7, 16, 17, 255, heights up to 255 (65 025 tiles)"""
    rng = np.random.default_rng(23)
    shapes = [(w, h) for w in (1, 3, 7, 16, 17, 255) for h in (1, 2, 37, 255)]
    per = 12
    rect = np.array([[0, 0, w, h] for w, h in shapes for _ in range(per)], np.int32)
    n = len(rect)
    cx, cy, cz = _conics(n, rng, 3.0, 400.0, 30.0, 0.3)
    mx = (rng.uniform(-0.05, 1.05, n) * rect[:, 2] * 16).astype(np.float32)
    my = (rng.uniform(-0.05, 1.05, n) * rect[:, 3] * 16).astype(np.float32)
    op = np.exp(rng.uniform(np.log(1.0 / 300.0), 0.0, n)).astype(np.float32)
    rec_thr, rec_op = _with_device_thr(mx, my, cx, cy, cz, op)
    mask, txy, cnt = dev_block_masks_rect(rec_thr, rect)
    assert int(cnt.max()) == 65025
    _row_major(rect, cnt, txy)
    truth, _ = _rect_truth(rec_op, rect, cnt, txy)
    print(f"rectangles: {n} splats, {int(cnt.sum())} tiles, device blocks kept {sl.popcount(mask)}, reachable {sl.popcount(truth)}")
    assert sl.popcount(truth) > 10000 and not (mask >> 8).any() and not (truth & ~mask).any(), int(((truth & ~mask) != 0).sum())


def _bits_of(v):
    return int(np.float32(v).view(np.uint32))


@pytest.mark.parametrize("first,last,stride", [(0x80000000, _bits_of(-87.0), 97), (0, _bits_of(16.0), 97), (_bits_of(-88.5) - 4096, _bits_of(-88.5), 1)],
                         ids=["minus87_to_minus0", "plus0_to_16", "below_minus88.5"])
def test_device_exp_spec_bits(first, last, stride):
    count = (last - first) // stride + 1
    a, b = _out(count), _out(count)
    _call("exp_spec_bits", first, count, stride, a.data_ptr(), b.data_ptr())
    spec, floor = _u32(a, count), _u32(b, count)
    x = (first + stride * np.arange(count, dtype=np.uint64)).astype(np.uint32).view(np.float32)
    want_floor = sl.exp_spec_floor32(x).view(np.uint32)
    want_spec = np.where(x < np.float32(-87.0), np.uint32(0), want_floor)      # exp_spec: 0 below -87, else the same polynomial and scaling
    assert np.array_equal(spec, want_spec), (int((spec != want_spec).sum()), x[spec != want_spec][:5])
    assert np.array_equal(floor, want_floor), (int((floor != want_floor).sum()), x[floor != want_floor][:5])
    if stride == 1:     # below -87: 0, and the floor form's exp_spec(-87)
        assert not spec.any() and (floor == sl.exp_spec32(np.array([-87.0], np.float32)).view(np.uint32)[0]).all()


def test_device_splat_power_bits():
    rng = np.random.default_rng(0)      # the 5000 tuples of test_decision_chain_pieces_bit_exact
    t = np.array([rng.normal(size=5) * [1, .5, 1, 8, 8] for _ in range(5000)]).astype(np.float32)
    cols = [_up(t[:, k], np.float32) for k in range(5)]
    out = _out(5000, torch.float32)
    _call("splat_powers", 5000, *[c.data_ptr() for c in cols], out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()[:5000]
    cx, cy, cz, dx, dy = t.T
    ref = np.float32(-0.5) * ((cx * dx) * dx + (cz * dy) * dy) - (cy * dx) * dy      # np.float32: one rounding per operation, source order
    assert ref.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_device_skip_threshold_is_conservative():
    rng = np.random.default_rng(11)
    op = np.concatenate([np.exp(rng.uniform(np.log(1e-3), 0.0, 100000)), [1e-3, 0.02, 0.3, 0.9, 1.0, 7.0]]).astype(np.float32)
    thr = dev_skip_thresholds(op)
    host = sl.skip_threshold32(op)      # within 1e-6 of the host build's (tests/test_stream_lists_standin.py)
    print(f"skip_threshold: max |device - host| = {np.abs(thr.astype(np.float64) - host).max():.3e}")
    for eps in (0.0, 1e-6, 1e-4, 1e-2, 1.0):
        alpha = np.fmin(np.float32(0.99), op * sl.exp_spec32(thr - np.float32(eps)))
        assert (alpha < np.float32(1.0) / np.float32(255.0)).all(), (eps, op[~(alpha < np.float32(1.0) / np.float32(255.0))][:5])
    assert np.abs(thr.astype(np.float64) - host).max() <= 1e-5


# =================================================================================== B, C. the lists and the contribution words
_STATES = {}


def _forward(s, env):
    from gpu_util import HipRun
    import diff_gaussian_rasterization._C as C
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h = HipRun(s, DEV)
        h.forward_native()
        torch.cuda.synchronize()
        return h, sl.export_state(h, mask_in_key="RADEGS_MASK_IN_KEY" in env)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        C.reload_env()


def _state(name):
    if name not in _STATES:
        _STATES[name] = _forward(sl.scenario_scene(name), dict(sl.SCENARIOS[name]["env"], RADEGS_STREAMS="1"))[1]
    return _STATES[name]


@pytest.mark.parametrize("name", list(sl.SCENARIOS))
def test_lists(name):
    st = _state(name)
    fig = sl.check_stream_state(st, dev_truth, tight=sl.SCENARIOS[name]["tight"])
    sl.check_scenario_property(name, st)
    print(f"{name}: kept {fig['kept']} reachable {fig['reachable']} ratio {fig['ratio']:.3f} instances {fig['instances']} list entries {fig['entries']}")


@pytest.mark.parametrize("name", [k for k, v in sl.SCENARIOS.items() if "C" in v["parts"]])
def test_contributions(name):
    st = _state(name)
    fig = sl.check_contributions(st)
    sl.check_scenario_property(name, st)
    print(f"{name}: {fig['history_words']} history words, longest list {fig['max_list']}, blocks that stopped early {fig['stopped_early']}")


def test_two_layouts_of_one_scene_give_the_same_lists():
    for a, b in zip(sl.list_contents(_state("ragged")), sl.list_contents(_state("ragged-mask-in-key"))):
        assert np.array_equal(a, b)


def test_lists_after_an_overflow_redo():
    """the sequence of test_entry_stream_storage_is_sized_from_the_previous_view_and_an_overflow_is_redone, on the first scene"""
    import diff_gaussian_rasterization._C as C
    s = sl.scenario_scene("ragged")
    env = dict(RADEGS_STREAMS="1", RADEGS_SPECULATE="1")
    C.binning_stats(reset=True)
    for _ in range(3):                                   # seed the (device, W, H) history
        _forward(s, env)
    _, misses0 = C.binning_stats(reset=True)
    assert misses0 == 0, misses0
    _, st = _forward(s, dict(env, RADEGS_SPECULATE_CHUNKS="40"))
    calls, misses = C.binning_stats(reset=True)
    assert (calls, misses) == (1, 1), (calls, misses)    # storage for 40 chunks: the forward was redone
    assert int(st.stream_meta[1]) > 40
    sl.check_stream_state(st, dev_truth, tight=True)
    sl.check_contributions(st)
    for a, b in zip(sl.list_contents(st), sl.list_contents(_state("ragged"))):
        assert np.array_equal(a, b)


def test_first_three_scenes_with_poisoned_buffers():
    """RADEGS_DEBUG_POISON=1 (tests/test_gpu_poison.py): a word the stage leaves unwritten reads as 0xFF.  A fresh child, a timeout, no retry."""
    env = dict(os.environ, RADEGS_DEBUG_POISON="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "ragged and (test_lists or test_contributions)"], env=env, cwd=os.path.dirname(HERE), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "6 passed" in r.stdout, r.stdout[-500:]
