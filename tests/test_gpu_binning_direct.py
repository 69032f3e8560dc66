"""What the binning stage leaves behind, looked at directly and exactly (csrc/radegs_kernels.hip: emit_instances_kernel, tile_ranges_kernel;
csrc/rg_launch.inc: plan_attempt, queue_instances).

Per case (tests/binning_cases.py) and path: one HipRun.forward_native(), then the words the binning READ are exported (splat_a's pixel mean,
depth_key, tiles_touched; radii from the result), the stage is restated from them in integers (binning_cases.restate) and everything it
WROTE must equal the restatement: num_rendered, point_list, the range of every tile (the empty ones included), tile_keys_sorted in the layout
the plan rule prescribes (binning_cases.layout: R 16-bit words, or R 32-bit words under the key mask) and, where the plan gathers packed
rectangles, the rect word.  For the small cases the exported inputs also equal the fp32 oracle's per-Gaussian state, which pins the input as
well as the output.  Every comparison is integer equality.

The paths: tile-wide and entry streams (told apart by radegs_last_forward_used_streams), streams with the block mask in the key, a
speculative forward whose capacity exceeds R (tile_ranges_kernel reads the count on the device and its vector loads run past it), and a
speculative forward whose capacity is too small and is redone.  The capacity of a speculative forward decides where the binning buffer keeps
tile_keys_sorted, so these tests force the prediction (RADEGS_SPECULATE_HINT) to a value they know: the case's own R, or 1.

The grids of 255 / 256 tiles along one axis and of 65 535 / 65 536 / 65 792 tiles sit on both sides of the two plan switches no other test
crosses; their images are never copied to the host."""
import functools
import os
import time

import numpy as np
import pytest
import torch

import binning_cases as bc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EXACT = dict(RADEGS_SPECULATE="0")
PATHS = {
    "tile-wide": dict(EXACT, RADEGS_STREAMS="0"),
    "streams": dict(EXACT, RADEGS_STREAMS="1"),
    "streams-mask-in-key": dict(EXACT, RADEGS_STREAMS="1", RADEGS_MASK_IN_KEY="1"),
}
SWITCHES = ("RADEGS_STREAMS", "RADEGS_MASK_IN_KEY", "RADEGS_SPECULATE", "RADEGS_SPECULATE_HINT", "RADEGS_SPECULATE_CHUNKS", "RADEGS_PRIMS")
FORCED_REDO = [n for n in bc.SMALL if n == "coop_threshold"]      # R > 4097, the smallest capacity a speculative forward allocates


def _forward(s, env):
    """one forward with exactly these switches (every other binning switch unset); -> (HipRun, used_streams, seconds)"""
    from gpu_util import HipRun
    import diff_gaussian_rasterization._C as C
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        h = HipRun(s, DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.forward_native()
        torch.cuda.synchronize()
        return h, C.last_forward_used_streams(), time.perf_counter() - t0
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        C.reload_env()


def _export(h, name, numel, capacity=None):
    """a state array as uint32 words; capacity: the instance count the binning buffer was carved for (a speculative forward that fitted)"""
    if numel == 0:
        return np.zeros(0, np.uint32)
    R = int(h.state[0])
    if capacity is not None and name in ("point_list", "tile_keys_sorted"):      # arrays of `capacity` words: the first numel of them
        R, numel, keep = int(capacity), int(capacity), numel
    else:
        keep = numel
    t = h.C.debug_export(name, torch.int32, numel, h.P, R, h.s.W, h.s.H, h.s.require_coord, h.state[9], h.state[10], h.state[11])
    return t.cpu().numpy().view(np.uint32)[:keep]


@functools.lru_cache(maxsize=None)
def _oracle_inputs(name):
    """the fp32 oracle's per-Gaussian words for a small case: radii, pixel mean (bits), depth key, tiles_touched"""
    from util import oracle_for
    s = bc.scene(name)
    o = oracle_for(s)
    o.forward()
    P = s.means3D.shape[0]
    radii, m2, tt = o.get("radii").copy(), o.get("means2D", (P, 2)).copy(), o.get("tiles_touched").copy()
    key = np.where(radii > 0, o.get("depths").astype(np.float32).view(np.uint32), np.uint32(bc.INVISIBLE_KEY))
    o.close()
    return radii, m2, key, tt


def check(name, h, used_streams, streams, mask_in_key=False, capacity=None):
    """everything the binning of forward `h` wrote against the restatement of what it read"""
    c = bc.CASES[name]
    s, P, R = h.s, h.P, int(h.state[0])
    lay = bc.layout(c.gx, c.gy, streams=streams, mask_in_key=mask_in_key)
    assert used_streams is streams, f"the forward ran {'entry streams' if used_streams else 'tile-wide'}"
    # ---- what the stage read
    radii = h.state[8].cpu().numpy()
    splat_a = _export(h, "splat_a", 16 * P).view(np.float32).reshape(P, 16)
    depth_key, tiles_touched = _export(h, "depth_key", P), _export(h, "tiles_touched", P)
    vis = tiles_touched > 0
    assert np.array_equal(radii > 0, vis) and (depth_key[~vis] == bc.INVISIBLE_KEY).all()
    if c.small:
        o_radii, o_m2, o_key, o_tt = _oracle_inputs(name)
        assert np.array_equal(radii, o_radii) and np.array_equal(tiles_touched, o_tt) and np.array_equal(depth_key, o_key)
        assert np.array_equal(splat_a[vis, 0:2].view(np.uint32), o_m2[vis].view(np.uint32)), "pixel means differ from the oracle's"
    b = bc.restate(radii, splat_a[:, 0], splat_a[:, 1], depth_key, tiles_touched, c.gx, c.gy)
    assert np.array_equal(b.rect_tiles.astype(np.uint32), tiles_touched), "tiles_touched is not the area of the restated rectangle"
    reached = c.reaches(b, depth_key)
    assert all(reached.values()), [k for k, v in reached.items() if not v]
    # ---- what it wrote
    assert R == b.num_rendered, (R, b.num_rendered)
    if lay.rect:
        assert np.array_equal(_export(h, "rect", P), bc.packed_rect(b)), "packed rectangles"
    point_list = _export(h, "point_list", R, capacity)
    if streams and not lay.mask_in_key:
        point_list = point_list & np.uint32(bc.GID_MASK)           # the block-mask byte belongs to the stream-list tests
    bad = np.flatnonzero(point_list != b.point_list.astype(np.uint32))
    assert not len(bad), f"point_list: {len(bad)} of {R} entries differ, first at {bad[:5]}: {point_list[bad[:5]]} for {b.point_list[bad[:5]]}"
    ranges = _export(h, "ranges", 2 * c.gx * c.gy).reshape(-1, 2)
    bad = np.flatnonzero((ranges != b.ranges).any(1))
    assert not len(bad), f"ranges: {len(bad)} tiles differ, first {bad[:5]}: {ranges[bad[:5]].tolist()} for {b.ranges[bad[:5]].tolist()}"
    words = _export(h, "tile_keys_sorted", R, capacity)
    if lay.key16:
        keys, want = words.view(np.uint16)[:R], b.keys16
    else:
        keys, want = (words & np.uint32(bc.GID_MASK)) if lay.mask_in_key else words, b.keys32
    bad = np.flatnonzero(keys != want)
    assert not len(bad), (f"tile_keys_sorted as {16 if lay.key16 else 32}-bit words: {len(bad)} of {R} differ, first at {bad[:5]}: "
                          f"{keys[bad[:5]]} for {want[bad[:5]]}")
    return b, lay


def _path_params(names):
    return [(n, p) for n in names for p in PATHS]


@pytest.mark.parametrize("name,path", _path_params(bc.SMALL), ids=lambda v: v)
def test_small_case(name, path):
    env = PATHS[path]
    h, used, _ = _forward(bc.scene(name), env)
    check(name, h, used, streams=env["RADEGS_STREAMS"] == "1", mask_in_key="RADEGS_MASK_IN_KEY" in env)


@pytest.mark.parametrize("name,path", [(n, p) for n in bc.LARGE for p in ("tile-wide", "streams")], ids=lambda v: v)
def test_large_grid(name, path):
    env = PATHS[path]
    h, used, seconds = _forward(bc.scene(name), env)
    _, lay = check(name, h, used, streams=env["RADEGS_STREAMS"] == "1")
    c = bc.CASES[name]
    print(f"{name} {path}: {c.gx * c.gy} tiles, rect {lay.rect}, key16 {lay.key16}, {lay.tile_bits} tile bits, forward {seconds * 1e3:.1f} ms wall")
    assert lay.rect == (max(c.gx, c.gy) <= 255) and lay.key16 == (c.gx * c.gy <= 65535)


@pytest.mark.parametrize("streams", ["0", "1"], ids=["tile-wide", "streams"])
@pytest.mark.parametrize("name", bc.SMALL)
def test_small_case_speculative_capacity_above_R(name, streams):
    """A second forward of the view whose capacity (R + R / 4 + 4096) exceeds R: the binning kernels are launched for the capacity and read
    the count on the device; tile_ranges_kernel's vector loads run past L up to the capacity."""
    import diff_gaussian_rasterization._C as C
    s = bc.scene(name)
    first, _, _ = _forward(s, dict(EXACT, RADEGS_STREAMS=streams))          # also lets the (device, W, H) learn a depth beyond the 3-pass window
    R = int(first.state[0])
    C.binning_stats(reset=True)
    cap = R + R // 4 + bc.SPEC_SLACK
    # (entry-stream storage that cannot overflow, stream_chunk_capacity_safe: what other views of this size needed does not decide this test)
    chunks = 8 * ((cap >> 4) + bc.CASES[name].gx * bc.CASES[name].gy + 1)
    h, used, _ = _forward(s, dict(RADEGS_STREAMS=streams, RADEGS_SPECULATE="1", RADEGS_SPECULATE_HINT=str(R), RADEGS_SPECULATE_CHUNKS=str(chunks)))
    assert C.binning_stats(reset=True) == (1, 0)
    check(name, h, used, streams=streams == "1", capacity=cap)


@pytest.mark.parametrize("streams", ["0", "1"], ids=["tile-wide", "streams"])
@pytest.mark.parametrize("name", FORCED_REDO)
def test_small_case_speculative_capacity_too_small_is_redone(name, streams):
    """predicted 1 instance -> capacity 4097 < R: instances are dropped on the device, the host sees the count and redoes the binning exactly"""
    import diff_gaussian_rasterization._C as C
    C.binning_stats(reset=True)
    h, used, _ = _forward(bc.scene(name), dict(RADEGS_STREAMS=streams, RADEGS_SPECULATE="1", RADEGS_SPECULATE_HINT="1"))
    assert C.binning_stats(reset=True) == (1, 1)
    assert int(h.state[0]) > 1 + bc.SPEC_SLACK
    check(name, h, used, streams=streams == "1")


def test_ties_beyond_the_three_pass_window_are_redone_with_four_passes():
    """`ties` at an image size no other test uses (47 x 31: the same 3 x 2 tiles), so this (device, W, H) has not yet learnt that its
    depths leave the three-pass sort's window: the speculative forward runs three passes, sees the flag and is redone with four."""
    import diff_gaussian_rasterization._C as C
    s = bc.ties(47, 31)
    C.binning_stats(reset=True)
    h, used, _ = _forward(s, dict(RADEGS_STREAMS="0", RADEGS_SPECULATE="1", RADEGS_SPECULATE_HINT="200"))
    assert C.binning_stats(reset=True) == (1, 1)
    radii = h.state[8].cpu().numpy()
    P = h.P
    splat_a = _export(h, "splat_a", 16 * P).view(np.float32).reshape(P, 16)
    key, tt = _export(h, "depth_key", P), _export(h, "tiles_touched", P)
    b = bc.restate(radii, splat_a[:, 0], splat_a[:, 1], key, tt, 3, 2)
    assert all(bc.ties_reaches(b, key).values())
    assert int(h.state[0]) == 200 and np.array_equal(_export(h, "point_list", 200), b.point_list.astype(np.uint32))
    assert np.array_equal(_export(h, "ranges", 12).reshape(-1, 2), b.ranges)
    again, _, _ = _forward(s, dict(RADEGS_STREAMS="0", RADEGS_SPECULATE="1", RADEGS_SPECULATE_HINT="200"))
    assert C.binning_stats(reset=True) == (1, 0)               # remembered: four passes straight away
    assert np.array_equal(_export(again, "point_list", 200, capacity=200 + 50 + bc.SPEC_SLACK), b.point_list.astype(np.uint32))
