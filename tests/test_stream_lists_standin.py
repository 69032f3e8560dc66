"""The checker of tests/stream_lists.py, proven without a GPU.  A host stand-in produces, for every scenario of the GPU file, the arrays a
stream forward leaves behind: the oracle's point_list / ranges / n_contrib, the product's host-compiled preprocess records and block masks
(hostcheck, in the emission's call pattern), a numpy list builder and the numpy replay.  check_stream_state and check_contributions must
pass on it -- which pins the replay to the oracle: both planes of n_contrib come out of the contribution words -- and must fail, naming
the array, the tile and the block, on each of nine single corruptions.  The same run confirms on the host arithmetic that every scenario
has the property it is in the table for and that the ordinary-splat scenes stay inside kept <= 1.25 x reachable + 100.

Also here, because the GPU machine has no compiler: the numpy restatements the GPU file relies on (exp_spec32 / fma32, skip_threshold32) against
the host build of csrc/rg_blend.h, and hostcheck's truth / rectangle helpers against the functions test_block_masks.py already proves."""
import numpy as np
import pytest

import stream_lists as sl
from hostcheck import hostcheck as hc
from test_block_masks import EMISSION_RECT, EMISSION_SETS, _emission_set, _family
from util import oracle_for

_CACHE = {}


def standin(name):
    """-> (StreamState of the stand-in, its replay, its flat lists (blk, gid, pos)); built once per scenario and never modified (tests copy it)"""
    if name in _CACHE:
        return _CACHE[name]
    s = sl.scenario_scene(name)
    P = s.means3D.shape[0]
    o = oracle_for(s)
    R = o.forward()
    f, _ = hc.preprocess_fwd(s)
    tiles_touched = o.get("tiles_touched").astype(np.uint32)
    vis = np.flatnonzero(tiles_touched > 0)
    splat_a = np.zeros((P, 16), np.float32)
    splat_a[vis, 0:6] = f[vis, 0:6]
    splat_a[vis, 6] = hc.skip_threshold_vec(f[vis, 5])
    rect = np.zeros(P, np.uint32)
    rect[vis] = np.ascontiguousarray(f[vis, 25]).view(np.uint32)
    W, H = s.W, s.H
    gx, gy = (W + 15) // 16, (H + 15) // 16
    tiles = gx * gy
    st = sl.StreamState(W=W, H=H, ranges=o.get("ranges").astype(np.uint32).reshape(tiles, 2), point_list=o.get("point_list").astype(np.uint32)[:R],
                        splat_a=splat_a, rect=rect, tiles_touched=tiles_touched, blk_count=None, blk_base=None, blk_order=None, blk_consumed=None,
                        stream_meta=None, blk_chunks=None, tile_keys_sorted=None, n_contrib=o.get("n_contrib").astype(np.uint32).reshape(2, H, W),
                        used_streams=True)
    # the block mask of every instance: the host ellipse_* functions asked per splat for its rectangle, looked up at the instance's tile
    x0, y0, x1, y1 = sl.unpack_rect(rect[vis])
    masks, off = hc.masks_rect_each(splat_a[vis], np.stack([x0, y0, x1, y1], 1))
    row_of = np.full(P, -1, np.int64)
    row_of[vis] = np.arange(len(vis))
    it = sl.instance_tiles(st)
    g = row_of[st.point_list]
    assert (g >= 0).all()
    local = (it // gx - y0[g]) * (x1 - x0)[g] + (it % gx - x0[g])
    inst_mask = masks[off[g].astype(np.int64) + local]
    # numpy list builder: block b of a tile gets the tile's entries whose mask has bit b, in list order
    r0 = st.ranges[:, 0].astype(np.int64)
    blk, gid, pos = [], [], []
    for b in range(8):
        sel = np.flatnonzero((inst_mask >> b) & 1)
        blk.append(it[sel] * 8 + b)
        gid.append(st.point_list[sel].astype(np.int64))
        pos.append(sel - r0[it[sel]])
    blk, gid, pos = np.concatenate(blk), np.concatenate(gid), np.concatenate(pos)
    o_ = np.lexsort((pos, blk))
    install(st, blk[o_], gid[o_], pos[o_])
    if _mask_in_key(name):
        st.tile_keys_sorted = (it | (inst_mask.astype(np.int64) << 24)).astype(np.uint32)
    rep = sl.replay(st)
    sl.write_contributions(st, rep)
    _CACHE[name] = (st, rep, (blk[o_], gid[o_], pos[o_]))
    return _CACHE[name]


def _mask_in_key(name):
    return "RADEGS_MASK_IN_KEY" in sl.SCENARIOS[name]["env"]


def install(st, blk, gid, pos):
    nb = 8 * st.tiles
    st.blk_count, st.blk_base, st.blk_chunks = sl.layout(nb, blk, gid, pos)
    st.blk_order = sl.expected_order(st.blk_count).astype(np.uint32)
    st.stream_meta = np.array([sl.TAG, st.blk_chunks.shape[0], 0, 0], np.uint32)
    st.blk_consumed = np.zeros(nb, np.uint32)


def host_truth(splat_a, gid, ox, oy):
    return hc.truth_masks(splat_a, gid, ox, oy)


@pytest.mark.parametrize("name", list(sl.SCENARIOS))
def test_standin_passes_and_has_the_scenario_property(name):
    st, rep, _ = standin(name)
    sc = sl.SCENARIOS[name]
    fig = sl.check_stream_state(st.copy(), host_truth, tight=sc["tight"])
    figc = sl.check_contributions(st.copy(), rep)       # n_contrib is the oracle's: the replay reproduces both of its planes
    sl.check_scenario_property(name, st)
    print(f"{name}: kept {fig['kept']} reachable {fig['reachable']} ratio {fig['ratio']:.3f} instances {fig['instances']} longest list {figc['max_list']} "
          f"blocks stopped early {figc['stopped_early']}")


def test_two_layouts_of_one_scene_agree():
    a, b = standin("ragged")[0], standin("ragged-mask-in-key")[0]
    for x, y in zip(sl.list_contents(a), sl.list_contents(b)):
        assert np.array_equal(x, y)


def _pick(st, lists, want):
    """index (into the flat lists) of an entry in the middle of a list of at least 3 entries for which want(k) holds"""
    blk = lists[0]
    cnt = st.blk_count.astype(np.int64)
    for k in range(1, len(blk) - 1):
        if blk[k - 1] == blk[k] == blk[k + 1] and cnt[blk[k]] >= 3 and want(k):
            return k
    raise AssertionError("no such entry")


def _corrupt(kind):
    """-> (corrupted StreamState, 'B' or 'C': the part that must notice, the array it must name, tile, block)"""
    base_st, rep, (blk, gid, pos) = standin("ragged")
    st = base_st.copy()
    it = sl.instance_tiles(st)
    r0 = st.ranges[:, 0].astype(np.int64)
    truth = host_truth(st.splat_a, st.point_list, ((it % st.gx) * 16).astype(np.float32), ((it // st.gx) * 16).astype(np.float32))
    reaches = lambda k: bool((truth[r0[blk[k] // 8] + pos[k]] >> (blk[k] % 8)) & 1)   # noqa: E731
    if kind == "drop one entry":
        k = _pick(st, (blk, gid, pos), reaches)
        install(st, np.delete(blk, k), np.delete(gid, k), np.delete(pos, k))
        return st, "B", "blk_chunks", blk[k] // 8, blk[k] % 8
    if kind == "swap two entries":
        k = _pick(st, (blk, gid, pos), lambda k: True)
        g2, p2 = gid.copy(), pos.copy()
        g2[[k, k + 1]], p2[[k, k + 1]] = gid[[k + 1, k]], pos[[k + 1, k]]
        install(st, blk, g2, p2)
        return st, "B", "blk_chunks", blk[k] // 8, blk[k] % 8
    if kind == "pos off by one":
        n_tile = st.ranges[:, 1].astype(np.int64) - r0
        k = _pick(st, (blk, gid, pos), lambda k: pos[k] + 1 < n_tile[blk[k] // 8])
        p2 = pos.copy()
        p2[k] += 1
        install(st, blk, gid, p2)
        return st, "B", "blk_chunks", blk[k] // 8, blk[k] % 8
    if kind == "entry in a block it cannot reach":
        for k in range(len(blk)):   # a splat that reaches one block of its tile only, copied into the opposite block
            inst = r0[blk[k] // 8] + pos[k]
            far = blk[k] // 8 * 8 + (7 - blk[k] % 8)
            if truth[inst] == (1 << (blk[k] % 8)) and not ((blk == far) & (pos == pos[k])).any() and \
                    sl.cannot_reach(st, gid[k:k + 1], blk[k:k + 1] // 8, np.array([7 - blk[k] % 8]))[0]:
                break
        else:
            raise AssertionError("no such entry")
        b2, g2, p2 = np.append(blk, far), np.append(gid, gid[k]), np.append(pos, pos[k])
        o_ = np.lexsort((p2, b2))
        install(st, b2[o_], g2[o_], p2[o_])
        return st, "B", "blk_chunks", far // 8, far % 8
    if kind == "overlapping chunk ranges":
        k = int(np.flatnonzero((st.blk_count.reshape(-1, 8)[:, :2] > 0).all(1))[0]) * 8   # blocks 0 and 1 of that tile both have lists
        st.blk_base[k + 1] = st.blk_base[k]
        return st, "B", "blk_base", k // 8, 1
    if kind == "one group of blk_order reversed":
        st.blk_order[:512] = st.blk_order[:512][::-1].copy()
        return st, "B", "blk_order", st.blk_order[0] // 8, st.blk_order[0] % 8
    if kind == "an id twice in blk_order":
        k = min(int(st.blk_order[5]), int(st.blk_order[4]))    # the lower of the id that is lost and the id that is there twice is named
        st.blk_order[5] = st.blk_order[4]
        return st, "B", "blk_order", k // 8, k % 8
    n_eff = rep[1]
    if kind == "one history bit flipped":
        k = int(np.flatnonzero(n_eff > 20)[0])
        st.blk_chunks[int(st.blk_base[k]) + 1, 32 + 9] ^= np.uint32(1 << 2)
        return st, "C", "blk_chunks", k // 8, k % 8
    if kind == "blk_consumed rounded down by 16":
        k = int(np.flatnonzero(n_eff > 20)[0])
        st.blk_consumed[k] -= 16
        return st, "C", "blk_consumed", k // 8, k % 8
    raise KeyError(kind)


CORRUPTIONS = ["drop one entry", "swap two entries", "pos off by one", "entry in a block it cannot reach", "overlapping chunk ranges",
               "one group of blk_order reversed", "an id twice in blk_order", "one history bit flipped", "blk_consumed rounded down by 16"]


@pytest.mark.parametrize("kind", CORRUPTIONS)
def test_every_corruption_is_noticed(kind):
    st, part, array, tile, blk = _corrupt(kind)
    with pytest.raises(AssertionError) as e:
        if part == "B":
            sl.check_stream_state(st, host_truth, tight=True)
        else:
            sl.check_stream_state(st.copy(), host_truth, tight=True)   # part B does not look at these words ...
            sl.check_contributions(st)                               # ... part C does
    msg = str(e.value)
    print(kind, "->", msg)
    assert msg.startswith(f"{array}: tile {int(tile)} block {int(blk)}:"), msg


# ---- the numpy restatements and the new hostcheck helpers ------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_numpy_exp_spec_is_the_host_builds():
    """every 97th bit pattern of [-87, -0] and [+0, 16] (the sweep of hc_exp_spec_sweep), the 4096 patterns below -88.5, the specials"""
    u = lambda v: int(np.float32(v).view(np.uint32))   # noqa: E731
    pats = np.concatenate([np.arange(0x80000000, u(-87.0) + 1, 97, dtype=np.uint64), np.arange(0, u(16.0) + 1, 97, dtype=np.uint64),
                           np.arange(u(-88.5) - 4096, u(-88.5) + 1, dtype=np.uint64)]).astype(np.uint32)
    x = np.concatenate([pats.view(np.float32), np.array([-87.0, -87.00001, -1e30, -np.inf, 0.0, -0.0], np.float32)])
    spec, floor = hc.exp_spec_vec(x)
    assert np.array_equal(_bits(sl.exp_spec32(x)), _bits(spec))
    assert np.array_equal(_bits(sl.exp_spec_floor32(x)), _bits(floor))
    rng = np.random.default_rng(5)   # fma32 itself, where the float64 sum is inexact: against the host's fmaf through exp_spec's first step
    a, b, c = (rng.normal(size=200000) * s for s in (1.0, 1.0, 1e-3))
    got = sl.fma32(a.astype(np.float32), b.astype(np.float32), c.astype(np.float32))
    import math
    if hasattr(math, "fma"):
        want = np.array([math.fma(float(np.float32(p)), float(np.float32(q)), float(np.float32(r))) for p, q, r in zip(a[:20000], b[:20000], c[:20000])])
        assert np.array_equal(_bits(got[:20000]), _bits(want.astype(np.float32)))


def test_numpy_skip_threshold_is_within_1e6_of_the_host_builds():
    rng = np.random.default_rng(11)
    op = np.concatenate([np.exp(rng.uniform(np.log(1e-3), 0.0, 100000)), [1e-3, 0.02, 0.3, 0.9, 1.0, 7.0]]).astype(np.float32)
    assert np.abs(sl.skip_threshold32(op).astype(np.float64) - hc.skip_threshold_vec(op)).max() <= 1e-6


def test_truth_and_rectangle_helpers_are_the_proven_functions():
    mx, my, cx, cy, cz, op, tx0, ty0 = _family("mixed", 20000)
    rec = np.zeros((len(mx), 16), np.float32)
    rec[:, :6] = np.stack([mx, my, cx, cy, cz, op], 1)
    _, truth = hc.block_masks(rec[:, :6], tx0, ty0)
    o = np.full(len(mx), tx0, np.float32), np.full(len(mx), ty0, np.float32)
    assert np.array_equal(hc.truth_masks(rec, None, *o), truth)
    perm = np.random.default_rng(1).permutation(len(mx)).astype(np.uint32)
    assert np.array_equal(hc.truth_masks(rec, perm, *o), truth[perm])
    mx, my, cx, cy, cz, op = _emission_set(*EMISSION_SETS[1], n=4000)
    rec = np.zeros((len(mx), 16), np.float32)
    rec[:, :6] = np.stack([mx, my, cx, cy, cz, op], 1)
    rec[:, 6] = hc.skip_threshold_vec(op)
    mask, _ = hc.block_masks_rect(rec[:, :6], *EMISSION_RECT)
    got, off = hc.masks_rect_each(rec, np.tile(np.array(EMISSION_RECT, np.int32), (len(mx), 1)))
    assert np.array_equal(got.reshape(mask.shape), mask) and off[1] == mask.shape[1]
