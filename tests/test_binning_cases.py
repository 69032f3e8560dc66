"""CPU tier of the direct binning tests (tests/binning_cases.py): the integer restatement of the binning stage is held to the
fp32 oracle, and every case is held to what it is named for.

How each case is checked: ALL of them -- the three 16.8-Mpixel grids included, whose oracle forward takes about 1.5 s each here --
against the oracle's own lists at the case's own size: point_list, ranges, tiles_touched and num_rendered of `oracle_for(scene)` equal the
restatement computed from that oracle's per-Gaussian arrays (radii, means2D, depths, tiles_touched).  The restatement's invariants (the
ranges partition [0, R), every range is in (depth key, index) order, every entry's Gaussian covers its tile) are asserted on top of that for
every case; the GPU tier relies on them where it restates from the device's own exports."""
import functools

import numpy as np
import pytest

import binning_cases as bc
from util import oracle_for

NAMES = list(bc.CASES)


class Run:
    pass


@functools.lru_cache(maxsize=None)
def run(name):
    r = Run()
    r.s = bc.scene(name)
    o = oracle_for(r.s)
    r.R = o.forward()
    r.b, r.key = bc.restate_oracle(o, r.s)
    r.oracle = {k: o.get(k).copy() for k in ("point_list", "ranges", "tiles_touched", "radii")}
    o.close()
    return r


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_the_oracles_binning(name):
    r = run(name)
    c = bc.CASES[name]
    assert r.R == r.b.num_rendered
    assert np.array_equal(r.oracle["tiles_touched"], r.b.rect_tiles.astype(np.uint32))
    assert np.array_equal(r.oracle["point_list"], r.b.point_list.astype(np.uint32))
    assert np.array_equal(r.oracle["ranges"].reshape(-1, 2), r.b.ranges)
    assert r.b.ranges.shape == (c.gx * c.gy, 2)
    assert np.array_equal((r.oracle["radii"] > 0), r.b.rect_tiles > 0)
    bc.check_invariants(r.b, r.key, c.gx, c.gy)
    assert np.array_equal(r.b.keys32, r.b.tile_ids) and np.array_equal(r.b.keys16.astype(np.int64), r.b.tile_ids & 0xFFFF)


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_what_it_is_named_for(name):
    r = run(name)
    reached = bc.CASES[name].reaches(r.b, r.key)
    assert reached and all(reached.values()), [k for k, v in reached.items() if not v]


def test_coop_threshold_has_splats_cut_by_the_border():
    r = run("coop_threshold")
    cut = bc.clipped_by_border(r.b, r.oracle["radii"], 20, 20)
    n = r.b.rect_tiles[cut]
    assert int(cut.sum()) >= 20 and {2, 15, 17, 63, 65} <= set(n.tolist())


def test_range_edges_cover_the_listed_sizes():
    for bits, Rs in ((16, bc.RANGE_R16), (32, bc.RANGE_R32)):
        for R in Rs:
            for arr in bc.ARRANGEMENTS:
                assert run(f"range_edges_{bits}-{R}-{arr}").R == R
    assert bc.RANGE_R16 == (1, 7, 8, 9, 2047, 2048, 2049, 4097) and bc.RANGE_R32 == (1, 3, 4, 5, 1023, 1024, 1025, 2049)
    assert bc.range_change_points(4097, 8, 2048) == [7, 8, 15, 16, 2039, 2040, 2047, 2048, 2055, 2056, 4095, 4096]
    assert bc.range_change_points(2049, 4, 1024) == [3, 4, 7, 8, 1019, 1020, 1023, 1024, 1027, 1028, 2047, 2048]


def test_layout_rule():
    """rect iff both grid dimensions <= 255; 16-bit keys iff higher_msb(tiles) <= 16 and no mask in the key (plan_attempt)"""
    from oracle import oracle as orc
    for n in (1, 2, 3, 255, 256, 32400, 65535, 65536, 65537, 65792, 129600, 1 << 20):
        assert bc.higher_msb(n) == orc.lib().oracle_higher_msb(n), n
    L = bc.layout
    assert L(240, 135) == bc.Layout(True, True, 15, False)                   # 3840 x 2160: the largest grid the suite rendered before
    assert L(255, 1).rect and not L(256, 1).rect and L(1, 255).rect and not L(1, 256).rect
    assert L(255, 257) == bc.Layout(False, True, 16, False)                  # 65 535 tiles
    assert L(256, 256) == bc.Layout(False, False, 17, False)                 # 65 536 tiles: ids fit 16 bits, the sort's bit count does not
    assert L(257, 256) == bc.Layout(False, False, 17, False)
    assert L(480, 270) == bc.Layout(False, False, 17, False)                 # 8K
    assert L(20, 20, streams=True, mask_in_key=True) == bc.Layout(True, False, 9, True)
    assert L(20, 20, streams=False, mask_in_key=True) == bc.Layout(True, True, 9, False)   # the mask exists in a stream forward only
    for name, c in bc.CASES.items():
        lay = L(c.gx, c.gy)
        assert lay.rect == (not name.startswith("grid_") or name in ("grid_255x1", "grid_1x255")), name
        assert lay.key16 == (name not in ("grid_256x256", "grid_257x256")), name


def test_restatement_sees_a_wrong_list():
    """the comparison the GPU tier makes is exact: one swapped pair inside a tie group, one range off by one, one key of another tile"""
    r = run("ties")
    b = r.b
    pl = b.point_list.copy()
    pl[[3, 4]] = pl[[4, 3]]
    assert not np.array_equal(pl, b.point_list)
    with pytest.raises(AssertionError):
        bc.check_invariants(b._replace(point_list=pl), r.key, 3, 2)
    rg = b.ranges.copy()
    rg[bc.TIES_TILE, 1] -= 1
    with pytest.raises(AssertionError):
        bc.check_invariants(b._replace(ranges=rg), r.key, 3, 2)
