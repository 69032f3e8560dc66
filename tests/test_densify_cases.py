"""CPU tier of the direct densification tests: every input condition tests/test_gpu_densify_direct.py relies on, asserted on the
NumPy reference alone (tests/densify_cases.py), and that reference pinned to the fixtures the upstream GaussianModel wrote."""
import numpy as np
import pytest
import torch

import densify_cases as dc
from test_densify_golden import check_against_fixture, load_fixture

F32 = np.float32


def ordinal(x):
    """float32 -> an integer that grows by one per representable value (finite values of one sign)"""
    return int(np.array(x, dtype=F32).view(np.int32))


def flags_match(case):
    flags, amb = dc.decide_case(case)
    P = case.scaling.shape[0]
    for k in ("clone", "split", "keep", "keep_clone", "keep_children"):
        want = case.expect.get(k, np.zeros(P, dtype=bool))
        assert np.array_equal(flags[k], want), (case.name, k, flags[k], want)
    return flags, amb


def test_max_grad_rows_are_on_or_one_ulp_off_the_threshold():
    c = dc.table_max_grad()
    g, _ = dc.mean_grads32(c.accum, c.accum_abs, c.denom)
    off = [ordinal(abs(x)) - ordinal(c.max_grad) for x in g]
    assert off == [0, -1, 1, 0, 1, -1] * 4
    assert c.max_grad == F32(0.0002) and set(c.denom.reshape(-1)) == {1.0, 2.0, 4.0, 8.0}
    assert F32(F32(F32(0.0002) * F32(5)) / F32(5)) != F32(0.0002)            # why denom = 5 is not in the table
    flags_match(c)


def test_Q_rows_are_on_or_one_ulp_off_the_threshold():
    c = dc.table_Q()
    _, ga = dc.mean_grads32(c.accum, c.accum_abs, c.denom)
    assert [ordinal(x) - ordinal(c.Q) for x in ga[:4]] == [0, 0, -1, 1] and ga[4] == 0
    assert not np.array_equal(c.accum_abs[0], c.accum_abs[1])                  # an equal quotient from other operands
    flags_match(c)


def test_denom0_rows_give_the_stated_quotients():
    c = dc.table_denom0()
    g, ga = dc.mean_grads32(c.accum, c.accum_abs, c.denom)
    assert g[0] == 0 and ga[0] == 0 and g[1] == np.inf and ga[1] == 0 and g[2] == 0 and ga[2] == np.inf
    assert g[3] == 0 and g[4] == 0 and ga[4] == 0 and g[5] == np.inf and g[6] == -np.inf and ga[7] == 0 and ga[8] == np.inf and g[9] == -np.inf
    assert np.isnan(c.accum[3, 0]) and np.isnan(c.accum_abs[7, 0])
    flags_match(c)


def test_scale_and_opacity_rows_are_exact_or_outside_the_band():
    one, half, D = 1.0, 0.5, float(dc.D)
    assert dc.table_dense().dense == F32(1.0) == F32(0.1) * F32(10.0) and D == 2.0 ** -20
    # exp(0) == 1 and sigmoid(0) == 0.5 exactly; the neighbours' distance in float32 ulps of the threshold, on their own side
    up1, down1 = float(np.nextafter(F32(1), F32(2))) - one, one - float(np.nextafter(F32(1), F32(0)))
    assert np.exp(0.0) == 1.0 and (np.exp(D) - one) / up1 >= 8 and (one - np.exp(-D)) / down1 >= 8
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    up5, down5 = float(np.nextafter(F32(0.5), F32(1))) - half, half - float(np.nextafter(F32(0.5), F32(0)))
    assert sig(0.0) == 0.5 and (half - sig(-D)) / down5 >= 8 - 1e-6 and (sig(D) - half) / up5 >= dc.BAND_ULPS
    for c in (dc.table_dense(), dc.table_big(True), dc.table_big(False), dc.table_min_opacity()):
        flags_match(c)
    c = dc.table_dense()
    assert sorted(set(c.scaling.max(axis=1).tolist())) == [-D, 0.0, D]
    assert {int(np.argmax(r)) for r in c.scaling} == {0, 1, 2}
    c = dc.table_min_opacity()
    assert sorted(set(c.opacity.reshape(-1).tolist())) == [-D, 0.0, D]
    big_on, big_off = dc.decide_case(dc.table_big(True))[0], dc.decide_case(dc.table_big(False))[0]
    assert not big_on["keep"].all() and big_off["keep"].all() and big_off["keep_clone"].sum() > big_on["keep_clone"].sum()


def test_children_rows_keep_their_distance_and_separate_cmax_from_smax():
    c = dc.table_children()
    flags, _ = flags_match(c)
    s = np.exp(c.scaling.astype(np.float64)).max(axis=1)
    big = float(c.big)
    rel = np.abs(s / 1.6 / big - 1.0)
    assert rel.min() >= 1e-4
    between = (s / 1.6 <= big) & (s > big) & flags["split"]                  # cmax <= big_threshold < smax: children kept
    assert between.sum() >= 2 and flags["keep_children"][between].all()
    assert (flags["split"] & ~flags["keep_children"]).sum() >= 2              # cmax > big_threshold: children pruned
    assert (~flags["split"] & ~flags["keep"] & (s > big)).sum() >= 2          # the same scales cold: the row is pruned on smax


def test_no_threshold_table_and_no_pattern_has_an_ambiguous_row():
    cases = dc.threshold_tables() + [c for c, _ in dc.pattern_cases()] + [c for c, _, _ in dc.chunk_edge_cases()]
    assert len(cases) == 8 + 72 + 28
    for c in cases:
        flags, amb = flags_match(c)
        assert not amb.any(), (c.name, np.argwhere(amb))
        assert c.scaling.shape[0] <= 5000


def test_every_pattern_has_the_row_count_it_is_named_for():
    seen = set()
    for c, P_out in dc.pattern_cases():
        kind, P = c.name.rsplit("_P", 1)[0], c.scaling.shape[0]
        seen.add((kind, P))
        flags, _ = dc.decide_case(c)
        src, counts = dc.expected_src_of(flags)
        assert counts[0] == P_out == src.size, (c.name, counts, P_out)
        want = dict(all_survive=P, all_clone=2 * P, all_split=2 * P, all_pruned=0, first_removed=P - 1, last_removed=P - 1,
                    alternate_removed=(P + 1) // 2).get(kind)
        if want is not None:
            assert P_out == want, c.name
        seg = src >> dc.SEG_SHIFT
        if kind == "all_split":
            assert not (seg == 0).any() and counts[2] == P
        if kind == "all_clone":
            assert (seg == 0).sum() == P == (seg == 1).sum() == counts[1]
        if kind == "all_pruned":
            assert counts[3] == P + counts[1] + counts[2] and (P < 3 or (counts[1] > 0 and counts[2] > 0))
    assert seen == {(k, P) for k in dc.PATTERNS for P in dc.PATTERN_P}
    sep = dc._runs(60)
    runs = np.diff(np.concatenate([[-1], np.flatnonzero(sep)])) - 1
    assert runs[:10].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9, 1]
    c, P_out = dc.pattern_case("runs_split", 257, 9)
    flags, _ = dc.decide_case(c)
    assert flags["split"].sum() == dc._runs(257).sum() > 40 and P_out == 257 + flags["split"].sum()
    assert {c.rest_floats for c, _ in dc.pattern_cases()} == {0, 9, 24, 45}


def test_chunk_edge_sizes_hit_the_stated_element_counts():
    hits = set()
    widths = lambda rest: {1, 3, 4} | ({rest} if rest else set())
    for c, P_out, W in dc.chunk_edge_cases():
        flags, _ = dc.decide_case(c)
        assert dc.expected_src_of(flags)[1][0] == P_out, c.name
        assert W in widths(c.rest_floats), c.name
        hits.add((W, P_out * W))
    # 4095 = 3^2 5 7 13, 4096 = 2^12, 4097 = 17 241: these are all the exact landings the widths allow ...
    assert {(W, n) for W, n in hits if n in (dc.CHUNK - 1, dc.CHUNK, dc.CHUNK + 1)} == dc.CHUNK_EXACT
    for W in (1, 3, 4, 9, 24, 45):
        assert {(W, n) for n in (4095, 4096, 4097) if n % W == 0} <= dc.CHUNK_EXACT
        # ... and every width has its last row count at or below the edge and its first above it
        below, above = dc.CHUNK // W * W, (dc.CHUNK // W + 1) * W
        assert (W, below) in hits and (W, above) in hits, W


def test_random_case_is_unmargined_and_populated():
    c = dc.random_case()
    assert c.scaling.shape[0] == 5000
    flags, amb = dc.decide_case(c)
    src, counts = dc.expected_src_of(flags)
    print("random case: counts", counts, "ambiguous rows", int(amb.any(axis=1).sum()), "Q", float(c.Q))
    assert amb.any(axis=1).sum() <= 5                                          # 0.1 %
    assert counts[1] >= 50 and counts[2] >= 50 and counts[3] >= 50
    assert flags["keep_clone"].sum() >= 50 and flags["keep_children"].sum() >= 50
    assert (c.denom == 0).sum() > 100 and np.isinf(dc.mean_grads32(c.accum, c.accum_abs, c.denom)[0]).sum() == 3
    again = dc.random_case()
    assert all(np.array_equal(a, b) for a, b in zip(c[1:6], again[1:6]))


def test_flip_changes_ambiguous_rows_only_and_enumerates_from_no_flip():
    c = dc.table_min_opacity()
    base, _ = dc.decide_case(c)
    amb = np.zeros((9, 4), dtype=bool)
    amb[0, 1] = amb[3, 1] = True                                               # a cold row and a clone source, both kept at sigmoid == 0.5
    got = [dc.decide_case(c, f)[0] for f in dc.assignments(amb)]
    assert len(got) == 4 and all(np.array_equal(got[0][k], base[k]) for k in base)
    assert base["keep"][0] and base["keep_clone"][3]
    assert not got[3]["keep"][0] and not got[3]["keep_clone"][3] and not got[3]["keep"][3]
    others = np.setdiff1d(np.arange(9), [0, 3])
    assert all(np.array_equal(got[3][k][others], base[k][others]) for k in base)


@pytest.mark.parametrize("name", ["densify_sh1", "densify_sh3"])
def test_reference_reproduces_the_upstream_fixture(name):
    d = load_fixture(name)
    mss = int(d["max_screen_size"])
    ext = float(d["extent"])
    flags, amb = dc.decide(d["accum"], d["accum_abs"], d["denom"], d["in_scaling"], d["in_opacity"], F32(d["Q"]), F32(d["max_grad"]),
                           F32(float(d["percent_dense"]) * ext), F32(d["min_opacity"]), None if mss <= 0 else F32(0.1 * ext))
    assert not amb.any()
    src, counts = dc.expected_src_of(flags)
    params = {n: d["in_" + n] for n in dc.PARAMS}
    m = {n: d["in_exp_avg_" + n] for n in dc.PARAMS}
    v = {n: d["in_exp_avg_sq_" + n] for n in dc.PARAMS}
    for dtype in (np.float64, np.float32):
        out = dc.apply_rows(src, params, m, v, d["z"], dtype)
        t = lambda x: {n: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for n, a in x.items()}
        check_against_fixture(d, t(out[0]), t(out[1]), t(out[2]), counts[1:])


def test_statistics_reference_on_its_own_cases():
    for P in dc.STATS_P:
        grad, radii, mask, st = dc.stats_view_case(P)
        for use_mask, use_radii in ((True, True), (True, False), (False, True)):
            out = dc.stats_step32(st, grad, mask if use_mask else None, radii if use_radii else None)
            vis = mask if use_mask else radii > 0
            for k in st:
                a, b = out[k].reshape(-1), st[k].reshape(-1)
                assert np.array_equal(a.view(np.uint32)[~vis], b.view(np.uint32)[~vis]), (P, k)      # invisible rows: the same bits
            if not use_radii:
                assert np.array_equal(out["max_radii2D"].view(np.uint32), st["max_radii2D"].view(np.uint32))
            assert out["denom"][0, 0] == st["denom"][0, 0] + 1
            if P > 9:
                cls = np.arange(P) % 10
                assert np.isnan(out["accum_abs_max"].reshape(-1)[cls == 6]).all() and np.isnan(out["accum_abs_max"].reshape(-1)[cls == 9]).all()
                assert np.isnan(out["accum"].reshape(-1)[cls == 5]).all() and np.isinf(out["accum"].reshape(-1)[cls == 4]).all()
                assert (out["accum_abs"].reshape(-1)[cls == 3] == F32(2e-42)).all() and F32(2e-42) > 0
                assert use_mask == bool(vis[7]) and use_mask != bool(vis[8]) and not vis[1]
        red, radii_max, st = dc.stats_reduced_case(P)
        out = dc.stats_step_reduced32(st, red, radii_max)
        unseen = red[:, 2] == 0
        assert set(red[:, 2].tolist()) <= {0.0, 1.0, 3.0} and (P < 8 or (red[unseen][:, :2] != 0).any())
        for k in st:
            assert np.array_equal(out[k].reshape(-1).view(np.uint32)[unseen], st[k].reshape(-1).view(np.uint32)[unseen]), (P, k)
        assert np.array_equal(out["denom"].reshape(-1)[~unseen], (st["denom"].reshape(-1) + red[:, 2])[~unseen])
        if P > 4:
            assert np.isnan(out["accum_abs_max"][4, 0]) and np.isnan(out["accum_abs"][4, 0])
