"""Case builders and the NumPy reference for the direct tests of the densification kernels (radegs_densify.hip): test
infrastructure, pure NumPy, no GPU.  Written from include/radegs.h, "Adaptive density control", and from nothing else.

  decide / expected_src_of / apply_rows   the plan and the apply as the header states them; decisions on float64 quantities with
                                          an `ambiguous` mask, values in float64 and in float32
  stats_step32 / stats_step_reduced32     the two statistics updates in float32, operation for operation
  threshold_tables                        one comparison of the plan at its threshold per case, the others out of reach
  pattern_cases / chunk_edge_cases        row patterns that drive every path of the apply kernel, sizes on the 4096-float chunk edge
  random_case                             5000 rows of smooth distributions with nothing moved off the thresholds

tests/test_densify_cases.py asserts on the CPU every condition a builder promises; tests/test_gpu_densify_direct.py runs the kernels."""
import itertools
import math
from collections import namedtuple

import numpy as np

F32 = np.float32
PARAMS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
SEG_SHIFT = 30
ROW_MASK = (1 << SEG_SHIFT) - 1
BAND_ULPS = 4.0
CHUNK = 4096                                    # floats of one output array that one block of the apply kernel writes
COMPARISONS = ("dense", "faint", "big", "big_child")
INF = F32(np.inf)


def f32(x):
    return np.ascontiguousarray(x, dtype=F32)


# ------------------------------------------------------------------------------------------------------------------- plan
def mean_grads32(accum, accum_abs, denom):
    """g = accum / denom and ga = accum_abs / denom in float32, one IEEE divide each; 0/0 = NaN -> 0, x/0 = Inf stays"""
    a, b, d = (f32(t).reshape(-1) for t in (accum, accum_abs, denom))
    with np.errstate(divide="ignore", invalid="ignore"):
        g, ga = a / d, b / d
    g[np.isnan(g)] = 0
    ga[np.isnan(ga)] = 0
    return g, ga


def _within_band(q64, thr):
    """|q - thr| < BAND_ULPS float32 ulps of thr, the ulp taken on q's side of thr (at a power of two the lower side's is half the upper's).
    A quantity exactly BAND_ULPS off is outside.  An infinite threshold has no band."""
    thr = F32(thr)
    if not np.isfinite(thr):
        return np.zeros(q64.shape, dtype=bool)
    t = float(thr)
    up, down = float(np.nextafter(thr, INF)) - t, t - float(np.nextafter(thr, -INF))
    with np.errstate(invalid="ignore"):
        return np.abs(q64 - t) < BAND_ULPS * np.where(q64 < t, down, up)


def decide(accum, accum_abs, denom, scaling, opacity, Q, max_grad, dense_threshold, min_opacity, big_threshold, flip=None):
    """Every decision of radegs_densify_plan, per input row.  Thresholds are the float32 values the C ABI receives; big_threshold None =
    prune_big off.  Returns (flags, ambiguous): flags a dict of bool [P] arrays
        clone, split            selected for cloning / splitting (upstream's report counts these)
        keep                    the row itself comes out: not split and not pruned
        keep_clone              its clone comes out
        keep_children           its two split children come out
    hot = |g| >= max_grad or ga >= Q is decided in float32 (divide only: the kernel's bits, never ambiguous).  The largest activated scale
    smax = max exp(s), the children's cmax = max exp(log(exp(s) / 1.6)) = max exp(s) / 1.6 and sigmoid(opacity) are float64; a row is
    ambiguous [P, 4 = COMPARISONS] where such a quantity lies within BAND_ULPS float32 ulps of the threshold it is compared with: expf
    and logf are 1-ulp functions and the sigmoid adds one add and one divide, so the kernel's float32 value may fall on either side (a raw operand of exactly 0 excepted: see below).
    flip: bool [P,4] or None; where True the comparison takes the other outcome (the tests enumerate it over ambiguous rows only)."""
    g, ga = mean_grads32(accum, accum_abs, denom)
    P = g.size
    with np.errstate(invalid="ignore"):
        hot = (np.abs(g) >= F32(max_grad)) | (ga >= F32(Q))
    s = np.exp(f32(scaling).reshape(P, 3).astype(np.float64))
    smax, cmax = s.max(axis=1), (s / 1.6).max(axis=1)
    sig = 1.0 / (1.0 + np.exp(-f32(opacity).reshape(P).astype(np.float64)))
    prune_big = big_threshold is not None
    big_t = F32(big_threshold) if prune_big else INF
    large = smax > float(F32(dense_threshold))            # split rather than clone
    faint = sig < float(F32(min_opacity))
    big, big_child = smax > float(big_t), cmax > float(big_t)
    ambiguous = np.stack([_within_band(smax, dense_threshold), _within_band(sig, min_opacity), _within_band(smax, big_t),
                          _within_band(cmax, big_t)], axis=1)
    # a raw operand of exactly 0 is exact in float32 too -- expf(0) == 1, and sigmoid(0) is then the one exact divide 1 / 2 -- so these
    # rows sit ON a threshold of 1 / 0.5 without being ambiguous
    exact_s, exact_o = f32(scaling).reshape(P, 3).max(axis=1) == 0, f32(opacity).reshape(P) == 0
    ambiguous[:, 0] &= ~exact_s
    ambiguous[:, 2] &= ~exact_s
    ambiguous[:, 1] &= ~exact_o
    if flip is not None:
        large, faint, big, big_child = large ^ flip[:, 0], faint ^ flip[:, 1], big ^ flip[:, 2], big_child ^ flip[:, 3]
    clone, split = hot & ~large, hot & large
    drop, drop_child = faint | big, faint | big_child
    flags = dict(clone=clone, split=split, keep=~split & ~drop, keep_clone=clone & ~drop, keep_children=split & ~drop_child)
    return flags, ambiguous


def expected_src_of(flags):
    """upstream's output order -- surviving unsplit originals, clones, first children, second children, each in source order -- as
    row | segment << 30 (uint32 [P_out]), and counts4 = (rows out, clone-selected, split-selected, pruned by the final prune)"""
    segs = (flags["keep"], flags["keep_clone"], flags["keep_children"], flags["keep_children"])
    src = np.concatenate([np.flatnonzero(k).astype(np.uint32) | np.uint32(n << SEG_SHIFT) for n, k in enumerate(segs)])
    P, n_clone, n_split = flags["keep"].size, int(flags["clone"].sum()), int(flags["split"].sum())
    return src, (int(src.size), n_clone, n_split, P + n_clone + n_split - int(src.size))


def decide_case(c, flip=None):
    return decide(c.accum, c.accum_abs, c.denom, c.scaling, c.opacity, c.Q, c.max_grad, c.dense, c.min_opacity, c.big, flip)


def assignments(ambiguous, limit=4096):
    """every flip array that differs from 'no flip' on ambiguous comparisons only, 'no flip' first"""
    where = np.argwhere(ambiguous)
    assert 2 ** len(where) <= limit, len(where)
    for bits in itertools.product((False, True), repeat=len(where)):
        flip = np.zeros(ambiguous.shape, dtype=bool)
        for (i, k), b in zip(where, bits):
            flip[i, k] = b
        yield flip


# ------------------------------------------------------------------------------------------------------------------ apply
def rotation_rows(q, dtype):
    """R(q / |q|) [P,3,3] of raw quaternions (w, x, y, z) [P,4], every operation in `dtype`"""
    q = np.asarray(q).astype(dtype)
    with np.errstate(all="ignore"):
        q = q / np.sqrt((q * q).sum(axis=1, keepdims=True, dtype=dtype))
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        one, two = dtype(1), dtype(2)
        R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                      two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                      two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=1)
    return R.reshape(-1, 3, 3)


def apply_rows(src_of, params, m, v, z, dtype):
    """Every output array of radegs_densify_apply from a given src_of, computed in `dtype` (np.float64 or np.float32) from the float32
    inputs.  params / m / v: dicts over PARAMS of [P, ...] arrays (a moment, or f_rest of width 0, may be None); z: [P,3,3], slot 0 the
    clone's draw, 1 / 2 the children's.  Copies are gathers; new rows' moments are zero; xyz' = xyz + R(q/|q|) (z o exp(s)) on new rows;
    children store log(exp(s) / 1.6).  Returns (params', m', v')."""
    src_of = np.asarray(src_of).astype(np.int64)
    seg, row = src_of >> SEG_SHIFT, src_of & ROW_MASK
    new = seg > 0
    out_p, out_m, out_v = {}, {}, {}
    for name in PARAMS:
        x = params.get(name)
        out_p[name] = None if x is None else np.asarray(x)[row].astype(dtype)
        for src, dst in ((m, out_m), (v, out_v)):
            t = src.get(name) if src else None
            if t is None:
                dst[name] = None
                continue
            o = np.asarray(t)[row].astype(dtype)
            o[new] = 0
            dst[name] = o
    with np.errstate(all="ignore"):
        s = np.exp(np.asarray(params["scaling"]).astype(dtype))
        if new.any():
            r, k = row[new], seg[new] - 1
            zs = np.asarray(z).astype(dtype)[r, k] * s[r]                                   # [n,3]
            R = rotation_rows(np.asarray(params["rotation"])[r], dtype)
            off = R[:, :, 0] * zs[:, 0:1] + R[:, :, 1] * zs[:, 1:2] + R[:, :, 2] * zs[:, 2:3]
            out_p["xyz"][new] = out_p["xyz"][new] + off
        child = seg >= 2
        if child.any():
            out_p["scaling"][child] = np.log(s[row[child]] / dtype(1.6))
    return out_p, out_m, out_v


# ------------------------------------------------------------------------------------------------------------- statistics
STAT_KEYS = ("accum", "accum_abs", "accum_abs_max", "denom")


def _max_nan(a, b):
    """max that propagates a NaN from either side, as the reference's torch.max does (include/radegs.h states the rule)"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a) | np.isnan(b), F32(np.nan), np.where(a > b, a, b)).astype(F32)


def _stats_update(stats, vis, add, add_abs, add_n, radii):
    out = {k: None if stats[k] is None else f32(stats[k]).copy() for k in stats}
    with np.errstate(all="ignore"):
        for key, val in (("accum", out["accum"].reshape(-1) + add), ("accum_abs", out["accum_abs"].reshape(-1) + add_abs),
                         ("accum_abs_max", _max_nan(out["accum_abs_max"].reshape(-1), add_abs)), ("denom", out["denom"].reshape(-1) + add_n)):
            out[key].reshape(-1)[vis] = val.astype(F32)[vis]
        if radii is not None and stats.get("max_radii2D") is not None:
            r = np.asarray(radii).astype(F32)
            out["max_radii2D"][vis] = np.where(out["max_radii2D"] > r, out["max_radii2D"], r)[vis]
    return out


def stats_step32(stats, grad, mask=None, radii=None):
    """radegs_densify_stats for one view in float32: stats = dict(accum, accum_abs, accum_abs_max, denom [P,1], max_radii2D [P] or None).
    visible = mask where a mask is given, else radii > 0.  sqrt(gx * gx + gy * gy): two products, one sum, one square root, each rounded."""
    g = f32(grad)
    vis = np.asarray(mask).astype(bool) if mask is not None else np.asarray(radii) > 0
    with np.errstate(all="ignore"):
        add = np.sqrt((g[:, 0] * g[:, 0]).astype(F32) + (g[:, 1] * g[:, 1]).astype(F32)).astype(F32)
    return _stats_update(stats, vis, add, np.abs(g[:, 2]), F32(1), radii)


def stats_step_reduced32(stats, reduced, radii_max=None):
    """radegs_densify_stats_reduced: reduced [P,3] = sum |grad xy|, sum |grad abs|, number of ranks that saw the row; rows whose count is
    0 are not written; accum_abs_max takes the max with the SUM column"""
    r = f32(reduced)
    return _stats_update(stats, r[:, 2] != 0, r[:, 0], r[:, 1], r[:, 2], radii_max)


# ------------------------------------------------------------------------------------------------------------------ cases
# expect: what the builder promises about the case (checked on the CPU against decide()): dict of bool [P] arrays by flag name
Case = namedtuple("Case", "name accum accum_abs denom scaling opacity Q max_grad dense min_opacity big rest_floats expect")
MAX_GRAD = F32(0.0002)
SMALL, LARGE = F32(math.log(0.01)), F32(math.log(0.2))     # raw scales far below / above every dense threshold used here
D = F32(2.0 ** -20)


def _case(name, accum, accum_abs, denom, scaling, opacity, Q=INF, max_grad=INF, dense=INF, min_opacity=F32(0), big=None, rest_floats=0,
          expect=None):
    P = len(accum)
    col = lambda a: f32(a).reshape(P, 1)
    return Case(name, col(accum), col(accum_abs), col(denom), f32(scaling).reshape(P, 3), col(opacity), F32(Q), F32(max_grad), F32(dense),
                F32(min_opacity), None if big is None else F32(big), rest_floats, expect or {})


def _b(*v):
    return np.array(v, dtype=bool)


def table_max_grad():
    """|g| >= max_grad: denom in {1, 2, 4, 8} (a division by a power of two is exact), accum = max_grad * denom exactly on the threshold,
    one ulp below, one above, and the negatives through |.|.  Everything hot is cloned (dense = inf), nothing is pruned."""
    accum, denom, hot = [], [], []
    for d in (1, 2, 4, 8):
        a = F32(MAX_GRAD * F32(d))
        lo, hi = np.nextafter(a, F32(0)), np.nextafter(a, INF)
        accum += [a, lo, hi, -a, -hi, -lo]
        hot += [True, False, True, True, True, False]
        denom += [d] * 6
    P = len(accum)
    hot = _b(*hot)
    return _case("max_grad", accum, np.zeros(P), denom, np.full((P, 3), SMALL), np.ones(P), max_grad=MAX_GRAD,
                 expect=dict(clone=hot, split=np.zeros(P, bool), keep=np.ones(P, bool), keep_clone=hot))


def table_Q():
    """ga >= Q with the device scalar set to row 0's own ga = fl(0.0007f / 3): that row and an equal one (both operands doubled) are hot,
    one ulp below is cold, one above hot"""
    a0 = F32(0.0007)
    q = F32(a0 / F32(3))
    accum_abs = [a0, F32(2) * a0, np.nextafter(q, F32(0)), np.nextafter(q, INF), F32(0)]
    denom = [3, 6, 1, 1, 1]
    hot = _b(True, True, False, True, False)
    return _case("Q", np.zeros(5), accum_abs, denom, np.full((5, 3), SMALL), np.ones(5), Q=q,
                 expect=dict(clone=hot, split=np.zeros(5, bool), keep=np.ones(5, bool), keep_clone=hot))


def table_denom0():
    """0/0 -> 0 cold; x/0 = Inf hot (through max_grad or through Q alone); NaN sums cold; Inf sums hot, -Inf through |.|"""
    nan, inf = np.nan, np.inf
    rows = [(0, 0, 0, False), (0.5, 0, 0, True), (0, 0.5, 0, True), (nan, 0, 3, False), (nan, nan, 0, False), (inf, 0, 2, True),
            (-inf, 0, 2, True), (0, nan, 1, False), (0, inf, 4, True), (-0.5, 0, 0, True)]
    a, b, d, hot = zip(*rows)
    hot, P = _b(*hot), len(rows)
    return _case("denom0", a, b, d, np.full((P, 3), SMALL), np.ones(P), Q=F32(0.001), max_grad=MAX_GRAD,
                 expect=dict(clone=hot, split=np.zeros(P, bool), keep=np.ones(P, bool), keep_clone=hot))


def table_dense():
    """smax <= dense_threshold = 1.0 (0.2 * 5.0 and 0.1 * 10.0 both give 1.0f): largest raw scale 0 -> exp == 1 exactly -> clone; +2^-20 ->
    split; -2^-20 -> clone; the largest scale in each of the three columns; the same rows cold: nothing"""
    tops = [F32(0), D, -D]
    scal, large = [], []
    for col in range(3):
        for t in tops:
            r = [F32(-1)] * 3
            r[col] = t
            scal.append(r)
            large.append(bool(t > 0))
    n = len(scal)
    scal, large = scal + scal, _b(*(large + large))
    hot = _b(*([True] * n + [False] * n))
    P = 2 * n
    return _case("dense", hot.astype(F32), np.zeros(P), np.ones(P), scal, np.ones(P), max_grad=MAX_GRAD, dense=F32(0.2) * F32(5.0),
                 expect=dict(clone=hot & ~large, split=hot & large, keep=~(hot & large), keep_clone=hot & ~large, keep_children=hot & large))


def _big_rows():
    scal = [[F32(0), F32(-1), F32(-2)], [F32(-1), D, F32(-2)], [F32(-2), F32(-1), -D], [F32(-1), F32(-1), F32(0)]] * 2
    big = _b(False, True, False, False, False, True, False, False)
    hot = _b(True, True, True, True, False, False, False, False)
    return scal, big, hot


def table_big(prune_big=True):
    """smax > big_threshold = 1.0 with prune_big: smax == 1 kept, exp(2^-20) pruned, the row and its clone alike (dense = inf: no split);
    prune_big = 0 with the same rows: nothing pruned"""
    scal, big, hot = _big_rows()
    drop = big if prune_big else np.zeros(8, bool)
    return _case("big" if prune_big else "big_off", hot.astype(F32), np.zeros(8), np.ones(8), scal, np.ones(8), max_grad=MAX_GRAD,
                 big=F32(1.0) if prune_big else None,
                 expect=dict(clone=hot, split=np.zeros(8, bool), keep=~drop, keep_clone=hot & ~drop))


def table_min_opacity():
    """sigmoid(o) < min_opacity = 0.5: raw 0 -> exactly 0.5 -> kept; -2^-20 (8 ulps below) faint; +2^-20 kept; on cold rows, on clone
    sources (the row and its clone go) and on split sources (both children go)"""
    op, scal, hot, large = [], [], [], []
    for h, lg in ((False, False), (True, False), (True, True)):
        for o in (F32(0), -D, D):
            op.append(o)
            scal.append([F32(1) if lg else F32(-1)] * 3)
            hot.append(h)
            large.append(lg)
    hot, large, faint = _b(*hot), _b(*large), np.array(op) < 0
    clone, split = hot & ~large, hot & large
    return _case("min_opacity", hot.astype(F32), np.zeros(9), np.ones(9), scal, op, max_grad=MAX_GRAD, dense=F32(1.0), min_opacity=F32(0.5),
                 expect=dict(clone=clone, split=split, keep=~split & ~faint, keep_clone=clone & ~faint, keep_children=split & ~faint))


CHILD_BIG = F32(1.0)
CHILD_REL = (-1e-2, -2e-4, 2e-4, 1e-2)        # max(s) / 1.6 relative to big_threshold: never closer than 1e-4 (exp(log(.)) has no exact operand)


def table_children():
    """the split children are pruned on cmax = max exp(log(s / 1.6)), not on their source's smax.  Sources 0 and 1 have
    cmax <= big_threshold < smax: split, and both children kept although the source itself is above the threshold.  Cold rows with the same
    scales: pruned (or kept) on smax.  One small source whose children and itself are far below."""
    scal = [[F32(math.log(1.6 * float(CHILD_BIG) * (1 + r))), F32(-3), F32(-3)] for r in CHILD_REL] + [[F32(-1)] * 3]
    n = len(scal)
    scal = scal + scal
    hot = _b(*([True] * n + [False] * n))
    child_big = _b(*([r > 0 for r in CHILD_REL] + [False]))
    src_big = _b(*([True] * len(CHILD_REL) + [False]))
    P = 2 * n
    return _case("children", hot.astype(F32), np.zeros(P), np.ones(P), scal, np.ones(P), max_grad=MAX_GRAD, dense=F32(0.01), big=CHILD_BIG,
                 expect=dict(clone=np.zeros(P, bool), split=hot, keep=~hot & ~np.tile(src_big, 2), keep_clone=np.zeros(P, bool),
                             keep_children=hot & ~np.tile(child_big, 2)))


def threshold_tables():
    return [table_max_grad(), table_Q(), table_denom0(), table_dense(), table_big(True), table_big(False), table_min_opacity(), table_children()]


# ---- row patterns: opacity removes a row, the scale chooses clone against split, accum makes a row hot ----
PATTERN_P = (1, 2, 3, 4, 5, 255, 256, 257)
PATTERN_REST = (0, 9, 24, 45)
PATTERN_DENSE, PATTERN_MIN_OPACITY = F32(0.05), F32(0.05)
KEPT_OPACITY, FAINT_OPACITY = F32(1.0), F32(-6.0)


def _runs(P):
    """True at the separator rows: runs of 1, 2, .. 9, 1, 2, .. ordinary rows, one separator after each"""
    sep = np.zeros(P, dtype=bool)
    i, run = 0, 1
    while True:
        i += run
        if i >= P:
            return sep
        sep[i] = True
        i, run = i + 1, run % 9 + 1


def pattern_roles(kind, P):
    """(hot, large, faint) bool [P] of a pattern, and the number of output rows it is named for"""
    z = np.zeros(P, dtype=bool)
    idx = np.arange(P)
    if kind == "all_survive":
        return z, z, z, P
    if kind == "all_clone":
        return ~z, z, z, 2 * P
    if kind == "all_split":
        return ~z, ~z, z, 2 * P
    if kind == "all_pruned":
        return idx % 3 > 0, idx % 3 > 1, ~z, 0                  # cold rows, clone sources and split sources alike: all faint
    if kind == "first_removed":
        return z, z, idx == 0, P - 1
    if kind == "last_removed":
        return z, z, idx == P - 1, P - 1
    if kind == "alternate_removed":
        return z, z, idx % 2 == 1, (P + 1) // 2
    sep = _runs(P)
    if kind == "runs_removed":
        return z, z, sep, P - int(sep.sum())
    if kind == "runs_split":
        return sep, sep, z, P + int(sep.sum())
    raise ValueError(kind)


PATTERNS = ("all_survive", "all_clone", "all_split", "all_pruned", "first_removed", "last_removed", "alternate_removed", "runs_removed",
            "runs_split")


def pattern_case(kind, P, rest_floats, name=None):
    hot, large, faint, P_out = pattern_roles(kind, P)
    scal = np.where(large[:, None], LARGE, SMALL) + f32(np.linspace(-0.25, 0.25, 3 * P)).reshape(P, 3)
    clone, split = hot & ~large, hot & large
    c = _case(name or f"{kind}_P{P}_rest{rest_floats}", hot.astype(F32) * F32(3), np.zeros(P), np.full(P, 3), scal,
              np.where(faint, FAINT_OPACITY, KEPT_OPACITY), max_grad=MAX_GRAD, dense=PATTERN_DENSE, min_opacity=PATTERN_MIN_OPACITY,
              rest_floats=rest_floats, expect=dict(clone=clone, split=split, keep=~split & ~faint, keep_clone=clone & ~faint,
                                                   keep_children=split & ~faint))
    return c, P_out


def pattern_cases():
    out = []
    for n, (kind, P) in enumerate(itertools.product(PATTERNS, PATTERN_P)):
        out.append(pattern_case(kind, P, PATTERN_REST[n % 4]))
    return out


# (width W, rest_floats of the model, P_out): P_out * W on 4095 / 4096 / 4097 wherever W divides one of them (4095 = 3^2 5 7 13,
# 4096 = 2^12, 4097 = 17 241), else the two row counts either side of the chunk edge
CHUNK_EDGES = ((1, 0, 4095), (1, 9, 4096), (1, 24, 4097), (3, 45, 1365), (3, 0, 1366), (4, 9, 1023), (4, 24, 1024), (4, 45, 1025),
               (9, 9, 455), (9, 9, 456), (24, 24, 170), (24, 24, 171), (45, 45, 91), (45, 45, 92))
CHUNK_EXACT = {(1, 4095), (1, 4096), (1, 4097), (3, 4095), (4, 4096), (9, 4095), (45, 4095)}      # (W, P_out * W) that land exactly


def chunk_edge_cases():
    """per entry of CHUNK_EDGES two cases with that P_out: every row survives (the 16-byte path up to the array's end) and runs of
    survivors separated by removed rows (the smallest P whose pattern leaves P_out rows).  Returns (case, P_out, W)."""
    out = []
    for W, rest, P_out in CHUNK_EDGES:
        out.append(pattern_case("all_survive", P_out, rest, f"edge_W{W}_{P_out}_survive") + (W,))
        P = P_out
        while pattern_roles("runs_removed", P)[3] < P_out:
            P += 1
        out.append(pattern_case("runs_removed", P, rest, f"edge_W{W}_{P_out}_runs") + (W,))
    return out


RANDOM_SEED, RANDOM_P = 20241, 5000


def random_case():
    """training-like smooth distributions, nothing moved off any threshold; Q is the reference's quantile of ga"""
    rng = np.random.default_rng(RANDOM_SEED)
    P = RANDOM_P
    denom = rng.integers(0, 12, P).astype(F32)
    g = float(MAX_GRAD) * np.exp(rng.standard_normal(P) - 0.7)
    ga = 4.0 * float(MAX_GRAD) * np.exp(rng.standard_normal(P) - 0.7)
    accum, accum_abs = f32(g * denom), f32(ga * denom)
    unseen = np.flatnonzero(denom == 0)
    accum[unseen[:3]], accum_abs[unseen[3:6]] = F32(0.001), F32(0.002)
    g32, ga32 = mean_grads32(accum, accum_abs, denom)
    finite = np.where(np.isfinite(ga32), ga32, F32(np.finfo(F32).max))
    Q = F32(np.quantile(finite.astype(np.float64), 1.0 - float((np.abs(g32) >= MAX_GRAD).mean())))
    scaling = f32(math.log(0.04) + 1.2 * rng.standard_normal((P, 3)))
    opacity = f32(2.0 * rng.standard_normal(P) - 1.0)
    return _case("random", accum, accum_abs, denom, scaling, opacity, Q=Q, max_grad=MAX_GRAD, dense=F32(0.01) * F32(5.0),
                 min_opacity=F32(0.05), big=F32(0.1) * F32(5.0), rest_floats=9)


def model_for(case, seed=0, special_rotations=False):
    """the rest of a case: six parameters (opacity and scaling the case's own), non-zero moments, unit normals; float32, seeded"""
    P, rest = case.scaling.shape[0], case.rest_floats
    rng = np.random.default_rng([7, seed, P, rest])
    rn = lambda *s: f32(rng.standard_normal(s))
    params = dict(xyz=2 * rn(P, 3), f_dc=rn(P, 1, 3), f_rest=f32(0.2) * rn(P, rest // 3, 3), opacity=case.opacity.copy(),
                  scaling=case.scaling.copy(), rotation=rn(P, 4))
    if special_rotations:
        params["rotation"][0] = 0
        params["rotation"][1] = F32(1e-25)
    m = {n: f32(0.1) * rn(*p.shape) for n, p in params.items()}
    v = {n: f32(0.01) * rn(*p.shape) ** 2 + F32(1e-8) for n, p in params.items()}
    return params, m, v, rn(P, 3, 3)


# ---- statistics ----
STATS_P = (1, 255, 256, 257)
STATS_SENTINEL = F32(-12345.5)


def stats_state(P, seed):
    rng = np.random.default_rng([11, seed, P])
    st = {k: f32(rng.random((P, 1))) for k in STAT_KEYS}
    st["max_radii2D"] = f32(30 * rng.random(P))
    return st


def stats_view_case(P, seed=0):
    """one view with every special row: gradient [P,3], radii (int32), mask (bool, differs from radii > 0: a visible row of radius 0 and an
    invisible row of radius > 0 among them), the state before.  Row classes cycle with the row index, so every P has the first ones:
      0 ordinary visible   1 invisible, its five statistics NaN / Inf / sentinel   2 -0.0 components   3 denormal components
      4 Inf in x   5 NaN in y   6 NaN abs-gradient   7 visible by the mask with radius 0   8 invisible by the mask with radius > 0
      9 NaN already in accum_abs_max, ordinary gradient"""
    rng = np.random.default_rng([13, seed, P])
    grad = f32(1e-3 * rng.standard_normal((P, 3)))
    radii = rng.integers(1, 60, P).astype(np.int32)
    mask = np.ones(P, dtype=bool)
    st = stats_state(P, seed)
    cls = np.arange(P) % 10
    vals = (F32(np.nan), F32(np.inf), STATS_SENTINEL, F32(-np.inf), F32(np.nan))
    for k, val in zip(STAT_KEYS + ("max_radii2D",), vals):
        st[k].reshape(-1)[cls == 1] = val
    radii[cls == 1], mask[cls == 1] = 0, False
    grad[cls == 2] = F32(-0.0)
    grad[cls == 3] = np.array([1e-40, -3e-41, 2e-42], dtype=F32)
    for k in ("accum_abs", "accum_abs_max"):                   # from zero, so that a flushed denormal would show
        st[k].reshape(-1)[cls == 3] = 0
    grad[cls == 4, 0] = F32(np.inf)
    grad[cls == 5, 1] = F32(np.nan)
    grad[cls == 6, 2] = F32(np.nan)
    radii[cls == 7] = 0
    mask[cls == 8] = False
    st["accum_abs_max"].reshape(-1)[cls == 9] = F32(np.nan)
    return grad, radii, mask, st


def stats_reduced_case(P, seed=0):
    """view_parallel's reduced statistics: counts 0, 1, 3 by row; every fourth count-0 row carries non-zero sums (still not written); the
    state of the count-0 rows holds NaN / Inf / a sentinel on every fifth; one NaN abs-sum on a seen row where P allows"""
    rng = np.random.default_rng([17, seed, P])
    count = np.array([1, 0, 3, 0, 1, 3, 0, 0], dtype=F32)[np.arange(P) % 8]
    red = np.stack([f32(rng.random(P)) * count, f32(rng.random(P)) * count, count], axis=1).astype(F32)
    zero_rows = np.flatnonzero(count == 0)
    red[zero_rows[::4], 0], red[zero_rows[::4], 1] = F32(0.25), F32(0.75)
    radii_max = rng.integers(0, 60, P).astype(np.int32)
    st = stats_state(P, seed)
    for k, val in zip(STAT_KEYS + ("max_radii2D",), (F32(np.nan), F32(np.inf), STATS_SENTINEL, F32(-np.inf), F32(np.nan))):
        st[k].reshape(-1)[zero_rows[::5]] = val
    if P > 4:
        red[4, 1] = F32(np.nan)
    return red, radii_max, st
