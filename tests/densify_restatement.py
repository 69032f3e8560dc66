"""Plain-torch restatement of adaptive density control as this library implements it (include/radegs.h, "Adaptive density
control"), written from that specification and not from any implementation: every decision is taken in ONE pass on the input
rows and the output is assembled segment by segment.  Device-agnostic (CPU tier: against the fixtures the reference's own
class wrote; GPU tier: the eager baseline the kernels are compared and timed against).  Also the input-margin test that lets
the tests demand row counts and row order exactly."""
import torch

PARAMS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def stats_step(stats, grad, visible, radii=None):
    """one view: stats = dict(accum, accum_abs, accum_abs_max, denom [P,1], max_radii2D [P]); returns the updated dict"""
    v = visible.reshape(-1, 1).bool()
    n = torch.sqrt(grad[:, 0:1] * grad[:, 0:1] + grad[:, 1:2] * grad[:, 1:2])
    a = grad[:, 2:3].abs()
    out = dict(accum=torch.where(v, stats["accum"] + n, stats["accum"]), accum_abs=torch.where(v, stats["accum_abs"] + a, stats["accum_abs"]),
               accum_abs_max=torch.where(v, torch.maximum(stats["accum_abs_max"], a), stats["accum_abs_max"]),
               denom=torch.where(v, stats["denom"] + 1, stats["denom"]), max_radii2D=stats["max_radii2D"])
    if radii is not None:
        out["max_radii2D"] = torch.where(v[:, 0], torch.maximum(stats["max_radii2D"], radii.float()), stats["max_radii2D"])
    return out


def stats_step_reduced(stats, reduced, radii_max=None):
    """the rank-reduced form: reduced[P,3] = sum |grad xy|, sum |grad abs|, number of ranks that saw the row"""
    v = reduced[:, 2:3] != 0
    out = dict(accum=torch.where(v, stats["accum"] + reduced[:, 0:1], stats["accum"]),
               accum_abs=torch.where(v, stats["accum_abs"] + reduced[:, 1:2], stats["accum_abs"]),
               accum_abs_max=torch.where(v, torch.maximum(stats["accum_abs_max"], reduced[:, 1:2]), stats["accum_abs_max"]),
               denom=torch.where(v, stats["denom"] + reduced[:, 2:3], stats["denom"]), max_radii2D=stats["max_radii2D"])
    if radii_max is not None:
        out["max_radii2D"] = torch.where(v[:, 0], torch.maximum(stats["max_radii2D"], radii_max.float()), stats["max_radii2D"])
    return out


def mean_grads(accum, accum_abs, denom):
    g, ga = (accum / denom).reshape(-1), (accum_abs / denom).reshape(-1)
    return torch.where(g.isnan(), torch.zeros_like(g), g), torch.where(ga.isnan(), torch.zeros_like(ga), ga)


def abs_threshold(accum, accum_abs, denom, max_grad):
    g, ga = mean_grads(accum, accum_abs, denom)
    return torch.quantile(ga, 1 - (g.abs() >= max_grad).float().mean())


def _quantities(accum, accum_abs, denom, scaling, opacity):
    g, ga = mean_grads(accum, accum_abs, denom)
    s = torch.exp(scaling)
    return g.abs(), ga, s.max(dim=1).values, torch.exp(torch.log(s / 1.6)).max(dim=1).values, torch.sigmoid(opacity).reshape(-1)


def rotation_matrices(q):
    q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


def densify(params, exp_avg, exp_avg_sq, accum, accum_abs, denom, z, Q, max_grad, min_opacity, extent, percent_dense, max_screen_size):
    """params / exp_avg / exp_avg_sq: dicts over PARAMS (a moment may be None).  Returns (params', exp_avg', exp_avg_sq',
    (cloned, split, pruned), src_rows) -- the host reads happen here freely: this is the statement, not the product."""
    gn, ga, smax, cmax, o = _quantities(accum, accum_abs, denom, params["scaling"], params["opacity"])
    T = percent_dense * extent
    hot = (gn >= max_grad) | (ga >= Q)
    clone, split = hot & (smax <= T), hot & (smax > T)
    drop, drop_child = o < min_opacity, o < min_opacity
    if max_screen_size:
        drop, drop_child = drop | (smax > 0.1 * extent), drop_child | (cmax > 0.1 * extent)
    keep = [~split & ~drop, clone & ~drop, split & ~drop_child, split & ~drop_child]
    idx = [torch.nonzero(k).reshape(-1) for k in keep]
    s = torch.exp(params["scaling"])
    R = rotation_matrices(params["rotation"])
    offs = [torch.bmm(R, (z[:, k] * s).unsqueeze(-1)).squeeze(-1) for k in range(3)]
    out_p, out_m, out_v = {}, {}, {}
    for name in PARAMS:
        x = params[name]
        segs = [x[idx[0]], x[idx[1]], x[idx[2]], x[idx[3]]]
        if name == "xyz":
            segs = [x[idx[0]]] + [x[idx[k + 1]] + offs[k][idx[k + 1]] for k in range(3)]
        if name == "scaling":
            segs[2], segs[3] = torch.log(s[idx[2]] / 1.6), torch.log(s[idx[3]] / 1.6)
        out_p[name] = torch.cat(segs, dim=0)
        n_new = sum(int(i.numel()) for i in idx[1:])
        for src, dst in ((exp_avg, out_m), (exp_avg_sq, out_v)):
            m = src.get(name) if src else None
            dst[name] = None if m is None else torch.cat([m[idx[0]], torch.zeros((n_new,) + tuple(m.shape[1:]), dtype=m.dtype, device=m.device)], dim=0)
    n_clone, n_split = int(clone.sum()), int(split.sum())
    P = int(smax.numel())
    counts = (n_clone, n_split, P + n_clone + n_split - int(out_p["xyz"].shape[0]))
    return out_p, out_m, out_v, counts, torch.cat([i + (k << 30) for k, i in enumerate(idx)])


def margins(accum, accum_abs, denom, scaling, opacity, Q, max_grad, min_opacity, extent, percent_dense, max_screen_size):
    """smallest relative gap between a compared quantity and its threshold, per comparison; a test on the INPUTS only"""
    gn, ga, smax, cmax, o = _quantities(accum, accum_abs, denom, scaling, opacity)

    def gap(v, t):
        v = v[torch.isfinite(v)].double()
        t = float(t)
        return float(((v - t).abs() / max(abs(t), 1e-30)).min()) if v.numel() else float("inf")
    m = dict(dense=gap(smax, percent_dense * extent), opacity=gap(o, min_opacity), max_grad=gap(gn, max_grad), Q=gap(ga, Q))
    if max_screen_size:
        m["big"] = min(gap(smax, 0.1 * extent), gap(cmax, 0.1 * extent))
    return m


def margin_ok(*args, rel=1e-5, **kwargs):
    return min(margins(*args, **kwargs).values()) > rel


# ---- seeded cases for the randomised sweep and the benchmark ----
DEFAULTS = dict(max_grad=0.0002, min_opacity=0.05, extent=5.0, percent_dense=0.01)


def random_decision_inputs(seed, P, hot_share=None):
    """(accum, accum_abs, denom [P,1], scaling [P,3], opacity [P,1]) as CPU tensors: a training-like state in which a few per cent
    of the rows are hot.  The distribution leaves a gap around every threshold so that the input margin (margins(), 1e-5 relative)
    holds for nearly every seed even at 200 k rows, where a smooth density would put a row inside the band almost surely:
      * |g| is <= 0.8 max_grad on cold rows and >= 1.25 max_grad on hot ones; the abs-gradient is bimodal in the same way, and as
        many rows are hot in it as in |g| (different rows), so upstream's quantile Q falls in the gap between the two modes;
      * rows whose largest scale (or its split children's) lies within 0.2 % of percent_dense * extent / 0.1 * extent, or whose
        opacity logit lies within 1e-3 of min_opacity's, are moved off by 1 % / 4e-3.
    Zeros in denom (0/0 -> 0) and up to three rows with denom = 0 < accum, accum_abs (Inf stays and selects) are part of it."""
    import math

    import numpy as np
    rng = np.random.default_rng([int(seed), int(P)])
    mg, ext, pd, mo = DEFAULTS["max_grad"], DEFAULTS["extent"], DEFAULTS["percent_dense"], DEFAULTS["min_opacity"]
    share = rng.uniform(0.02, 0.10) if hot_share is None else hot_share
    denom = rng.integers(0, 12, P).astype(np.float32)
    seen, unseen = np.flatnonzero(denom > 0), np.flatnonzero(denom == 0)
    n_hot = min(len(seen), max(1, int(round(P * share)))) if len(seen) else 0
    g = 0.8 * mg * rng.random(P)
    ga = 4.0 * mg * rng.random(P)
    if n_hot:
        g[rng.choice(seen, n_hot, replace=False)] = 1.25 * mg * np.exp(0.5 * np.abs(rng.standard_normal(n_hot)))
        ga[rng.choice(seen, n_hot, replace=False)] = 8.0 * mg * np.exp(0.5 * np.abs(rng.standard_normal(n_hot)))
    accum, accum_abs = (g * denom).astype(np.float32), (ga * denom).astype(np.float32)
    inf_rows = unseen[:3]
    accum[inf_rows], accum_abs[inf_rows] = 0.001, 0.002
    scaling = (math.log(0.04) + 1.2 * rng.standard_normal((P, 3))).astype(np.float32)
    for thr in (pd * ext, 0.1 * ext, 1.6 * 0.1 * ext):
        near = np.abs(np.exp(scaling.astype(np.float64)).max(axis=1) / thr - 1.0) < 2e-3
        scaling[near] += np.float32(0.01)
    opacity = (2.0 * rng.standard_normal((P, 1))).astype(np.float32)
    opacity[np.abs(opacity - math.log(mo / (1 - mo))) < 1e-3] += np.float32(4e-3)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return f(accum.reshape(P, 1)), f(accum_abs.reshape(P, 1)), f(denom.reshape(P, 1)), f(scaling), f(opacity)


def random_model(seed, P, sh_degree, device, decision_inputs=None):
    """the rest of a case on `device`: six parameters, non-zero moments, unit normals; returns (params, exp_avg, exp_avg_sq, z)"""
    accum, accum_abs, denom, scaling, opacity = decision_inputs if decision_inputs is not None else random_decision_inputs(seed, P)
    gen = torch.Generator(device=device).manual_seed(1000003 * int(seed) + int(P))
    rn = lambda *s: torch.randn(*s, generator=gen, device=device, dtype=torch.float32)
    M = (sh_degree + 1) ** 2
    params = dict(xyz=2.0 * rn(P, 3), f_dc=rn(P, 1, 3), f_rest=0.2 * rn(P, M - 1, 3), opacity=opacity.to(device), scaling=scaling.to(device),
                  rotation=rn(P, 4))
    m = {n: 0.1 * rn(*p.shape) for n, p in params.items()}
    v = {n: 0.01 * rn(*p.shape) ** 2 + 1e-8 for n, p in params.items()}
    return params, m, v, rn(P, 3, 3)


def sweep_cases():
    """(seed, P, sh_degree, max_screen_size) of the randomised sweep: 56 cases, P from 7 to 200 000"""
    import numpy as np
    rng = np.random.default_rng(2024)
    sizes = [63, 7, 255, 257, 2049, 200_000, 200_000, 199_999] + [int(10 ** rng.uniform(2.5, 5.3)) for _ in range(48)]
    return [(s, min(P, 200_000), (1, 3, 0, 2)[s % 4], 20 if s % 2 else None) for s, P in enumerate(sizes)]
