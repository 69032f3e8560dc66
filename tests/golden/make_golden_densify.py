"""Generates tests/golden/densify_sh1{,_in,_out}.npz, densify_sh3{,_in,_out}.npz and densify_stats.npz from the REFERENCE's own GaussianModel
(/root/reference/scene/gaussian_model.py: densify_and_prune 717-741, add_densification_stats 743-747, and train.py:186's
max_radii2D update) run on the CPU.  Build container only.

The module's unavailable imports are stubbed and the object is created without __init__, as make_golden_filter3d.py does.
Additionally `device="cuda"` factory calls are routed to the CPU, and torch.normal is replaced by a function that returns the
matching rows of a RECORDED array z[P,3,3] of standard-normal draws times `std` -- slot 0 for the clone, slots 1 / 2 for the two
split children (upstream draws (n_clone,3), then (2 n_split,3) in repeat(2,1) order: all first children, then all second).

Decisions sit on thresholds and exp / sigmoid differ by an ulp between libraries, so this script ASSERTS that no compared
quantity lies within 1e-5 relative of its threshold (and that Q lies strictly between two neighbouring order statistics) and
prints the smallest gaps: a condition on the inputs that lets the tests demand row counts and row order exactly.  On a failed
assertion change the seed, never the margin."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import densify_restatement as dr  # noqa: E402  (only its margin test: the data below comes from the reference alone)

for name, attrs in {"plyfile": ("PlyData", "PlyElement"), "simple_knn": (), "simple_knn._C": ("distCUDA2",), "trimesh": (), "cv2": ()}.items():
    m = types.ModuleType(name)
    for a in attrs:
        setattr(m, a, None)
    sys.modules.setdefault(name, m)
sys.path.insert(0, "/root/reference")
pkg = types.ModuleType("scene")            # keep scene/__init__.py (dataset readers, PIL, ...) from running
pkg.__path__ = ["/root/reference/scene"]
sys.modules["scene"] = pkg
from scene.gaussian_model import GaussianModel  # noqa: E402

for fn in ("zeros", "ones", "empty", "full", "tensor", "rand", "randn"):   # device="cuda" -> CPU
    def _route(*a, __f=getattr(torch, fn), **k):
        if str(k.get("device", "")).startswith("cuda"):
            k.pop("device")
        return __f(*a, **k)
    setattr(torch, fn, _route)

GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"), ("scaling", "_scaling"),
          ("rotation", "_rotation"))
MAX_GRAD, MIN_OPACITY, EXTENT, PERCENT_DENSE = 0.0002, 0.05, 5.0, 0.01


def make_model(P, sh_degree, rng):
    gm = object.__new__(GaussianModel)
    gm.setup_functions()
    gm.percent_dense = PERCENT_DENSE
    M = (sh_degree + 1) ** 2
    init = dict(_xyz=rng.standard_normal((P, 3)) * 2.0, _features_dc=rng.standard_normal((P, 1, 3)), _features_rest=0.2 * rng.standard_normal((P, M - 1, 3)),
                _opacity=2.0 * rng.standard_normal((P, 1)), _scaling=np.log(0.04) + 1.2 * rng.standard_normal((P, 3)),
                _rotation=rng.standard_normal((P, 4)))
    for k, v in init.items():
        setattr(gm, k, torch.nn.Parameter(torch.from_numpy(v.astype(np.float32))))
    gm.optimizer = torch.optim.Adam([{"params": [getattr(gm, a)], "lr": 1e-3, "name": n} for n, a in GROUPS], lr=0.0, eps=1e-15)
    for _ in range(2):                      # two real steps: non-zero moments, step = 2
        for _, a in GROUPS:
            p = getattr(gm, a)
            p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32))
        gm.optimizer.step()
    gm.optimizer.zero_grad(set_to_none=True)
    denom = rng.integers(0, 12, (P, 1)).astype(np.float32)            # zeros included: 0/0 = NaN -> 0
    accum = denom * MAX_GRAD * np.exp(0.9 * rng.standard_normal((P, 1)) - 0.9).astype(np.float32)
    accum_abs = denom * 4 * MAX_GRAD * np.exp(0.9 * rng.standard_normal((P, 1))).astype(np.float32)
    seen = np.flatnonzero(denom[:, 0] == 0)[:4]
    accum[seen[:3]] = 0.001                                           # denom = 0 < accum: Inf stays and selects
    accum_abs[seen[1:4]] = 0.002
    gm.xyz_gradient_accum = torch.from_numpy(accum.astype(np.float32))
    gm.xyz_gradient_accum_abs = torch.from_numpy(accum_abs.astype(np.float32))
    gm.xyz_gradient_accum_abs_max = torch.from_numpy((accum_abs * 0.5).astype(np.float32))
    gm.denom = torch.from_numpy(denom)
    gm.max_radii2D = torch.from_numpy((1000.0 * rng.random(P)).astype(np.float32))   # the dead term: far above max_screen_size
    return gm


def snapshot(gm, prefix):
    d = {}
    for n, a in GROUPS:
        p = getattr(gm, a)
        st = gm.optimizer.state[p]
        d[f"{prefix}_{n}"] = p.detach().numpy().copy()
        d[f"{prefix}_exp_avg_{n}"] = st["exp_avg"].numpy().copy()
        d[f"{prefix}_exp_avg_sq_{n}"] = st["exp_avg_sq"].numpy().copy()
        d[f"{prefix}_step_{n}"] = np.asarray(float(st["step"]))
    return d


def densify_fixture(path, P, sh_degree, max_screen_size, seed):
    rng = np.random.default_rng(seed)
    gm = make_model(P, sh_degree, rng)
    z = rng.standard_normal((P, 3, 3)).astype(np.float32)
    data = snapshot(gm, "in")
    stats = dict(accum=gm.xyz_gradient_accum.clone(), accum_abs=gm.xyz_gradient_accum_abs.clone(), denom=gm.denom.clone())
    data.update(accum=stats["accum"].numpy(), accum_abs=stats["accum_abs"].numpy(), denom=stats["denom"].numpy(),
                accum_abs_max=gm.xyz_gradient_accum_abs_max.numpy().copy(), max_radii2D=gm.max_radii2D.numpy().copy(), z=z)
    Q = dr.abs_threshold(stats["accum"], stats["accum_abs"], stats["denom"], MAX_GRAD)
    # ---- the margin condition on the inputs ----
    m = dr.margins(stats["accum"], stats["accum_abs"], stats["denom"], gm._scaling.detach(), gm._opacity.detach(), Q, MAX_GRAD, MIN_OPACITY, EXTENT,
                   PERCENT_DENSE, max_screen_size)
    print(os.path.basename(path), "smallest relative gaps to the thresholds:", {k: f"{v:.3e}" for k, v in m.items()})
    assert min(m.values()) > 1e-5, "a compared quantity within 1e-5 of its threshold: change the seed"
    _, ga = dr.mean_grads(stats["accum"], stats["accum_abs"], stats["denom"])
    srt = torch.sort(ga).values
    k = int(torch.searchsorted(srt, Q))
    assert 0 < k < P and float(srt[k - 1]) < float(Q) < float(srt[k]), "Q on an order statistic: change the seed"
    # ---- torch.normal := recorded z * std, rows found by their std (= exp(_scaling) of the selected source row) ----
    s0 = torch.exp(gm._scaling.detach()).numpy().astype(np.float64)
    calls = []

    def rows_of(std):
        d = np.abs(std.numpy().astype(np.float64)[:, None, :] - s0[None, :, :]).max(axis=2) / np.abs(s0).max(axis=1)[None, :]
        idx = d.argmin(axis=1)
        assert (d[np.arange(len(idx)), idx] < 1e-6).all() and (np.sort(d, axis=1)[:, 1] > 1e-4).all()
        return idx

    def fake_normal(mean, std):
        n = std.shape[0]
        if not calls:
            idx = rows_of(std)
            out = torch.from_numpy(z[idx, 0]) * std
        else:
            assert n % 2 == 0
            idx = rows_of(std[:n // 2])
            assert np.array_equal(idx, rows_of(std[n // 2:]))
            out = torch.cat([torch.from_numpy(z[idx, 1]), torch.from_numpy(z[idx, 2])]) * std
        assert (np.diff(idx) > 0).all()
        calls.append(idx)
        return mean + out
    real_normal, torch.normal = torch.normal, fake_normal
    try:
        with torch.no_grad():
            ret = gm.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size)
    finally:
        torch.normal = real_normal
    assert len(calls) == 2 and (len(calls[0]), len(calls[1])) == ret[:2]
    data.update(snapshot(gm, "out"))
    data.update(Q=np.asarray(float(Q), dtype=np.float32), ret=np.asarray(ret, dtype=np.int64), sh_degree=np.asarray(sh_degree),
                max_screen_size=np.asarray(-1 if max_screen_size is None else max_screen_size), max_grad=np.asarray(MAX_GRAD),
                min_opacity=np.asarray(MIN_OPACITY), extent=np.asarray(EXTENT), percent_dense=np.asarray(PERCENT_DENSE),
                out_stats_rows=np.asarray([gm.xyz_gradient_accum.shape[0], gm.denom.shape[0], gm.max_radii2D.shape[0]]))
    assert float(gm.xyz_gradient_accum.abs().sum() + gm.denom.abs().sum() + gm.max_radii2D.abs().sum()) == 0.0
    # three parts, so that every committed file stays below 1 MiB: statistics + z + settings | input model | output model
    sizes = []
    for part, pick in (("", lambda k: not k.startswith(("in_", "out_"))), ("_in", lambda k: k.startswith("in_")), ("_out", lambda k: k.startswith("out_"))):
        f = path[:-4] + part + ".npz"
        np.savez_compressed(f, **{k: v for k, v in data.items() if pick(k)})
        sizes.append(os.path.getsize(f))
        assert sizes[-1] < (1 << 20), (f, sizes[-1])
    print("  ", P, "->", gm._xyz.shape[0], "rows; (cloned, split, pruned) =", ret, "; Q =", float(Q), ";", sizes, "bytes")


def stats_fixture(path, P, seed):
    rng = np.random.default_rng(seed)
    gm = object.__new__(GaussianModel)
    gm.xyz_gradient_accum = torch.zeros((P, 1))
    gm.xyz_gradient_accum_abs = torch.zeros((P, 1))
    gm.xyz_gradient_accum_abs_max = torch.zeros((P, 1))
    gm.denom = torch.zeros((P, 1))
    gm.max_radii2D = torch.zeros(P)
    data = {}
    for v in range(3):
        grad = (1e-3 * rng.standard_normal((P, 3)) * np.exp(rng.standard_normal((P, 1)))).astype(np.float32)
        grad[:, 2] = np.abs(grad[:, 2]) * (1.0 if v else -1.0)       # a signed third column in the first view: |.| is part of the contract
        radii = (rng.integers(0, 60, P) * (rng.random(P) < 0.6)).astype(np.int32)
        vis = radii > 0
        if v == 1:                                                   # an explicit mask that is NOT radii > 0
            vis = vis & (rng.random(P) < 0.7)
        holder = types.SimpleNamespace(grad=torch.from_numpy(grad))
        mask = torch.from_numpy(vis)
        with torch.no_grad():
            gm.max_radii2D[mask] = torch.max(gm.max_radii2D[mask], torch.from_numpy(radii)[mask])
            gm.add_densification_stats(holder, mask)
        data.update({f"grad{v}": grad, f"radii{v}": radii, f"mask{v}": vis, f"accum{v}": gm.xyz_gradient_accum.numpy().copy(),
                     f"accum_abs{v}": gm.xyz_gradient_accum_abs.numpy().copy(), f"accum_abs_max{v}": gm.xyz_gradient_accum_abs_max.numpy().copy(),
                     f"denom{v}": gm.denom.numpy().copy(), f"max_radii2D{v}": gm.max_radii2D.numpy().copy()})
    np.savez_compressed(path, **data)
    print(os.path.basename(path), P, "rows, 3 views;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    densify_fixture(os.path.join(HERE, "densify_sh1.npz"), 3000, 1, 20, seed=1)
    densify_fixture(os.path.join(HERE, "densify_sh3.npz"), 1500, 3, None, seed=2)
    stats_fixture(os.path.join(HERE, "densify_stats.npz"), 2000, seed=3)
