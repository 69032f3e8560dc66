"""Times adaptive density control at C2 scale -- P = 1 M Gaussians, SH degree 3, a few per cent of the rows hot --
against the reference formulation in eager torch (tests/densify_restatement.py) in one process on one GPU:
  * the per-iteration statistics step: GPU time per call AND host wall time of the call (the removed host waits are the point);
  * densify_and_prune: time per call, the apply kernel's own time and achieved GB/s on its algorithmic bytes
    (P_in * R * 12 read + P_out * R * 12 written, R = 59 floats), and the allocator's peak memory of both formulations.
GPU box only.  Prints one JSON line at the end."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "rade-gs_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
import densify_restatement as dr
import gaussian_model_ops as gmo

assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda:0")
P = int(os.environ.get("DENSIFY_BENCH_P", 1_000_000))
SH = 3
R = 14 + 3 * ((SH + 1) ** 2 - 1)
cfg = dict(dr.DEFAULTS, max_screen_size=20)
res = {"P": P, "sh_degree": SH, "floats_per_row": R}


def settle(seconds=1.5):
    """keep the GPU busy until its clock has settled"""
    x = torch.randn(4096, 4096, device=dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(20):
            x = (x @ x).clamp_(-1, 1)
        torch.cuda.synchronize()


def time_calls(fn, n, warm=5):
    """(GPU ms per call by events over n back-to-back calls, host wall ms per call until the call RETURNS, wall ms per call incl. the final wait)"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return e0.elapsed_time(e1) / n, (t1 - t0) * 1e3 / n, (t2 - t0) * 1e3 / n


# ------------------------------------------------------------------ statistics ------------------------------------------------------------------
class Stats:
    def __init__(self):
        for n in ("xyz_gradient_accum", "xyz_gradient_accum_abs", "xyz_gradient_accum_abs_max", "denom"):
            setattr(self, n, torch.zeros(P, 1, device=dev))
        self.max_radii2D = torch.zeros(P, device=dev)


grad = 1e-3 * torch.randn(P, 3, device=dev)
radii = (torch.randint(1, 60, (P,), device=dev, dtype=torch.int32) * (torch.rand(P, device=dev) < 0.6)).int()
sf, se = Stats(), Stats()


def stats_fused():
    gmo.add_densification_stats(sf, grad, None, radii)


def stats_eager():
    """the reference's formulation: every statement reads and writes the visible rows through boolean-mask indexing, each of
    which is a nonzero() the host waits for"""
    vis = radii > 0
    g = grad[vis]
    n_xy, n_abs = torch.sqrt(g[:, 0:1] * g[:, 0:1] + g[:, 1:2] * g[:, 1:2]), g[:, 2:3].abs()
    se.max_radii2D[vis] = torch.maximum(se.max_radii2D[vis], radii[vis].float())
    se.xyz_gradient_accum[vis] = se.xyz_gradient_accum[vis] + n_xy
    se.xyz_gradient_accum_abs[vis] = se.xyz_gradient_accum_abs[vis] + n_abs
    se.xyz_gradient_accum_abs_max[vis] = torch.maximum(se.xyz_gradient_accum_abs_max[vis], n_abs)
    se.denom[vis] = se.denom[vis] + 1


sw = dict(accum=torch.zeros(P, 1, device=dev), accum_abs=torch.zeros(P, 1, device=dev), accum_abs_max=torch.zeros(P, 1, device=dev),
          denom=torch.zeros(P, 1, device=dev), max_radii2D=torch.zeros(P, device=dev))


def stats_eager_where():
    """the same update in eager torch without any mask indexing (tests/densify_restatement.py): no host wait, ~20 kernels"""
    global sw
    sw = dr.stats_step(sw, grad, radii > 0, radii)


settle()
rounds = []
for _ in range(3):                       # alternate the two: the spread between rounds is the noise
    rounds.append((time_calls(stats_fused, 200), time_calls(stats_eager, 50), time_calls(stats_eager_where, 50)))
best = lambda k, j: min(r[k][j] for r in rounds)
res["stats"] = dict(fused_gpu_ms=best(0, 0), fused_host_call_ms=best(0, 1), fused_wall_ms=best(0, 2), eager_gpu_ms=best(1, 0), eager_host_call_ms=best(1, 1),
                    eager_wall_ms=best(1, 2), eager_where_gpu_ms=best(2, 0), eager_where_host_call_ms=best(2, 1), eager_where_wall_ms=best(2, 2),
                    rounds=[[list(x) for x in r] for r in rounds], bytes_per_row=12 + 4 + 5 * 8)
print(f"stats step, P={P}: fused {best(0, 0):.4f} ms GPU / {best(0, 1):.4f} ms host per call; eager {best(1, 0):.4f} ms GPU / {best(1, 1):.4f} ms host per call "
      f"({best(1, 2) / best(0, 2):.1f}x wall); eager without mask indexing {best(2, 0):.4f} ms GPU / {best(2, 1):.4f} ms host", flush=True)
assert torch.equal(sf.denom > 0, (radii > 0).reshape(-1, 1)) and torch.equal(sf.xyz_gradient_accum_abs_max, se.xyz_gradient_accum_abs_max)

# ------------------------------------------------------------------ densify_and_prune ------------------------------------------------------------------
inputs = dr.random_decision_inputs(7, P, hot_share=0.05)
params, m, v, z = dr.random_model(7, P, SH, dev, inputs)
accum, accum_abs, denom = (t.to(dev) for t in inputs[:3])
Q = dr.abs_threshold(accum, accum_abs, denom, cfg["max_grad"])
lst = lambda d: [d[n] for n in dr.PARAMS]
big = 0.1 * cfg["extent"]


def plan():
    return gmo.densify_plan(accum, accum_abs, denom, params["scaling"], params["opacity"], cfg["max_grad"], Q, cfg["percent_dense"] * cfg["extent"],
                            cfg["min_opacity"], big)


def fused_full():
    """what gaussian_model_ops.densify_and_prune does between the statistics and the optimizer surgery (Q included)"""
    q = dr.abs_threshold(accum, accum_abs, denom, cfg["max_grad"])
    ws, counts = gmo.densify_plan(accum, accum_abs, denom, params["scaling"], params["opacity"], cfg["max_grad"], q, cfg["percent_dense"] * cfg["extent"],
                                  cfg["min_opacity"], big)
    P_out = counts.tolist()[0]
    return gmo.densify_apply(ws, P_out, lst(params), lst(m), lst(v), z)


def eager_full():
    q = dr.abs_threshold(accum, accum_abs, denom, cfg["max_grad"])
    return dr.densify(params, m, v, accum, accum_abs, denom, z, q, **cfg)


ws, counts = plan()
P_out, cloned, split, pruned = counts.tolist()
ref = eager_full()
assert ref[3] == (cloned, split, pruned), (ref[3], cloned, split, pruned)
out = gmo.densify_apply(ws, P_out, lst(params), lst(m), lst(v), z)
assert all(torch.equal(a, ref[0][n]) for a, n in zip(out[0], dr.PARAMS) if n not in ("xyz", "scaling"))
assert all(torch.equal(a, ref[1][n]) for a, n in zip(out[1], dr.PARAMS)) and all(torch.equal(a, ref[2][n]) for a, n in zip(out[2], dr.PARAMS))
del out, ref
torch.cuda.empty_cache()


def peak(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    pk = torch.cuda.max_memory_allocated() - base
    del r
    return pk


res["densify"] = dict(P_out=P_out, cloned=cloned, split=split, pruned=pruned, peak_extra_bytes_fused=peak(fused_full), peak_extra_bytes_eager=peak(eager_full))
torch.cuda.empty_cache()
outs = [[torch.empty((P_out,) + tuple(x.shape[1:]), device=dev) for x in lst(g)] for g in (params, m, v)]
tab = gmo.RadegsDensifyTensors()
for j, g in enumerate((params, m, v)):
    for k, x in enumerate(lst(g)):
        tab.inp[6 * j + k], tab.out[6 * j + k] = x.data_ptr(), outs[j][k].data_ptr()
import ctypes
from diff_gaussian_rasterization import _C
L = gmo._lib()


def apply_only():
    rc = L.radegs_densify_apply(P, P_out, R - 14, ctypes.byref(tab), _C._ptr(z), _C._ptr(ws), _C._stream(dev))
    assert rc == 0


settle()
rounds = []
for _ in range(3):
    rounds.append((time_calls(apply_only, 100)[0], time_calls(lambda: plan(), 100)[0], time_calls(fused_full, 10, warm=2)[2], time_calls(eager_full, 10, warm=2)[2]))
apply_ms, plan_ms, fused_ms, eager_ms = (min(r[k] for r in rounds) for k in range(4))
alg_bytes = (P + P_out) * R * 12
res["densify"].update(apply_kernel_ms=apply_ms, plan_ms=plan_ms, fused_ms=fused_ms, eager_ms=eager_ms, apply_algorithmic_bytes=alg_bytes,
                      apply_GBps=alg_bytes / (apply_ms * 1e-3) / 1e9, apply_fraction_of_8TBps=alg_bytes / (apply_ms * 1e-3) / 8e12, rounds=[list(r) for r in rounds])
d = res["densify"]
print(f"densify_and_prune, P={P} -> {P_out} (cloned {cloned}, split {split}, pruned {pruned}): fused {fused_ms:.3f} ms (plan {plan_ms:.3f}, apply kernel "
      f"{apply_ms:.3f} ms = {d['apply_GBps']:.0f} GB/s on {alg_bytes / 1e6:.0f} MB = {100 * d['apply_fraction_of_8TBps']:.1f} % of 8 TB/s) vs eager {eager_ms:.3f} ms "
      f"({eager_ms / fused_ms:.1f}x); peak extra memory fused {d['peak_extra_bytes_fused'] / 1e6:.0f} MB, eager {d['peak_extra_bytes_eager'] / 1e6:.0f} MB", flush=True)
print(json.dumps(res))
