"""Times the deterministic backward (RADEGS_DETERMINISTIC / radegs_backward_ordered) against the default one, in one process
on one GPU: forward + backward of one view of C2 and C5 (synth_scene.make_config), switch off and switch on.  Each leg is warm: 5 warm-up
steps, then untimed steps until 40 ms of GPU work have gone by (the settle rule of bench.py), then 20 timed steps, each between two HIP
events on the launch stream; the figure is the median.  A further 5 steps per leg run with the library's per-stage events on
(_C.profile_enable): the ordered path's split into fill (acc_zero), blend (blend_bwd), sort (ordered_sort), segment sum (ordered_sums) and
per-Gaussian tail (preprocess_bwd) -- every recorded stage boundary costs ~10 us of stream bubble, so the stages add up to more than the
step.  GPU box only.  Writes profiles/deterministic_bwd_bench.json (DETERMINISTIC_BENCH_OUT overrides the path) and prints it as one JSON
line."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "rade-gs_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
from diff_gaussian_rasterization import _C as C
from synth_scene import make_config, to_device, upstream_grads

assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda:0")
CONFIGS = os.environ.get("DETERMINISTIC_BENCH_CONFIGS", "C2,C5").split(",")
STEPS, WARMUP, SETTLE_MS = 20, 5, 40.0
BWD_STAGES = ("acc_zero", "blend_bwd", "ordered_sort", "ordered_sums", "preprocess_bwd")
res = {"steps": STEPS, "warmup": WARMUP, "settle_ms": SETTLE_MS, "configs": {}}

for name in CONFIGS:
    cpu = make_config(name)
    s = to_device(cpu, dev)
    g = {k: v.to(dev) for k, v in upstream_grads(cpu, 0).items()}
    e = torch.Tensor([])
    H, W = s.H, s.W
    last = {}

    def step():
        fw = C.rasterize_gaussians(s.bg, s.means3D, e, s.opacities, s.scales, s.rotations, 1.0, e, s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy,
                                   s.kernel_size, H, W, s.shs, s.sh_degree, s.campos, False, s.require_coord, s.require_depth, False)
        R, color, coord, mcoord, alpha, normal, depth, mdepth, radii, geom, binning, img = fw
        last["R"] = R
        return C.rasterize_gaussians_backward(s.bg, s.means3D, radii, e, s.scales, s.rotations, 1.0, e, s.viewmatrix, s.projmatrix, s.tanfovx,
                                              s.tanfovy, s.kernel_size, g["color"], g["coord"], g["mcoord"], g["depth"], g["mdepth"], g["alpha"],
                                              g["normal"], normal, s.shs, s.sh_degree, s.campos, geom, R, binning, img, alpha, s.require_coord,
                                              s.require_depth, False)

    rec = {"P": int(s.means3D.shape[0]), "width": W, "height": H, "require_coord": bool(s.require_coord)}
    for leg, on in (("default", False), ("ordered", True)):
        C.set_deterministic_backward(on)
        for _ in range(WARMUP):
            step()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(4):
            step()
        torch.cuda.synchronize(dev)
        est_ms = (time.perf_counter() - t0) * 1e3 / 4
        for _ in range(min(200, max(4, int(SETTLE_MS / max(est_ms, 1e-3)) + 1)) - 4):
            step()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(STEPS + 1)]
        marks[0].record()
        for i in range(STEPS):
            step()
            marks[i + 1].record()
        torch.cuda.synchronize(dev)
        spans = [marks[i].elapsed_time(marks[i + 1]) for i in range(STEPS)]
        C.profile_collect()
        C.profile_enable(True)
        for _ in range(5):
            step()
        torch.cuda.synchronize(dev)
        C.profile_enable(False)
        st = C.profile_collect()
        rec[leg] = {"ms_per_view_median": statistics.median(spans), "ms_per_view_min": min(spans), "ms_per_view_max": max(spans),
                    "backward_stages_ms": {k: st[k][0] / st[k][1] for k in BWD_STAGES if st.get(k, (0, 0))[1]}}
    C.set_deterministic_backward(False)
    rec["num_rendered"] = int(last["R"])
    rec["ordered_scratch_bytes"] = int(C.library().radegs_backward_ordered_scratch_bytes(rec["P"], rec["num_rendered"], int(rec["require_coord"])))
    rec["ordered_over_default"] = rec["ordered"]["ms_per_view_median"] / rec["default"]["ms_per_view_median"]
    print(json.dumps({name: rec}), flush=True)
    res["configs"][name] = rec
    del s, g
    C._ORDERED_SCRATCH.clear()
    torch.cuda.empty_cache()

out = os.environ.get("DETERMINISTIC_BENCH_OUT", os.path.join(ROOT, "profiles", "deterministic_bwd_bench.json"))
with open(out, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
