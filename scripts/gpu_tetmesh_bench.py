"""Times mesh extraction in one process on one GPU:
  * marching tetrahedra, plan + emit, at V = 9 M / T = 58 M (a scene of 1 M Gaussians: 9 points each, 6-7 tets per point) and at
    V = 900 k / T = 5.8 M, on the random topology of tests/tetmesh_restatement.py::random_case (generated on the device here), against the
    reference's formulation in eager torch (tests/tetmesh_restatement.py::marching_unique_torch) on the same GPU where it fits, and on the
    CPU with 16 threads at the smaller size; the outputs of the two GPU paths are compared exactly;
  * one view of the cull-alpha accumulation at PN = 9 M, fused against its eager torch form.
GPU times are HIP events around back-to-back calls; GB/s are the bytes each stage moves BY DESIGN (the formulas below), not counters.
GPU box only.  Writes profiles/tetmesh_bench.json (TETMESH_BENCH_OUT overrides the path) and prints it as one JSON line."""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "rade-gs_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
import tetmesh
import tetmesh_restatement as tr
from diff_gaussian_rasterization import _C

assert torch.cuda.is_available(), "needs the GPU"
dev = torch.device("cuda:0")
SIZES = [tuple(int(x) for x in s.split(":")) for s in os.environ.get("TETMESH_BENCH_SIZES", "900000:5800000,9000000:58000000").split(",")]
CPU_MAX_T = int(os.environ.get("TETMESH_BENCH_CPU_MAX_T", 6_000_000))
PN = int(os.environ.get("TETMESH_BENCH_PN", 9_000_000))
res = {"sizes": []}
L = tetmesh._lib()


def settle(seconds=1.5):
    """keep the GPU busy until its clock has settled"""
    x = torch.randn(4096, 4096, device=dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(20):
            x = (x @ x).clamp_(-1, 1)
        torch.cuda.synchronize()


def gpu_ms(fn, n, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def wall_ms(fn, n, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        r = fn()
        torch.cuda.synchronize()
        del r
    return (time.perf_counter() - t0) * 1e3 / n


def random_case(V, T, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    base = torch.randint(0, V, (T, 1), device=dev, generator=g)
    tets = torch.cat([base, base + torch.cumsum(torch.randint(1, 40, (T, 3), device=dev, generator=g), 1)], 1) % V
    tets = torch.gather(tets, 1, torch.argsort(torch.rand((T, 4), device=dev, generator=g), dim=1)).int().contiguous()
    sdf = torch.randn(V, device=dev, generator=g)
    sdf[torch.rand(V, device=dev, generator=g) < 0.6] = -100.0
    sdf[torch.randint(0, V, (5,), device=dev, generator=g)] = 0.0
    return torch.randn((V, 3), device=dev, generator=g), tets, sdf, torch.rand(V, device=dev, generator=g)


for V, T in SIZES:
    vertices, tets, sdf, scales = random_case(V, T, 1)
    nbytes = L.radegs_tetmesh_plan_bytes(V, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    stream = _C._stream(dev)

    def plan():
        rc = L.radegs_tetmesh_plan(V, T, _C._ptr(tets), _C._ptr(sdf), _C._ptr(ws), nbytes, _C._ptr(counts), stream)
        assert rc == 0, rc
    plan()
    nv, nf = counts.tolist()
    outs = (torch.empty((nv, 2, 3), device=dev), torch.empty((nv, 2, 1), device=dev), torch.empty((nv, 2, 1), device=dev),
            torch.empty((nf, 3), dtype=torch.int64, device=dev), torch.empty((nv, 2), dtype=torch.int64, device=dev))

    def emit():
        rc = L.radegs_tetmesh_emit(V, T, _C._ptr(tets), _C._ptr(sdf), _C._ptr(vertices), _C._ptr(scales), _C._ptr(ws), nv, nf, _C._ptr(outs[0]),
                                   _C._ptr(outs[1]), _C._ptr(outs[2]), _C._ptr(outs[3]), _C._ptr(outs[4]), stream)
        assert rc == 0, rc
    emit()
    # sizes the byte formulas need (read back once, outside the timed windows)
    occ = sdf > 0
    o = occ[tets.long().reshape(-1)].reshape(-1, 4).sum(1)
    crossing_tets = int(((o > 0) & (o < 4)).sum())
    E = int((o * (4 - o)).sum())                                   # k inside corners, 4 - k outside: k (4 - k) crossing edges
    del occ, o
    cap, bits = 4 * T, max(1, (V - 1).bit_length())
    passes = (bits + 7) // 8
    sort_bytes = passes * E * (4 + 8 + 8)                          # per 8-bit pass: histogram reads keys, scatter reads and writes keys + values
    plan_bytes = (4 * V + V // 8                                   # occupancy mask
                  + T * (16 + 12 + 1) + 3 * T * 16                 # classify; scan of the 3 T flags (read, gathered copy, read, write)
                  + T * 5 + crossing_tets * 16 + E * 8             # emit_edges
                  + 2 * sort_bytes + E * 12                        # two sorts and the gather between them
                  + cap * 4 + E * 16 + cap * 16 + E * 12)          # head flags, their scan over the capacity, scatter of the ids
    emit_bytes = (E * 4 + nv * (12 + 16 + 2 * 20 + 40)             # vertex_kernel: flags; ids + keys, interp_v, two gathered rows, the written rows
                  + T * 1 + crossing_tets * (12 + 16) + nf * 24)   # face_kernel
    settle()
    rounds = []
    for _ in range(3):
        rounds.append((gpu_ms(plan, 5), gpu_ms(emit, 5)))
    plan_ms, emit_ms = min(r[0] for r in rounds), min(r[1] for r in rounds)

    def hip_full():
        return tetmesh.marching_tetrahedra(vertices[None], tets, sdf[None], scales[None])

    def eager_full():
        return tr.marching_unique_torch(vertices, tets, sdf, scales)
    rec = dict(V=V, T=T, crossing_tets=crossing_tets, crossing_edge_instances=E, n_verts=nv, n_faces=nf, workspace_bytes=nbytes, sort_passes_per_key=passes,
               plan_ms=plan_ms, emit_ms=emit_ms, plan_design_bytes=plan_bytes, emit_design_bytes=emit_bytes,
               plan_GBps=plan_bytes / (plan_ms * 1e-3) / 1e9, emit_GBps=emit_bytes / (emit_ms * 1e-3) / 1e9, rounds=[list(r) for r in rounds])
    rec["hip_wall_ms"] = wall_ms(hip_full, 3)                      # allocation, index-range check, the one host read and both calls
    del ws
    torch.cuda.empty_cache()
    try:
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ref = eager_full()
        torch.cuda.synchronize()
        rec["eager_gpu_peak_extra_bytes"] = torch.cuda.max_memory_allocated() - base
        same = all(torch.equal(a.reshape(b.shape), b) for a, b in zip(outs, ref))
        rec["hip_equals_eager_gpu"] = bool(same)
        del ref
        rec["eager_gpu_wall_ms"] = wall_ms(eager_full, 2, warm=0)
        rec["eager_gpu_over_hip"] = rec["eager_gpu_wall_ms"] / rec["hip_wall_ms"]
    except torch.cuda.OutOfMemoryError as e:
        rec["eager_gpu_wall_ms"] = None
        rec["eager_gpu_note"] = "did not fit: " + str(e).split("\n")[0]
    torch.cuda.empty_cache()
    if T <= CPU_MAX_T:
        torch.set_num_threads(16)
        c = [t.cpu() for t in (vertices, tets, sdf, scales)]
        t0 = time.perf_counter()
        ref = tr.marching_unique_torch(*c)
        rec["eager_cpu16_wall_ms"] = (time.perf_counter() - t0) * 1e3
        rec["hip_equals_eager_cpu"] = bool(all(torch.equal(a.cpu().reshape(b.shape), b) for a, b in zip(outs, ref)))
        del ref, c
    print(json.dumps(rec), flush=True)
    res["sizes"].append(rec)
    del vertices, tets, sdf, scales, outs, counts
    torch.cuda.empty_cache()

# ------------------------------------------------------------ one view of the cull-alpha accumulation ------------------------------------------------------------
W, H = 1920, 1080
g = torch.Generator(device=dev).manual_seed(2)
alpha = torch.rand(PN, device=dev, generator=g)
coord = torch.stack([torch.rand(PN, device=dev, generator=g) * (1.4 * W) - 0.2 * W, torch.rand(PN, device=dev, generator=g) * (1.4 * H) - 0.2 * H], 1).contiguous()
render = torch.zeros((9, H, W), device=dev)
render[7] = (torch.rand((H, W), device=dev, generator=g) < 0.8).float()
gt = (torch.rand((1, H, W), device=dev, generator=g) < 0.9).float()
view = type("View", (), dict(image_width=W, image_height=H, gt_mask=gt))()
acc = tetmesh.CullAlpha(PN, dev)
state = dict(final=torch.ones(PN, device=dev), weight=torch.zeros(PN, dtype=torch.int32, device=dev))


def cull_fused():
    acc.add_view((render, alpha, None, coord, None, None), view)


def cull_eager():
    """the per-view work of the reference's loop in eager torch: normalise the coordinates (on a copy: the reference owns a fresh tensor per
    view), multiply the masks, sample, compare, two selects"""
    pc = coord.clone()
    pc[:, 0] = (pc[:, 0] * 2 + 1) / (W - 1) - 1
    pc[:, 1] = (pc[:, 1] * 2 + 1) / (H - 1) - 1
    m = render[7][None] * gt
    prob = torch.nn.functional.grid_sample(m[None], pc[None, None], padding_mode="zeros", align_corners=False)[0, 0, 0]
    valid = prob > 0.5
    state["final"] = torch.where(valid, torch.min(alpha, state["final"]), state["final"])
    state["weight"] = torch.where(valid, state["weight"] + 1, state["weight"])


cull_fused()
cull_eager()
# binary masks put samples exactly on 0.5, where the two bilinear formulas may round apart: a count, not a condition
res["cull_alpha"] = dict(PN=PN, width=W, height=H, weight_mismatches=int((acc.weight != state["weight"]).sum()),
                         final_mismatches=int((acc.final_sdf != state["final"]).sum()))
settle()
rounds = []
for _ in range(3):
    rounds.append((gpu_ms(cull_fused, 50), gpu_ms(cull_eager, 20)))
fused_ms, eager_ms = min(r[0] for r in rounds), min(r[1] for r in rounds)
cull_bytes = PN * (8 + 4 + 4 + 4 + 4 + 4)                           # coordinate, alpha, final_sdf and weight read; both written where valid
res["cull_alpha"].update(fused_ms=fused_ms, eager_ms=eager_ms, eager_over_fused=eager_ms / fused_ms, design_bytes=cull_bytes,
                         fused_GBps=cull_bytes / (fused_ms * 1e-3) / 1e9, rounds=[list(r) for r in rounds])
out = os.environ.get("TETMESH_BENCH_OUT", os.path.join(ROOT, "profiles", "tetmesh_bench.json"))
with open(out, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
