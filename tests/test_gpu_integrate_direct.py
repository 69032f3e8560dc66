"""The integrate kernels (points_preprocess_kernel, the counting sort, integrate_kernel: csrc/rg_integrate.inc) against the float32 chain (a)
and the float64 restatement (b) of tests/integrate_cases.py, on the MI355X.

Per case ONE call of _C.integrate_gaussians_to_points under KEEP_ACC; the records that launch READ (splat_a, ranges, point_list through
debug_export; inte_rec, p2d, pdepth, ppix, pt_sorted, pix_incl through debug_export_points) go through (a) and (b) once (module cache).
  exact, against (a):  n_contrib plane 0 == last and plane 1 == 0; out9[8]; ppix; pix_incl; pix_count all zero after the scatter; pt_sorted a
                       permutation of the projected ids with every id inside its own pixel's range; p2d, pdepth and out_coordinate2d bit for
                       bit at the projected points (against project32 of the points); unprojected points keep the initial values;
                       color_integrated is the kernel's own pixel colour
  inside 2 C_INT of (b): out9 planes 0-4, 6 and 7; final_T; alpha_integrated, color_integrated and sdf
Which phase-2 form a tile took is named by its list's length (<= 768: the used bits, point-major; longer: the replay): no switch exists, and
`reach` holds both (`cap` only replays).  The number of float32 words that differ from (a) and the largest difference in ulps are printed per output,
not asserted.  Measured on the MI355X (profiles/integrate_direct_margins.txt): 0 differing words, 0 ulps, in every output of every case
(cap 0/5376 0/768 0/60 0/180 0/60 words of out9 / final_T / alpha_integrated / color_integrated / sdf, reach 0/16128 0/2304 0/2703 0/8109
0/2703, band 0/28672 0/4096 0/4000 0/12000 0/4000, step 0/7168 0/1024 0/1020 0/3060 0/1020, edges 0/19215 0/2745 0/329 0/987 0/329): the
kernels need exactly what chain (a) needs, at worst c = 0.620 (plane 7 of `step`) of the 1.24 allowed.  With the reject test of
points_preprocess_kernel in its earlier form (`ix < 0 || ...`, which a NaN passes) `edges` alone failed, at its three non-finite points only:
ppix 0 instead of 0xFFFFFFFF for points 326, 327, 328, alpha_integrated 0 instead of 1 (c = inf), and the condition "the non-finite points
are not projected"; 12 of the 15 tests passed.

RADEGS_INTEGRATE_MARGINS=<file>: the c every case and output needed is written there when the module finishes."""
import os

import numpy as np
import pytest
import torch

import integrate_cases as ic

pytestmark = pytest.mark.gpu

BOUND = 2 * ic.C_INT
MARGINS, ULPS = {}, {}


class Launch:
    """one integrate call of one case, and what it left"""


@pytest.fixture(scope="module")
def cache():
    store = {}
    yield store
    path = os.environ.get("RADEGS_INTEGRATE_MARGINS")
    if path and MARGINS:
        with open(path, "w") as f:
            f.write(f"C_INT = {ic.C_INT} (integrate_cases.py: what chain (a) needs against (b) over all cases); the kernels' bound is 2 C_INT = {BOUND}\n")
            f.write("c needed per case and output; then float32 words that differ from chain (a) / of how many (largest difference in ulps)\n")
            for case, c in MARGINS.items():
                worst = max(c, key=c.get)
                f.write(f"{case:8s} worst {worst} {c[worst]:.3f} | " + " ".join(f"{k} {v:.3f}" for k, v in c.items()) + "\n")
                f.write(f"{case:8s} " + " ".join(f"{k} {d}/{n} ({u})" for k, (d, n, u) in ULPS[case].items()) + "\n")


def launch(cache, name):
    if name in cache:
        return cache[name]
    import diff_gaussian_rasterization._C as C
    from synth_scene import to_device
    assert torch.cuda.is_available(), "these tests need the MI355X box"
    s, pts = ic.CASES[name].build()
    assert s.kernel_size == 0.0
    dev = torch.device("cuda:0")
    d = to_device(s, dev)
    p = torch.from_numpy(pts).to(dev)
    e = torch.Tensor([])
    L = Launch()
    L.s, L.pts = s, pts
    keep = C.KEEP_ACC
    C.KEEP_ACC = True
    try:
        st = C.integrate_gaussians_to_points(d.bg, p, d.means3D, e, d.opacities, d.scales, d.rotations, 1.0, e, e, d.viewmatrix, d.projmatrix,
                                             s.tanfovx, s.tanfovy, 0.0, None, s.H, s.W, d.shs, s.sh_degree, d.campos, False, False)
        torch.cuda.synchronize()
        L.inp = ic.input_from_hip(C, s, len(pts), st)
        L.n_contrib = C.debug_export("n_contrib", torch.int32, 2 * s.H * s.W, s.means3D.shape[0], st[0], s.W, s.H, False, st[7], st[8],
                                     st[9]).cpu().numpy().view(np.uint32).reshape(2, s.H, s.W)
    finally:
        C.KEEP_ACC = keep
        C.LAST_POINT_STATE = None
    out9, ai, ci, c2, sdf = (t.cpu().numpy() for t in st[1:6])
    L.got = dict(out9=out9, final_T=L.inp.final_T, alpha_integrated=ai, color_integrated=ci, coordinate2d=c2, sdf=sdf, n_contrib=L.n_contrib)
    L.dec = ic.decide(L.inp)
    L.w = ic.walk32(L.inp, L.dec)
    L.ref = ic.restate64(L.inp, L.dec, L.w)
    cache[name] = L
    return L


def ulps(a, b):
    """(words that differ, words, largest difference in ulps) of two float32 arrays of finite numbers"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b))
    return int((d != 0).sum()), int(d.size), int(d.max()) if d.size else 0


@pytest.mark.parametrize("name", list(ic.CASES))
def test_conditions_hold_on_the_kernels_records(cache, name):
    L = launch(cache, name)
    cond = ic.CASES[name].conditions(L.inp, L.dec, L.w)
    assert cond and all(cond.values()), [k for k, v in cond.items() if not v]
    forms = {"cached": bool((L.inp.n <= ic.BITS_REACH).any()), "replay": bool((L.inp.n > ic.BITS_REACH).any())}
    print(f"{name}: phase-2 forms by list length {forms}")
    if name in ("cap", "reach"):
        assert forms["replay"] and (forms["cached"] or name == "cap"), forms


@pytest.mark.parametrize("name", list(ic.CASES))
def test_exact_against_chain_a(cache, name):
    L = launch(cache, name)
    inp, s = L.inp, L.s
    # the projection, the bins and the sort
    p2d, pdepth, ppix = ic.project32(L.pts, s.viewmatrix.numpy().reshape(-1), *ic.focal32(s), s.W, s.H)
    bad = np.flatnonzero(inp.ppix != ppix)
    assert not len(bad), (f"ppix of point {bad[0]} {L.pts[bad[0]].tolist()}: kernel {int(inp.ppix[bad[0]]):#x}, project32 {int(ppix[bad[0]]):#x}; "
                          f"{len(bad)} points: {bad[:8].tolist()}")
    proj = inp.projected
    assert np.array_equal(inp.p2d[proj].view(np.uint32), p2d[proj].view(np.uint32)), "p2d at the projected points"
    assert np.array_equal(inp.pdepth[proj].view(np.uint32), pdepth[proj].view(np.uint32)), "pdepth at the projected points"
    _, incl = ic.bins_of(ppix, s.W, s.H)
    assert np.array_equal(inp.pix_incl, incl), "pix_incl"
    assert not inp.pix_count.any(), "pix_count is not all zero after the scatter"
    assert np.array_equal(np.sort(inp.pt_sorted), np.flatnonzero(proj)), "pt_sorted is no permutation of the projected ids"
    first = np.concatenate([[0], incl[:-1].astype(np.int64)])
    pix_of_slot = inp.ppix[inp.pt_sorted].astype(np.int64)
    slot = np.arange(len(inp.pt_sorted))
    assert ((slot >= first[pix_of_slot]) & (slot < incl[pix_of_slot])).all(), "an id of pt_sorted outside its own pixel's range"
    # the walk
    wrong = ic.exact_differences(inp, L.dec, L.w, L.got)
    assert not wrong, wrong
    q = L.w.q
    own = L.got["out9"][0:3, inp.ppix[q] // s.W, inp.ppix[q] % s.W].T
    assert np.array_equal(L.got["color_integrated"][q].view(np.uint32), own.view(np.uint32)), "color_integrated is not the kernel's own pixel colour"


@pytest.mark.parametrize("name", list(ic.CASES))
def test_inside_two_c_int_of_the_restatement(cache, name):
    L = launch(cache, name)
    for k in ("out9", "alpha_integrated", "color_integrated", "sdf", "final_T"):
        assert np.isfinite(L.got[k]).all(), f"{k} is not finite"
    c = ic.need(L.got, L.ref)
    a = ic.chain_outputs(L.dec, L.w)
    ULPS[name] = {k: ulps(L.got[k][list(ic.PLANES)] if k == "out9" else L.got[k], a[k][list(ic.PLANES)] if k == "out9" else a[k]) for k in ic.OUTPUTS}
    MARGINS[name] = c
    print(f"{name}: " + " ".join(f"{k} {v:.3f}" for k, v in c.items()))
    print(f"{name}: words differing from chain (a) / of (largest ulps): " + " ".join(f"{k} {d}/{n} ({u})" for k, (d, n, u) in ULPS[name].items()))
    worst = max(c, key=c.get)
    assert c[worst] <= BOUND, f"{name}: {worst} needs c = {c[worst]:.3g} > 2 C_INT = {BOUND}"
