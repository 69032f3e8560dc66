"""GPU tier of adaptive density control: the HIP kernels and their Python layer against the fixtures the reference's
own GaussianModel wrote (tests/golden/make_golden_densify.py) and against tests/densify_restatement.py run in eager torch on the
same GPU.  Exact: output count, upstream's 3-tuple, row order, every copied parameter, every moment, zero moments on new rows,
`step`, the re-created statistics.  Computed xyz' / _scaling': 1e-5 abs / 1e-4 rel."""
import os
import warnings
from collections import namedtuple

import math
import numpy as np
import pytest
import torch

import densify_restatement as dr
from test_densify_golden import GOLDEN, check_against_fixture, fixture_args, load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATTR = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")
STATS = ("xyz_gradient_accum", "xyz_gradient_accum_abs", "xyz_gradient_accum_abs_max", "denom")


class Model:
    """stand-in with upstream's attribute names (scene/gaussian_model.py): six parameters, five statistics, percent_dense, optimizer"""

    def __init__(self, params, accum, accum_abs, denom, percent_dense, opt_cls, exp_avg=None, exp_avg_sq=None, step=2.0, stateless=(),
                 extra_group=False):
        P = params["xyz"].shape[0]
        dev = params["xyz"].device
        for n, a in ATTR.items():
            setattr(self, a, torch.nn.Parameter(params[n].clone().contiguous()))
        groups = [{"params": [getattr(self, a)], "lr": 1e-3, "name": n} for n, a in ATTR.items()]
        if extra_group:
            self.net = torch.nn.Parameter(torch.randn(5, 7, device=dev))
            groups.append({"params": [self.net], "lr": 1e-3, "name": "appearance_network"})
        self.optimizer = opt_cls(groups, lr=0.0, eps=1e-15)
        for n, a in ATTR.items():
            if exp_avg is not None and n not in stateless:
                self.optimizer.state[getattr(self, a)] = dict(step=torch.tensor(step), exp_avg=exp_avg[n].clone(), exp_avg_sq=exp_avg_sq[n].clone())
        if extra_group:
            self.optimizer.state[self.net] = dict(step=torch.tensor(step), exp_avg=torch.ones_like(self.net), exp_avg_sq=torch.ones_like(self.net))
        self.xyz_gradient_accum, self.xyz_gradient_accum_abs, self.denom = accum.clone(), accum_abs.clone(), denom.clone()
        self.xyz_gradient_accum_abs_max = accum_abs.clone() * 0.5
        self.max_radii2D = torch.full((P,), 1000.0, device=dev)    # the dead term: would prune everything if it lived
        self.percent_dense = percent_dense
        self.filter_3D = torch.full((P, 1), 0.002, device=dev)


def optimizers():
    import fused_adam
    return [fused_adam.Adam, torch.optim.Adam]


def within_bar(a, b):
    return bool(((a.double() - b.double()).abs() <= 1e-5 + 1e-4 * b.double().abs()).all())


def compare_with_restatement(out_p, out_m, out_v, ref_p, ref_m, ref_v, src):
    """fused against the eager restatement, on the device: exact but for the displaced xyz rows and the children's _scaling rows"""
    seg = src >> 30
    for n in dr.PARAMS:
        a, b = out_p[n], ref_p[n]
        assert a.shape == b.shape, (n, a.shape, b.shape)
        if n == "xyz":
            assert torch.equal(a[seg == 0], b[seg == 0]) and within_bar(a[seg > 0], b[seg > 0]), n
        elif n == "scaling":
            assert torch.equal(a[seg < 2], b[seg < 2]) and within_bar(a[seg >= 2], b[seg >= 2]), n
        else:
            assert torch.equal(a, b), n
        for got, want in ((out_m, ref_m), (out_v, ref_v)):
            if want[n] is None:
                assert got[n] is None, n
            else:
                assert torch.equal(got[n], want[n]), n
                assert not got[n][seg > 0].any(), n


def run_plan_apply(params, m, v, accum, accum_abs, denom, z, Q, cfg):
    import gaussian_model_ops as gmo
    ws, counts = gmo.densify_plan(accum, accum_abs, denom, params["scaling"], params["opacity"], cfg["max_grad"], Q,
                                  cfg["percent_dense"] * cfg["extent"], cfg["min_opacity"], 0.1 * cfg["extent"] if cfg["max_screen_size"] else None)
    P_out, *ret = counts.tolist()
    lst = lambda d: [None if d is None else d[n] for n in dr.PARAMS]
    p, a, b = gmo.densify_apply(ws, P_out, lst(params), lst(m), lst(v), z)
    dic = lambda l: dict(zip(dr.PARAMS, l))
    return dic(p), dic(a), dic(b), tuple(ret)


# ------------------------------------------------------------------ statistics ------------------------------------------------------------------
class StatsModel:
    def __init__(self, P):
        for n in STATS:
            setattr(self, n, torch.zeros((P, 1), device=DEV))
        self.max_radii2D = torch.zeros(P, device=DEV)


def test_stats_fixture_three_views_without_a_host_sync():
    import gaussian_model_ops as gmo
    with np.load(os.path.join(GOLDEN, "densify_stats.npz")) as f:
        d = {k: f[k] for k in f.files}
    P = d["grad0"].shape[0]
    model = StatsModel(P)
    views = [(torch.from_numpy(d[f"grad{v}"]).to(DEV), torch.from_numpy(d[f"radii{v}"]).to(DEV), torch.from_numpy(d[f"mask{v}"]).to(DEV)) for v in range(3)]
    holder = namedtuple("Holder", "grad")
    torch.cuda.synchronize()
    names = dict(accum="xyz_gradient_accum", accum_abs="xyz_gradient_accum_abs", accum_abs_max="xyz_gradient_accum_abs_max", denom="denom",
                 max_radii2D="max_radii2D")
    snaps = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for v, (grad, radii, mask) in enumerate(views):
            # view 0: the mask is `radii > 0`, taken by the kernel (update_filter=None); views 1, 2: an explicit bool mask; view 2 hands the
            # gradient over as upstream does, on a tensor's .grad
            if v == 0:
                gmo.add_densification_stats(model, grad, None, radii)
            elif v == 1:
                gmo.add_densification_stats(model, grad, mask, radii)
            else:
                gmo.add_densification_stats(model, holder(grad), mask, radii)
            snaps.append({k: getattr(model, a).clone() for k, a in names.items()})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for v, snap in enumerate(snaps):
        for k in ("accum_abs", "accum_abs_max", "denom", "max_radii2D"):
            assert np.array_equal(snap[k].cpu().numpy(), d[f"{k}{v}"]), (k, v)                      # bit-exact
        a, b = snap["accum"].cpu().numpy().astype(np.float64), d[f"accum{v}"].astype(np.float64)
        err = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
        print(f"view {v}: accum max relative error {err[b != 0].max():.3e}")
        assert (np.abs(a - b) <= 5e-7 * np.abs(b)).all(), (v, float(err[b != 0].max()))
        untouched = ~(d["mask0"] | (d["mask1"] if v >= 1 else False) | (d["mask2"] if v >= 2 else False))
        assert not snap["accum"].cpu().numpy()[untouched].any() and not snap["denom"].cpu().numpy()[untouched].any()


def test_stats_without_radii_leaves_max_radii2D_alone_and_rejects_bad_input():
    import gaussian_model_ops as gmo
    P = 1000
    model = StatsModel(P)
    model.max_radii2D += 7.0
    g = torch.randn(P, 3, device=DEV)
    mask = torch.rand(P, device=DEV) < 0.5
    gmo.add_densification_stats(model, g, mask)
    assert torch.equal(model.max_radii2D, torch.full((P,), 7.0, device=DEV))
    assert torch.equal(model.denom[:, 0], mask.float())
    assert torch.equal(model.xyz_gradient_accum_abs[:, 0], g[:, 2].abs() * mask)
    with pytest.raises(RuntimeError):
        gmo.add_densification_stats(model, g)                         # neither mask nor radii
    with pytest.raises(RuntimeError):
        gmo.add_densification_stats(model, g.double(), mask)          # float32 only
    with pytest.raises(RuntimeError):
        gmo.add_densification_stats(model, g.cpu(), mask.cpu())       # GPU only


def test_stats_reduced_form_from_view_parallel_buffers():
    import gaussian_model_ops as gmo
    gen = torch.Generator(device=DEV).manual_seed(3)
    P = 5000
    model = StatsModel(P)
    for n in STATS:
        getattr(model, n).copy_(torch.rand(P, 1, generator=gen, device=DEV))
    model.max_radii2D.copy_(30 * torch.rand(P, generator=gen, device=DEV))
    count = torch.randint(0, 4, (P,), generator=gen, device=DEV).float()             # ranks that saw the row: 0 = nobody
    reduced = torch.stack([torch.rand(P, generator=gen, device=DEV) * count, torch.rand(P, generator=gen, device=DEV) * count, count], dim=1).contiguous()
    radii_max = torch.randint(0, 60, (P,), generator=gen, device=DEV, dtype=torch.int32)
    before = dict(accum=model.xyz_gradient_accum.clone(), accum_abs=model.xyz_gradient_accum_abs.clone(),
                  accum_abs_max=model.xyz_gradient_accum_abs_max.clone(), denom=model.denom.clone(), max_radii2D=model.max_radii2D.clone())
    want = dr.stats_step_reduced(before, reduced, radii_max)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        gmo.add_reduced_densification_stats(model, reduced, radii_max)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = dict(accum=model.xyz_gradient_accum, accum_abs=model.xyz_gradient_accum_abs, accum_abs_max=model.xyz_gradient_accum_abs_max, denom=model.denom,
               max_radii2D=model.max_radii2D)
    for k in want:
        assert torch.equal(got[k], want[k]), k          # sums of two floats and maxima: bit-exact
    unseen = count == 0
    assert unseen.any() and all(torch.equal(got[k][unseen], before[k][unseen]) for k in want)


# ------------------------------------------------------------------ densify: fixtures ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["densify_sh1", "densify_sh3"])
def test_plan_and_apply_reproduce_the_reference(name):
    d = load_fixture(name)
    params, m, v, accum, accum_abs, denom, z, cfg = fixture_args(d, DEV)
    Q = torch.tensor(float(d["Q"]), device=DEV)
    out_p, out_m, out_v, ret = run_plan_apply(params, m, v, accum, accum_abs, denom, z, Q, cfg)
    check_against_fixture(d, out_p, out_m, out_v, ret)


@pytest.mark.parametrize("opt_index", [0, 1], ids=["fused_adam", "torch_adam"])
@pytest.mark.parametrize("name", ["densify_sh1", "densify_sh3"])
def test_densify_and_prune_on_a_model_reproduces_the_reference(name, opt_index):
    import gaussian_model_ops as gmo
    d = load_fixture(name)
    params, m, v, accum, accum_abs, denom, z, cfg = fixture_args(d, DEV)
    model = Model(params, accum, accum_abs, denom, cfg["percent_dense"], optimizers()[opt_index], m, v)
    filter_before = model.filter_3D
    old = {n: getattr(model, a) for n, a in ATTR.items()}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            ret = gmo.densify_and_prune(model, cfg["max_grad"], cfg["min_opacity"], cfg["extent"], cfg["max_screen_size"], unit_normals=z)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message)]
    assert len(syncs) == 1, [str(w.message) for w in caught]          # the one host read: the new row count
    state = model.optimizer.state
    out_p = {n: getattr(model, a) for n, a in ATTR.items()}
    check_against_fixture(d, out_p, {n: state[out_p[n]]["exp_avg"] for n in ATTR}, {n: state[out_p[n]]["exp_avg_sq"] for n in ATTR}, ret)
    P_out = d["out_xyz"].shape[0]
    for n, a in ATTR.items():
        p = out_p[n]
        g = next(g for g in model.optimizer.param_groups if g["name"] == n)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and len(g["params"]) == 1 and g["params"][0] is p
        assert old[n] not in state and float(state[p]["step"]) == 2.0 and set(state[p]) == {"step", "exp_avg", "exp_avg_sq"}
    assert len(state) == 6
    for n in STATS:
        t = getattr(model, n)
        assert t.shape == (P_out, 1) and t.dtype == torch.float32 and t.is_cuda and not t.any(), n
    assert model.max_radii2D.shape == (P_out,) and not model.max_radii2D.any()
    assert model.filter_3D is filter_before                          # the caller recomputes it (train.py:196-199)
    for p in out_p.values():                                         # training goes on with the carried state
        p.grad = torch.ones_like(p)
    model.optimizer.step()
    assert all(float(state[p]["step"]) == 3.0 and torch.isfinite(p).all() for p in out_p.values())


# ------------------------------------------------------------------ densify: edge cases ------------------------------------------------------------------
def small_case(P=4000, seed=11, sh_degree=1):
    inputs = dr.random_decision_inputs(seed, P)
    params, m, v, z = dr.random_model(seed, P, sh_degree, DEV, inputs)
    accum, accum_abs, denom = (t.to(DEV) for t in inputs[:3])
    return params, m, v, z, accum, accum_abs, denom


def test_no_gaussians():
    import gaussian_model_ops as gmo
    params = dict(xyz=torch.zeros(0, 3), f_dc=torch.zeros(0, 1, 3), f_rest=torch.zeros(0, 3, 3), opacity=torch.zeros(0, 1), scaling=torch.zeros(0, 3),
                  rotation=torch.zeros(0, 4))
    params = {k: t.to(DEV) for k, t in params.items()}
    e = torch.zeros(0, 1, device=DEV)
    model = Model(params, e, e, e, 0.01, optimizers()[0])
    assert gmo.densify_and_prune(model, 0.0002, 0.05, 5.0, 20) == (0, 0, 0)
    assert model._xyz.shape == (0, 3)
    ws, counts = gmo.densify_plan(e, e, e, params["scaling"], params["opacity"], 0.0002, torch.zeros((), device=DEV), 0.05, 0.05, None)
    assert counts.tolist() == [0, 0, 0, 0]


def test_nothing_hot_nothing_pruned_is_the_identity():
    params, m, v, z, accum, accum_abs, denom = small_case()
    accum, accum_abs = torch.zeros_like(accum), denom * 1e-5
    cfg = dict(max_grad=1e9, min_opacity=0.0, extent=5.0, percent_dense=0.01, max_screen_size=None)      # sigmoid < 0 never: nothing is faint
    out_p, out_m, out_v, ret = run_plan_apply(params, m, v, accum, accum_abs, denom, z, torch.tensor(float("inf"), device=DEV), cfg)
    assert ret == (0, 0, 0)
    for n in dr.PARAMS:
        assert torch.equal(out_p[n], params[n]) and torch.equal(out_m[n], m[n]) and torch.equal(out_v[n], v[n]), n


def test_everything_pruned():
    import gaussian_model_ops as gmo
    params, m, v, z, accum, accum_abs, denom = small_case()
    P = params["xyz"].shape[0]
    for opt_cls in optimizers():
        model = Model(params, accum, accum_abs, denom, 0.01, opt_cls, m, v)
        cloned, split, pruned = gmo.densify_and_prune(model, 0.0002, 2.0, 5.0, 20, unit_normals=z)     # sigmoid < 2: every candidate is faint
        assert pruned == P + cloned + split and cloned > 0 and split > 0
        for n, a in ATTR.items():
            p = getattr(model, a)
            assert p.shape[0] == 0 and p.shape[1:] == params[n].shape[1:]
            assert model.optimizer.state[p]["exp_avg"].shape == p.shape
        assert model.denom.shape == (0, 1) and model.max_radii2D.shape == (0,)


def test_max_screen_size_none_and_zero_switch_the_world_size_prune_off():
    params, m, v, z, accum, accum_abs, denom = small_case(seed=12)
    Q = dr.abs_threshold(accum, accum_abs, denom, dr.DEFAULTS["max_grad"])
    outs = {}
    for mss in (None, 0, 20):
        cfg = dict(dr.DEFAULTS, max_screen_size=mss)
        outs[mss] = run_plan_apply(params, m, v, accum, accum_abs, denom, z, Q, cfg)
        ref = dr.densify(params, m, v, accum, accum_abs, denom, z, Q, **cfg)
        assert outs[mss][3] == ref[3]
        compare_with_restatement(*outs[mss][:3], *ref[:3], ref[4].to(DEV))
    assert outs[None][3] == outs[0][3] and outs[20][3][2] > outs[None][3][2]
    assert (torch.exp(outs[20][0]["scaling"]).max(dim=1).values <= 0.5).all()
    assert not (torch.exp(outs[None][0]["scaling"]).max(dim=1).values <= 0.5).all()


@pytest.mark.parametrize("opt_index", [0, 1], ids=["fused_adam", "torch_adam"])
def test_group_without_state_and_foreign_groups(opt_index):
    """a group that has not been stepped yet gets parameters only; appearance groups are left exactly as they are"""
    import gaussian_model_ops as gmo
    params, m, v, z, accum, accum_abs, denom = small_case(seed=13, sh_degree=2)
    model = Model(params, accum, accum_abs, denom, 0.01, optimizers()[opt_index], m, v, stateless=("rotation", "f_rest"), extra_group=True)
    net, net_state = model.net, model.optimizer.state[model.net]
    Q = dr.abs_threshold(accum, accum_abs, denom, dr.DEFAULTS["max_grad"])
    m_ref = {n: (None if n in ("rotation", "f_rest") else t) for n, t in m.items()}
    v_ref = {n: (None if n in ("rotation", "f_rest") else t) for n, t in v.items()}
    ref = dr.densify(params, m_ref, v_ref, accum, accum_abs, denom, z, Q, max_screen_size=20, **dr.DEFAULTS)
    ret = gmo.densify_and_prune(model, dr.DEFAULTS["max_grad"], dr.DEFAULTS["min_opacity"], dr.DEFAULTS["extent"], 20, unit_normals=z)
    assert ret == ref[3]
    st = model.optimizer.state
    out_p = {n: getattr(model, a) for n, a in ATTR.items()}
    out_m = {n: st[out_p[n]]["exp_avg"] if out_p[n] in st else None for n in ATTR}
    out_v = {n: st[out_p[n]]["exp_avg_sq"] if out_p[n] in st else None for n in ATTR}
    compare_with_restatement(out_p, out_m, out_v, *ref[:3], ref[4].to(DEV))
    assert out_p["rotation"] not in st and out_p["f_rest"] not in st and len(st) == 5
    g = model.optimizer.param_groups[-1]
    assert g["name"] == "appearance_network" and g["params"][0] is net and st[net] is net_state and torch.equal(net_state["exp_avg"], torch.ones_like(net))


def test_rejects_what_it_cannot_run():
    import gaussian_model_ops as gmo
    params, m, v, z, accum, accum_abs, denom = small_case(P=500)
    model = Model({k: t.double() for k, t in params.items()}, accum, accum_abs, denom, 0.01, torch.optim.Adam)
    with pytest.raises(RuntimeError):
        gmo.densify_and_prune(model, 0.0002, 0.05, 5.0, 20)
    model = Model({k: t.cpu() for k, t in params.items()}, accum.cpu(), accum_abs.cpu(), denom.cpu(), 0.01, torch.optim.Adam)
    with pytest.raises(RuntimeError):
        gmo.densify_and_prune(model, 0.0002, 0.05, 5.0, 20)
    model = Model(params, accum, accum_abs, denom, 0.01, torch.optim.Adam)
    with pytest.raises(RuntimeError):
        gmo.densify_and_prune(model, 0.0002, 0.05, 5.0, 20, unit_normals=z[:, :2].contiguous())


def test_drawn_normals_displace_clones_by_their_own_scale():
    """unit_normals=None: torch.randn is drawn; a clone's offset in its source's frame, divided by the scales, is standard normal"""
    import gaussian_model_ops as gmo
    params, m, v, z, accum, accum_abs, denom = small_case(P=60000, seed=14)
    model = Model(params, accum, accum_abs, denom, 0.01, torch.optim.Adam, m, v)
    Q = dr.abs_threshold(accum, accum_abs, denom, dr.DEFAULTS["max_grad"])
    src = dr.densify(params, m, v, accum, accum_abs, denom, z, Q, max_screen_size=None, **dr.DEFAULTS)[4].to(DEV)
    torch.manual_seed(0)
    gmo.densify_and_prune(model, dr.DEFAULTS["max_grad"], dr.DEFAULTS["min_opacity"], dr.DEFAULTS["extent"], None)
    new = (src >> 30) > 0
    row = (src & ((1 << 30) - 1))[new]
    off = model._xyz.detach()[new] - params["xyz"][row]
    local = torch.bmm(dr.rotation_matrices(params["rotation"][row]).transpose(1, 2), off.unsqueeze(-1)).squeeze(-1) / torch.exp(params["scaling"][row])
    assert int(new.sum()) > 3000
    assert abs(float(local.mean())) < 0.05 and abs(float(local.std()) - 1.0) < 0.05, (float(local.mean()), float(local.std()))


# ------------------------------------------------------------------ randomised sweep ------------------------------------------------------------------
def test_randomised_sweep_against_the_eager_restatement():
    cases = dr.sweep_cases()
    assert len(cases) >= 50 and max(c[1] for c in cases) == 200_000
    redrawn = 0
    for seed, P, sh_degree, mss in cases:
        cfg = dict(dr.DEFAULTS, max_screen_size=mss)
        for attempt in range(20):                                  # a seed whose inputs violate the margin is re-drawn, never dropped
            inputs = dr.random_decision_inputs(seed + 1000 * attempt, P)
            accum, accum_abs, denom = (t.to(DEV) for t in inputs[:3])
            Q = dr.abs_threshold(accum, accum_abs, denom, cfg["max_grad"])
            if dr.margin_ok(accum, accum_abs, denom, inputs[3].to(DEV), inputs[4].to(DEV), Q, cfg["max_grad"], cfg["min_opacity"], cfg["extent"],
                            cfg["percent_dense"], mss):
                break
            redrawn += 1
        else:
            raise AssertionError(f"seed {seed}: no draw satisfied the margin")
        params, m, v, z = dr.random_model(seed + 1000 * attempt, P, sh_degree, DEV, inputs)
        if seed % 5 == 4:                                          # some cases without optimizer state in two groups
            m, v = dict(m, f_dc=None, scaling=None), dict(v, f_dc=None, scaling=None)
        ref_p, ref_m, ref_v, ref_ret, src = dr.densify(params, m, v, accum, accum_abs, denom, z, Q, **cfg)
        out_p, out_m, out_v, ret = run_plan_apply(params, m, v, accum, accum_abs, denom, z, Q, cfg)
        assert ret == ref_ret, (seed, P, ret, ref_ret)
        assert ref_ret[0] + ref_ret[1] > 0, (seed, P, ref_ret)
        compare_with_restatement(out_p, out_m, out_v, ref_p, ref_m, ref_v, src.to(DEV))
    print(f"randomised sweep: {len(cases)} cases, {redrawn} re-drawn for the input margin")
    assert redrawn <= 0.05 * len(cases), redrawn


# ------------------------------------------------------------------ training loop ------------------------------------------------------------------
View = namedtuple("View", "image_width image_height FoVx FoVy")


def test_training_loop_with_statistics_and_one_densification():
    """tests/test_gpu_train_loop.py's wiring with the missing stage: statistics every step, one densify_and_prune mid-way that changes P,
    then training goes on with the carried optimizer state"""
    import fused_adam
    import gaussian_model_ops as gmo
    import graphics_utils as gu
    import loss_utils as lu
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from synth_scene import make_scene, to_device
    dev = torch.device(DEV)
    s = to_device(make_scene(3000, 192, 128, sh_degree=1, mu_px=4.0, seed=90, kernel_size=0.1, require_coord=False, require_depth=True,
                             filter3d=False), dev)
    view = View(s.W, s.H, 2 * math.atan(s.tanfovx), 2 * math.atan(s.tanfovy))
    rs = GaussianRasterizationSettings(image_height=s.H, image_width=s.W, tanfovx=s.tanfovx, tanfovy=s.tanfovy, kernel_size=s.kernel_size,
                                       bg=s.bg, scale_modifier=1.0, viewmatrix=s.viewmatrix, projmatrix=s.projmatrix, sh_degree=s.sh_degree,
                                       campos=s.campos, prefiltered=False, require_depth=True, require_coord=False, debug=False)
    rast = GaussianRasterizer(rs)

    def render(xyz, f, op_raw, sc_raw, rot, means2D=None):
        filter_3D = torch.full((xyz.shape[0], 1), 0.002, device=dev)
        scales, opacity = gmo.scaling_n_opacity_with_3D_filter(sc_raw, op_raw, filter_3D)
        return rast(means3D=xyz, means2D=torch.zeros_like(xyz, requires_grad=True) if means2D is None else means2D, shs=f, colors_precomp=None,
                    opacities=opacity, scales=scales, rotations=torch.nn.functional.normalize(rot), cov3D_precomp=None)

    gt = dict(xyz=s.means3D, f=s.shs[:, :4].contiguous(), op=torch.logit(s.opacities.clamp(1e-4, 1 - 1e-4)), sc=torch.log(s.scales), rot=s.rotations)
    with torch.no_grad():
        target = render(gt["xyz"], gt["f"], gt["op"], gt["sc"], gt["rot"])[0]
    g = torch.Generator(device="cpu").manual_seed(0)
    P = s.means3D.shape[0]
    f0 = gt["f"] + 0.3 * torch.randn(P, 4, 3, generator=g).to(dev)
    params = dict(xyz=gt["xyz"] + 0.01 * torch.randn(P, 3, generator=g).to(dev), f_dc=f0[:, :1].contiguous(), f_rest=f0[:, 1:].contiguous(),
                  opacity=gt["op"] + 0.5 * torch.randn(P, 1, generator=g).to(dev), scaling=gt["sc"] + 0.2 * torch.randn(P, 3, generator=g).to(dev),
                  rotation=gt["rot"].clone())
    zeros = torch.zeros(P, 1, device=dev)

    class Patched(Model):
        pass
    gmo.patch_gaussian_model(Patched)                    # the two methods under upstream's names and signatures, as train.py calls them
    model = Patched(params, zeros, zeros, zeros, 0.01, fused_adam.Adam)
    model.max_radii2D.zero_()
    for grp, lr in zip(model.optimizer.param_groups, (1e-4, 5e-3, 5e-3, 2e-2, 5e-3, 1e-3)):
        grp["lr"] = lr
    extent = float((s.means3D.max(dim=0).values - s.means3D.min(dim=0).values).max()) * 0.55
    losses, sizes, ret = [], [], None
    for it in range(60):
        means2D = torch.zeros_like(model._xyz, requires_grad=True)
        out = render(model._xyz, torch.cat((model._features_dc, model._features_rest), dim=1), model._opacity, model._scaling, model._rotation, means2D)
        image, radii, depth, mdepth, normal = out[0], out[1], out[4], out[5], out[7]
        loss = lu.photometric_loss(image, target, 0.2) + 0.05 * gu.normal_consistency_loss(view, normal, depth, mdepth, 0.6)
        model.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        losses.append(float(loss.item()))
        sizes.append(model._xyz.shape[0])
        with torch.no_grad():
            if it % 2:
                model.add_densification_stats(means2D, radii > 0)                                 # upstream's call ...
                model.max_radii2D = torch.maximum(model.max_radii2D, radii.float() * (radii > 0))  # ... and train.py:186 next to it
            else:
                gmo.add_densification_stats(model, means2D, None, radii)                           # both in the one launch
            if it == 24:
                seen = model.denom > 0
                mean_grad = (model.xyz_gradient_accum / model.denom)[seen]
                assert int(seen.sum()) > P // 2 and float(model.max_radii2D.max()) > 0
                thr = float(torch.quantile(mean_grad, 0.9))                                         # a threshold that does select
                ret = model.densify_and_prune(thr, 0.02, extent, 20)
        model.optimizer.step()
    print("loop: rows", sizes[0], "->", sizes[-1], "(cloned, split, pruned) =", ret, "loss", losses[0], losses[25], losses[-1])
    assert ret is not None and ret[0] + ret[1] > 0 and sizes[-1] != sizes[0] and sizes[-1] == sizes[0] + ret[0] + ret[1] - ret[2]
    assert all(math.isfinite(x) for x in losses)
    assert losses[-1] < losses[25], (losses[25], losses[-1])          # lower at the end than right after densification
    st = model.optimizer.state
    # the step count was carried through; the step right after the densification finds no gradient on the new tensors and skips them, as upstream
    assert all(float(st[getattr(model, a)]["step"]) == 59.0 for a in ATTR.values())
    assert all(torch.isfinite(getattr(model, a)).all() for a in ATTR.values())
