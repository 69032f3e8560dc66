"""Direct GPU tests of the four densification kernels (radegs_densify.hip) against the NumPy reference of tests/densify_cases.py:
every comparison of the plan at its threshold, every row pattern and array-end position of the apply kernel, misaligned inputs and
outputs with guard words, pre-filled outputs and workspace, and the statistics update on special values.  The plan and the copies are
held exactly; the computed xyz' / _scaling' by step_edge_cases.rule (as accurate as the float32 NumPy statement, both against float64)."""
import ctypes

import numpy as np
import pytest
import torch

import densify_cases as dc
import step_edge_cases as sec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
GUARD = 64                       # floats either side of every slice (a multiple of 4: offsets count from a 16-byte boundary)
SENTINEL = -12345.5              # no input of any case holds it
GROUPS = ("param", "exp_avg", "exp_avg_sq")


class Slice:
    """`data` as a contiguous slice `off` floats past a 16-byte boundary of a larger buffer, guard words either side"""

    def __init__(self, data, off=0):
        data = np.ascontiguousarray(data)
        self.n, self.shape = data.size, data.shape
        kind = torch.float32 if data.dtype == np.float32 else torch.int32
        assert data.dtype in (np.float32, np.int32)
        self.raw = torch.full((GUARD + off + self.n + GUARD,), SENTINEL if kind == torch.float32 else -77, dtype=kind, device=DEV)
        self.fill = self.raw[0].clone()
        assert self.raw.data_ptr() % 16 == 0
        self.lo = GUARD + off
        self.view = self.raw[self.lo:self.lo + self.n].view(self.shape)
        self.view.copy_(torch.from_numpy(data))
        assert self.n == 0 or self.view.data_ptr() % 16 == 4 * off
        assert self.view.is_contiguous()

    def host(self):
        return self.view.detach().cpu().numpy().copy()

    def guards_intact(self):
        return bool((self.raw[:self.lo] == self.fill).all()) and bool((self.raw[self.lo + self.n:] == self.fill).all())


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def same_values(a, b):
    """bit for bit, except that any NaN equals any NaN (payloads are not specified)"""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _libs():
    import gaussian_model_ops as gmo
    from diff_gaussian_rasterization import _C
    return gmo, _C, gmo._lib()


# ------------------------------------------------------------------------------------------------------------------- plan
def run_plan(case, tensors=None):
    """radegs_densify_plan through the C ABI on a workspace and counts4 pre-filled with 0xFF bytes; returns (workspace, counts4 as a
    list, src_of uint32 [P_out] read from the head of the workspace)"""
    gmo, _C, L = _libs()
    P = case.scaling.shape[0]
    t = tensors or [Slice(x).view for x in (case.accum, case.accum_abs, case.denom, case.scaling, case.opacity)]
    q = torch.tensor([float(case.Q)], dtype=torch.float32, device=DEV)
    nbytes = L.radegs_densify_plan_bytes(P)
    ws = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=DEV)
    counts = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    assert ws.data_ptr() % 16 == 0 and nbytes >= 8 * P
    rc = L.radegs_densify_plan(P, *[_C._ptr(x) for x in t], float(case.max_grad), _C._ptr(q), float(case.dense), float(case.min_opacity),
                               int(case.big is not None), float(case.big) if case.big is not None else 0.0, _C._ptr(ws), nbytes,
                               _C._ptr(counts), _C._stream(torch.device(DEV)))
    assert rc == 0, (case.name, rc)
    torch.cuda.synchronize()
    c = counts.tolist()
    assert 0 <= c[0] <= 2 * P, (case.name, c)
    return ws, c, ws[:4 * c[0]].cpu().numpy().view(np.uint32).copy()


def check_plan(case):
    """counts4 and src_of equal the reference exactly, twice with the same bits.  Where the reference marks rows ambiguous, one assignment
    of those rows' ambiguous comparisons must reproduce the whole src_of and counts4; the assignment found is named.  Returns the run."""
    ws, counts, src = run_plan(case)
    _, counts2, src2 = run_plan(case)
    assert counts == counts2 and np.array_equal(src, src2), (case.name, "two runs differ")
    flags, amb = dc.decide_case(case)
    want_src, want_counts = dc.expected_src_of(flags)
    if tuple(counts) == want_counts and np.array_equal(src, want_src):
        return ws, counts, src
    n = min(src.size, want_src.size)
    assert amb.any(), (case.name, counts, want_counts, "output rows that differ", np.flatnonzero(src[:n] != want_src[:n])[:8].tolist(),
                       src[:16].tolist(), want_src[:16].tolist())
    for flip in dc.assignments(amb):
        s, c = dc.expected_src_of(dc.decide_case(case, flip)[0])
        if tuple(counts) == c and np.array_equal(src, s):
            print(f"{case.name}: equal to the reference with the ambiguous comparisons (row, {dc.COMPARISONS}) flipped at",
                  np.argwhere(flip).tolist(), "of", np.argwhere(amb).tolist())
            return ws, counts, src
    raise AssertionError((case.name, "no assignment of the ambiguous rows reproduces src_of", np.argwhere(amb).tolist(), counts, want_counts))


# ------------------------------------------------------------------------------------------------------------------ apply
def device_model(model, absent=(), in_off=lambda i: 0):
    """the 18 input arrays and z as Slices: {(group, name): Slice}; moment pairs of the groups in `absent` are left out"""
    params, m, v, z = model
    d = {}
    for j, group in enumerate((params, m, v)):
        for k, name in enumerate(dc.PARAMS):
            if j and name in absent:
                continue
            d[(j, name)] = Slice(group[name], in_off(6 * j + k))
    return d, Slice(z, in_off(18))


def run_apply(ws, P, P_out, rest, ins, z, out_off=lambda i: 0):
    """radegs_densify_apply through the C ABI; every output a Slice pre-filled with SENTINEL.  After the call no sentinel is left inside an
    output and every output guard is intact.  Returns {(group, name): ndarray}."""
    gmo, _C, L = _libs()
    t = gmo.RadegsDensifyTensors()
    outs = {}
    for (j, name), x in ins.items():
        k = dc.PARAMS.index(name)
        if x.n == 0:
            continue
        o = Slice(np.full((P_out,) + x.shape[1:], SENTINEL, dtype=F32), out_off(6 * j + k))
        t.inp[6 * j + k], t.out[6 * j + k] = x.view.data_ptr(), o.view.data_ptr()
        outs[(j, name)] = o
    rc = L.radegs_densify_apply(P, P_out, rest, ctypes.byref(t), _C._ptr(z.view), _C._ptr(ws), _C._stream(torch.device(DEV)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = {}
    for key, o in outs.items():
        assert o.guards_intact(), (key, "output guard overwritten")
        got[key] = o.host()
        left = np.flatnonzero(got[key].reshape(-1) == F32(SENTINEL))
        assert left.size == 0, (key, "elements never written", left[:8].tolist(), got[key].size)
    return got


class Computed:
    """collects the computed elements of many cases per class for one rule() each"""

    def __init__(self):
        self.parts = {"xyz new rows": [], "scaling children": []}

    def add(self, label, hip, o32, ref64):
        self.parts[label].append((hip.reshape(-1), o32.reshape(-1), ref64.reshape(-1)))

    def judge(self, tag, bars=None):
        ok = True
        for label, parts in self.parts.items():
            if parts:
                hip, o32, ref = (np.concatenate(x) for x in zip(*parts))
                ok &= sec.report(f"densify {tag} {label}", sec.rule(hip, o32, ref, **(bars or {}).get(label, {})))
        assert ok, tag


def check_apply(name, src, model, got, acc, absent=(), skip_sources=()):
    """`got` against apply_rows fed the kernel's own src_of: copies and every moment bit for bit, new rows' moments exactly zero; the computed
    elements go to `acc` for the rule (those of the source rows `skip_sources` excepted: their values are judged by the caller)"""
    params, m, v, z = model
    ref64 = dc.apply_rows(src, params, m, v, z, np.float64)
    ref32 = dc.apply_rows(src, params, m, v, z, np.float32)
    seg, row = src >> dc.SEG_SHIFT, src & dc.ROW_MASK
    new, child = seg > 0, seg >= 2
    for name_ in dc.PARAMS:
        if params[name_].size == 0 and params[name_].shape[0]:
            assert (0, name_) not in got
            continue
        a = got[(0, name_)]
        computed = new if name_ == "xyz" else child if name_ == "scaling" else np.zeros(src.size, dtype=bool)
        assert same_bits(a[~computed], ref32[0][name_][~computed]), (name, name_, "copied rows")
        sel = computed & ~np.isin(row, skip_sources)
        if sel.any():
            acc.add("xyz new rows" if name_ == "xyz" else "scaling children", a[sel], ref32[0][name_][sel], ref64[0][name_][sel])
        for j in (1, 2):
            if name_ in absent:
                assert (j, name_) not in got
                continue
            b = got[(j, name_)]
            assert same_bits(b, ref32[j][name_]), (name, GROUPS[j], name_)
            assert not b[new].any() and not bits(b[new]).any(), (name, GROUPS[j], name_, "new rows' moments")


def plan_and_apply(case, acc, seed=0):
    """plan and apply of one case, each twice with identical bits; returns (src_of, outputs)"""
    P = case.scaling.shape[0]
    ws, counts, src = check_plan(case)
    model = dc.model_for(case, seed)
    if counts[0] == 0:
        return src, {}
    ins, z = device_model(model)
    got = run_apply(ws, P, counts[0], case.rest_floats, ins, z)
    again = run_apply(ws, P, counts[0], case.rest_floats, ins, z)
    assert got.keys() == again.keys() and all(same_bits(got[k], again[k]) for k in got), (case.name, "two runs differ")
    assert len(got) == (18 if case.rest_floats else 15)
    check_apply(case.name, src, model, got, acc)
    return src, got


# Bars of step_edge_cases.rule per class, where a class needs other than 4 / 2 (max / rms of the kernel's error over the float32 NumPy
# statement's, both against float64).  None does.  Measured on MI355X (the `RULE densify ...` lines): xyz' on new rows between x0.9 and
# x1.08 max, x0.99 and x1.02 rms in every test.  _scaling' on children between x1 / x1.46 and, in the random case, x3.54 / x2.66: that
# rms ratio is above 2 and the comparison still holds by the rule as it stands, on its one-ulp term (rms 2.21e-7 against 2 * 8.3e-8 + one
# ulp of the median |log|, 2.38e-7).  Why the ratio is what it is: log(exp(s) / 1.6) goes through expf and logf, 1-ulp functions on the
# device, and raw scales of -3 .. -8 make one ulp of the result 2.4e-7 .. 4.8e-7; NumPy's float32 exp and log are nearer half an ulp.
BARS = {}


def test_plan_at_every_threshold():
    """one comparison per table exactly on its threshold and one ulp / one step either side (tests/densify_cases.py, threshold tables):
    counts4 and src_of equal the reference exactly; the apply runs on each table as well.
    Measured: xyz new rows x1 max / x1.02 rms; scaling children x2.26 / x1.74."""
    acc = Computed()
    for case in dc.threshold_tables():
        assert not dc.decide_case(case)[1].any(), case.name
        plan_and_apply(case, acc)
    acc.judge("thresholds", BARS)


@pytest.mark.parametrize("kind", dc.PATTERNS)
def test_row_patterns(kind):
    """P in {1, 2, 3, 4, 5, 255, 256, 257}, rest_floats cycling through 0, 9, 24, 45: the 16-byte path, the word path at removed and at new
    rows and at each array's end.  Measured over all kinds: xyz new rows x0.9 .. x1.08 max, x1 .. x1.01
    rms; scaling children x1 .. x1.56 max, x1.52 .. x1.55 rms."""
    acc = Computed()
    n = 0
    for case, P_out in dc.pattern_cases():
        if case.name.startswith(kind + "_P"):
            src, got = plan_and_apply(case, acc)
            assert src.size == P_out, (case.name, src.size, P_out)
            n += 1
    assert n == len(dc.PATTERN_P)
    acc.judge(kind, BARS)


def test_output_sizes_on_the_chunk_edge():
    """P_out * W on 4095 / 4096 / 4097 floats (or the two row counts either side of the edge) for every width of the model: the last
    block of an array holds one float, is exactly full, or is absent"""
    acc = Computed()
    for case, P_out, W in dc.chunk_edge_cases():
        src, got = plan_and_apply(case, acc)
        assert src.size == P_out and any(a.size == P_out * W for a in got.values()), case.name
    acc.judge("chunk edges", BARS)


def test_random_case_without_margins():
    """5000 rows of smooth distributions, nothing moved off a threshold: ambiguous rows (within 4 float32 ulps, none with the committed seed)
    may take either decision, all others are exact.  Measured: xyz new rows x1 / x1.01; scaling children x3.54 max / x2.66 rms
    (held at 4 / 2: see BARS)."""
    acc = Computed()
    case = dc.random_case()
    src, got = plan_and_apply(case, acc)
    seg = src >> dc.SEG_SHIFT
    assert all((seg == k).sum() >= 50 for k in range(4))
    acc.judge("random", BARS)


def test_degenerate_rotations_give_the_float32_statement_s_pattern():
    """rotation (0,0,0,0) and 1e-25 (1,1,1,1) (|q|^2 underflows to 0 in float32) on clone sources: which elements are finite is compared with
    the float32 NumPy statement only -- float64 does not underflow there; the other rows go by the rule (measured x1 / x1)"""
    acc = Computed()
    case, _ = dc.pattern_case("all_clone", 8, 9)
    ws, counts, src = check_plan(case)
    model = dc.model_for(case, 1, special_rotations=True)
    ins, z = device_model(model)
    got = run_apply(ws, 8, counts[0], 9, ins, z)
    check_apply(case.name, src, model, got, acc, skip_sources=(0, 1))
    ref32 = dc.apply_rows(src, *model, np.float32)[0]["xyz"]
    assert np.array_equal(np.isfinite(got[(0, "xyz")]), np.isfinite(ref32))
    assert not np.isfinite(ref32[8:10]).any() and np.isfinite(ref32[10:]).all() and np.isfinite(ref32[:8]).all()
    acc.judge("degenerate rotations", BARS)


# ----------------------------------------------------------------------------------------------------------------- layout
LAYOUT_ABSENT = ((), ("f_dc", "scaling"), dc.PARAMS)


def layout_cases():
    return [dc.pattern_case("runs_split", 257, 9)[0], dc.pattern_case("runs_removed", 1230, 0)[0], dc.pattern_case("all_clone", 255, 45)[0]]


@pytest.mark.parametrize("absent", LAYOUT_ABSENT, ids=["all_moments", "no_f_dc_scaling_moments", "no_moments"])
def test_misaligned_inputs_through_the_python_layer(absent):
    """every input of plan and apply a slice 0..3 floats off a 16-byte boundary, the offsets differing per array, guard words either side:
    the results equal those of the aligned C-ABI call bit for bit and no guard is touched"""
    gmo, _C, L = _libs()
    for n, case in enumerate(layout_cases()):
        P = case.scaling.shape[0]
        model = dc.model_for(case, 2)
        params, m, v, z = model
        ws0, counts0, src0 = run_plan(case)
        ins0, z0 = device_model(model, absent)
        want = run_apply(ws0, P, counts0[0], case.rest_floats, ins0, z0)
        ins, zs = device_model(model, absent, in_off=lambda i: (i * 7 + n + i // 4) % 4)
        stats = [Slice(x, o) for x, o in ((case.accum, 1), (case.accum_abs, 3), (case.denom, 2))]
        assert {s.lo % 4 for s in ins.values()} == {0, 1, 2, 3}
        q = torch.tensor(float(case.Q), dtype=torch.float32, device=DEV)
        ws, counts = gmo.densify_plan(*[s.view for s in stats], ins[(0, "scaling")].view, ins[(0, "opacity")].view, float(case.max_grad), q,
                                      float(case.dense), float(case.min_opacity), None if case.big is None else float(case.big))
        assert counts.tolist() == counts0
        assert np.array_equal(ws[:4 * counts0[0]].cpu().numpy().view(np.uint32), src0)
        lst = lambda j: [ins[(j, name)].view if (j, name) in ins else None for name in dc.PARAMS]
        out = gmo.densify_apply(ws, counts0[0], lst(0), lst(1), lst(2), zs.view)
        torch.cuda.synchronize()
        for j in range(3):
            for k, name in enumerate(dc.PARAMS):
                if j and name in absent:
                    assert out[j][k] is None
                elif ins[(j, name)].n == 0:
                    assert out[j][k].shape == (counts0[0], 0, 3)
                else:
                    assert same_bits(out[j][k].cpu().numpy(), want[(j, name)]), (case.name, GROUPS[j], name)
        for s in list(ins.values()) + stats + [zs]:
            assert s.guards_intact(), case.name
        for key, s in ins.items():
            assert same_bits(s.host(), model[key[0]][key[1]]), (case.name, key, "input changed")


@pytest.mark.parametrize("absent", LAYOUT_ABSENT, ids=["all_moments", "no_f_dc_scaling_moments", "no_moments"])
def test_misaligned_inputs_and_outputs_through_the_c_abi(absent):
    """RadegsDensifyTensors with every input 0..3 and every output 1..3 floats off a 16-byte boundary (the word path for whole arrays), outputs
    pre-filled with a sentinel: nothing left unwritten, guards intact, the bits of the aligned call; compared with the reference as well.
    Measured: xyz new rows x1 max / x0.99 rms; scaling children x1 / x1.46."""
    acc = Computed()
    for n, case in enumerate(layout_cases()):
        P = case.scaling.shape[0]
        model = dc.model_for(case, 2)
        ws, counts, src = run_plan(case)
        ins0, z0 = device_model(model, absent)
        want = run_apply(ws, P, counts[0], case.rest_floats, ins0, z0)
        ins, zs = device_model(model, absent, in_off=lambda i: (i * 5 + n) % 4)
        got = run_apply(ws, P, counts[0], case.rest_floats, ins, zs, out_off=lambda i: 1 + (i + n) % 3)
        present = [name for name in dc.PARAMS if name != "f_rest" or case.rest_floats]
        assert got.keys() == want.keys() and len(got) == len(present) + 2 * len([name for name in present if name not in absent])
        for key in got:
            assert same_bits(got[key], want[key]), (case.name, key)
        for s in list(ins.values()) + [zs]:
            assert s.guards_intact(), case.name
        check_apply(case.name, src, model, got, acc, absent)
    acc.judge("misaligned", BARS)


# ------------------------------------------------------------------------------------------------------------- statistics
class StatsModel:
    NAMES = dict(accum="xyz_gradient_accum", accum_abs="xyz_gradient_accum_abs", accum_abs_max="xyz_gradient_accum_abs_max", denom="denom",
                 max_radii2D="max_radii2D")

    def __init__(self, state):
        for k, attr in self.NAMES.items():
            setattr(self, attr, torch.from_numpy(state[k].copy()).to(DEV))

    def host(self):
        torch.cuda.synchronize()
        return {k: getattr(self, attr).cpu().numpy() for k, attr in self.NAMES.items()}


def _check_stats(tag, got, want, before, visible):
    for k in want:
        assert same_values(got[k], want[k]), (tag, k, np.flatnonzero(bits(got[k]).reshape(-1) != bits(want[k]).reshape(-1))[:8].tolist())
        assert np.array_equal(bits(got[k]).reshape(-1)[~visible], bits(before[k]).reshape(-1)[~visible]), (tag, k, "an invisible row changed")


@pytest.mark.parametrize("P", dc.STATS_P)
def test_statistics_of_one_view_bit_for_bit(P):
    """visibility from the mask, from radii > 0, and from the mask with radii given (a visible row of radius 0, an invisible one of radius
    > 0); max_radii2D untouched without radii; invisible rows holding NaN / Inf / a sentinel keep their bits; -0.0, denormal, Inf and NaN
    gradient components; a NaN abs-gradient and a stored NaN both leave NaN in accum_abs_max (include/radegs.h)"""
    gmo, _C, L = _libs()
    grad, radii, mask, st = dc.stats_view_case(P)
    g, r, k = (torch.from_numpy(x).to(DEV) for x in (grad, radii, mask))
    for tag, use_mask, use_radii in (("mask", True, False), ("radii", False, True), ("mask+radii", True, True)):
        model = StatsModel(st)
        gmo.add_densification_stats(model, g, k if use_mask else None, r if use_radii else None)
        want = dc.stats_step32(st, grad, mask if use_mask else None, radii if use_radii else None)
        _check_stats((P, tag), model.host(), want, st, mask if use_mask else radii > 0)
        if not use_radii:
            assert np.array_equal(bits(model.host()["max_radii2D"]), bits(st["max_radii2D"]))
    if P > 9:
        out = model.host()
        assert np.isnan(out["accum_abs_max"][6, 0]) and np.isnan(out["accum_abs_max"][9, 0]) and out["accum_abs"][3, 0] == F32(2e-42)


@pytest.mark.parametrize("P", dc.STATS_P)
def test_statistics_reduced_form_bit_for_bit(P):
    """counts 0, 1 and 3; a row with count 0 but non-zero sums is not written; with and without radii_max; a NaN abs-sum"""
    gmo, _C, L = _libs()
    red, radii_max, st = dc.stats_reduced_case(P)
    x, r = torch.from_numpy(red).to(DEV), torch.from_numpy(radii_max).to(DEV)
    for tag, use_radii in (("radii_max", True), ("no radii_max", False)):
        model = StatsModel(st)
        gmo.add_reduced_densification_stats(model, x, r if use_radii else None)
        want = dc.stats_step_reduced32(st, red, radii_max if use_radii else None)
        _check_stats((P, tag), model.host(), want, st, red[:, 2] != 0)
        if not use_radii:
            assert np.array_equal(bits(model.host()["max_radii2D"]), bits(st["max_radii2D"]))
