"""CPU tier of the direct integrate tests (tests/integrate_cases.py): every case meets its conditions on the float32 oracle's
state; chain (a) reproduces that oracle exactly where the two must agree (last contributors, point counts, which points are projected -- and,
as measured, every float32 word of the five outputs, which is reported, not required); project32 equals the oracle's projection bit for bit;
C_INT is what chain (a) needs against the float64 restatement (b); and every mutation of (a) is SEEN by the checks the GPU tests make."""
import functools

import numpy as np
import pytest

import integrate_cases as ic
from util import oracle_for

NAMES = list(ic.CASES)


class Run:
    pass


@functools.lru_cache(maxsize=None)
def run(name):
    r = Run()
    r.s, r.pts = ic.CASES[name].build()
    o = oracle_for(r.s)
    ref = o.integrate(r.pts)
    r.inp = ic.input_from_oracle(o, r.s, r.pts)
    H, W = r.s.H, r.s.W
    r.oracle = dict(out9=ref[0].copy(), final_T=o.get("final_T").reshape(H, W).copy(), alpha_integrated=ref[1].copy(), color_integrated=ref[2].copy(),
                    coordinate2d=ref[3].copy(), sdf=ref[4].copy(), n_contrib=o.get("n_contrib").reshape(2, H, W).copy())
    o.close()
    r.dec = ic.decide(r.inp)
    r.w = ic.walk32(r.inp, r.dec)
    r.ref = ic.restate64(r.inp, r.dec, r.w)
    r.need = ic.need(ic.chain_outputs(r.dec, r.w), r.ref)
    return r


@pytest.mark.parametrize("name", NAMES)
def test_case_meets_its_conditions(name):
    r = run(name)
    cond = ic.CASES[name].conditions(r.inp, r.dec, r.w)
    assert cond and all(cond.values()), [k for k, v in cond.items() if not v]


@pytest.mark.parametrize("name", NAMES)
def test_chain_reproduces_the_oracle_exactly(name):
    r = run(name)
    bad = ic.exact_differences(r.inp, r.dec, r.w, r.oracle)
    assert not bad, bad
    # which points are projected: the oracle leaves (0, 0) at the others (a NaN for the non-finite ones), chain (a) the initial values
    assert np.array_equal(r.inp.projected, r.oracle["alpha_integrated"] != 1.0)
    assert int(r.inp.projected.sum()) == int(r.oracle["out9"][8].sum())
    got = ic.chain_outputs(r.dec, r.w)
    for k, v in got.items():
        a, b = (v[list(ic.PLANES)], r.oracle[k][list(ic.PLANES)]) if k == "out9" else (v, r.oracle[k])
        print(f"{name} {k}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} words differ from the oracle")


@pytest.mark.parametrize("name", NAMES)
def test_project32_is_the_oracles_projection(name):
    r = run(name)
    s = r.s
    p2d, pdepth, ppix = ic.project32(r.pts, s.viewmatrix.numpy().reshape(-1), *ic.focal32(s), s.W, s.H)
    assert np.array_equal(ppix, r.inp.ppix)
    assert np.array_equal(p2d.view(np.uint32), r.inp.p2d.view(np.uint32)) and np.array_equal(pdepth.view(np.uint32), r.inp.pdepth.view(np.uint32))
    assert np.array_equal(p2d.view(np.uint32), r.oracle["coordinate2d"].view(np.uint32))


def test_c_int_is_what_chain_a_needs():
    worst = max(max(run(n).need.values()) for n in NAMES)
    print({n: {k: round(v, 4) for k, v in run(n).need.items()} for n in NAMES})
    assert worst <= ic.C_INT <= 1.25 * worst, f"chain (a) needs c = {worst:.4g} over all cases; integrate_cases.C_INT = {ic.C_INT}"


def test_band_seed():
    """What the search recorded for BAND_SEED."""
    r = run("band")
    hi, lo = ic.near_threshold(r.w, 1e-4)
    hi3, lo3 = ic.near_threshold(r.w, 1e-3)
    print("band: pairs inside 1e-4 above / below", int(hi.sum()), int(lo.sum()), "inside 1e-3", int(hi3.sum() + lo3.sum()),
          "corner-only uses", int(ic.corner_only(r.dec).sum()), "centre passed, a corner rejected", ic.centre_rejected_corner(r.inp, r.dec))
    assert int(hi.sum()) >= 3 and int(lo.sum()) >= 3


MUTATION_PARAMS = [pytest.param(m, n, id=f"{m.replace(' ', '_')}-{n}") for m, cases in ic.MUTATIONS.items() for n in cases]


@pytest.mark.parametrize("mutation,name", MUTATION_PARAMS)
def test_mutated_chain_is_rejected(mutation, name):
    """Sharpness: a chain (a) with ONE thing wrong must break an exact check against the unmutated chain or need more than the 2 C_INT the
    HIP kernels get against (b)."""
    r = run(name)
    m = ic.mutate(mutation, r.inp, r.dec, r.w, r.s, r.pts)
    assert m is not None, "the case has nothing to mutate this way"
    d2, w2, i2 = m
    got = ic.chain_outputs(d2, w2)
    c = ic.need(got, r.ref)
    full = dict(got, n_contrib=np.stack([d2.last, 0 * d2.last]), coordinate2d=w2.coordinate2d)
    full["out9"] = np.concatenate([got["out9"][:8], i2.pix_points[None].astype(np.float32)])
    exact = ic.exact_differences(r.inp, r.dec, r.w, full)
    if not np.array_equal(i2.ppix, r.inp.ppix):
        exact["ppix"] = int((i2.ppix != r.inp.ppix).sum())
    worst = max(c, key=c.get)
    print(f"{mutation} on {name}: exact checks broken {exact}; most moved {worst}, c = {c[worst]:.3g}")
    assert exact or c[worst] > 2 * ic.C_INT, f"the mutation hides inside 2 C_INT = {2 * ic.C_INT}: the most it moves is {worst}, c = {c[worst]:.3g}"


def test_nonfinite_points_keep_the_initial_values_in_the_oracle():
    """The three non-finite points of `edges`: the reference's reject test lets a NaN projection through, and then no pixel claims the point."""
    r = run("edges")
    o = r.oracle
    assert (o["alpha_integrated"][-3:] == 1).all() and (o["color_integrated"][-3:] == 0).all() and (o["sdf"][-3:] == -1000).all()
    assert not r.inp.projected[-3:].any() and (r.w.alpha_integrated[-3:] == 1).all() and (r.w.sdf[-3:] == -1000).all()
