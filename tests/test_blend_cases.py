"""CPU tier of the direct blend tests (tests/blend_cases.py): the cases meet their conditions, the float32 decision chain
reproduces the fp32 oracle's contributor numbers exactly, the float64 restatement of the blend reproduces both oracles, C_REF is what the
fp32 oracle needs, and every mutation of the reference is SEEN by the criterion the GPU tests use (so that criterion can fail)."""
import functools

import numpy as np
import pytest

import blend_cases as bc
from util import oracle_backward, oracle_for

PARAMS = [pytest.param(*p, id=bc.case_id(p)) for p in bc.CASE_MODES]


class Run:
    pass


@functools.lru_cache(maxsize=None)
def run(name, coord, depth):
    """One case in one mode: the fp32 oracle's state, images and per-Gaussian blend sums, chain (a) and restatement (b) over that state."""
    r = Run()
    r.s = bc.CASES[name].build(coord, depth)
    r.g = bc.cotangents(r.s)
    o = oracle_for(r.s)
    o.forward()
    oracle_backward(o, r.g)
    r.inp = bc.input_from_oracle(o, r.s)
    r.n_contrib = o.get("n_contrib").reshape(2, r.s.H, r.s.W).copy()
    r.images, r.sums = bc.oracle_images(o), bc.oracle_sums(o, r.inp.P, coord)
    o.close()
    r.dec = bc.decide(r.inp)
    r.ref = bc.restate(r.inp, r.dec, r.g)
    return r


def need(r, ref):
    """{what: c} of the fp32 oracle's images and sums against a reference"""
    d = {f"image {k}": v for k, v in bc.images_need(r.inp, r.images, ref).items()}
    d.update({f"sum {k}": v for k, v in bc.sums_need(r.inp, r.sums, ref).items()})
    return d


@pytest.mark.parametrize("name,coord,depth", PARAMS)
def test_case_meets_its_conditions(name, coord, depth):
    r = run(name, coord, depth)
    cond = bc.CASES[name].conditions(r.inp, r.dec)
    assert cond and all(cond.values()), [k for k, v in cond.items() if not v]
    assert all(bool((v != 0).any()) for v in r.g.values()), "a cotangent is all zero"


@pytest.mark.parametrize("name,coord,depth", PARAMS)
def test_decision_chain_reproduces_the_oracle_exactly(name, coord, depth):
    r = run(name, coord, depth)
    got = bc.n_contrib_planes(r.dec)
    for plane, what in ((0, "last"), (1, "median")):
        bad = np.argwhere(got[plane] != r.n_contrib[plane])
        assert not len(bad), f"{what} contributor of pixel (x {bad[0][1]}, y {bad[0][0]}): chain {got[plane][tuple(bad[0])]}, oracle {r.n_contrib[plane][tuple(bad[0])]}; {len(bad)} pixels"


@pytest.mark.parametrize("name,coord,depth", PARAMS)
def test_restatement_reproduces_the_fp32_oracle(name, coord, depth):
    r = run(name, coord, depth)
    c = need(r, r.ref)
    worst = max(c, key=c.get)
    assert c[worst] <= bc.C_REF, f"{worst} needs c = {c[worst]:.3g} > C_REF = {bc.C_REF}"


@pytest.mark.parametrize("name,coord,depth", PARAMS)
def test_restatement_reproduces_the_float64_oracle(name, coord, depth):
    """The float64 oracle's own state through chain (a) in float64 (which must give that oracle's decisions) and restatement (b): 1e-10 of A."""
    s = bc.CASES[name].build(coord, depth)
    g = bc.cotangents(s)
    o = oracle_for(s, precision=64)
    o.forward()
    oracle_backward(o, g)
    inp = bc.input_from_oracle(o, s)
    dec = bc.decide(inp, np.float64)
    assert np.array_equal(bc.n_contrib_planes(dec), o.get("n_contrib").reshape(2, s.H, s.W))
    ref = bc.restate(inp, dec, g)
    one = 2.0 ** 24 - 16.0            # n with 2^-24 (n + 16) == 1: needed_c then returns |x - r| / A
    images, sums = bc.oracle_images(o), bc.oracle_sums(o, inp.P, coord)
    for k in bc.IMAGES:
        rel, at = bc.needed_c(images[k], ref.images[k], ref.images_A[k], one)
        assert rel <= 1e-10, (k, rel, at)
    for c in range(25 if coord else 16):
        rel, at = bc.needed_c(sums[:, c], ref.sums[:, c], ref.sums_A[:, c], one)
        assert rel <= 1e-10, (f"slot {c}", rel, at)


def test_c_ref_is_what_the_fp32_oracle_needs():
    worst = max(max(need(run(*p), run(*p).ref).values()) for p in bc.CASE_MODES)
    assert worst <= bc.C_REF <= 1.25 * worst, f"the fp32 oracle needs c = {worst:.4g} over all cases; blend_cases.C_REF = {bc.C_REF}"


MUTATION_PARAMS = [pytest.param(m, *p, id=f"{m.replace(' ', '_')}-{bc.case_id(p)}") for m, cases in bc.MUTATIONS.items()
                   for p in bc.CASE_MODES if p[0] in cases]


@pytest.mark.parametrize("mutation,name,coord,depth", MUTATION_PARAMS)
def test_mutated_reference_is_rejected(mutation, name, coord, depth):
    """Sharpness: against the reference with ONE thing wrong, the fp32 oracle's values must fail the bound the HIP kernels get."""
    r = run(name, coord, depth)
    kw = bc.mutate(mutation, r.inp, r.dec)
    assert kw is not None, "the case has nothing to mutate this way"
    c = need(r, bc.restate(r.inp, r.dec, r.g, **kw))
    worst = max(c, key=c.get)
    assert c[worst] > 2 * bc.C_REF, f"the mutation hides inside 2 C_REF = {2 * bc.C_REF}: the most it moves is {worst}, c = {c[worst]:.3g}"


def test_straight_through_clamp_is_what_the_oracle_differentiates():
    """The one place the older float64 second opinion (tests/torch_restatement.py, clamp_max) is wrong: with the gate, the clamped pairs'
    share of the opacity sum disappears; the oracle (backward.cu:852, 979) keeps it."""
    r = run("clamp", False, True)
    gated = bc.restate(r.inp, r.dec, r.g, gate_clamp=True)
    a = r.dec.a_raw.astype(np.float64)
    only_clamped = np.flatnonzero(r.inp.n[:4] == 1)[:1]                       # the op = 5 splat alone in tile 0
    gid = r.inp.point_list[r.inp.ranges[only_clamped[0], 0]]
    assert (r.dec.act[only_clamped[0], 0] & (a[only_clamped[0], 0] > bc.C99)).any()
    assert abs(r.sums[gid, 15] - r.ref.sums[gid, 15]) <= bc.C_REF * bc.EPS * 17 * r.ref.sums_A[gid, 15]
    assert abs(gated.sums[gid, 15] - r.ref.sums[gid, 15]) > 0.1 * abs(r.ref.sums[gid, 15])
