"""The four blend kernels against the float64 restatement of the blend alone (tests/blend_cases.py), on the MI355X.

Per case and mode: HipRun.forward_native(), then splat_a / splat_b / ranges / point_list -- the records the blend kernels of that launch
READ -- go through the float32 decision chain (a) and the float64 restatement (b), once (module cache); every forward path must give (a)'s
contributor numbers exactly and (b)'s images inside 2 C_REF, every backward path (b)'s per-Gaussian sums inside 2 C_REF (LAST_ACC through
gpu_util.hip_sums_as_reference), and the ordered backward's per-instance wave totals (LAST_PARTIALS: no cross-tile summation at all) too.

Paths, by the library's switches: forward RADEGS_STREAMS=0 | 1 (told apart by radegs_last_forward_used_streams and the tag in stream_meta);
backward RADEGS_BWD_PPL=2 | 4 after a tile-wide forward, the stream backward after a stream forward, RADEGS_DETERMINISTIC=1 (told apart by
LAST_PARTIALS).  Which of packed<2>, packed<4> and the stream backward a default-order launch took cannot be seen from outside: the tests
set the switches rg_launch.inc::choose_blend_bwd reads and rely on it.

RADEGS_BLEND_MARGINS=<file>: the c every path needed, per case and slot, is written there when the module finishes."""
import contextlib
import os

import numpy as np
import pytest
import torch

import blend_cases as bc
from stream_lists import TAG

pytestmark = pytest.mark.gpu

PARAMS = [pytest.param(*p, id=bc.case_id(p)) for p in bc.CASE_MODES]
BOUND = 2 * bc.C_REF
FORWARD_PATHS = {"tile": {"RADEGS_STREAMS": "0"}, "streams": {"RADEGS_STREAMS": "1"}}
# backward path -> (forward it follows, switches)
BACKWARD_PATHS = {"packed2": ("tile", {"RADEGS_BWD_PPL": "2", "RADEGS_DETERMINISTIC": "0"}),
                  "packed4": ("tile", {"RADEGS_BWD_PPL": "4", "RADEGS_DETERMINISTIC": "0"}),
                  "streams": ("streams", {"RADEGS_STREAMS_BWD": "1", "RADEGS_DETERMINISTIC": "0"}),
                  "ordered": ("tile", {"RADEGS_DETERMINISTIC": "1"}),
                  "ordered-after-streams": ("streams", {"RADEGS_DETERMINISTIC": "1"})}
MARGINS = {}


@contextlib.contextmanager
def switches(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Launch:
    """one forward of one case through one path, and what it left"""


@pytest.fixture(scope="module")
def cache():
    store = {}
    yield store
    path = os.environ.get("RADEGS_BLEND_MARGINS")
    if path and MARGINS:
        with open(path, "w") as f:
            f.write(f"C_REF = {bc.C_REF} (blend_cases.py: the fp32 oracle's need over all cases); the kernels' bound is 2 C_REF = {BOUND}\n")
            f.write("c needed per path, case and slot (image name, sum slot s<k> of LAST_ACC, partial slot p<k> of LAST_PARTIALS); worst first\n")
            for (path_name, case), c in sorted(MARGINS.items()):
                worst = max(c, key=c.get)
                f.write(f"{path_name:22s} {case:28s} worst {worst} {c[worst]:.3f} | " + " ".join(f"{k} {v:.3f}" for k, v in c.items()) + "\n")


def forward(cache, name, coord, depth, path):
    key = (name, coord, depth, path)
    if key in cache:
        return cache[key]
    from gpu_util import HipRun
    assert torch.cuda.is_available(), "these tests need the MI355X box"
    s = bc.CASES[name].build(coord, depth)
    L = Launch()
    with switches(dict(FORWARD_PATHS[path], RADEGS_DETERMINISTIC="0")):
        L.h = HipRun(s, "cuda:0")
        L.st = L.h.forward_native()
        torch.cuda.synchronize()
        L.used_streams = L.h.C.last_forward_used_streams()
        L.meta = L.h.export("stream_meta", torch.int32, 4).view(np.uint32)
    L.inp = bc.input_from_hip(L.h)
    L.n_contrib = L.h.export("n_contrib", torch.int32, 2 * s.H * s.W).view(np.uint32).reshape(2, s.H, s.W)
    res = [t.detach().cpu().numpy() for t in L.st[1:8]]
    L.images = dict(color=res[0], coord=res[1], mcoord=res[2], alpha=res[3], normal=res[4], depth=res[5], mdepth=res[6])
    rkey = (name, coord, depth, "reference")
    if rkey not in cache:                      # the reference: once per case and mode, from the records of the first launch ...
        dec = bc.decide(L.inp)
        g = bc.cotangents(s)
        cache[rkey] = (L.inp, dec, bc.restate(L.inp, dec, g), g)
    else:                                      # ... which every other launch of the case must have read too
        first = cache[rkey][0]
        assert np.array_equal(first.point_list, L.inp.point_list) and np.array_equal(first.ranges, L.inp.ranges)
        used = np.unique(first.point_list)      # (the records of Gaussians in no list are not written)
        assert np.array_equal(first.rec[used].view(np.uint32), L.inp.rec[used].view(np.uint32))
        assert first.planes is None or np.array_equal(first.planes[used].view(np.uint32), L.inp.planes[used].view(np.uint32))
    L.inp, L.dec, L.ref, L.g = cache[rkey]
    cache[key] = L
    return L


def check(c, what):
    worst = max(c, key=c.get)
    assert c[worst] <= BOUND, f"{what}: {worst} needs c = {c[worst]:.3g} > 2 C_REF = {BOUND}"


@pytest.mark.parametrize("path", list(FORWARD_PATHS))
@pytest.mark.parametrize("name,coord,depth", PARAMS)
def test_forward(cache, name, coord, depth, path):
    L = forward(cache, name, coord, depth, path)
    streams = path == "streams"
    assert L.used_streams is streams, f"asked for the {path} forward; radegs_last_forward_used_streams says {L.used_streams}"
    assert (int(L.meta[0]) == TAG) == streams, f"stream_meta[0] = {int(L.meta[0]):#x} after the {path} forward"
    cond = bc.CASES[name].conditions(L.inp, L.dec)          # the case is still the case on the kernel's own records
    assert all(cond.values()), [k for k, v in cond.items() if not v]
    want = bc.n_contrib_planes(L.dec)
    for plane, what in ((0, "last"), (1, "median")):
        bad = np.argwhere(L.n_contrib[plane] != want[plane])
        assert not len(bad), (f"{what} contributor of pixel (x {bad[0][1]}, y {bad[0][0]}): kernel {L.n_contrib[plane][tuple(bad[0])]}, "
                              f"chain {want[plane][tuple(bad[0])]}; {len(bad)} pixels")
    c = bc.images_need(L.inp, L.images, L.ref)
    print(f"forward {path} {bc.case_id((name, coord, depth))}: " + " ".join(f"{k} {v:.3f}" for k, v in c.items()))
    MARGINS[(f"forward {path}", bc.case_id((name, coord, depth)))] = c
    check(c, f"{path} forward")


@pytest.mark.parametrize("path", list(BACKWARD_PATHS))
@pytest.mark.parametrize("name,coord,depth", PARAMS)
def test_backward(cache, name, coord, depth, path):
    from gpu_util import hip_sums_as_reference
    from test_gpu_deterministic import _backward
    fwd, env = BACKWARD_PATHS[path]
    L = forward(cache, name, coord, depth, fwd)
    with switches(dict(FORWARD_PATHS[fwd], **env)):
        _, acc, part = _backward(L.h, L.st, L.g, keep=True)
    ordered = path.startswith("ordered")
    assert (part is not None) == ordered, f"asked for the {path} backward; LAST_PARTIALS is {'set' if part is not None else 'None'}"
    sums = hip_sums_as_reference(torch.from_numpy(acc), L.h.s)
    c = {f"s{k}": v for k, v in bc.sums_need(L.inp, sums, L.ref).items()}
    if ordered:
        assert part.shape == (L.inp.R, L.inp.rec_len)
        c.update({f"p{k}": v for k, v in bc.partials_need(L.inp, part, L.ref).items()})
    print(f"backward {path} {bc.case_id((name, coord, depth))}: " + " ".join(f"{k} {v:.3f}" for k, v in c.items()))
    MARGINS[(f"backward {path}", bc.case_id((name, coord, depth)))] = c
    check(c, f"{path} backward")
