"""gaussian_model_ops.model_activations (csrc/radegs_activate.hip) on the GPU: the bytes of torch.cat, the bits of radegs_filter3d for scales
and opacity, the bits of tests/activation_restatement.py for the rotations, the reference's recorded values inside 1e-5 / 1e-4, and the
memory either side of every output untouched.  Shapes: one row, a quad of rows more or less (the 16-byte groups), a tile of 64 more or
less, several tiles with and without a tail; K = 0 (no rest rows at all), 3, 8, 15."""
import os

import numpy as np
import pytest
import torch

import activation_restatement as ar

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
POISON = 0x7FC0DEAD                              # a quiet NaN with a payload no arithmetic produces
GUARD = 64                                       # floats either side of a carved output: 256 bytes
SHAPES = [(P, K) for P in (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000) for K in (0, 3, 8, 15)]


def close(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= 1e-5 + 1e-4 * np.abs(b.astype(np.float64))


def same_bits(a, b):
    """equal as float32 bit patterns, NaN standing for NaN (payload and sign of a NaN are the library's)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def inputs(P, K, seed):
    rng = np.random.default_rng(seed)
    rot = rng.standard_normal((P, 4)).astype(np.float32)
    deg = ar.degenerate_rotations()
    n = min(P, len(deg))
    rot[P - n:] = deg[:n]                                   # the degenerate rows sit in the tail tile
    f3 = (0.02 * np.exp(0.5 * rng.standard_normal((P, 1)))).astype(np.float32)
    f3[rng.random(P) < 0.25] = 0.0
    d = dict(f_dc=rng.standard_normal((P, 1, 3)), f_rest=0.2 * rng.standard_normal((P, K, 3)), rot=rot,
             sc=np.log(0.04) + 1.2 * rng.standard_normal((P, 3)), op=2.0 * rng.standard_normal((P, 1)), f3=f3,
             g_shs=rng.standard_normal((P, K + 1, 3)), g_rot=rng.standard_normal((P, 4)), g_sc=rng.standard_normal((P, 3)),
             g_op=rng.standard_normal((P, 1)))
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in d.items()}


def gpu(d):
    return {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}


class Carved:
    """tensors of the given shapes inside ONE buffer filled with a NaN pattern, each starting on a 16-byte boundary with guards either side"""

    def __init__(self, shapes):
        sizes = [int(np.prod(s)) for s in shapes]
        offs, at = [], GUARD
        for n in sizes:
            offs.append(at)
            at = (at + n + GUARD + 3) // 4 * 4
        self.buf = torch.full((at + GUARD,), POISON, dtype=torch.int32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.spans = list(zip(offs, sizes))
        self.tensors = tuple(self.buf[o:o + n].view(torch.float32).view(s) for (o, n), s in zip(self.spans, shapes))
        assert all(t.data_ptr() % 16 == 0 for t in self.tensors)

    def check(self):
        raw = self.buf.cpu().numpy()
        inside = np.zeros(raw.shape, bool)
        for o, n in self.spans:
            inside[o:o + n] = True
            assert not (raw[o:o + n] == POISON).any(), "an output element was left unwritten"
        assert (raw[~inside] == POISON).all(), "bytes outside an output were written"


def eager_scale_opacity(t, g_sc, g_op):
    """radegs_filter3d through its own binding: (scales, opacity, g_scaling_raw, g_opacity_raw); a None cotangent is absent"""
    import gaussian_model_ops as gmo
    sc, op = t["sc"].clone().requires_grad_(True), t["op"].clone().requires_grad_(True)
    scales, opacity = gmo.scaling_n_opacity_with_3D_filter(sc, op, t["f3"])
    outs, cots = [o for o, g in ((scales, g_sc), (opacity, g_op)) if g is not None], [g for g in (g_sc, g_op) if g is not None]
    if outs and sc.shape[0]:
        torch.autograd.backward(outs, cots)
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad      # noqa: E731
    return scales.detach(), opacity.detach(), zero(sc), zero(op)


@pytest.mark.parametrize("P,K", SHAPES)
def test_bits_and_bounds(P, K):
    import gaussian_model_ops as gmo
    d = inputs(P, K, 1000 * K + P)
    t = gpu(d)
    fwd = Carved([(P, K + 1, 3), (P, 4), (P, 3), (P, 1)])
    out = gmo.model_activations_forward(t["f_dc"], t["f_rest"], t["rot"], t["sc"], t["op"], t["f3"], out=fwd.tensors)
    assert all(a is b for a, b in zip(out, fwd.tensors))
    bwd = Carved([(P, 1, 3), (P, K, 3), (P, 4), (P, 3), (P, 1)])
    gmo.model_activations_backward(K, t["rot"], t["sc"], t["op"], t["f3"], t["g_shs"], t["g_rot"], t["g_sc"], t["g_op"], out=bwd.tensors)
    torch.cuda.synchronize()
    fwd.check()
    bwd.check()
    shs, rotations, scales, opacity = (x.cpu().numpy() for x in fwd.tensors)
    g_dc, g_rest, g_rot, g_sc, g_op = (x.cpu().numpy() for x in bwd.tensors)
    # SH rows: the bytes of torch.cat and of the two slices
    assert np.array_equal(shs.view(np.uint32), torch.cat((t["f_dc"], t["f_rest"]), dim=1).cpu().numpy().view(np.uint32))
    assert np.array_equal(g_dc.view(np.uint32), d["g_shs"][:, :1].copy().view(np.uint32))
    assert np.array_equal(g_rest.view(np.uint32), d["g_shs"][:, 1:].copy().view(np.uint32))
    # scales and opacity: radegs_filter3d's bits, both directions
    e_scales, e_opacity, e_gsc, e_gop = (x.cpu().numpy() for x in eager_scale_opacity(t, t["g_sc"], t["g_op"]))
    assert same_bits(scales, e_scales) and same_bits(opacity, e_opacity)
    assert same_bits(g_sc, e_gsc) and same_bits(g_op, e_gop)
    # rotations: the stated chain's bits, the degenerate rows included
    assert same_bits(rotations, ar.normalize_forward(d["rot"]))
    assert same_bits(g_rot, ar.normalize_backward(d["rot"], d["g_rot"]))
    # a second call gives the same bytes
    again = gmo.model_activations_forward(t["f_dc"], t["f_rest"], t["rot"], t["sc"], t["op"], t["f3"])
    again_b = gmo.model_activations_backward(K, t["rot"], t["sc"], t["op"], t["f3"], t["g_shs"], t["g_rot"], t["g_sc"], t["g_op"])
    for a, b in zip(again + again_b, fwd.tensors + bwd.tensors):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_against_the_reference(degree):
    import gaussian_model_ops as gmo
    g = dict(np.load(os.path.join(GOLDEN, f"activations_sh{degree}.npz")))
    t = {k: torch.from_numpy(v).to(DEV) for k, v in g.items() if v.dtype == np.float32}
    K = g["features_rest"].shape[1]
    out = gmo.model_activations_forward(t["features_dc"], t["features_rest"], t["rotation"], t["scaling"], t["opacity"], t["filter_3D"])
    grads = gmo.model_activations_backward(K, t["rotation"], t["scaling"], t["opacity"], t["filter_3D"], t["g_shs"], t["g_rotations"], t["g_scales"],
                                           t["g_opacity"])
    for x, name in zip(out, ("out_shs", "out_rotations", "out_scales", "out_opacity")):
        assert close(x.cpu().numpy(), g[name]).all(), name
    assert np.array_equal(out[0].cpu().numpy(), g["out_shs"])
    for x, name in zip(grads, ("grad_features_dc", "grad_features_rest", "grad_rotation", "grad_scaling", "grad_opacity")):
        a = x.cpu().numpy()
        assert close(a, g[name]).all(), (name, float(np.abs(a - g[name]).max()))


@pytest.mark.parametrize("absent", ["g_shs", "g_rot", "g_sc", "g_op", "all"])
def test_absent_cotangents(absent):
    import gaussian_model_ops as gmo
    P, K = 257, 3
    d = inputs(P, K, 77)
    t = gpu(d)
    names = ("g_shs", "g_rot", "g_sc", "g_op")
    full = gmo.model_activations_backward(K, t["rot"], t["sc"], t["op"], t["f3"], *[t[n] for n in names])
    cots = [None if absent in (n, "all") else t[n] for n in names]
    out = Carved([(P, 1, 3), (P, K, 3), (P, 4), (P, 3), (P, 1)])
    gmo.model_activations_backward(K, t["rot"], t["sc"], t["op"], t["f3"], *cots, out=out.tensors)
    torch.cuda.synchronize()
    out.check()                                             # nothing is left unwritten
    g_dc, g_rest, g_rot, g_sc, g_op = out.tensors
    bits = lambda a, b: same_bits(a.cpu().numpy(), b.cpu().numpy())      # noqa: E731
    if cots[0] is None:
        assert not g_dc.any() and not g_rest.any()
    else:
        assert bits(g_dc, full[0]) and bits(g_rest, full[1])
    if cots[1] is None:
        assert not g_rot.view(torch.int32).any()            # exactly +0, the NaN and zero quaternions' rows too
    else:
        assert bits(g_rot, full[2])
    # scales / opacity: what radegs_filter3d gives for the same absent cotangents
    _, _, e_gsc, e_gop = eager_scale_opacity(t, cots[2], cots[3])
    assert bits(g_sc, e_gsc) and bits(g_op, e_gop)
    if cots[3] is None:
        assert not g_op.any()
    if cots[2] is not None and cots[3] is not None:
        assert bits(g_sc, full[3]) and bits(g_op, full[4])


@pytest.mark.parametrize("K", [0, 3])
def test_autograd_end_to_end(K):
    import gaussian_model_ops as gmo
    P = 130
    d = inputs(P, K, 5)
    t = gpu(d)
    leaves = [t[k].clone().requires_grad_(True) for k in ("f_dc", "f_rest", "rot", "sc", "op")] + [t["f3"].clone().requires_grad_(True)]
    outs = gmo.model_activations(*leaves)
    assert [tuple(o.shape) for o in outs] == [(P, K + 1, 3), (P, 4), (P, 3), (P, 1)]
    (sum((o * t[n]).sum() for o, n in zip(outs, ("g_shs", "g_rot", "g_sc", "g_op")))).backward()
    direct = gmo.model_activations_backward(K, t["rot"], t["sc"], t["op"], t["f3"], t["g_shs"], t["g_rot"], t["g_sc"], t["g_op"])
    for leaf, want in zip(leaves[:5], direct):
        assert leaf.grad is not None and same_bits(leaf.grad.cpu().numpy(), want.cpu().numpy())
    assert leaves[5].grad is None                           # filter_3D carries no gradient, as upstream
    # an output nothing uses arrives as an absent cotangent, not as zeros
    leaves2 = [x.detach().clone().requires_grad_(True) for x in leaves[:5]]
    o2 = gmo.model_activations(*leaves2, t["f3"])
    (o2[1] * t["g_rot"]).sum().backward()
    only = gmo.model_activations_backward(K, t["rot"], t["sc"], t["op"], t["f3"], None, t["g_rot"], None, None)
    for leaf, want in zip(leaves2, only):
        assert same_bits(leaf.grad.cpu().numpy(), want.cpu().numpy())


def test_bad_arguments_raise():
    import gaussian_model_ops as gmo
    P, K = 10, 3
    t = gpu(inputs(P, K, 9))
    args = [t[k] for k in ("f_dc", "f_rest", "rot", "sc", "op", "f3")]
    names = ("_features_dc", "_features_rest", "_rotation", "_scaling", "_opacity", "filter_3D")
    for i, name in enumerate(names):
        bad = list(args)
        bad[i] = args[i][:-1]
        with pytest.raises(RuntimeError, match="same number of rows"):
            gmo.model_activations(*bad)
        bad[i] = args[i].double()
        with pytest.raises(RuntimeError, match=f"`{name}` must be float32"):
            gmo.model_activations(*bad)
        bad[i] = args[i].cpu()
        with pytest.raises(RuntimeError, match=f"`{name}` must be a GPU tensor"):
            gmo.model_activations(*bad)
        wide = torch.cat([args[i], args[i]], dim=-1)
        bad[i] = wide
        with pytest.raises(RuntimeError, match=f"`{name}` must be float32 of shape"):
            gmo.model_activations(*bad)
        bad[i] = wide[..., ::2]                              # the right shape, every second column of a wider tensor
        assert bad[i].shape == args[i].shape and not bad[i].is_contiguous()
        with pytest.raises(RuntimeError, match=f"`{name}` must be a contiguous"):
            gmo.model_activations(*bad)
    with pytest.raises(RuntimeError, match="`out` must hold"):
        gmo.model_activations_forward(*args, out=(torch.empty((P, K + 1, 3), device=DEV),) * 3)
    with pytest.raises(RuntimeError, match="`out` must hold contiguous float32 tensors"):
        gmo.model_activations_forward(*args, out=tuple(torch.empty((P + 1, c), device=DEV) for c in (4, 4, 3, 1)))
    with pytest.raises(RuntimeError, match="must have 10 rows"):
        gmo.model_activations_backward(K, t["rot"], t["sc"], t["op"], t["f3"], None, t["g_rot"][:-1], None, None)
    # the C entry points themselves refuse what the binding never sends
    L = gmo._lib()
    p = [x.data_ptr() for x in args]
    o = [torch.empty_like(x) for x in (torch.cat((args[0], args[1]), 1), args[2], args[3], args[4])]
    q = [x.data_ptr() for x in o]
    assert L.radegs_model_activate_forward(-1, K, *p, *q, None) == -1
    assert L.radegs_model_activate_forward(P, 80, *p, *q, None) == -1
    assert L.radegs_model_activate_forward(P, K, p[0], None, *p[2:], *q, None) == -1
    assert L.radegs_model_activate_forward(P, 0, *p, *q, None) == -1             # K == 0 with a rest pointer
    assert L.radegs_model_activate_forward(P, K, p[0] + 4, *p[1:], *q, None) == -1     # not 16-byte aligned
    assert L.radegs_model_activate_forward(P, K, *p, q[0], None, q[2], q[3], None) == -1
    assert L.radegs_model_activate_forward(0, K, *([None] * 10), None) == 0
    assert L.radegs_model_activate_backward(0, K, *([None] * 13), None) == 0
    assert L.radegs_model_activate_backward(P, K, *([None] * 13), None) == -1
    torch.cuda.synchronize()


def test_views_into_a_larger_buffer_are_taken():
    """rows [1:] of a parameter start 12 bytes into f_dc's storage: the binding copies what is not 16-byte aligned, the result is the same"""
    import gaussian_model_ops as gmo
    P, K = 70, 3
    t = gpu(inputs(P + 1, K, 12))
    args = [t[k][1:] for k in ("f_dc", "f_rest", "rot", "sc", "op", "f3")]
    assert args[0].data_ptr() % 16 != 0 and all(a.is_contiguous() for a in args)
    a = gmo.model_activations_forward(*args)
    b = gmo.model_activations_forward(*[x.clone() for x in args])
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
