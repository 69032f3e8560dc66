"""TEST INFRASTRUCTURE for the direct tests of the four blend kernels (tests/test_blend_cases.py on the CPU, tests/test_gpu_blend_direct.py
on the MI355X).  Pure numpy / torch, importable without a GPU.

    BlendInput             what a blend kernel reads: per-Gaussian records in the splat_a layout {mx,my,cx,cy, cz,op,thr,ts, r,g,b,rpx,
                           rpy,nx,ny,nz}, the coord-mode planes {cpx0,cpy0,cpx1,cpy1,cpx2,cpy2,vp0,vp1,vp2}, the tile ranges, point_list
    decide(inp)            (a) the decision chain of csrc/rg_blend.h in numpy float32, one rounding per operation: for every (pixel, list
                           position) act (blended), kill (terminated here), med (blended while T > 0.5); last / median contributor per pixel
    restate(inp, dec, g)   (b) the blend ALONE in float64 torch, differentiated by autograd over one record row PER INSTANCE (tile, list
                           position); takes act / median from (a) as given; epilogue of forward.cu:631-692; the 0.99 clamp is straight-through,
                           which is what the reference's backward does (backward.cu:852, 979: no gate) and what torch.clamp_max does not
    needed_c(x, r, A, n)   the criterion: |x - r| <= c 2^-24 (n + 16) A, solved for c
    CASES                  the case builders and the conditions each must meet

The criterion.  `A` is the sum of the absolute values of the terms whose signed sum is `r`, `n` the length of the tile list the value was
accumulated over (the longest one of a Gaussian's tiles for a per-Gaussian sum).  For the sums that run through dL/dalpha the terms are
taken at the finest grain the kernels add them at -- dL/dalpha_i = T_i <w, v_i> - (sum_{j>i} <w, v_j> alpha_j T_j + T_final <w, bg>) / (1 - alpha_i)
is counted as T_i <|w|, |v_i|> + (sum_{j>i} <|w|, |v_j|> alpha_j T_j + T_final |<w, bg>|) / (1 - alpha_i) -- because that, not the
magnitude of their difference, is what an fp32 evaluation's error scales with.  Both backwards (and the reference's) start from
T_final = 1 - alpha_out and recover T_i by division, so every backward term carries the difference 1 / prod - alpha_out / prod: its
absolute sum is |term| (1 + alpha_out) / T_final, which is why a nearly opaque pixel's terms weigh little in this criterion -- as little
as fp32 lets any implementation of that algorithm know them.  C_REF is the smallest c the fp32 ORACLE needs over all
cases and modes (tests/test_blend_cases.py recomputes it); the HIP kernels get 2 C_REF: fma contraction, the hardware exp2 / rcp +
Newton step and a different but fixed in-wave order are legitimate."""
from typing import NamedTuple

import numpy as np
import torch

from stream_lists import exp_spec32, splat_power32
from synth_scene import make_scene, upstream_grads

F = np.float32
EPS = 2.0 ** -24
NONE_MEDIAN = 0xFFFFFFFF
C99 = float(F(0.99))
K255_32 = F(1.0) / F(255.0)
BG = (0.2, 0.4, 0.6)

# The smallest c the fp32 oracle needs over every case and mode below (0.5522: the alpha image of `clamp`), rounded up to two digits.
# test_blend_cases.py::test_c_ref_is_what_the_fp32_oracle_needs holds the stored number to the measured one: not smaller, at most 1.25 x larger.
C_REF = 0.56
MODES_ALL = ((False, False), (False, True), (True, False), (True, True))      # (coord, depth)
MODES_GEO = ((False, True), (True, True))


# ================================================================================================ the kernel's input
class BlendInput:
    def __init__(self, W, H, coord, depth, bg, fx, fy, rec, planes, ranges, point_list):
        self.W, self.H, self.coord, self.depth = int(W), int(H), bool(coord), bool(depth)
        self.geo = self.coord or self.depth
        self.bg = np.asarray(bg, np.float64).reshape(3)
        self.fx, self.fy = float(fx), float(fy)
        self.rec = np.ascontiguousarray(rec)                                   # [P, 16] float32 (or float64: the float64 oracle's state)
        self.planes = None if planes is None else np.ascontiguousarray(planes)  # [P, 9]
        self.gx, self.gy = (self.W + 15) // 16, (self.H + 15) // 16
        self.tiles = self.gx * self.gy
        self.ranges = np.asarray(ranges).astype(np.int64).reshape(self.tiles, 2)
        self.point_list = np.asarray(point_list).astype(np.int64).reshape(-1)
        self.n = self.ranges[:, 1] - self.ranges[:, 0]
        self.R = int(self.point_list.shape[0])
        self.P = int(self.rec.shape[0])
        self.L = int(self.n.max()) if self.tiles else 0
        assert (self.n >= 0).all() and int(self.n.sum()) == self.R, "ranges do not cover point_list"
        t, i = np.arange(self.tiles)[:, None], np.arange(256)[None, :]
        self.px = (t % self.gx) * 16 + (i % 16)                               # [tiles, 256]
        self.py = (t // self.gx) * 16 + (i // 16)
        self.inside = (self.px < self.W) & (self.py < self.H)
        self.rec_len = 32 if self.coord else 16

    def instance_index(self):
        """idx [tiles, L]: position in point_list of list entry e of every tile (clipped), valid [tiles, L]"""
        e = np.arange(max(self.L, 1))[None, :]
        valid = e < self.n[:, None]
        idx = np.minimum(self.ranges[:, :1] + e, max(self.R - 1, 0))
        return idx, valid

    def instance_n(self):
        """length of the tile list every instance sits in [R]; the longest such list per Gaussian [P]"""
        idx, valid = self.instance_index()
        n_inst = np.zeros(self.R, np.int64)
        n_inst[idx[valid]] = np.broadcast_to(self.n[:, None], idx.shape)[valid]
        n_g = np.zeros(self.P, np.int64)
        np.maximum.at(n_g, self.point_list, n_inst)
        return n_inst, n_g

    def to_image(self, v):
        """[..., tiles, 256] -> [..., H, W]"""
        v = np.asarray(v)
        out = np.zeros(v.shape[:-2] + (self.H, self.W), v.dtype)
        out[..., self.py[self.inside], self.px[self.inside]] = v[..., self.inside]
        return out

    def from_image(self, img):
        """[..., H, W] -> [..., tiles, 256], zero outside the image"""
        img = np.asarray(img)
        v = img[..., np.minimum(self.py, self.H - 1), np.minimum(self.px, self.W - 1)]
        return np.where(self.inside, v, np.zeros((), img.dtype))


def focal(s):
    return s.W / (2.0 * s.tanfovx), s.H / (2.0 * s.tanfovy)


def input_from_oracle(o, s):
    """The per-Gaussian state and the lists of an Oracle after forward(), as the records a blend kernel would read."""
    P = s.means3D.shape[0]
    dt = o.dt
    rec = np.zeros((P, 16), dt)
    co = o.get("conic_opacity", (P, 4))
    rec[:, 0:2] = o.get("means2D", (P, 2))
    rec[:, 2:5] = co[:, 0:3]
    rec[:, 5] = co[:, 3]
    rec[:, 7] = o.get("ts", (P,))
    rec[:, 8:11] = o.get("rgb", (P, 3))
    rec[:, 11:13] = o.get("ray_planes", (P, 2))
    rec[:, 13:16] = o.get("normals", (P, 3))
    planes = None
    if s.require_coord:
        planes = np.concatenate([o.get("camera_planes", (P, 6)), o.get("view_points", (P, 3))], 1)
    fx, fy = focal(s)
    return BlendInput(s.W, s.H, s.require_coord, s.require_depth, s.bg.numpy(), fx, fy, rec, planes, o.get("ranges"), o.get("point_list"))


def input_from_hip(h):
    """The same from a HipRun after forward_native(): the records the blend kernels of that launch read."""
    s = h.s
    P, R = h.P, int(h.state[0])
    tiles = ((s.W + 15) // 16) * ((s.H + 15) // 16)
    rec = h.export("splat_a", torch.float32, 16 * P).reshape(P, 16)
    planes = h.export("splat_b", torch.float32, 12 * P).reshape(P, 12)[:, :9] if s.require_coord else None
    ranges = h.export("ranges", torch.int32, 2 * tiles).view(np.uint32)
    pl = h.export("point_list", torch.int32, R).view(np.uint32) if R else np.zeros(0, np.uint32)
    fx, fy = focal(s)
    return BlendInput(s.W, s.H, s.require_coord, s.require_depth, s.bg.numpy(), fx, fy, rec, planes, ranges, pl)


# ================================================================================================ (a) the decision chain
class Decisions(NamedTuple):
    act: np.ndarray      # [tiles, L, 256] bool: the entry is blended into the pixel
    kill: np.ndarray     # the pixel terminates AT this entry (which is not blended)
    med: np.ndarray      # blended while T > 0.5
    live: np.ndarray     # the pixel reached the alpha test here: inside, not terminated, !(power > 0)
    a_raw: np.ndarray    # op * G as the chain formed it (float32, or float64 for the float64 oracle's state)
    T_before: np.ndarray
    last: np.ndarray     # [H, W] uint32 contributor numbers (1-based list positions; 0: none)
    median: np.ndarray   # [H, W] uint32 (NONE_MEDIAN: none; always none without a geometry map, forward.cu:613-617)


def decide(inp, dtype=np.float32):
    """dtype float32: dx = mx - px; splat_power32; exp_spec32; min(0.99f, op G); T (1 - alpha); the compares < 1/255, < 1e-4f, > 0.5f --
    each one float32 operation.  dtype float64 (the float64 oracle, oracle/radegs_oracle.cpp with R = double): the same with exp()."""
    f32 = dtype == np.float32
    X = F if f32 else np.float64
    tiles, L = inp.tiles, inp.L
    shape = (tiles, max(L, 1), 256)
    act, kill, med, live = (np.zeros(shape, bool) for _ in range(4))
    a_raw, T_before = np.zeros(shape, dtype), np.zeros(shape, dtype)
    T = np.ones((tiles, 256), dtype)
    done = ~inp.inside
    last = np.zeros((tiles, 256), np.uint32)
    median = np.full((tiles, 256), NONE_MEDIAN, np.uint32)
    pxf, pyf = inp.px.astype(dtype), inp.py.astype(dtype)
    A = inp.rec.astype(dtype)
    c99 = F(0.99) if f32 else np.float64(F(0.99))
    k255 = K255_32 if f32 else np.float64(1.0) / np.float64(255.0)
    kdone = F(0.0001) if f32 else np.float64(F(0.0001))
    with np.errstate(all="ignore"):
        for e in range(L):
            tl = np.flatnonzero(inp.n > e)
            r = A[inp.point_list[inp.ranges[tl, 0] + e]][:, None, :]          # [k, 1, 16]
            dx, dy = r[..., 0] - pxf[tl], r[..., 1] - pyf[tl]
            if f32:
                power = splat_power32(r[..., 2], r[..., 3], r[..., 4], dx, dy)
                G = exp_spec32(power)
            else:
                power = X(-0.5) * (r[..., 2] * dx * dx + r[..., 4] * dy * dy) - r[..., 3] * dx * dy
                G = np.exp(power)
            ar = r[..., 5] * G
            alpha = np.fmin(c99, ar)
            Tb = T[tl]
            lv = ~done[tl] & ~(power > X(0.0))
            ok = lv & ~(alpha < k255)
            test_T = Tb * (X(1.0) - alpha)
            kl = ok & (test_T < kdone)
            ac = ok & ~kl
            md = ac & (Tb > X(0.5))
            act[tl, e], kill[tl, e], med[tl, e], live[tl, e] = ac, kl, md, lv
            a_raw[tl, e], T_before[tl, e] = ar, Tb
            T[tl] = np.where(ac, test_T, Tb)
            done[tl] |= kl
            last[tl] = np.where(ac, np.uint32(e + 1), last[tl])
            if inp.geo:
                median[tl] = np.where(md, np.uint32(e + 1), median[tl])
    return Decisions(act, kill, med, live, a_raw, T_before, inp.to_image(last), _median_image(inp, median))


def _median_image(inp, median_tp):
    out = np.full((inp.H, inp.W), NONE_MEDIAN, np.uint32)
    out[inp.py[inp.inside], inp.px[inp.inside]] = median_tp[inp.inside]
    return out


def n_contrib_planes(dec):
    """[2, H, W] as the kernels and the oracle store it"""
    return np.stack([dec.last, dec.median])


# ================================================================================================ (b) the float64 restatement
IMAGES = ("color", "alpha", "coord", "mcoord", "depth", "mdepth", "normal")


class Restated:
    """images / images_A: {name: [C, H, W] float64}; part / part_A: [R, rec] per instance in the units the kernels leave in a partial record
    (slots 9, 10, 12, 13, 14 raw moments of h = op G dL/dalpha, 11 the absolute-value sum, plane sums not yet divided by the focal lengths);
    sums / sums_A: [P, rec] per Gaussian in the reference's units (gpu_util.reference_sums / hip_sums_as_reference)."""


def restate(inp, dec, g, gate_clamp=False, median=None, act=None):
    """g: the seven cotangents (synth_scene.upstream_grads).  act / median override the pinned decisions (the mutations of the sharpness tests);
    gate_clamp=True is the mutation 'the gradient stops at the 0.99 clamp' (torch.clamp_max's own autograd)."""
    dt = torch.float64
    tiles, L, R, P, REC = inp.tiles, inp.L, inp.R, inp.P, inp.rec_len
    out = Restated()
    act_np = dec.act if act is None else act
    med_img = dec.median if median is None else median
    W, H = inp.W, inp.H
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    inside = torch.from_numpy(inp.inside)
    pxf, pyf = tt(inp.px), tt(inp.py)
    pnx, pny = (pxf - W / 2.0) / inp.fx, (pyf - H / 2.0) / inp.fy
    ln = torch.sqrt(pnx * pnx + pny * pny + 1)
    cot = {k: tt(inp.from_image(g[k].numpy() if isinstance(g[k], torch.Tensor) else g[k])) for k in IMAGES}   # [C, tiles, 256]
    bg = tt(inp.bg)
    zero_tp = torch.zeros((tiles, 256), dtype=dt)

    if R == 0 or L == 0:
        img = {k: np.zeros((cot[k].shape[0], H, W)) for k in IMAGES}
        img["color"] = inp.to_image((bg[:, None, None] * inside.to(dt)[None]).numpy())
        out.images, out.images_A = img, {k: np.abs(v) for k, v in img.items()}
        out.part = out.part_A = np.zeros((R, REC))
        out.sums = out.sums_A = np.zeros((P, REC))
        return out

    idx_np, valid_np = inp.instance_index()
    idx, valid = torch.from_numpy(idx_np), torch.from_numpy(valid_np)
    # ---- the leaves: one row per instance ----
    leaf = tt(inp.rec[inp.point_list]).requires_grad_(True)                                   # [R, 16]
    recx = leaf[idx][:, :, None, :].expand(tiles, L, 256, 16).clone()                          # per (instance, pixel): its gradient is the TERM
    recx.retain_grad()
    mx, my, cx, cy, cz, op, ts = (recx[..., k] for k in (0, 1, 2, 3, 4, 5, 7))
    rgb = [recx[..., 8 + c] for c in range(3)]
    rpx, rpy = recx[..., 11], recx[..., 12]
    nrm = [recx[..., 13 + c] for c in range(3)]
    if inp.coord:
        pleaf = tt(inp.planes[inp.point_list]).requires_grad_(True)                           # [R, 9]
        plx = pleaf[idx][:, :, None, :].expand(tiles, L, 256, 9).clone()
        plx.retain_grad()
    actf = torch.from_numpy(act_np & valid_np[:, :, None]).to(dt)
    e1 = torch.arange(1, L + 1)[None, :, None]
    medsel = ((e1 == torch.from_numpy(inp.from_image(med_img).astype(np.int64))[:, None, :]) & (actf > 0)).to(dt)

    dx, dy = mx - pxf[:, None, :], my - pyf[:, None, :]
    power = -0.5 * (cx * dx * dx + cz * dy * dy) - cy * dx * dy
    G = torch.exp(torch.where(actf > 0, power, torch.zeros_like(power)))
    G.retain_grad()
    a_raw = op * G
    alpha = torch.clamp_max(a_raw, C99) if gate_clamp else a_raw + (torch.clamp_max(a_raw, C99) - a_raw).detach()
    alpha = alpha * actf
    cp = torch.cumprod(1.0 - alpha, dim=1)
    T = torch.cat([torch.ones((tiles, 1, 256), dtype=dt), cp[:, :-1]], 1)                      # transmittance in front of the entry
    T_fin = cp[:, -1]
    aT = alpha * T

    acc = {}

    def keep(name, v):
        v.retain_grad()
        acc[name] = v
        return v
    Cc = [keep(f"C{c}", (rgb[c] * aT).sum(1)) for c in range(3)]
    weight = keep("w", aT.sum(1))
    last = torch.from_numpy(inp.from_image(dec.last).astype(np.int64)) > 0
    if act is not None:
        last = torch.from_numpy(act_np.any(1))
    safe_w = torch.where(last, weight, torch.ones_like(weight))
    img = {"color": torch.stack([Cc[c] + T_fin * bg[c] for c in range(3)]), "alpha": weight[None]}
    img_A = {"color": torch.stack([(rgb[c] * aT).abs().sum(1) + (T_fin * bg[c]).abs() for c in range(3)]), "alpha": weight[None]}
    vals = [(rgb[c], f"C{c}") for c in range(3)]                                               # (blended quantity, its accumulator) pairs
    if inp.depth:
        t = ts + (rpx * dx + rpy * dy)
        Dep, mDep = keep("D", (t * aT).sum(1)), (t * medsel).sum(1)
        img["depth"] = torch.where(last, Dep / ln / safe_w, zero_tp)[None]
        img["mdepth"] = (mDep / ln)[None]
        t_abs = (ts.abs() + (rpx * dx).abs() + (rpy * dy).abs()).detach()
        img_A["depth"] = torch.where(last, (t_abs * aT).sum(1) / ln / safe_w, zero_tp)[None]
        img_A["mdepth"] = ((t_abs * medsel).sum(1) / ln)[None]
        vals.append((t, "D"))
    if inp.coord:
        cv = [plx[..., 6 + c] + plx[..., 2 * c] * dx + plx[..., 2 * c + 1] * dy for c in range(3)]
        Co = [keep(f"K{c}", (cv[c] * aT).sum(1)) for c in range(3)]
        img["coord"] = torch.stack([torch.where(last, Co[c] / safe_w, zero_tp) for c in range(3)])
        img["mcoord"] = torch.stack([(cv[c] * medsel).sum(1) for c in range(3)])
        cv_abs = [(plx[..., 6 + c].abs() + (plx[..., 2 * c] * dx).abs() + (plx[..., 2 * c + 1] * dy).abs()).detach() for c in range(3)]
        img_A["coord"] = torch.stack([torch.where(last, (cv_abs[c] * aT).sum(1) / safe_w, zero_tp) for c in range(3)])
        img_A["mcoord"] = torch.stack([(cv_abs[c] * medsel).sum(1) for c in range(3)])
        vals += [(cv[c], f"K{c}") for c in range(3)]
    if inp.geo:
        Nn = [keep(f"N{c}", (nrm[c] * aT).sum(1)) for c in range(3)]
        nsq = Nn[0] * Nn[0] + Nn[1] * Nn[1] + Nn[2] * Nn[2]
        nlen = torch.clamp_min(torch.sqrt(torch.where(last, nsq, torch.ones_like(nsq))), 1.0e-12)   # (sqrt'(0) = inf never enters the graph)
        img["normal"] = torch.stack([torch.where(last, Nn[c] / nlen, zero_tp) for c in range(3)])
        img_A["normal"] = torch.stack([torch.where(last, (nrm[c] * aT).abs().sum(1) / nlen, zero_tp) for c in range(3)])
        vals += [(nrm[c], f"N{c}") for c in range(3)]
    loss = sum((img[k] * cot[k] * inside.to(dt)[None]).sum() for k in img)
    loss.backward()

    def image(v):
        return inp.to_image(v.detach().numpy())
    out.images = {k: (image(img[k]) if k in img else np.zeros((cot[k].shape[0], H, W))) for k in IMAGES}
    out.images_A = {k: (image(img_A[k]) if k in img_A else np.zeros((cot[k].shape[0], H, W))) for k in IMAGES}

    # ---- the per-(instance, pixel) terms and their absolute values ----
    with torch.no_grad():
        gr = recx.grad                                                                         # [tiles, L, 256, 16]
        gp = plx.grad if inp.coord else None
        Gd, dxd, dyd, opd = G.detach(), dx.detach(), dy.detach(), op.detach()
        cxd, cyd, czd = cx.detach(), cy.detach(), cz.detach()
        h = Gd * (G.grad if G.grad is not None else torch.zeros_like(Gd))                      # op G dL/dalpha
        # |dL/dalpha| at the grain the kernels add it at (see the module text)
        w_abs = acc["w"].grad.abs() if acc["w"].grad is not None else zero_tp
        if inp.geo:                                                                            # the quotient rule's own terms: g Dep / w^2, g Co / w^2
            ww = safe_w.detach() ** 2
            w_abs = cot["alpha"][0].abs() * inside.to(dt)
            if inp.depth:
                w_abs = w_abs + torch.where(last, (cot["depth"][0] * acc["D"].detach() / ln).abs() / ww, zero_tp)
            if inp.coord:
                for c in range(3):
                    w_abs = w_abs + torch.where(last, (cot["coord"][c] * acc[f"K{c}"].detach()).abs() / ww, zero_tp)
        # the normal's cotangent is (g - <g, n> n) / |N| (backward.cu:776): for a splat facing the camera its z component is what is left of
        # g_z - g_z n_z^2, so it is counted as (|g_c| + sum_j |g_j n_j| |n_c|) / |N|
        cot_abs = {name: (a.grad.abs() if a.grad is not None else zero_tp) for name, a in acc.items()}
        if inp.geo:
            nhat = [(Nn[c] / nlen).detach() for c in range(3)]
            gn = sum((cot["normal"][j] * nhat[j]).abs() for j in range(3))
            for c in range(3):
                cot_abs[f"N{c}"] = torch.where(last, (cot["normal"][c].abs() + gn * nhat[c].abs()) / nlen.detach(), zero_tp)
        Vabs = w_abs[:, None, :] * torch.ones_like(Gd)
        for v, name in vals:
            Vabs = Vabs + cot_abs[name][:, None, :] * v.detach().abs()
        aTd, Td, ad = aT.detach(), T.detach(), alpha.detach()
        VaT = Vabs * aTd
        behind = torch.flip(torch.cumsum(torch.flip(VaT, [1]), 1), [1]) - VaT                  # sum over the entries behind this one
        bgw = sum(bg[c] * cot_abs[f"C{c}"] for c in range(3))
        # Both backwards start from T_final = 1 - alpha_out (backward.cu:706) and recover T_i = T_final / prod_{j >= i} (1 - alpha_j): every
        # term below carries T_i, the difference of 1 / prod and alpha_out / prod -- absolute sum T_i kappa, kappa = (1 + alpha_out) / T_final
        kappa = ((2.0 - T_fin) / T_fin).detach()[:, None, :]
        A_alpha = kappa * (actf > 0).to(dt) * (Td * Vabs + (behind + (T_fin.detach() * bgw)[:, None, :]) / (1.0 - ad))
        A_h = opd * Gd * A_alpha
        ex, ey = cxd * dxd + cyd * dyd, czd * dyd + cyd * dxd
        tt_ = ey.abs() * (0.5 * H) + ex.abs() * (0.5 * W)
        term = torch.zeros((tiles, L, 256, REC), dtype=dt)
        term_A = torch.zeros_like(term)
        for c, k in ((0, 8), (1, 9), (2, 10), (3, 7), (4, 11), (5, 12), (6, 13), (7, 14), (8, 15), (15, 5)):
            term[..., c] = gr[..., k]
            term_A[..., c] = kappa * gr[..., k].abs()
        # the median entry's share of a plane cotangent does not pass through T
        med_t = medsel * (cot["mdepth"][0] / ln)[:, None, :] if inp.depth else torch.zeros_like(Gd)
        dtA = kappa * (gr[..., 7] - med_t).abs() + med_t.abs()
        term_A[..., 3], term_A[..., 4], term_A[..., 5] = dtA, dtA * dxd.abs(), dtA * dyd.abs()
        if inp.geo:
            for c in range(3):
                term_A[..., 6 + c] = kappa * aTd * cot_abs[f"N{c}"][:, None, :]
        term_A[..., 15] = Gd * A_alpha
        for c, (v, va) in {9: (h * dxd, A_h * dxd.abs()), 10: (h * dyd, A_h * dyd.abs()), 11: (h.abs() * tt_, A_h * tt_),
                           12: (h * dxd * dxd, A_h * dxd * dxd), 13: (h * dxd * dyd, A_h * (dxd * dyd).abs()),
                           14: (h * dyd * dyd, A_h * dyd * dyd)}.items():
            term[..., c], term_A[..., c] = v, va
        # the reference's mean2D sums: dL/dmean per pixel = -h (conic (dx, dy)) + the plane paths; |.| at the grain of those products
        mean_x, mean_y = gr[..., 0] * (0.5 * W), gr[..., 1] * (0.5 * H)
        mean_xA = A_h * ((cxd * dxd).abs() + (cyd * dyd).abs()) + dtA * rpx.detach().abs()
        mean_yA = A_h * ((czd * dyd).abs() + (cyd * dxd).abs()) + dtA * rpy.detach().abs()
        if inp.coord:
            pld = plx.detach()
            for c in range(3):
                term[..., 16 + c], term[..., 19 + 2 * c], term[..., 20 + 2 * c] = gp[..., 6 + c], gp[..., 2 * c], gp[..., 2 * c + 1]
                med_c = medsel * cot["mcoord"][c][:, None, :]
                dcA = kappa * (gp[..., 6 + c] - med_c).abs() + med_c.abs()
                term_A[..., 16 + c], term_A[..., 19 + 2 * c], term_A[..., 20 + 2 * c] = dcA, dcA * dxd.abs(), dcA * dyd.abs()
                mean_xA = mean_xA + dcA * pld[..., 2 * c].abs()
                mean_yA = mean_yA + dcA * pld[..., 2 * c + 1].abs()
        mean_xA, mean_yA = mean_xA * (0.5 * W), mean_yA * (0.5 * H)

        def per_instance(v):                                                                   # [tiles, L, 256(, REC)] -> [R(, REC)]
            s = v.sum(2)
            o = torch.zeros((R,) + tuple(s.shape[2:]), dtype=dt)
            o[idx[valid]] = s[valid]
            return o
        part, part_A = per_instance(term), per_instance(term_A)
        # ---- per Gaussian, in the reference's units ----
        ref, ref_A = part.clone(), part_A.clone()
        ref[:, 9], ref[:, 10], ref_A[:, 9], ref_A[:, 10] = (per_instance(v) for v in (mean_x, mean_y, mean_xA, mean_yA))
        for a in (ref, ref_A):
            a[:, 4] /= inp.fx
            a[:, 5] /= inp.fy
            if inp.coord:
                a[:, 19:25:2] /= inp.fx
                a[:, 20:25:2] /= inp.fy
        ref[:, 12:15] *= -0.5
        ref_A[:, 12:15] *= 0.5
        gid = torch.from_numpy(inp.point_list)
        sums = torch.zeros((P, REC), dtype=dt).index_add_(0, gid, ref)
        sums_A = torch.zeros((P, REC), dtype=dt).index_add_(0, gid, ref_A)
    out.part, out.part_A, out.sums, out.sums_A = part.numpy(), part_A.numpy(), sums.numpy(), sums_A.numpy()
    return out


# ================================================================================================ the criterion
def needed_c(x, r, A, n):
    """The smallest c with |x - r| <= c 2^-24 (n + 16) A everywhere (inf where A == 0 and x != r) and where it is reached."""
    x, r, A = np.asarray(x, np.float64), np.asarray(r, np.float64), np.asarray(A, np.float64)
    n = np.broadcast_to(np.asarray(n, np.float64), x.shape)
    d = np.abs(x - r)
    with np.errstate(all="ignore"):
        c = np.where(d == 0, 0.0, d / (EPS * (n + 16.0) * A))
    c = np.where(np.isnan(c), np.inf, c)
    if c.size == 0:
        return 0.0, None
    k = int(np.argmax(c))
    return float(c.reshape(-1)[k]), np.unravel_index(k, c.shape)


def image_n(inp):
    """[H, W]: the length of the pixel's tile list"""
    return inp.to_image(np.broadcast_to(inp.n[:, None], (inp.tiles, 256)).copy())


def images_need(inp, images, ref):
    """{image name: c} for a set of fp32 images (dict name -> [C, H, W]) against a Restated"""
    n = image_n(inp)[None]
    return {k: needed_c(images[k], ref.images[k], ref.images_A[k], n)[0] for k in IMAGES}


def sums_need(inp, sums, ref):
    """{slot: c} for per-Gaussian sums [P, rec] in the reference's units"""
    _, n_g = inp.instance_n()
    return {c: needed_c(sums[:, c], ref.sums[:, c], ref.sums_A[:, c], n_g)[0] for c in range(25 if inp.coord else 16)}


def partials_need(inp, part, ref):
    n_i, _ = inp.instance_n()
    return {c: needed_c(part[:, c], ref.part[:, c], ref.part_A[:, c], n_i)[0] for c in range(min(part.shape[1], 25))}


def oracle_images(o):
    col, _, coord, mcoord, depth, mdepth, alpha, normal = o.outputs()
    return dict(color=col, alpha=alpha, coord=coord, mcoord=mcoord, depth=depth, mdepth=mdepth, normal=normal)


def oracle_sums(o, P, coord):
    """gpu_util.reference_sums over the blend half's own accumulators, in the oracle's precision"""
    rec = np.zeros((P, 32 if coord else 16), np.float64)
    rec[:, 0:3] = o.get("acc_dcolors").reshape(P, 3)
    rec[:, 3] = o.get("dL_dts").reshape(P)
    rec[:, 4:6] = o.get("dL_dray_planes").reshape(P, 2)
    rec[:, 6:9] = o.get("dL_dnormals").reshape(P, 3)
    rec[:, 9:12] = o.get("acc_dmeans2D").reshape(P, 3)
    dc = o.get("acc_dconic").reshape(P, 4)
    rec[:, 12], rec[:, 13], rec[:, 14] = dc[:, 0], dc[:, 1], dc[:, 3]
    rec[:, 15] = o.get("acc_dopacity").reshape(P)
    if coord:
        rec[:, 16:19] = o.get("dL_dview_points").reshape(P, 3)
        rec[:, 19:25] = o.get("dL_dcamera_planes").reshape(P, 6)
    return rec


# ================================================================================================ the cases
def _scene(W, H, coord, depth, u, v, z, sigma, opac, seed, aniso=0.0):
    """Gaussians whose centres project to pixel (u, v) of an identity camera at depth z, with a footprint of `sigma` pixels (times
    exp(aniso randn) per axis, under a random rotation when aniso > 0), opacity `opac`, random SH degree-0 colours."""
    u, v, z, sigma, opac = (np.asarray(a, np.float64).reshape(-1) for a in (u, v, z, sigma, opac))
    n = u.shape[0]
    s = make_scene(n, W, H, sh_degree=0, seed=0, kernel_size=0.0, require_coord=coord, require_depth=depth, near_cull_frac=0.0,
                   filter3d=False, bg=BG)
    rng = np.random.default_rng(1000 + seed)
    fx, fy = focal(s)
    means = np.stack([(u - (W - 1) / 2.0) * z / fx, (v - (H - 1) / 2.0) * z / fy, z], 1)
    scales = (sigma * z / fx)[:, None] * np.exp(aniso * rng.standard_normal((n, 3)))
    q = np.zeros((n, 4))
    q[:, 0] = 1.0
    if aniso > 0:
        q = rng.standard_normal((n, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    shs = np.zeros((n, 16, 3))
    shs[:, 0, :] = rng.uniform(-1.5, 1.5, (n, 3))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
    return s._replace(means3D=t(means), shs=t(shs), rotations=t(q), scales=t(scales), opacities=t(opac.reshape(n, 1)))


def _stack(u, v, k, sigma, opac, z0=2.0, dz=0.03):
    """k equal splats on one ray, front to back"""
    return [(u, v, z0 + dz * i, sigma, opac) for i in range(k)]


def _from_rows(W, H, coord, depth, rows, seed, aniso=0.0):
    a = np.asarray(rows, np.float64)
    return _scene(W, H, coord, depth, a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4], seed, aniso)


# tile centres of a 64 x 64 image: pixel (8, 8) of tile (i, j)
def _centre(tile):
    return 16 * (tile % 4) + 8, 16 * (tile // 4) + 8


# fixed by a search on the CPU (band: seeds 0 .. 23 give 3 .. 11 pairs on either side of the threshold; seed 1 has 10 above, 11 below, 123 in the ring)
BAND_SEED, LENGTHS_SEED, RAGGED_SEED = 1, 0, 0


def band(coord, depth, seed=BAND_SEED):
    rng = np.random.default_rng(seed)
    n = 170
    return _scene(64, 64, coord, depth, rng.uniform(-8, 72, n), rng.uniform(-8, 72, n), rng.uniform(2, 10, n), rng.uniform(5, 16, n),
                  rng.uniform(0.01, 0.06, n), seed, aniso=0.25)


def band_pairs(dec, width):
    """live pairs with |255 op G - 1| < width: (above the threshold, below it)"""
    with np.errstate(all="ignore"):
        d = dec.a_raw.astype(np.float64) * 255.0 - 1.0
    near = dec.live & (np.abs(d) < width)
    return near & (dec.a_raw >= dec.a_raw.dtype.type(1.0) / dec.a_raw.dtype.type(255.0)), near & ~(dec.a_raw >= dec.a_raw.dtype.type(1.0) / dec.a_raw.dtype.type(255.0))


def band_conditions(inp, dec):
    hi, lo = band_pairs(dec, 1e-4)
    hi3, lo3 = band_pairs(dec, 1e-3)
    ring = int(hi3.sum() + lo3.sum() - hi.sum() - lo.sum())
    return {"8 live pairs inside 1e-4 of alpha = 1/255": int(hi.sum() + lo.sum()) >= 8, "3 of them above": int(hi.sum()) >= 3,
            "3 of them below": int(lo.sum()) >= 3, "50 more inside 1e-3": ring >= 50}


CLAMP_OPS = (5.0, 1.0, 0.995, 0.985)


def clamp(coord, depth):
    rows = []
    for k, op in enumerate(CLAMP_OPS):                        # tiles 0..3: one splat alone
        u, v = _centre(k)
        rows += _stack(u, v, 1, 2.0, op)
    for k, op in enumerate(CLAMP_OPS):                        # tiles 4..7: in front of faint ones
        u, v = _centre(4 + k)
        rows += _stack(u, v, 1, 2.0, op) + [(u + 0.4 * i - 1, v - 0.3 * i + 0.5, 3.0 + 0.1 * i, 1.8, 0.05 + 0.04 * i) for i in range(6)]
    for k, (a, b) in enumerate(((5.0, 5.0), (5.0, 1.0), (1.0, 5.0), (0.995, 5.0))):   # tiles 8..11: two clamped, the second terminates
        u, v = _centre(8 + k)
        rows += [(u, v, 2.0, 2.0, a), (u, v, 2.5, 2.2, b)] + [(u + 1, v - 1, 3.0 + 0.1 * i, 1.8, 0.3) for i in range(3)]
    for k, op in enumerate(CLAMP_OPS):                        # tiles 12..15: the centre between four pixels
        u, v = _centre(12 + k)
        rows += [(u + 0.5, v + 0.5, 2.0, 1.5, op), (u - 0.5, v + 0.5, 2.5, 1.5, 0.4)]
    return _from_rows(64, 64, coord, depth, rows, 0)


def clamp_conditions(inp, dec):
    a = dec.a_raw.astype(np.float64)
    clamped = dec.act & (a > C99)
    single = inp.n[:4] == 1
    second_kills = [bool((dec.kill[8 + k, 1] & (dec.a_raw[8 + k, 1] > C99)).any()) for k in range(4)]
    return {"16 clamped pairs": int(clamped.sum()) >= 16, "16 pairs with a_raw in (0.9, 0.99)": int((dec.act & (a > 0.9) & (a < C99)).sum()) >= 16,
            "every clamped splat is also blended unclamped": all((dec.act[t] & (a[t] < C99)).any() for t in np.flatnonzero(clamped.any((1, 2)))),
            "one clamped splat alone": bool(single.all() and clamped[0].any() and clamped[1].any()),
            "a clamped splat in front of faint ones": bool(clamped[4, 0].any() and dec.act[4, 1:].any()),
            "a second clamped splat terminates": all(second_kills)}


TERMINATION_K = (2, 16, 17, 64, 65, 128, 129)
_TERM_TILES = (5, 6, 9, 10, 1, 4, 7)
TERMINATION_TAIL = 40    # entries behind contributor k: enough for the pixels next to the centre to terminate too


def termination(coord, depth):
    rows = []
    for k, tile in zip(TERMINATION_K, _TERM_TILES):
        u, v = _centre(tile)
        op = 1.0 if k == 2 else 1.0 - 1e-4 ** (1.0 / (k - 0.5))      # (1 - op)^(k - 1) >= 1e-4 > (1 - op)^k; k = 2: the clamp, 0.01 * 0.01
        rows += _stack(u, v, k + TERMINATION_TAIL, 2.2, op, dz=0.01)
    return _from_rows(64, 64, coord, depth, rows, 0)


def termination_conditions(inp, dec):
    last = dec.last
    behind = dec.last.astype(np.int64) < image_n(inp)
    c = {}
    for k, tile in zip(TERMINATION_K, _TERM_TILES):
        u, v = _centre(tile)
        c[f"the centre pixel of stack {k} terminates at contributor {k}"] = bool(last[v, u] == k - 1 and dec.kill[tile, k - 1, 8 * 16 + 8])
        c[f"the list of stack {k} is 8 longer"] = bool(inp.n[tile] >= k + 8)
    c["every k - 1 is a last contributor"] = set(k - 1 for k in TERMINATION_K) <= set(np.unique(last).tolist())
    c["100 pixels have entries behind their last contributor"] = int((behind & (last > 0)).sum()) >= 100
    done = dec.kill.any(1)                                               # [tiles, 256]
    blocks = done.reshape(inp.tiles, 4, 4, 2, 8)                           # rows of 4, then 8 x 4 blocks: [tile, brow, row, bcol, col]
    mixed = blocks.any((2, 4)) & ~blocks.all((2, 4))
    c["an 8 x 4 block holds terminated and live pixels"] = bool(mixed.any())
    later = [bool((last[_centre(t)[1] - 1:_centre(t)[1] + 2, _centre(t)[0] - 1:_centre(t)[0] + 2] >= k - 1).all()) for k, t in zip(TERMINATION_K, _TERM_TILES)]
    c["off-centre pixels terminate later or never"] = all(later)
    return c


MEDIAN_M = (1, 2, 16, 17, 64, 65)
_MED_TILES = (5, 6, 9, 10, 1, 4)


def median(coord, depth):
    rows = []
    for m, tile in zip(MEDIAN_M, _MED_TILES):
        u, v = _centre(tile)
        rows += _stack(u, v, m + 8, 2.0, 1.0 - 0.5 ** (1.0 / (m - 0.5)), dz=0.02)      # (1 - op)^(m - 1) > 0.5 >= (1 - op)^m
    u, v = _centre(7)
    rows += _stack(u, v, 5, 2.0, 0.05)                                                   # never crosses: the median is the last contributor
    return _from_rows(64, 64, coord, depth, rows, 0)


def median_conditions(inp, dec):
    c = {}
    for m, tile in zip(MEDIAN_M, _MED_TILES):
        u, v = _centre(tile)
        c[f"the centre pixel of stack {m} has median contributor {m}"] = bool(dec.median[v, u] == m)
    c["every m is a median contributor"] = set(MEDIAN_M) <= set(np.unique(dec.median).tolist())
    never = (dec.last > 0) & (dec.median == dec.last)
    c["pixels that never cross: median == last"] = int(never.sum()) >= 16 and bool(never[_centre(7)[1], _centre(7)[0]])
    first = dec.act[:, 0] & (dec.a_raw[:, 0] > 0.5)
    c["pixels whose first alpha exceeds 0.5"] = bool(first.any())
    return c


LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 0)


def lengths(coord, depth, seed=LENGTHS_SEED):
    rng = np.random.default_rng(seed)
    rows = []
    for tile, n in enumerate(LENGTHS):
        u0, v0 = 16 * (tile % 4), 16 * (tile // 4)
        for i in range(n):
            rows.append((u0 + rng.uniform(5.5, 10.5), v0 + rng.uniform(5.5, 10.5), rng.uniform(2, 6), rng.uniform(0.8, 1.2),
                         rng.uniform(0.3, 1.0) * min(0.5, 5.0 / n)))
    return _from_rows(64, 64, coord, depth, rows, seed, aniso=0.1)


def lengths_conditions(inp, dec):
    blocks_hit = dec.act.reshape(inp.tiles, -1, 4, 4, 2, 8).any((3, 5))        # [tile, entry, brow, bcol]
    nblk = blocks_hit.reshape(inp.tiles, -1, 8).sum(2)
    return {"the list lengths are the set": sorted(inp.n.tolist()) == sorted(LENGTHS) and inp.n.tolist() == list(LENGTHS),
            "nobody terminates": not dec.kill.any(), "every entry is blended somewhere": bool((dec.act.any(2) | ~inp.instance_index()[1]).all()),
            "splats straddle block borders": int((nblk > 1).sum()) >= 100,
            "block lists differ from tile lists": int(((nblk >= 1) & (nblk < 8)).sum()) >= 100}


RAGGED_SIZES = ((1, 1), (17, 9), (33, 5), (16, 16), (15, 31))


def ragged(W, H):
    def build(coord, depth, seed=RAGGED_SEED):
        rng = np.random.default_rng(seed + 31 * W + H)
        n = 40
        u, v = rng.uniform(-6, W + 5, n), rng.uniform(-6, H + 5, n)
        u[:8], v[8:16] = W - 1, H - 1                                          # on the last column / the last row
        u[16:20], v[16:20] = W + 2.0, rng.uniform(0, H, 4)                      # outside, next to it
        u[20:24], v[20:24] = rng.uniform(0, W, 4), H + 2.0
        return _scene(W, H, coord, depth, u, v, rng.uniform(2, 8, n), rng.uniform(1.0, 5.0, n), rng.uniform(0.05, 0.9, n), seed, aniso=0.25)
    return build


def ragged_conditions(inp, dec):
    mx, my = inp.rec[:, 0].astype(np.float64), inp.rec[:, 1].astype(np.float64)
    listed = np.zeros(inp.P, bool)
    listed[inp.point_list] = True
    blended = np.zeros(inp.P, bool)
    idx, valid = inp.instance_index()
    hit = dec.act.any(2) & valid
    blended[inp.point_list[idx[hit]]] = True
    outside = (mx > inp.W - 0.5) | (my > inp.H - 0.5) | (mx < -0.5) | (my < -0.5)
    edge = (np.abs(mx - (inp.W - 1)) < 0.01) | (np.abs(my - (inp.H - 1)) < 0.01)
    return {"a blended splat has its centre outside the image": bool((blended & outside).any()),
            "a blended splat has its centre on the last row or column": bool((blended & edge).any()),
            "lanes outside the image, or exactly one full tile": bool((~inp.inside).any()) or (inp.W, inp.H) == (16, 16),
            "half of the pixels are blended into": float((dec.last > 0).mean()) >= 0.5}


class Case(NamedTuple):
    name: str
    build: object          # (coord, depth) -> Scene
    conditions: object     # (BlendInput, Decisions) -> {text: bool}
    modes: tuple


CASES = {c.name: c for c in [
    Case("band", band, band_conditions, MODES_ALL), Case("clamp", clamp, clamp_conditions, MODES_GEO),
    Case("termination", termination, termination_conditions, MODES_ALL), Case("median", median, median_conditions, MODES_GEO),
    Case("lengths", lengths, lengths_conditions, MODES_GEO)] + [
    Case(f"ragged-{W}x{H}", ragged(W, H), ragged_conditions, MODES_GEO) for W, H in RAGGED_SIZES]}
CASE_MODES = [(name, coord, depth) for name, c in CASES.items() for coord, depth in c.modes]


def case_id(p):
    return f"{p[0]}-{'coord' if p[1] else ''}{'+' if p[1] and p[2] else ''}{'depth' if p[2] else ''}{'colour' if not (p[1] or p[2]) else ''}"


def cotangents(s):
    """all seven cotangents non-zero, whatever the mode produces (the kernels must ignore those of maps they do not write)"""
    g = upstream_grads(s._replace(require_coord=True, require_depth=True), 7)
    assert all(bool((v != 0).any()) for v in g.values())
    return g


# ================================================================================================ the mutations (sharpness)
def mutate(name, inp, dec):
    """One mutation of the reference -> kwargs for restate(), or None where the case has nothing to mutate that way."""
    if name == "flip one in-band decision":
        hi, lo = band_pairs(dec, 1e-4)
        cand = np.argwhere((hi & dec.act) | (lo & ~dec.kill & (dec.T_before > 0.3)))
        if not len(cand):
            return None
        t, e, p = cand[0]
        act = dec.act.copy()
        act[t, e, p] = ~act[t, e, p]
        return dict(act=act)
    if name == "gate the gradient at the clamp":
        return dict(gate_clamp=True) if (dec.act & (dec.a_raw > C99)).any() else None
    if name == "move one median by one entry":
        m = dec.median.astype(np.int64)
        tp = inp.from_image(m)                                        # [tiles, 256]
        prev_act = np.zeros_like(tp, dtype=bool)
        ok = inp.inside & (tp >= 2) & (tp != NONE_MEDIAN)
        t_, p_ = np.nonzero(ok)
        prev_act[t_, p_] = dec.act[t_, tp[t_, p_] - 2, p_]
        cand = np.argwhere(prev_act)
        if not len(cand):
            return None
        t, p = cand[len(cand) // 2]
        med = dec.median.copy()
        med[inp.py[t, p], inp.px[t, p]] -= 1
        return dict(median=med)
    if name == "drop the last entry of a 64-entry batch":
        tl = np.flatnonzero((inp.n >= 64) & dec.act[:, min(63, dec.act.shape[1] - 1)].any(1)) if dec.act.shape[1] >= 64 else []
        if not len(tl):
            return None
        act = dec.act.copy()
        act[tl[0], 63] = False
        return dict(act=act)
    if name == "blend the terminating entry":
        if not dec.kill.any():
            return None
        gain = np.where(dec.kill, np.fmin(dec.a_raw.astype(np.float64), C99) * dec.T_before, 0.0)
        t, e, p = np.unravel_index(int(np.argmax(gain)), gain.shape)
        act = dec.act.copy()
        act[t, e, p] = True
        return dict(act=act)
    raise KeyError(name)


MUTATIONS = {"flip one in-band decision": ("band",), "gate the gradient at the clamp": ("clamp",),
             "move one median by one entry": ("median",), "drop the last entry of a 64-entry batch": ("lengths", "termination"),
             "blend the terminating entry": ("termination", "clamp")}
