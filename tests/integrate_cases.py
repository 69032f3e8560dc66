"""TEST INFRASTRUCTURE for the direct tests of the integrate kernels (csrc/rg_integrate.inc; tests/test_integrate_cases.py on the CPU,
tests/test_gpu_integrate_direct.py on the MI355X).  Pure numpy, importable without a GPU.

    IntegrateInput         what integrate_kernel reads: the splat_a records, the inte_rec pairs, the tile ranges, point_list, bg, and the
                           projected query points (p2d, pdepth, ppix, pt_sorted, pix_incl)
    project32(...)         points_preprocess_kernel in numpy float32, one rounding per operation
    decide(inp)            (a), the image: five_sample and image_pass in float32 -- per (pixel, entry) used, pass0 and the five cT; per pixel
                           last, n_local, capped, the median plane, final_T and the seven written planes of out9
    walk32(inp, dec)       (a), the points: point_alpha, point_blend and store_point in float32 -- per (point, entry) visited (used and
                           position <= last), step-rejected, blended (alpha >= 1/255); the four point outputs
    restate64(inp, dec, w) (b) the same values in float64, every decision of (a) taken as given, from the float32 records as given
    CASES, MUTATIONS       the case builders with the conditions each must meet; what the criterion must be able to see

Order of operations: that of rg_integrate.inc and rg_math.h, whose unit is built -ffp-contract=off.  Neither the exponent threshold of the
staged record (splat_a slot 6) nor the strip's batch cull (stage_record) is restated: both only skip work that cannot pass, so (a) follows the
oracle's arithmetic and the GPU tests, which ask for (a)'s decisions exactly, see it if either ever decides something.

The criterion is blend_cases.needed_c: |x - r| <= c 2^-24 (n + 16) A.  `n` is the number of entries walked: the length of the pixel's tile
list for the accumulated image planes and final_T, the pixel's last contributor for alpha_integrated; 0 for what is no sum over the list
(the median and maximum depth planes 4 and 6, sdf).  `A` is the sum of the absolute values of the terms at the grain they are added:
    colour               sum |rgb_i| alpha_i T_i + T_final |bg|          plane 7   sum alpha_i T_i            final_T   T_final
    planes 3, 4, 6       (|ts| + |rpx dx| + |rpy dy|) alpha_i T_i, or of the one entry selected
    alpha_integrated     sum T_i alpha_i (1 + K_i) over the blended entries; K_i = 1/2 sum_jk |inv_jk| a_j a_k with a = (|dx|, |dy|,
                         |B.w| + |min(qd, depth)|) for an unclamped entry -- the operands of the cancelling subtraction, which are what a
                         float32 evaluation's error scales with -- and 0 for a clamped one (alpha = 0.99 whatever the exponent)
    sdf                  |mid_dc| + |mid_px dx| + |mid_py dy| + |qd|
C_INT is the smallest c chain (a) needs against (b) over all cases (tests/test_integrate_cases.py recomputes it); the kernels get 2 C_INT
for the reasons given in blend_cases.py: the hardware exp2 / rcp + Newton step and a different but fixed order are legitimate.

The +80 clamp of deviation (3) needs a stored matrix that is not positive semi-definite, which the public entry cannot
produce (an ill-conditioned Gaussian stores zero): out of scope here."""
import functools
from typing import NamedTuple

import numpy as np
import torch

import blend_cases as bc
from blend_cases import _from_rows, _stack, needed_c
from stream_lists import exp_spec32, splat_power32

F = np.float32
EPS = 2.0 ** -24
K255 = F(1.0) / F(255.0)
K99 = F(0.99)
KDONE = F(0.0001)
NOT_PROJECTED = 0xFFFFFFFF
MAX_CONTRIBUTORS = 2048            # kMaxContributors
BITS_REACH = 12 * 64               # kUsedBatches * 64: longer lists replay the 5-sample test in phase 2
OFFX = np.array([0.0, -0.5, 0.5, -0.5, 0.5], F)
OFFY = np.array([0.0, -0.5, -0.5, 0.5, 0.5], F)

# The smallest c chain (a) needs against (b) over every case below, measured on the CPU (0.6200: plane 7, the alpha image, of `step`; the
# worst of cap / reach / band / edges are 0.41 / 0.47 / 0.09 / 0.43), rounded up to two digits.  tests/test_integrate_cases.py::
# test_c_int_is_what_chain_a_needs holds the stored number to the measured one: not smaller, at most 1.25 x larger.
C_INT = 0.62


# ================================================================================================ the kernel's input
class IntegrateInput(bc.BlendInput):
    def __init__(self, W, H, bg, rec, inte, ranges, point_list, p2d, pdepth, ppix, pt_sorted, pix_incl):
        super().__init__(W, H, False, True, bg, 1.0, 1.0, rec, None, ranges, point_list)
        self.inte = np.ascontiguousarray(inte, F).reshape(-1, 8)
        self.PN = int(np.asarray(ppix).shape[0])
        self.p2d = np.ascontiguousarray(p2d, F).reshape(self.PN, 2)
        self.pdepth = np.ascontiguousarray(pdepth, F).reshape(self.PN)
        self.ppix = np.ascontiguousarray(ppix).astype(np.uint32).reshape(self.PN)
        self.pt_sorted = np.ascontiguousarray(pt_sorted).astype(np.uint32).reshape(-1)
        self.pix_incl = np.ascontiguousarray(pix_incl).astype(np.uint32).reshape(self.H * self.W)
        self.projected = self.ppix != NOT_PROJECTED
        self.pix_points = np.diff(np.concatenate([[0], self.pix_incl.astype(np.int64)])).reshape(self.H, self.W)

    def point_slots(self):
        """of every projected point (ids q): its tile and its lane in the tile"""
        q = np.flatnonzero(self.projected)
        pix = self.ppix[q].astype(np.int64)
        x, y = pix % self.W, pix // self.W
        return q, (y // 16) * self.gx + x // 16, (y % 16) * 16 + x % 16


def bins_of(ppix, W, H):
    """pt_sorted and pix_incl of a counting sort on the pixel index (the order inside a pixel is free: no output depends on it)"""
    ppix = np.asarray(ppix, np.uint32)
    q = np.flatnonzero(ppix != NOT_PROJECTED)
    order = q[np.argsort(ppix[q], kind="stable")]
    counts = np.bincount(ppix[q].astype(np.int64), minlength=W * H)
    return order.astype(np.uint32), np.cumsum(counts).astype(np.uint32)


def _records_from_oracle(o, P):
    rec = np.zeros((P, 16), F)
    co = o.get("conic_opacity", (P, 4))
    rec[:, 0:2] = o.get("means2D", (P, 2))
    rec[:, 2:5] = co[:, 0:3]
    rec[:, 5] = co[:, 3]
    rec[:, 7] = o.get("ts", (P,))
    rec[:, 8:11] = o.get("rgb", (P, 3))
    rec[:, 11:13] = o.get("ray_planes", (P, 2))
    inte = np.zeros((P, 8), F)
    inte[:, 0:6] = o.get("invraycov", (P, 6))
    inte[:, 6] = o.get("condition", (P,))
    return rec, inte


def input_from_oracle(o, s, pts):
    """From the float32 oracle's state after o.integrate(pts)."""
    P, PN = s.means3D.shape[0], len(pts)
    rec, inte = _records_from_oracle(o, P)
    p2d, pdepth = o.get("points2D", (PN, 2)), o.get("point_depths", (PN,))
    # a projected point has pv.z > 0.2.  A point whose projection is NaN passes the reference's reject test (so the oracle keeps NaN here) and
    # then belongs to no pixel: not projected, as far as any output can tell
    proj = pdepth > 0
    p2d, pdepth = np.where(proj[:, None], p2d, F(0)), np.where(proj, pdepth, F(0))
    with np.errstate(all="ignore"):
        pix = np.floor(p2d[:, 1]).astype(np.int64) * s.W + np.floor(p2d[:, 0]).astype(np.int64)
    ppix = np.where(proj, pix, NOT_PROJECTED).astype(np.uint32)
    pt_sorted, pix_incl = bins_of(ppix, s.W, s.H)
    tiles = ((s.W + 15) // 16) * ((s.H + 15) // 16)
    return IntegrateInput(s.W, s.H, s.bg.numpy(), rec, inte, o.get("ranges")[: 2 * tiles], o.get("point_list"), p2d, pdepth, ppix, pt_sorted,
                          pix_incl)


def input_from_hip(C, s, PN, st):
    """From the state one _C.integrate_gaussians_to_points under KEEP_ACC left: st is its 10-tuple, the point state is C.LAST_POINT_STATE."""
    P, R, W, H = s.means3D.shape[0], int(st[0]), s.W, s.H
    tiles = ((W + 15) // 16) * ((H + 15) // 16)

    def main(name, dtype, n):
        return C.debug_export(name, dtype, n, P, R, W, H, False, st[7], st[8], st[9]).cpu().numpy()

    def pt(name, dtype, n):
        return C.debug_export_points(name, dtype, n, P, PN, W, H).cpu().numpy()
    rec = main("splat_a", torch.float32, 16 * P).reshape(P, 16)
    ranges = main("ranges", torch.int32, 2 * tiles).view(np.uint32)
    pl = main("point_list", torch.int32, R).view(np.uint32) if R else np.zeros(0, np.uint32)
    ppix = pt("ppix", torch.int32, PN).view(np.uint32)
    n_proj = int((ppix != NOT_PROJECTED).sum())
    inp = IntegrateInput(W, H, s.bg.numpy(), rec, pt("inte_rec", torch.float32, 8 * P), ranges, pl, pt("p2d", torch.float32, 2 * PN),
                         pt("pdepth", torch.float32, PN), ppix, pt("pt_sorted", torch.int32, PN).view(np.uint32)[:n_proj],
                         pt("pix_incl", torch.int32, H * W).view(np.uint32))
    inp.pix_count = pt("pix_count", torch.int32, H * W).view(np.uint32)
    inp.final_T = pt("final_T", torch.float32, H * W).reshape(H, W)
    return inp


# ================================================================================================ the projection
def focal32(s):
    return F(s.W) / (F(2.0) * F(s.tanfovx)), F(s.H) / (F(2.0) * F(s.tanfovy))


def project32(points, view, fx, fy, W, H, nan_passes=False):
    """points_preprocess_kernel: xform43 in the header's order; the division in float32, the add in double, the cast; the reject test (written
    as acceptance; nan_passes=True: the rejecting form, which a NaN passes -- the mutation); sqrtf; floor.  view: the 16 floats as the kernel
    gets them (the transposed matrix).  Returns p2d, pdepth (zero where not projected) and ppix."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    m = np.ascontiguousarray(view, F).reshape(16)
    fx, fy = F(fx), F(fy)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        pv = [((m[k] * x + m[4 + k] * y) + m[8 + k] * z) + m[12 + k] for k in range(3)]
        front = ~(pv[2] <= F(0.2))
        den = pv[2] + F(0.0000001)
        ix = (((fx * pv[0]) / den).astype(np.float64) + W / 2.0).astype(F)
        iy = (((fy * pv[1]) / den).astype(np.float64) + H / 2.0).astype(F)
        if nan_passes:
            ok = front & ~((ix < 0) | (ix >= W) | (iy < 0) | (iy >= H))
        else:
            ok = front & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        depth = np.sqrt((pv[0] * pv[0] + pv[1] * pv[1]) + pv[2] * pv[2])
        fxi = np.where(np.isnan(ix), 0, np.floor(ix)).astype(np.int64)          # f2i_sat(NaN) == 0
        fyi = np.where(np.isnan(iy), 0, np.floor(iy)).astype(np.int64)
    pix = (fyi * W + fxi).astype(np.uint32)
    p2d = np.where(ok[:, None], np.stack([ix, iy], 1), F(0)).astype(F)
    return p2d, np.where(ok, depth, F(0)).astype(F), np.where(ok, pix, np.uint32(NOT_PROJECTED)).astype(np.uint32)


# ================================================================================================ (a) the image
class Decisions(NamedTuple):
    used: np.ndarray       # [tiles, L, 256] bool: some sample of the 5-sample test passed (and the pixel was not done)
    pass0: np.ndarray      # the centre sample passed
    cT: np.ndarray         # [tiles, L, 256, 5] float32: the five transmittances BEFORE the entry
    last: np.ndarray       # [H, W] uint32: last contributor (1-based list position; 0: none)
    n_local: np.ndarray    # [H, W] used entries
    capped: np.ndarray     # [H, W] bool: stopped by the cap
    median: np.ndarray     # [H, W] int64: 1-based position of the entry whose plane the pixel keeps (0: none)
    final_T: np.ndarray    # [H, W] float32
    out9: np.ndarray       # [9, H, W] float32; planes 5 and 8 are not the image pass's
    would_use: np.ndarray  # [tiles, L, 256] bool: `used` of the same chain WITHOUT the cap


def _five(inp, e, tl, cT):
    """the five samples of list entry e for the tiles tl: pass [k, 256, 5], alpha, depth, test_T"""
    r = inp.rec[inp.point_list[inp.ranges[tl, 0] + e]][:, None, None, :]            # [k, 1, 1, 16]
    pixfx = (inp.px[tl].astype(F) + F(0.5))[:, :, None]
    pixfy = (inp.py[tl].astype(F) + F(0.5))[:, :, None]
    with np.errstate(all="ignore"):
        dx, dy = (r[..., 0] - pixfx) - OFFX, (r[..., 1] - pixfy) - OFFY
        depth = r[..., 7] + (r[..., 11] * dx + r[..., 12] * dy)
        power = splat_power32(r[..., 2], r[..., 3], r[..., 4], dx, dy)
        alpha = np.fmin(K99, r[..., 5] * exp_spec32(power))
        test_T = cT * (F(1.0) - alpha)
        ok = ~(power > F(0.0)) & ~(alpha < K255) & ~(test_T < KDONE)
    return ok, alpha, depth, test_T, r


def decide(inp, cap=MAX_CONTRIBUTORS):
    tiles, L = inp.tiles, inp.L
    shape = (tiles, max(L, 1), 256)
    used, pass0, would = (np.zeros(shape, bool) for _ in range(3))
    cT_all = np.ones(shape + (5,), F)
    cT, cTw = np.ones((tiles, 256, 5), F), np.ones((tiles, 256, 5), F)             # cTw: the chain without the cap
    done = ~inp.inside
    last, n_local, median = (np.zeros((tiles, 256), np.int64) for _ in range(3))
    C = np.zeros((8, tiles, 256), F)
    bg = inp.bg.astype(F)
    for e in range(L):
        tl = np.flatnonzero(inp.n > e)
        okw = _five(inp, e, tl, cTw[tl])
        cTw[tl] = np.where(okw[0], okw[3], cTw[tl])
        would[tl, e] = okw[0].any(2) & inp.inside[tl]
        cT_all[tl, e] = cT[tl]
        ok, alpha, depth, test_T, r = _five(inp, e, tl, cT[tl])
        ok = ok & ~done[tl][:, :, None]
        u, p0 = ok.any(2), ok[:, :, 0]
        T = cT[tl][:, :, 0]
        with np.errstate(all="ignore"):
            a0, d0 = alpha[:, :, 0], depth[:, :, 0]
            dmax = np.where(ok, depth, F(-np.inf)).max(2)
            Ct = C[:, tl]
            Ct[6] = np.where(u & (dmax > Ct[6]), dmax, Ct[6])
            for ch in range(3):
                Ct[ch] = np.where(p0, Ct[ch] + (r[:, :, 0, 8 + ch] * a0) * T, Ct[ch])
            Ct[7] = np.where(p0, Ct[7] + a0 * T, Ct[7])
            Ct[3] = np.where(p0, Ct[3] + (d0 * a0) * T, Ct[3])
            med = p0 & (T > F(0.5))
            Ct[4] = np.where(med, d0, Ct[4])
            C[:, tl] = Ct
        median[tl] = np.where(med, e + 1, median[tl])
        cT[tl] = np.where(ok, test_T, cT[tl])
        used[tl, e], pass0[tl, e] = u, p0
        last[tl] = np.where(u, e + 1, last[tl])
        n_local[tl] += u
        done[tl] |= n_local[tl] >= cap
    T = cT[:, :, 0]
    out9 = np.zeros((9, tiles, 256), F)
    for ch in range(3):
        out9[ch] = C[ch] + T * bg[ch]
    out9[3], out9[4], out9[6], out9[7] = C[3], C[4], C[6], C[7]
    img = inp.to_image
    return Decisions(used, pass0, cT_all, img(last).astype(np.uint32), img(n_local), img((n_local >= cap) & inp.inside), img(median), img(T),
                     img(out9), would)


# ================================================================================================ (a) the points
class Walk(NamedTuple):
    q: np.ndarray          # [M] ids of the projected points, tile / lane of their pixel
    tile: np.ndarray
    lane: np.ndarray
    visited: np.ndarray    # [M, L] bool: used by the point's pixel, position <= its last contributor
    stepped: np.ndarray    # visited, ill-conditioned, qd < depth: the step returns 0
    blended: np.ndarray    # visited and alpha >= 1/255
    alpha: np.ndarray      # [M, L] float32 what point_alpha returned at the visited entries
    nearer: np.ndarray     # [M, L] bool: visited, well-conditioned, fminf(qd, depth) returned qd
    alpha_integrated: np.ndarray   # [PN] float32, initial values where not projected
    color_integrated: np.ndarray   # [PN, 3]
    coordinate2d: np.ndarray       # [PN, 2]
    sdf: np.ndarray                # [PN]


def _point_geometry(inp, e, tile, qx, qy, qd, X):
    """(dx, dy, depth, dz, well, record, inverse) of list entry e at the points (of tiles with a list that long), in precision X"""
    g = inp.point_list[inp.ranges[tile, 0] + e]
    r, I = inp.rec[g].astype(X), inp.inte[g].astype(X)
    dx, dy = r[:, 0] - qx, r[:, 1] - qy
    depth = r[:, 7] + (r[:, 11] * dx + r[:, 12] * dy)
    well = inp.inte[g, 6] != 0
    dz = np.where(well, r[:, 7] - np.fmin(qd, depth), r[:, 7])
    return dx, dy, depth, dz, well, r, I


def _point_power(dx, dy, dz, I, X):
    wx = (I[:, 0] * dx + I[:, 1] * dy) + I[:, 2] * dz
    wy = (I[:, 1] * dx + I[:, 3] * dy) + I[:, 4] * dz
    wz = (I[:, 2] * dx + I[:, 4] * dy) + I[:, 5] * dz
    return X(-0.5) * ((dx * wx + dy * wy) + dz * wz)


def walk32(inp, dec, step_le=False, flip=None, past_last=None, used=None):
    """step_le: `qd <= depth` in place of `<`; flip (m, e): that blend decision inverted; past_last m: that point also visits the entry behind
    its pixel's last contributor; used: other used bits (the mutations)."""
    q, tile, lane = inp.point_slots()
    M, L = len(q), max(inp.L, 1)
    visited, stepped, blended, nearer = (np.zeros((M, L), bool) for _ in range(4))
    alpha_all = np.zeros((M, L), F)
    qx, qy, qd = inp.p2d[q, 0], inp.p2d[q, 1], inp.pdepth[q]
    pa, pT = np.zeros(M, F), np.ones(M, F)
    ubits = dec.used if used is None else used
    lastq = dec.last[inp.ppix[q] // inp.W, inp.ppix[q] % inp.W].astype(np.int64)
    bound = lastq.copy()
    if past_last is not None:
        bound[past_last] += 1
    for e in range(inp.L):
        sel = np.flatnonzero((inp.n[tile] > e) & (e < bound))
        if not len(sel):
            continue
        u = ubits[tile[sel], e, lane[sel]]
        if past_last is not None:
            u = u | ((sel == past_last) & (e == lastq[past_last]))
        sel = sel[u]
        if not len(sel):
            continue
        with np.errstate(all="ignore"):
            dx, dy, depth, dz, well, r, I = _point_geometry(inp, e, tile[sel], qx[sel], qy[sel], qd[sel], F)
            rej = ~well & ((qd[sel] <= depth) if step_le else (qd[sel] < depth))
            a = np.fmin(K99, r[:, 5] * exp_spec32(np.fmin(_point_power(dx, dy, dz, I, F), F(80.0))))
            a = np.where(rej, F(0.0), a).astype(F)
            bl = ~(a < K255)
            if flip is not None and flip[1] == e:
                bl = np.where(sel == flip[0], ~bl, bl)
            pa[sel] = np.where(bl, pa[sel] + a * pT[sel], pa[sel])
            pT[sel] = np.where(bl, pT[sel] * (F(1.0) - a), pT[sel])
        visited[sel, e], stepped[sel, e], blended[sel, e], alpha_all[sel, e] = True, rej, bl, a
        nearer[sel, e] = well & ~(depth < qd[sel])
    PN = inp.PN
    ai, ci, c2, sdf = np.ones(PN, F), np.zeros((PN, 3), F), np.zeros((PN, 2), F), np.full(PN, -1000.0, F)
    ai[q] = pa
    py_, px_ = inp.ppix[q] // inp.W, inp.ppix[q] % inp.W
    ci[q] = dec.out9[0:3, py_, px_].T
    c2[q] = inp.p2d[q]
    sdf[q] = _sdf(inp, dec, q, F)[0]
    return Walk(q, tile, lane, visited, stepped, blended, alpha_all, nearer, ai, ci, c2, sdf)


def _sdf(inp, dec, q, X):
    """store_point's signed distance (and the sum of the absolute values of its terms); a pixel without a median plane keeps zeros"""
    py_, px_ = inp.ppix[q] // inp.W, inp.ppix[q] % inp.W
    t = (py_ // 16) * inp.gx + px_ // 16
    m = dec.median[py_, px_]
    g = inp.point_list[np.minimum(inp.ranges[t, 0] + np.maximum(m, 1) - 1, max(inp.R - 1, 0))] if inp.R else np.zeros(len(q), np.int64)
    r = np.where((m > 0)[:, None], inp.rec[g] if inp.R else np.zeros((len(q), 16), F), F(0)).astype(X)
    qx, qy, qd = inp.p2d[q, 0].astype(X), inp.p2d[q, 1].astype(X), inp.pdepth[q].astype(X)
    dx, dy = r[:, 0] - qx, r[:, 1] - qy
    depth = r[:, 7] + (r[:, 11] * dx + r[:, 12] * dy)
    return depth - qd, np.abs(r[:, 7]) + np.abs(r[:, 11] * dx) + np.abs(r[:, 12] * dy) + np.abs(qd)


# ================================================================================================ (b) the float64 restatement
class Restated:
    """out9 / out9_A [9, H, W] (planes 0-4, 6, 7), final_T / final_T_A [H, W]; alpha_integrated, color_integrated, sdf and their _A per point;
    n_pix [H, W] and n_pt [PN]: the entries walked"""


def restate64(inp, dec, w):
    D = np.float64
    tiles, L = inp.tiles, inp.L
    T = np.ones((tiles, 256), D)
    S, A = np.zeros((8, tiles, 256), D), np.zeros((8, tiles, 256), D)
    pixfx, pixfy = inp.px.astype(D) + 0.5, inp.py.astype(D) + 0.5
    rec = inp.rec.astype(D)
    for e in range(L):
        tl = np.flatnonzero(inp.n > e)
        r = rec[inp.point_list[inp.ranges[tl, 0] + e]][:, None, None, :]
        dx, dy = (r[..., 0] - pixfx[tl][:, :, None]) - OFFX.astype(D), (r[..., 1] - pixfy[tl][:, :, None]) - OFFY.astype(D)
        dterm = np.abs(r[..., 7]) + np.abs(r[..., 11] * dx) + np.abs(r[..., 12] * dy)
        depth = r[..., 7] + (r[..., 11] * dx + r[..., 12] * dy)
        # which samples passed is (a)'s decision
        ok = _passed(inp, dec, e, tl)
        u, p0 = dec.used[tl, e], dec.pass0[tl, e]
        with np.errstate(all="ignore"):
            power = -0.5 * (r[..., 2] * dx * dx + r[..., 4] * dy * dy) - r[..., 3] * dx * dy
            a0 = np.minimum(float(K99), r[..., 5] * np.exp(power))[:, :, 0]
        a0 = np.where(p0, a0, 0.0)
        dmax = np.where(ok, depth, -np.inf).max(2)
        dmaxA = np.where(ok, dterm, 0.0).max(2)
        St, At, Tt = S[:, tl], A[:, tl], T[tl]
        upd = u & (dmax > St[6])
        St[6], At[6] = np.where(upd, dmax, St[6]), np.where(upd, dmaxA, At[6])
        for ch in range(3):
            St[ch] += r[:, :, 0, 8 + ch] * a0 * Tt
            At[ch] += np.abs(r[:, :, 0, 8 + ch]) * a0 * Tt
        St[7] += a0 * Tt
        At[7] += a0 * Tt
        St[3] += depth[:, :, 0] * a0 * Tt
        At[3] += dterm[:, :, 0] * a0 * Tt
        med = inp.from_image(dec.median)[tl] == e + 1
        St[4], At[4] = np.where(med, depth[:, :, 0], St[4]), np.where(med, dterm[:, :, 0], At[4])
        S[:, tl], A[:, tl] = St, At
        T[tl] = Tt * (1.0 - a0)
    out = Restated()
    o9, o9A = np.zeros((9, tiles, 256), D), np.zeros((9, tiles, 256), D)
    for ch in range(3):
        o9[ch], o9A[ch] = S[ch] + T * inp.bg[ch], A[ch] + T * abs(inp.bg[ch])
    for k in (3, 4, 6, 7):
        o9[k], o9A[k] = S[k], A[k]
    out.out9, out.out9_A, out.final_T, out.final_T_A = inp.to_image(o9), inp.to_image(o9A), inp.to_image(T), inp.to_image(T)
    n_list = bc.image_n(inp)
    out.n_pix = np.stack([n_list, n_list, n_list, n_list, 0 * n_list, 0 * n_list, 0 * n_list, n_list, 0 * n_list])
    out.n_list = n_list
    # ---- the points ----
    q, tile = w.q, w.tile
    M, PN = len(q), inp.PN
    qx, qy, qd = inp.p2d[q, 0].astype(D), inp.p2d[q, 1].astype(D), inp.pdepth[q].astype(D)
    pa, paA, pT = np.zeros(M, D), np.zeros(M, D), np.ones(M, D)
    for e in range(L):
        sel = np.flatnonzero(w.blended[:, e])
        if not len(sel):
            continue
        with np.errstate(all="ignore"):
            dx, dy, depth, dz, well, r, I = _point_geometry(inp, e, tile[sel], qx[sel], qy[sel], qd[sel], D)
            raw = r[:, 5] * np.exp(np.minimum(_point_power(dx, dy, dz, I, D), 80.0))
        a = np.minimum(float(K99), raw)
        az = np.abs(r[:, 7]) + np.where(well, np.abs(np.fmin(qd[sel], depth)), 0.0)
        v = [np.abs(dx), np.abs(dy), az]
        idx = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
        K = 0.5 * sum(np.abs(I[:, idx[j][k]]) * v[j] * v[k] for j in range(3) for k in range(3))
        K = np.where(raw > float(K99), 0.0, K)
        pa[sel] += a * pT[sel]
        paA[sel] += a * pT[sel] * (1.0 + K)
        pT[sel] *= 1.0 - a
    out.alpha_integrated, out.alpha_integrated_A = np.ones(PN), np.ones(PN)
    out.alpha_integrated[q], out.alpha_integrated_A[q] = pa, paA
    py_, px_ = inp.ppix[q] // inp.W, inp.ppix[q] % inp.W
    out.color_integrated, out.color_integrated_A = np.zeros((PN, 3)), np.zeros((PN, 3))
    out.color_integrated[q], out.color_integrated_A[q] = out.out9[0:3, py_, px_].T, out.out9_A[0:3, py_, px_].T
    out.sdf, out.sdf_A = np.full(PN, -1000.0), np.full(PN, 1000.0)
    out.sdf[q], out.sdf_A[q] = _sdf(inp, dec, q, D)
    out.n_pt = np.zeros(PN, np.int64)
    out.n_pt[q] = dec.last[py_, px_]
    out.n_pt_list = np.zeros(PN, np.int64)
    out.n_pt_list[q] = n_list[py_, px_]
    return out


def _passed(inp, dec, e, tl):
    """[k, 256, 5] which samples of entry e passed in chain (a): recomputed from the recorded cT (the same float32 arithmetic)"""
    ok = _five(inp, e, tl, dec.cT[tl, e])[0]
    return ok & dec.used[tl, e][:, :, None]


OUTPUTS = ("out9", "final_T", "alpha_integrated", "color_integrated", "sdf")
PLANES = (0, 1, 2, 3, 4, 6, 7)


def need(got, ref):
    """{output: c} of a set of float32 results (out9 [9, H, W], final_T [H, W], alpha_integrated, color_integrated, sdf) against a Restated"""
    c = {f"out9[{k}]": needed_c(got["out9"][k], ref.out9[k], ref.out9_A[k], ref.n_pix[k])[0] for k in PLANES}
    c["final_T"] = needed_c(got["final_T"], ref.final_T, ref.final_T_A, ref.n_list)[0]
    c["alpha_integrated"] = needed_c(got["alpha_integrated"], ref.alpha_integrated, ref.alpha_integrated_A, ref.n_pt)[0]
    c["color_integrated"] = needed_c(got["color_integrated"], ref.color_integrated, ref.color_integrated_A, ref.n_pt_list[:, None])[0]
    c["sdf"] = needed_c(got["sdf"], ref.sdf, ref.sdf_A, 0)[0]
    return c


def chain_outputs(dec, w):
    return dict(out9=dec.out9, final_T=dec.final_T, alpha_integrated=w.alpha_integrated, color_integrated=w.color_integrated, sdf=w.sdf)


def exact_differences(inp, dec, w, got):
    """What must agree exactly between chain (a) and a set of results (got: chain_outputs' keys plus n_contrib [2, H, W], ppix, pix_incl,
    coordinate2d and optionally pix_count, pt_sorted, p2d, pdepth): {what: number of differing elements}, empty when all agree."""
    bad = {}

    def cmp(name, a, b):
        a, b = np.asarray(a), np.asarray(b)
        n = int((a.view(np.uint32) != b.view(np.uint32)).sum()) if a.dtype == F else int((a != b).sum())
        if n:
            bad[name] = n
    cmp("n_contrib plane 0 == last", got["n_contrib"][0], dec.last)
    cmp("n_contrib plane 1 == 0", got["n_contrib"][1], 0 * dec.last)
    cmp("out9[8] == points per pixel", got["out9"][8], inp.pix_points.astype(F))
    proj = inp.projected
    cmp("coordinate2d at projected points", got["coordinate2d"][proj], w.coordinate2d[proj])
    for k, init in (("alpha_integrated", 1.0), ("color_integrated", 0.0), ("coordinate2d", 0.0), ("sdf", -1000.0)):
        cmp(f"{k} keeps its initial value at unprojected points", got[k][~proj], np.full_like(got[k][~proj], init))
    return bad


# ================================================================================================ the cases
class Case(NamedTuple):
    name: str
    build: object          # () -> (Scene, points [PN, 3] float32)
    conditions: object     # (IntegrateInput, Decisions, Walk) -> {text: bool}


def _ray_points(s, ix, iy, z):
    """world points (identity pose) that project to pixel coordinates (ix, iy) at view depth z"""
    fx, fy = bc.focal(s)
    ix, iy, z = (np.asarray(a, np.float64).reshape(-1) for a in np.broadcast_arrays(ix, iy, z))
    return np.stack([(ix - s.W / 2.0) * z / fx, (iy - s.H / 2.0) * z / fy, z], 1).reshape(-1, 3).astype(F)


def _scene_of(W, H, rows, seed=0, aniso=0.0):
    return _from_rows(W, H, False, True, rows, seed, aniso)


def pixel_of(inp, x, y):
    return (y // 16) * inp.gx + x // 16, (y % 16) * 16 + x % 16


def near_threshold(w, width):
    """visited, not step-rejected (point, entry) pairs with |255 alpha - 1| < width: (at or above the threshold, below it)"""
    d = w.alpha.astype(np.float64) * 255.0 - 1.0
    near = w.visited & ~w.stepped & (np.abs(d) < width)
    return near & w.blended, near & ~w.blended


# ---- cap ----
CAP_K = (2047, 2048, 2100)
CAP_SIGMA, CAP_OPACITY, CAP_DZ = 2.0, 0.0043, 0.004
CAP_SEED = 38       # of the query points: fixed by a search on the CPU for 'no pair within 1e-3 of alpha = 1/255'
CAP_COUNTS = (1, 5, 9)


@functools.lru_cache(maxsize=None)
def cap():
    """Three tiles, one stack each on the tile's pixel corner (8, 8).  The splats are faint (alpha 0.0043 where G = 1: 2100 of them leave
    T = 1.2e-4 > 1e-4) and NARROW enough to stay inside their tile -- on a 48 x 16 image wide ones would put all three stacks into every
    list -- so a stack is used by the pixels that have a sample within ~0.8 px of (8, 8) and by no other: both kinds of pixel exist."""
    rows = []
    for t, k in enumerate(CAP_K):
        rows += _stack(16 * t + 8, 8, k, CAP_SIGMA, CAP_OPACITY, z0=2.0, dz=CAP_DZ)
    s = _scene_of(48, 16, rows)
    return s, cap_points(s, CAP_SEED)


def cap_points(s, seed):
    rng = np.random.default_rng(500 + seed)
    pts = []
    for t, k in enumerate(CAP_K):
        z_back = 2.0 + CAP_DZ * k + 0.5
        zs = np.array([1.5, 2.0 + CAP_DZ * (100 + rng.random()), 2.0 + CAP_DZ * (250 + rng.random()), z_back, z_back + 1, z_back + 2, 1.7, z_back + 3,
                       z_back + 20])
        # the four pixels around (8, 8) are used through their corner sample: 1, 5 and 9 points in three of them, near the corner (blended)
        for (px, py, sx, sy), cnt in zip(((8, 8, 0.3, 0.3), (7, 8, 0.7, 0.3), (8, 7, 0.3, 0.7)), CAP_COUNTS):
            pts.append(_ray_points(s, 16 * t + px + sx + 0.05 * rng.random(cnt), py + sy + 0.05 * rng.random(cnt), zs[:cnt] if cnt > 1 else zs[4:5]))
        pts.append(_ray_points(s, 16 * t + 7.05 + 0.1 * rng.random(4), 7.05 + 0.1 * rng.random(4), zs[[0, 3, 4, 5]]))   # far from the corner: visited, never blended
        pts.append(_ray_points(s, 16 * t + 12.5, 3.5, z_back))                                              # a pixel that uses nothing
    return np.concatenate(pts)


def cap_conditions(inp, dec, w):
    c = {"the three lists": inp.n.tolist() == list(CAP_K)}
    for t, k in enumerate(CAP_K):
        x, y = 16 * t + 8, 8
        c[f"stack {k}: the centre pixel uses {min(k, 2048)} entries"] = bool(dec.n_local[y, x] == min(k, 2048) and dec.last[y, x] == min(k, 2048))
        c[f"stack {k}: capped or not"] = bool(dec.capped[y, x]) == (k >= 2048)
    tile, lane = pixel_of(inp, 40, 8)
    c["40 entries behind the cap would be used"] = int(dec.would_use[tile, 2048:, lane].sum()) >= 40
    c["final_T > 1e-4 at every capped pixel"] = bool(dec.capped.any() and (dec.final_T[dec.capped] > 1e-4).all())
    c["pixels that use nothing"] = bool((dec.last == 0).any())
    counts = set(inp.pix_points[dec.capped].tolist())
    c["1, 5 and 9 points in capped pixels"] = set(CAP_COUNTS) <= counts
    capq = dec.capped[inp.ppix[w.q] // inp.W, inp.ppix[w.q] % inp.W]
    nb = w.blended.sum(1)
    c["points in front of, inside and behind a capped stack"] = bool((capq & (nb == 0) & (inp.pdepth[w.q] < 2)).any() and (capq & (nb > 50) & (nb < 1900)).any()
                                                                     and (capq & (nb == 2048)).any())
    c["visited but never blended points in capped pixels"] = bool((capq & (nb == 0) & (w.visited.sum(1) == 2048) & (inp.pdepth[w.q] > 10.5)).any())
    hi, lo = near_threshold(w, 1e-3)
    c["no pair within 1e-3 of alpha = 1/255"] = not (hi.any() or lo.any())
    return c


# ---- reach ----
REACH_N = (0, 1, 63, 64, 65, 767, 768, 769, 832)
REACH_PIXEL_COUNTS = (0, 1, 4, 5, 8, 9)
REACH_STRIP_TOTALS = (0, 1, 63, 64, 65, 129)
REACH_OPACITY = 0.006
REACH_EXTRA = 60              # an opaque stack in tile 8 (its list then has 832 + 60 + 2 entries): terminates, mixed `last` in the strips


@functools.lru_cache(maxsize=None)
def reach():
    """Nine tiles of 48 x 48 with lists of REACH_N equal splats (sigma 2.0: inside the tile) on the tile centre, faint enough for the last
    entry to be used still ((1 - 0.006)^832 = 6.7e-3).  Strips 0..3 of every tile hold 1 + 63 = 64, 65, 129 and 63 query points -- pixel
    counts 0, 1, 4, 5, 8, 9 -- and one tile row further down totals of 0 and 1 are found in tiles' strips that are left empty / hold one point.
    Tile 8 also carries an opaque stack BEHIND its 832 faint splats so that >= 100 pixels have entries behind their last contributor."""
    rows = []
    for t, n in enumerate(REACH_N):
        u, v = 16 * (t % 3) + 8, 16 * (t // 3) + 8
        rows += _stack(u, v, n - (n == 769), 2.0, REACH_OPACITY, z0=2.0, dz=0.002)
        if n == 769:      # the 769th entry is the first whose used bit has no place in LDS: a strong splat on a pixel that holds nine points
            rows += [(u - 1.5, v - 0.5, 2.0 + 0.002 * 768 + 0.05, 1.0, 0.5)]
        if t == 8:
            rows += _stack(u, v, REACH_EXTRA, 2.0, 0.45, z0=5.0, dz=0.01)
            rows += [(37.5, 46.0, 7.0, 0.2, 0.03)]      # LAST in the list and used by no pixel: behind every pixel's last contributor
            rows += [(46.5, 46.0, 1.9, 0.2, 0.03)]      # FIRST in the list, between the samples of pixel (46, 46), which uses nothing: used by no pixel, 0.03 at a point next to it
    s = _scene_of(48, 48, rows)
    rng = np.random.default_rng(11)
    pts = []

    def fill(x0, y0, counts, zlo, zhi):
        """pixel k of the row starting at (x0, y0) gets counts[k] points"""
        for k, cnt in enumerate(counts):
            if cnt:
                pts.append(_ray_points(s, x0 + k + 0.1 + 0.8 * rng.random(cnt), y0 + 0.1 + 0.8 * rng.random(cnt), rng.uniform(zlo, zhi, cnt)))
    for t, n in enumerate(REACH_N):
        x0, y0 = 16 * (t % 3), 16 * (t // 3)
        zhi = 2.0 + 0.002 * n + 1.0 + (1.5 if t == 8 else 0.0)
        # strip 1 (rows 4..7): 64 points; strip 2 (rows 8..11): 65 through the centre pixels, strip 3 (rows 12..15): 129; strip 0: 63
        fill(x0 + 4, y0 + 7, (9, 9, 9, 9, 8, 8, 5, 5, 1, 1), 1.5, zhi)              # 64
        fill(x0 + 5, y0 + 8, (9, 9, 9, 9, 9, 8, 8, 4), 1.5, zhi)                   # 65
        fill(x0 + 2, y0 + 12, (9,) * 13 + (8, ), 1.5, zhi)                          # 125
        fill(x0 + 6, y0 + 13, (4,), 1.5, zhi)                                        # + 4 = 129
        if t % 3 != 0:
            fill(x0 + 3, y0 + 3, (9, 9, 9, 9, 9, 9, 5, 4), 1.5, zhi)               # 63; the tiles of column 0 keep strip 0 for totals 0 and 1
        elif t == 3:
            fill(x0 + 8, y0 + 3, (1,), 1.5, zhi)
    pts.append(_ray_points(s, [46.5, 46.52], [46.05, 46.1], [8.0, 9.0]))        # behind everything, next to the splat no pixel uses
    return s, np.concatenate(pts)


def strip_totals(inp):
    gy4 = inp.gy * 4
    pp = np.zeros((inp.gy * 16, inp.gx * 16), np.int64)
    pp[: inp.H, : inp.W] = inp.pix_points
    return pp.reshape(gy4, 4, inp.gx, 16).sum((1, 3))          # [strip rows, tile columns]


def reach_conditions(inp, dec, w):
    c = {"the nine lists": inp.n.tolist() == list(REACH_N[:8]) + [REACH_N[8] + REACH_EXTRA + 2]}
    tot = strip_totals(inp)
    for t in range(9):
        mine = tot[4 * (t // 3): 4 * (t // 3) + 4, t % 3]
        if t % 3:            # (tile 8 has two more points in its last strip, next to the splat no pixel uses)
            c[f"tile {t}: strips of 63, 64, 65 and 129 points"] = sorted(mine.tolist()) == [63, 64, 65, 129 + 2 * (t == 8)]
        y0, x0 = 16 * (t // 3), 16 * (t % 3)
        c[f"tile {t}: pixels of 0, 1, 4, 5, 8, 9 points"] = set(REACH_PIXEL_COUNTS) <= set(inp.pix_points[y0:y0 + 16, x0:x0 + 16].reshape(-1).tolist())
    c["strip totals 0, 1, 63, 64, 65, 129"] = set(REACH_STRIP_TOTALS) <= set(tot.reshape(-1).tolist())
    has_pt = inp.from_image(inp.pix_points) > 0                                 # [tiles, 256]
    for t, pos in ((6, 705), (7, 705), (7, 769)):
        c[f"tile {t}: a pixel with a query point uses an entry at position >= {pos}"] = bool((dec.used[t, pos - 1:inp.n[t]].any(0) & has_pt[t]).any())
    c["every list's last entry is used (tiles 1..7)"] = all(bool(dec.used[t, inp.n[t] - 1].any()) for t in range(1, 8))
    behind = (dec.last.astype(np.int64) < bc.image_n(inp)) & (dec.last > 0)
    c["100 pixels have entries behind their last contributor"] = int(behind.sum()) >= 100
    lt = inp.from_image(dec.last)[8].reshape(4, 64)
    c["strips with mixed last"] = bool(((lt.max(1) > 832) & ((lt > 0).sum(1) > 1) & (lt.min(1) < lt.max(1))).any())
    return c


# ---- band ----
# fixed by a search on the CPU (the first seed that meets band_conditions): 9 / 6 pairs inside 1e-4 above / below the threshold, 95 more inside
# 1e-3, 7852 corner-only uses, 7624 pairs the centre passed and a corner rejected (test_integrate_cases.py::test_band_seed prints them)
BAND_SEED = 0


@functools.lru_cache(maxsize=None)
def band(seed=None):
    seed = BAND_SEED if seed is None else seed
    rng = np.random.default_rng(100 + seed)
    n = 170
    s = bc._scene(64, 64, False, True, rng.uniform(-8, 72, n), rng.uniform(-8, 72, n), rng.uniform(2, 10, n), rng.uniform(5, 16, n),
                  rng.uniform(0.01, 0.06, n), seed, aniso=0.25)
    m = 4000
    pts = _ray_points(s, rng.uniform(0, 64, m), rng.uniform(0, 64, m), rng.uniform(1.0, 12.0, m))
    return s, pts


def corner_only(dec):
    return dec.used & ~dec.pass0


def centre_rejected_corner(inp, dec):
    """(pixel, entry) pairs the centre sample passed and some corner sample did not"""
    n = 0
    for e in range(inp.L):
        tl = np.flatnonzero(inp.n > e)
        ok = _passed(inp, dec, e, tl)
        n += int((ok[:, :, 0] & ~ok[:, :, 1:].all(2)).sum())
    return n


def band_conditions(inp, dec, w):
    hi, lo = near_threshold(w, 1e-4)
    hi3, lo3 = near_threshold(w, 1e-3)
    ring = int(hi3.sum() + lo3.sum() - hi.sum() - lo.sum())
    return {"3 pairs inside 1e-4 above alpha = 1/255": int(hi.sum()) >= 3, "3 below": int(lo.sum()) >= 3, "50 more inside 1e-3": ring >= 50,
            "100 pairs used by a corner sample only": int(corner_only(dec).sum()) >= 100,
            "100 pairs passed by the centre and rejected at a corner": centre_rejected_corner(inp, dec) >= 100}


# ---- step ----
def _flat(s, which):
    sc = s.scales.clone()
    sc[which, 2] = 1e-6                      # test_hostcheck._flat_scene: lambda_min <= 1e-8, inte_rec flag 0, stored matrix zero
    return s._replace(scales=sc)


STEP_CENTRES = ((8, 8), (24, 8), (8, 24), (24, 24), (16, 16))


def step_scene():
    rows = []
    for i, (u, v) in enumerate(STEP_CENTRES):
        for j in range(6):
            rows.append((u + 0.3 * j, v - 0.2 * j, 2.0 + 0.37 * j + 0.05 * i, 4.0, 0.25))
    s = _scene_of(32, 32, rows, seed=3, aniso=0.2)
    return _flat(s, np.arange(len(rows)) % 2 == 0)


@functools.lru_cache(maxsize=None)
def step():
    """Flat (ill-conditioned: a step at the depth plane) and well-conditioned Gaussians in the same lists; query points along pixel rays at
    d (1 + k 2^-23), k = -8..8, around the depth d at which the ray meets each entry's depth plane (found from the float32 oracle's records
    by project32 in float64, then refined by the rounding of the points themselves: the conditions below are what counts)."""
    from util import oracle_for
    s = step_scene()
    o = oracle_for(s)
    o.integrate(np.zeros((1, 3), F) + F(5.0))
    P = s.means3D.shape[0]
    rec, inte = _records_from_oracle(o, P)
    o.close()
    fx, fy = bc.focal(s)
    rng = np.random.default_rng(17)
    pts = []
    for g in range(P):
        for _ in range(2):
            ix, iy = rec[g, 0] + 0.5 + rng.uniform(-2, 2), rec[g, 1] + 0.5 + rng.uniform(-2, 2)
            if not (0.5 < ix < 31.5 and 0.5 < iy < 31.5):
                continue
            d = float(rec[g, 7]) + float(rec[g, 11]) * (float(rec[g, 0]) - ix) + float(rec[g, 12]) * (float(rec[g, 1]) - iy)
            ray = np.array([(ix - 16.0) / fx, (iy - 16.0) / fy, 1.0])
            ray /= np.linalg.norm(ray)
            k = np.arange(-8, 9)
            pts.append((ray[None, :] * (d * (1.0 + k * 2.0 ** -23))[:, None]).astype(F))
    return s, np.concatenate(pts)


def step_conditions(inp, dec, w):
    q, tile = w.q, w.tile
    lo_ill = hi_ill = near_w = far_w = 0
    for e in range(inp.L):
        sel = np.flatnonzero(w.visited[:, e])
        if not len(sel):
            continue
        dx, dy, depth, dz, well, r, I = _point_geometry(inp, e, tile[sel], inp.p2d[q[sel], 0], inp.p2d[q[sel], 1], inp.pdepth[q[sel]], F)
        qd = inp.pdepth[q[sel]]
        ulps = np.abs(qd.view(np.int32).astype(np.int64) - depth.astype(F).view(np.int32).astype(np.int64))
        close4 = ulps <= 4
        lo_ill += int((~well & close4 & w.stepped[sel, e]).sum())
        hi_ill += int((~well & close4 & ~w.stepped[sel, e]).sum())
        near_w += int((well & close4 & w.nearer[sel, e]).sum())
        far_w += int((well & close4 & ~w.nearer[sel, e]).sum())
    ill = inp.inte[np.unique(inp.point_list), 6] == 0
    return {"flat and well-conditioned Gaussians in the lists": bool(ill.any() and (~ill).any()),
            "qd < depth within 4 ulps of an ill-conditioned plane": lo_ill >= 3, "qd >= depth within 4 ulps of one": hi_ill >= 3,
            "qd == depth exactly at an ill-conditioned plane": _exact_hits(inp, w) >= 1,
            "fminf returns qd within 4 ulps of a well-conditioned plane": near_w >= 3, "fminf returns depth within 4 ulps": far_w >= 3}


def _exact_hits(inp, w):
    n = 0
    for e in range(inp.L):
        sel = np.flatnonzero(w.visited[:, e])
        if len(sel):
            dx, dy, depth, dz, well, r, I = _point_geometry(inp, e, w.tile[sel], inp.p2d[w.q[sel], 0], inp.p2d[w.q[sel], 1], inp.pdepth[w.q[sel]], F)
            n += int((~well & (depth == inp.pdepth[w.q[sel]])).sum())
    return n


# ---- edges ----
EDGE_W, EDGE_H = 61, 45
NONFINITE = np.array([[np.nan, 0, 3], [0, 0, np.inf], [-np.inf, 0, 3]], F)


def edges_scene():
    rng = np.random.default_rng(23)
    rows = [(rng.uniform(0, 36), rng.uniform(0, 45), rng.uniform(2, 6), rng.uniform(1.5, 3.0), rng.uniform(0.1, 0.8)) for _ in range(50)]
    rows += [(60.0, 44.0, 3.0, 1.5, 0.5), (59.0, 43.5, 3.5, 1.2, 0.3)]             # the last pixel's tile (ragged in both directions)
    rows += [(8.0, 40.0, 2.0, 0.35, 0.0041)]                                       # used through one corner sample only by the pixels around it
    return _scene_of(EDGE_W, EDGE_H, rows, seed=4, aniso=0.0)


def _search(s, axis, want, pix, tries=100000, seed=0):
    """a float32 point (random depth, a few ulps around the coordinate that projects to `pix`) whose projection (the arithmetic of
    project32) meets `want(ix_or_iy as float32, its double sum)`"""
    fx, fy = focal32(s)
    f, S = (fx, s.W) if axis == 0 else (fy, s.H)
    rng = np.random.default_rng(seed)
    z = rng.uniform(2.5, 3.5, tries).astype(F)
    v = ((pix - S / 2.0) * z.astype(np.float64) / float(f) * (1.0 + rng.integers(-8, 9, tries) * 2.0 ** -24)).astype(F)
    pts = np.zeros((tries, 3), F)
    pts[:, 2], pts[:, axis] = z, v
    dsum = ((f * v) / (z + F(0.0000001))).astype(np.float64) + S / 2.0
    hit = np.flatnonzero(want(dsum.astype(F), dsum))
    assert len(hit), "no candidate found"
    return pts[hit[0]]


@functools.lru_cache(maxsize=None)
def edges():
    s = edges_scene()
    W, H = s.W, s.H
    below = lambda S: np.nextafter(F(S), F(0))                                     # noqa: E731
    pts = [np.array([0.01, 0.01, 0.2], F), np.array([0.01, 0.01, np.nextafter(F(0.2), F(1))], F)]
    pts.append(_search(s, 0, lambda v, d: v == F(0.0), 0.0))
    pts.append(_search(s, 0, lambda v, d: v == below(W), W))
    pts.append(_search(s, 0, lambda v, d: (d < W) & (v == F(W)), W))
    pts.append(_search(s, 1, lambda v, d: (d < H) & (v == F(H)), H))
    pts.append(_search(s, 1, lambda v, d: v == F(0.0), 0.0))
    pts.append(_search(s, 1, lambda v, d: v == below(H), H))
    for axis in (0, 1):                                                            # integer ix / iy on pixel borders
        for border in (1, 16, 17, 32):
            pts.append(_search(s, axis, lambda v, d, b=border: v == F(b), border, seed=border))
    pts = [np.asarray(p, F).reshape(1, 3) for p in pts]
    pts.append(_ray_points(s, 60 + np.array([0.2, 0.5, 0.9]), 44 + np.array([0.1, 0.6, 0.95]), [2.5, 3.2, 4.0]))      # pixel (60, 44)
    pts.append(_ray_points(s, 50 + np.array([0.5, 3.5, 8.5]), 5 + np.array([0.5, 9.5, 20.5]), [2.5, 3.2, 4.0]))       # tiles with empty lists
    pts.append(_ray_points(s, np.array([7.2, 8.2, 7.5, 8.5]), np.array([39.2, 39.3, 40.6, 40.4]), [1.5, 2.5, 3.0, 1.9]))   # corner uses only
    rng = np.random.default_rng(29)
    pts.append(_ray_points(s, rng.uniform(-3, 64, 300), rng.uniform(-3, 48, 300), rng.uniform(0.1, 7.0, 300)))
    pts.append(NONFINITE)
    return s, np.concatenate(pts)


def edges_conditions(inp, dec, w):
    s, pts = CASES["edges"].build()
    fx, fy = focal32(s)
    W, H = inp.W, inp.H
    x, y = inp.p2d[:, 0], inp.p2d[:, 1]
    pr = inp.projected
    below = lambda S: np.nextafter(F(S), F(0))                                     # noqa: E731
    with np.errstate(all="ignore"):
        dsx = ((fx * pts[:, 0]) / (pts[:, 2] + F(0.0000001))).astype(np.float64) + W / 2.0
        dsy = ((fy * pts[:, 1]) / (pts[:, 2] + F(0.0000001))).astype(np.float64) + H / 2.0
    nonfinite = ~np.isfinite(pts).all(1)
    c = {"pv.z == 0.2f is rejected, its successor accepted": bool(not pr[0] and pr[1] and pts[0, 2] == F(0.2)),
         "ix == 0.0f": bool((pr & (x == 0) & (pts[:, 0] != 0)).any()), "iy == 0.0f": bool((pr & (y == 0) & (pts[:, 1] != 0)).any()),
         "the largest float below W": bool((pr & (x == below(W))).any()), "the largest float below H": bool((pr & (y == below(H))).any()),
         "a double sum below W that the cast rounds to W": bool((~pr & (dsx < W) & (dsx.astype(F) == F(W)) & (pts[:, 2] > 1)).any()),
         "a double sum below H that the cast rounds to H": bool((~pr & (dsy < H) & (dsy.astype(F) == F(H)) & (pts[:, 2] > 1)).any()),
         "integer ix on pixel borders": all(bool((pr & (x == F(b))).any()) for b in (1, 16, 17, 32)),
         "integer iy on pixel borders": all(bool((pr & (y == F(b))).any()) for b in (1, 16, 17, 32)),
         "points in pixel (60, 44)": int(inp.pix_points[44, 60]) >= 3,
         "the non-finite points are the last three": bool(nonfinite[-3:].all() and not nonfinite[:-3].any()),
         "the non-finite points are not projected": bool(not pr[-3:].any())}
    empty = np.flatnonzero(inp.n == 0)
    in_empty = np.isin(w.tile, empty)
    c["points in a tile with an empty list"] = bool(len(empty) and in_empty.sum() >= 3)
    qe = w.q[in_empty]
    c["... have alpha 0, the background colour and sdf = -qd"] = bool((w.alpha_integrated[qe] == 0).all() and (w.color_integrated[qe] == inp.bg.astype(F)).all()
                                                                   and (w.sdf[qe] == -inp.pdepth[qe]).all())
    py_, px_ = inp.ppix[w.q] // W, inp.ppix[w.q] % W
    conly = (dec.last[py_, px_] > 0) & (dec.median[py_, px_] == 0) & ~dec.pass0[w.tile, :, w.lane].any(1)
    c["points in a pixel whose only uses are corner uses (no median plane)"] = bool(conly.any())
    return c


CASES = {c.name: c for c in [Case("cap", cap, cap_conditions), Case("reach", reach, reach_conditions), Case("band", band, band_conditions),
                             Case("step", step, step_conditions), Case("edges", edges, edges_conditions)]}


# ================================================================================================ the mutations (sharpness)
def mutate(name, inp, dec, w, s=None, pts=None):
    """One mutation of chain (a) -> (Decisions, Walk, IntegrateInput) of the mutated chain, or None where the case has nothing to mutate."""
    if name == "cap at 2049":
        if not dec.capped.any():
            return None
        d2 = decide(inp, cap=MAX_CONTRIBUTORS + 1)
        return d2, walk32(inp, d2), inp
    if name == "batch 12's bits missing in the tile of 769":
        t = np.flatnonzero(inp.n == 769)
        if not len(t):
            return None
        used = dec.used.copy()
        used[t[0], 768:] = False
        return dec, walk32(inp, dec, used=used), inp
    if name == "qd <= depth":
        return (dec, walk32(inp, dec, step_le=True), inp) if _exact_hits(inp, w) else None
    if name == "one in-band point decision flipped":
        hi, lo = near_threshold(w, 1e-4)
        cand = np.argwhere(hi | lo)
        if not len(cand):
            return None
        # the pair whose flip moves alpha_integrated most: alpha T is largest early in a walk
        m, e = max((tuple(c) for c in cand), key=lambda c: -int(w.blended[c[0], :c[1]].sum()))
        return dec, walk32(inp, dec, flip=(int(m), int(e))), inp
    if name == "a point walked one entry past its pixel's last contributor":
        q, tile = w.q, w.tile
        lastq = dec.last[inp.ppix[q] // inp.W, inp.ppix[q] % inp.W].astype(np.int64)
        cand = np.flatnonzero(lastq < inp.n[tile])
        if not len(cand):
            return None
        with np.errstate(all="ignore"):                             # the point at which that entry would weigh most
            dx, dy, depth, dz, well, r, I = _point_geometry(inp, lastq[cand], tile[cand], inp.p2d[q[cand], 0], inp.p2d[q[cand], 1], inp.pdepth[q[cand]], F)
            a = np.where(~well & (inp.pdepth[q[cand]] < depth), 0, r[:, 5] * exp_spec32(np.fmin(_point_power(dx, dy, dz, I, F), F(80.0))))
        pT = 1.0 - w.alpha_integrated[q[cand]]
        return dec, walk32(inp, dec, past_last=int(cand[int(np.argmax(a * pT))])), inp
    if name == "the NaN point binned into pixel 0":
        if pts is None or np.isfinite(pts).all():
            return None
        p2d, pdepth, ppix = project32(pts, s.viewmatrix.numpy().reshape(-1), *focal32(s), s.W, s.H, nan_passes=True)
        pt_sorted, pix_incl = bins_of(ppix, s.W, s.H)
        i2 = IntegrateInput(inp.W, inp.H, inp.bg, inp.rec, inp.inte, inp.ranges, inp.point_list, p2d, pdepth, ppix, pt_sorted, pix_incl)
        return dec, walk32(i2, dec), i2
    raise KeyError(name)


MUTATIONS = {"cap at 2049": ("cap",), "batch 12's bits missing in the tile of 769": ("reach",), "qd <= depth": ("step",),
             "one in-band point decision flipped": ("band",), "a point walked one entry past its pixel's last contributor": ("reach",),
             "the NaN point binned into pixel 0": ("edges",)}
