"""Scenes and packers for the direct tests of the per-Gaussian kernels (preprocess_fwd_kernel / preprocess_bwd_kernel,
csrc/rg_per_gaussian.inc): test infrastructure, no GPU.

Builders return a Case: the Scene, what the call takes besides it (precomputed colours / covariance, scale_modifier), one class name
per row (for failure messages) and -- after `prepare()` -- the oracle's forward plus the class counts computed FROM THE ORACLE'S OWN
ARRAYS, so that tests/test_per_gaussian_cases.py can demand on the CPU that every class the GPU test relies on is populated.

Packers lay the oracle's arrays out the way the device stores them (csrc/rg_layout.h, the write-out of preprocess_fwd_kernel) and the
way radegs_backward_from_sums takes the per-Gaussian sums (include/radegs.h)."""
import numpy as np
import torch

from synth_scene import make_scene
from util import cov3d_of, oracle_for

NEAR = np.float32(0.2)                          # auxiliary.h:166: visible means view z > 0.2f
NEAR_BITS = int(NEAR.view(np.uint32))
TILE = 16


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case:
    def __init__(self, name, scene, cls=None, colors=None, cov3D=None, scale_modifier=1.0, groups=None):
        self.name, self.s, self.colors, self.cov3D, self.scale_modifier = name, scene, colors, cov3D, float(scale_modifier)
        self.P = scene.means3D.shape[0]
        self.cls = np.array(["random"] * self.P, dtype=object) if cls is None else cls
        self.groups = groups or {}
        self.o = self.counts = self.ill = None

    def with_coord(self, coord):
        c = Case(self.name + ("_coord" if coord else "_nocoord"), self.s._replace(require_coord=bool(coord)), self.cls, self.colors,
                 self.cov3D, self.scale_modifier, self.groups)
        return c

    def oracle(self):
        return oracle_for(self.s, colors=self.colors, cov3D=self.cov3D, scale_modifier=self.scale_modifier)

    def prepare(self):
        """run the oracle's forward (once) and count the classes from its arrays"""
        if self.o is None:
            self.o = self.oracle()
            self.o.forward()
            self.ill = ill_conditioned(self)
            self.counts = class_counts(self)
        return self


# ------------------------------------------------------------------------------------------------------------------ scene builders
def _pix_to_cam(px, py, z, s):
    """camera-space x, y of the point that lands on pixel (px, py) at depth z (the inverse of ndc2Pix, auxiliary.h:57-60)"""
    return ((2.0 * px + 1.0) / s.W - 1.0) * s.tanfovx * z, ((2.0 * py + 1.0) / s.H - 1.0) * s.tanfovy * z


def boundary_scene(coord, sh_degree=3, kernel_size=0.0, P=3000, W=203, H=136, seed=31):
    """A random scene (identity pose: view z == means3D[:, 2] exactly) with rows overwritten so that every branch of the per-Gaussian
    forward is taken by a known set of rows: see the group names below."""
    s = make_scene(P, W, H, sh_degree=sh_degree, mu_px=3.0, seed=seed, kernel_size=kernel_size, pose="identity", require_coord=coord,
                   require_depth=True)
    rng = np.random.default_rng(seed + 1000)
    m, sc, rot = s.means3D.numpy().copy(), s.scales.numpy().copy(), s.rotations.numpy().copy()
    op, sh = s.opacities.numpy().copy(), s.shs.numpy().copy()
    focal = W / (2.0 * s.tanfovx)
    cls = np.array(["random"] * P, dtype=object)
    groups = {}
    nxt = [0]

    def take(name, n):
        r = np.arange(nxt[0], nxt[0] + n)
        nxt[0] += n
        groups[name] = r
        cls[r] = name
        return r

    def place(rows, px, py, z, sigma_px):
        x, y = _pix_to_cam(np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(z, np.float64), s)
        m[rows, 0], m[rows, 1], m[rows, 2] = x, y, z
        sc[rows] = (np.asarray(z, np.float64) * sigma_px / focal)[..., None] * np.exp(0.2 * rng.standard_normal((len(rows), 3)))

    # z at 0.2f and k ulps either side of it: k <= 0 is culled (p_view.z <= 0.2f), k > 0 is visible
    ks = np.array([-8, -5, -3, -2, -1, 0, 1, 2, 3, 5, 8] * 3)
    r = take("near_plane", len(ks))
    zb = (NEAR_BITS + ks).astype(np.uint32).view(np.float32)
    place(r, rng.uniform(40, W - 40, len(r)), rng.uniform(30, H - 30, len(r)), np.full(len(r), 1.0), 3.0)
    sc[r] *= 0.2
    m[r, 0] *= 0.2; m[r, 1] *= 0.2; m[r, 2] = zb
    # centres just outside each image edge, the footprint (radius ~ 3 sigma = 24 px) still reaches in: the rectangle clamps at 0 / at the grid
    n = 8
    for name, px, py in (("edge_left", rng.uniform(-9, -2, n), rng.uniform(10, H - 10, n)), ("edge_right", rng.uniform(W + 1, W + 8, n), rng.uniform(10, H - 10, n)),
                         ("edge_top", rng.uniform(10, W - 10, n), rng.uniform(-9, -2, n)), ("edge_bottom", rng.uniform(10, W - 10, n), rng.uniform(H + 1, H + 8, n))):
        place(take(name, n), px, py, rng.uniform(2.0, 6.0, n), 8.0)
    # far outside with a tiny footprint: beyond the near plane, but the tile rectangle is empty
    r = take("empty_rect", 12)
    px = np.where(np.arange(12) % 2 == 0, -rng.uniform(60, 90, 12), W + rng.uniform(60, 90, 12))
    py = np.where(np.arange(12) % 4 < 2, -rng.uniform(60, 90, 12), H + rng.uniform(60, 90, 12))
    place(r, px, py, rng.uniform(2.0, 6.0, 12), 0.5)
    # one splat over every tile (two rows: one centred, one off-centre)
    r = take("cover_all", 2)
    place(r, np.array([W / 2.0, W / 3.0]), np.array([H / 2.0, H / 1.5]), np.array([4.0, 6.0]), 150.0)
    op[r] = 0.05
    # exactly zero covariance: det == 0 at kernel_size 0 (forward.cu:392-393)
    r = take("zero_cov", 4)
    place(r, rng.uniform(40, W - 40, 4), rng.uniform(30, H - 30, 4), rng.uniform(2.0, 6.0, 4), 3.0)
    sc[r] = 0.0
    # one axis squashed: the ill-conditioned (lambda_min <= 1e-8) branch; tests/test_hostcheck.py::_flat_scene
    for name, val in (("flat_1e-6", 1e-6), ("flat_0", 0.0)):
        r = take(name, 90)
        sc[r, rng.integers(0, 3, len(r))] = val
    r = take("opacity_0", 20); op[r] = 0.0
    r = take("opacity_1", 20); op[r] = 1.0
    # rotations as given, not normalised
    r = take("rot_scaled", 300)
    rot[r] *= rng.uniform(0.5, 2.0, (len(r), 1))
    # a third of the rows: DC coefficient -3 in one, two or all three channels -> every combination of clamp flags (random rows keep flag 0)
    r = take("dc_clamped", P // 3)
    combo = 1 + np.arange(len(r)) % 7
    for c in range(3):
        sh[r[(combo >> c) & 1 == 1], 0, c] = -3.0
    for k in range(1, 8):
        cls[r[combo == k]] = "dc_clamped_%d" % k
    assert nxt[0] < P - 500, "the groups leave too few plain random rows"

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))

    s = s._replace(means3D=t(m), scales=t(sc), rotations=t(rot), opacities=t(op), shs=t(sh))
    return Case("boundary_deg%d_ks%g" % (sh_degree, kernel_size), s, cls, groups=groups).with_coord(coord)


TAIL_P = (1, 127, 128, 129, 255, 256, 257, 513)    # one under, on and one over the 128-row backward block / the 256-thread forward block


def tail_scene(P):
    """P rows, the last one in the middle of the image (so the last block of either kernel has a visible row whatever the seed draws).  P = 127
    and 257 carry 9 SH rows at degree 2: rows of 27 floats take preprocess_bwd_kernel's word-by-word slab loop, the others its 16-byte one."""
    deg = 2 if P in (127, 257) else 3
    s = make_scene(P, 64, 48, sh_degree=deg, mu_px=3.0, seed=500 + P, kernel_size=0.1, pose="identity", require_coord=False, require_depth=True)
    m = s.means3D.clone()
    m[-1] = torch.tensor([0.01, 0.02, 3.0])
    s = s._replace(means3D=m)
    if deg == 2:
        s = s._replace(shs=s.shs[:, :9].contiguous())
    return Case("tail_P%d" % P, s)


def tail_scenes():
    return [tail_scene(P) for P in TAIL_P]


def precomp_scene(variant=0):
    """0: colors_precomp + cov3D_precomp at SH degree 0.  1: scales + rotations with scale_modifier = 0.7, SH degree 0 of 16 rows."""
    s = make_scene(2000, 160, 120, sh_degree=0, mu_px=2.0, seed=5, kernel_size=0.1, pose="identity", require_coord=True, require_depth=True)
    if variant == 0:
        colors = torch.from_numpy(np.random.default_rng(55).random((2000, 3), dtype=np.float32))
        return Case("precomp_colors_cov3D", s, colors=colors, cov3D=cov3d_of(s))
    return Case("scale_modifier_0.7", s, scale_modifier=0.7)


def random_pose_scene():
    s = make_scene(2000, 203, 136, sh_degree=3, mu_px=3.0, seed=77, kernel_size=0.1, pose="random", require_coord=True, require_depth=True)
    return Case("random_pose_coord", s)


# ---------------------------------------------------------------------------------------------------------------------- class counts
def ill_conditioned(c):
    """[P] bool: the oracle's own conditioning flag (computeCov2D's lambda_min <= 1e-8 branch).  The oracle keeps it on the integrate path only
    (`condition`), so a second instance runs that path's preprocess over the same Gaussians."""
    if c.cov3D is not None or c.colors is not None:
        return np.zeros(c.P, bool)
    o2 = c.oracle()
    o2.integrate(c.s.means3D.numpy()[:1])
    return o2.get("condition") == 0


def clamp_bits(o, P):
    cl = o.get("clamped").reshape(P, 3)
    return (cl[:, 0] + 2 * cl[:, 1] + 4 * cl[:, 2]).astype(np.uint8)


def class_counts(c):
    o, s, P = c.o, c.s, c.P
    radii, tiles = o.get("radii"), o.get("tiles_touched")
    vis = radii > 0
    z = s.means3D.numpy()[:, 2]
    dz = bits(z).astype(np.int64) - NEAR_BITS
    within = (np.abs(dz) <= 8) & (z > 0)
    m2 = o.get("means2D", (P, 2))
    rad = radii.astype(np.float32)
    gx, gy = (s.W + TILE - 1) // TILE, (s.H + TILE - 1) // TILE
    with np.errstate(invalid="ignore"):
        lo_x, lo_y = (m2[:, 0] - rad) / np.float32(TILE), (m2[:, 1] - rad) / np.float32(TILE)
        hi_x = (((m2[:, 0] + rad) + np.float32(TILE)) - np.float32(1)) / np.float32(TILE)
        hi_y = (((m2[:, 1] + rad) + np.float32(TILE)) - np.float32(1)) / np.float32(TILE)
        n = dict(near_visible=int((within & vis & (dz > 0)).sum()), near_culled=int((within & ~vis & (dz <= 0)).sum()),
                 edge_left=int((vis & (m2[:, 0] < 0) & (lo_x < 0)).sum()), edge_top=int((vis & (m2[:, 1] < 0) & (lo_y < 0)).sum()),
                 edge_right=int((vis & (m2[:, 0] > s.W - 1) & (hi_x > gx)).sum()), edge_bottom=int((vis & (m2[:, 1] > s.H - 1) & (hi_y > gy)).sum()))
    # beyond the near plane with a non-zero covariance, and still culled: the reference returns at the empty rectangle BEFORE it writes the radius
    # (forward.cu:402-403, 418), so such a row has radius 0 -- `radii > 0 with tiles_touched == 0` cannot occur and is counted to show it
    er = c.groups.get("empty_rect", np.zeros(0, np.int64))
    n["empty_rect_culled"] = int(((z[er] > NEAR) & (radii[er] == 0) & (tiles[er] == 0)).sum())
    n["radius_without_tiles"] = int((vis & (tiles == 0)).sum())
    clb = clamp_bits(o, P) if c.colors is None else np.zeros(P, np.uint8)
    for k in range(8):
        n["clamp_%d" % k] = int((vis & (clb == k)).sum())
    n["ill_conditioned_visible"] = int((vis & c.ill).sum())
    n["cover_all"] = int((tiles == gx * gy).sum())
    n["last_block_128_visible"] = int(vis[128 * ((P - 1) // 128):].sum())
    n["last_block_256_visible"] = int(vis[256 * ((P - 1) // 256):].sum())
    n["visible"] = int(vis.sum())
    return n


# ---------------------------------------------------------------------------------------------------------------------------- packers
def expected_rect(m2, radii, W, H):
    """getRect (auxiliary.h:62-72) in float32, left to right, (int) truncation, clamped to the grid; packed x0 | y0 << 8 | w << 16 | h << 24
    (csrc/rg_layout.h: GeomState::rect); 0 for an invisible row."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rad, T, one = radii.astype(np.float32), np.float32(TILE), np.float32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        def lo(p, g):
            return np.clip(np.nan_to_num((p - rad) / T).astype(np.int64), 0, g)

        def hi(p, g):
            return np.clip(np.nan_to_num((((p + rad) + T) - one) / T).astype(np.int64), 0, g)

        x0, y0, x1, y1 = lo(m2[:, 0], gx), lo(m2[:, 1], gy), hi(m2[:, 0], gx), hi(m2[:, 1], gy)
    rect = (x0 | (y0 << 8) | ((x1 - x0) << 16) | ((y1 - y0) << 24)).astype(np.uint32)
    return np.where(radii > 0, rect, np.uint32(0)).astype(np.uint32)


def expected_state(o, s, colors=None):
    """The oracle's forward arrays in the device's layout: splat_a [P,16] f32 { mx, my, cx, cy | cz, op, thr, ts | r, g, b, rpx | rpy, nx, ny, nz }
    (slot 6, the skip threshold, is left 0: it is the device's logf), splat_b [P,12] { cp0..cp5, vpx, vpy, vpz, 0, 0, 0 }, clamped [P] u8 (bit c =
    channel c), rect [P] u32, depth_key [P] u32 (bits of view z; 0xFFFFFFFF for an invisible row).  Only visible rows mean anything in
    splat_a / splat_b / clamped."""
    P = s.means3D.shape[0]
    radii = o.get("radii")
    vis = radii > 0
    a, b = np.zeros((P, 16), np.float32), np.zeros((P, 12), np.float32)
    m2, co = o.get("means2D", (P, 2)), o.get("conic_opacity", (P, 4))
    a[:, 0:2] = m2
    a[:, 2:5] = co[:, 0:3]
    a[:, 5] = co[:, 3]
    a[:, 7] = o.get("ts")
    a[:, 8:11] = o.get("rgb", (P, 3)) if colors is None else np.asarray(colors, np.float32)
    rp = o.get("ray_planes", (P, 2))
    a[:, 11], a[:, 12] = rp[:, 0], rp[:, 1]
    a[:, 13:16] = o.get("normals", (P, 3))
    b[:, 0:6] = o.get("camera_planes", (P, 6))
    b[:, 6:9] = o.get("view_points", (P, 3))
    clamped = clamp_bits(o, P) if colors is None else np.zeros(P, np.uint8)
    depth_key = np.where(vis, bits(o.get("depths")), np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return dict(splat_a=a, splat_b=b, clamped=clamped, rect=expected_rect(m2, radii, s.W, s.H), depth_key=depth_key)


def oracle_sums(o, P, coord):
    """[P, 16 | 32] f32: the oracle's render-kernel sums (as they stand BEFORE its per-Gaussian backward rescales some of them in place:
    acc_*) in the order of radegs_backward_from_sums = gpu_util.reference_sums; tests/test_hostcheck.py::_check_bwd builds the same 25."""
    rec = np.zeros((P, 32 if coord else 16), np.float32)
    rec[:, 0:3] = o.get("acc_dcolors", (P, 3))
    rec[:, 3] = o.get("dL_dts")
    rec[:, 4:6] = o.get("dL_dray_planes", (P, 2))
    rec[:, 6:9] = o.get("dL_dnormals", (P, 3))
    rec[:, 9:12] = o.get("acc_dmeans2D", (P, 3))
    dc = o.get("acc_dconic", (P, 4))
    rec[:, 12], rec[:, 13], rec[:, 14] = dc[:, 0], dc[:, 1], dc[:, 3]
    rec[:, 15] = o.get("acc_dopacity")
    if coord:
        rec[:, 16:19] = o.get("dL_dview_points", (P, 3))
        rec[:, 19:25] = o.get("dL_dcamera_planes", (P, 6))
    return rec


def host_acc(sums):
    """[P, 25] in SplatAcc order (what hostcheck.preprocess_bwd takes) from a [P, 16 | 32] record"""
    acc = np.zeros((sums.shape[0], 25), np.float32)
    w = min(25, sums.shape[1])
    acc[:, :w] = sums[:, :w]
    return acc


GRAD_COLUMNS = (("dL_dmeans3D", slice(0, 3)), ("dL_dopacity", slice(3, 4)), ("dL_dcov3D", slice(4, 10)), ("dL_dscales", slice(10, 13)),
                ("dL_drotations", slice(13, 17)))


def arbitrary_sums(c, coord, seed=0):
    """Sums the oracle's blend never produces: standard normal, a tenth of the rows scaled by 1e+-6, some rows all zero, some slots -0.0; cleared
    on the ill-conditioned and the unnormalised-rotation rows (their amplification would overflow fp32).  Needs c.prepare()."""
    rng = np.random.default_rng(seed)
    P = c.P
    sums = rng.standard_normal((P, 32 if coord else 16)).astype(np.float32)
    big = rng.random(P) < 0.1
    sums[big] *= np.where(rng.random(int(big.sum())) < 0.5, np.float32(1e6), np.float32(1e-6))[:, None].astype(np.float32)
    sums[rng.random(P) < 0.05] = 0.0
    sums[rng.random(sums.shape) < 0.03] = np.float32(-0.0)
    clear = c.ill.copy()
    for g in ("rot_scaled", "zero_cov", "flat_1e-6", "flat_0", "cover_all"):
        clear[c.groups.get(g, np.zeros(0, np.int64))] = True
    sums[clear] = 0.0
    return sums


# ------------------------------------------------------------------------------------------------------------- registry and comparison
BUILDERS = {"boundary_deg3_ks0_nocoord": lambda: boundary_scene(False), "boundary_deg3_ks0_coord": lambda: boundary_scene(True),
            "boundary_deg1_ks0_nocoord": lambda: boundary_scene(False, sh_degree=1), "boundary_deg1_ks0.1_coord": lambda: boundary_scene(True, sh_degree=1, kernel_size=0.1),
            "precomp_colors_cov3D": lambda: precomp_scene(0), "scale_modifier_0.7": lambda: precomp_scene(1), "random_pose_coord": random_pose_scene}
BUILDERS.update({"tail_P%d" % P: (lambda P=P: tail_scene(P)) for P in TAIL_P})
BOUNDARY = [k for k in BUILDERS if k.startswith("boundary")]
TAILS = [k for k in BUILDERS if k.startswith("tail")]
_CASES = {}


def get_case(name):
    """the prepared Case `name`: built once per process, shared by the tests that need it, never modified"""
    if name not in _CASES:
        _CASES[name] = BUILDERS[name]().prepare()
    return _CASES[name]


def _as_words(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        a = a.view(np.uint32)
    return a.reshape(a.shape[0], -1)


def field_diff(field, got, want, rows, cls):
    """None when `got` and `want` ([P, ...], float32 compared as bit patterns) agree on `rows` (bool [P]); otherwise the failure message: the
    field, how many rows differ, the first such row, its class, and what it holds."""
    g, w = _as_words(got), _as_words(want)
    assert g.shape == w.shape, (field, g.shape, w.shape)
    bad = (g != w).any(1) & rows
    if not bad.any():
        return None
    r = int(np.nonzero(bad)[0][0])
    cols = np.nonzero(g[r] != w[r])[0].tolist()
    return "%s: %d of %d rows differ; first row %d (class %s), words %s: got %s want %s" % (
        field, int(bad.sum()), int(rows.sum()), r, cls[r], cols, np.asarray(got).reshape(g.shape[0], -1)[r, cols].tolist(),
        np.asarray(want).reshape(w.shape[0], -1)[r, cols].tolist())


def assert_fields(pairs, rows, cls, what):
    msgs = [m for m in (field_diff(k, g, w, rows, cls) for k, (g, w) in pairs.items()) if m]
    assert not msgs, what + "\n  " + "\n  ".join(msgs)


# The slab of preprocess_bwd_kernel / sh_grad_from_views_kernel, restated: word e of a block's contiguous [nrows][rowf] slab lives at LDS word
# g * (rowf + 1) + c with g = mulhi(e, ceil(2^32 / rowf)) standing in for e // rowf (csrc/rg_per_gaussian.inc::SlabMap), `threads` words per step.
def slab_positions(nrows, rowf, threads=128, tail=True):
    """-> (e, LDS word) for every word the copy touches; tail=False: the copy of a block that ignores a short last block (for the mutation check)"""
    n = (nrows if tail else threads) * rowf
    e = np.arange(n, dtype=np.uint64)
    magic = np.uint64(0xFFFFFFFF // rowf + 1)
    g = (e * magic) >> np.uint64(32)
    c = e - g * np.uint64(rowf)
    return e.astype(np.int64), (g * np.uint64(rowf + 1) + c).astype(np.int64), g.astype(np.int64), c.astype(np.int64)
