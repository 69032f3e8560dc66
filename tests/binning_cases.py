"""TEST INFRASTRUCTURE for the direct tests of the binning stage (tests/test_binning_cases.py on the CPU, tests/test_gpu_binning_direct.py on
the MI355X).  Pure numpy / torch, importable without a GPU.

Binning is everything between the per-Gaussian kernel and the blend: depth sort, gather-scan, emit_instances_kernel, tile sort,
tile_ranges_kernel (csrc/radegs_kernels.hip, csrc/rg_launch.inc).

    restate(radii, px, py, depth_key, tiles_touched, gx, gy)
                           the stage in integers, from the per-Gaussian words its kernels read: every Gaussian's tile rectangle (getRect:
                           truncation, then clamp -- the float32 operations of auxiliary.h:62-72 one by one), num_rendered, the instance list
                           as np.lexsort((gaussian index, depth key, tile id)) over all (Gaussian, tile) pairs -- the reference's stable
                           64-bit sort, and what depth sort + row-major emission + stable tile sort must equal --, the sorted tile ids as
                           16-bit and as 32-bit words, ranges[tiles][2] with (0, 0) at every empty tile
    layout(gx, gy, ...)    the rule plan_attempt applies (rg_launch.inc), stated once: packed rectangles iff both grid dimensions <= 255;
                           16-bit tile keys iff higher_msb(gx * gy) <= 16 and the block mask does not ride in the key
    CASES                  the case builders, and what each case must reach (checked on the CPU against the fp32 oracle)

The splats are placed in pixel space under the identity pose with a 1-degree field of view (the perspective terms of the 2D covariance
then change a radius of 2000 px by less than 0.2 px): opaque, isotropic, with the radius chosen in advance, so that a rectangle is known
by construction -- and then asserted on the oracle's state, never assumed."""
import functools
from typing import Callable, NamedTuple

import numpy as np
import torch

from synth_scene import make_scene

F = np.float32
TILE = 16
FOV_DEG = 1.0
INVISIBLE_KEY = 0xFFFFFFFF       # depth key of a Gaussian the per-Gaussian kernel culled (rg_per_gaussian.inc)
GID_MASK = (1 << 24) - 1         # kGidMask (rg_layout.h): below the block-mask byte
COOP_THRESHOLD = 16              # kEmitCoopThreshold (radegs_kernels.hip): more tiles than this -> the whole wave writes the splat
SORT27_Z = 13107.0               # the three-pass depth sort's window ends here (rg_launch.inc)
SPEC_SLACK = 4096                # a speculative capacity is hint + hint / 4 + this (plan_attempt)


# ================================================================================================ the layout rule
def higher_msb(n):
    """getHigherMsb (rasterizer_impl.cu:35-50): the number of tile-id bits the tile sort looks at"""
    n = int(n)
    msb, step = 16, 16
    while step > 1:
        step //= 2
        msb = msb + step if n >> msb else msb - step
    return msb + 1 if n >> msb else msb


class Layout(NamedTuple):
    rect: bool          # the scan gathers packed 8-bit rectangles and the emission reads them (otherwise: tile_rect from splat_a and radii)
    key16: bool         # 16-bit tile keys, 8 per thread of tile_ranges_kernel (otherwise 32-bit keys, 4 per thread)
    tile_bits: int      # end bit of the tile sort
    mask_in_key: bool   # the top byte of a 32-bit key is the block mask of the entry streams


def layout(gx, gy, streams=False, mask_in_key=False):
    """plan_attempt / queue_instances (rg_launch.inc) for the library's own primitives.  mask_in_key: RADEGS_MASK_IN_KEY=1 (or 2^24
    Gaussians and more); it only takes effect in a stream forward."""
    bits = higher_msb(gx * gy)
    in_key = bool(streams and mask_in_key)
    return Layout(rect=gx <= 255 and gy <= 255, key16=bits <= 16 and not in_key, tile_bits=bits, mask_in_key=in_key)


# ================================================================================================ the restatement
class Binning(NamedTuple):
    x0: np.ndarray              # [P] int64 tile rectangle [x0, x1) x [y0, y1); all four 0 at an invisible Gaussian
    y0: np.ndarray
    x1: np.ndarray
    y1: np.ndarray
    rect_tiles: np.ndarray      # [P] (x1 - x0) (y1 - y0): must equal tiles_touched
    num_rendered: int
    point_list: np.ndarray      # [R] int64 Gaussian index of every instance, in (tile, depth key, index) order
    tile_ids: np.ndarray        # [R] int64 its tile
    keys16: np.ndarray          # [R] uint16 the sorted keys as 16-bit words (meaningful while every tile id < 65 536)
    keys32: np.ndarray          # [R] uint32 ... as 32-bit words (under key_mask where the layout carries a mask byte)
    ranges: np.ndarray          # [tiles, 2] uint32, (0, 0) at every empty tile


def tile_rects(px, py, radii, gx, gy):
    """getRect (auxiliary.h:62-72) in float32, one rounding per operation, in the reference's order: (int)((p - r) / 16) and
    (int)((p + r + 16 - 1) / 16) evaluated left to right, truncated toward zero, THEN clamped to [0, grid]."""
    px, py, r = np.asarray(px, F), np.asarray(py, F), np.asarray(radii).astype(F)
    t = F(TILE)

    def lo(p, g):
        return np.clip(np.trunc((p - r) / t).astype(np.int64), 0, g)

    def hi(p, g):
        return np.clip(np.trunc((((p + r) + t) - F(1.0)) / t).astype(np.int64), 0, g)

    return lo(px, gx), lo(py, gy), hi(px, gx), hi(py, gy)


def restate(radii, px, py, depth_key, tiles_touched, gx, gy):
    """The binning of one view from the words its kernels read.  A Gaussian takes part iff tiles_touched > 0 (what the scan adds up);
    its rectangle comes from its pixel mean and radius."""
    radii, tiles_touched = np.asarray(radii).astype(np.int64).reshape(-1), np.asarray(tiles_touched).astype(np.int64).reshape(-1)
    key = np.asarray(depth_key).astype(np.int64).reshape(-1)
    P = radii.shape[0]
    vis = tiles_touched > 0
    x0, y0, x1, y1 = (np.where(vis, a, 0) for a in tile_rects(px, py, radii, gx, gy))
    w, n = x1 - x0, (x1 - x0) * (y1 - y0)
    R = int(n.sum())
    g = np.repeat(np.arange(P), n)                                        # the (Gaussian, tile) pairs, rows outer / columns inner
    local = np.arange(R) - np.repeat(np.cumsum(n) - n, n)
    tile = (y0[g] + local // np.maximum(w[g], 1)) * gx + x0[g] + local % np.maximum(w[g], 1)
    order = np.lexsort((g, key[g], tile))
    point_list, tile_ids = g[order], tile[order]
    tiles = gx * gy
    first = np.searchsorted(tile_ids, np.arange(tiles), "left")
    last = np.searchsorted(tile_ids, np.arange(tiles), "right")
    ranges = np.where((last > first)[:, None], np.stack([first, last], 1), 0).astype(np.uint32)
    return Binning(x0, y0, x1, y1, n, R, point_list, tile_ids, tile_ids.astype(np.uint16), tile_ids.astype(np.uint32), ranges)


def packed_rect(b):
    """the rect word of the per-Gaussian kernel (rg_preprocess.h): x0 | y0 << 8 | w << 16 | h << 24, 0 at an invisible Gaussian"""
    w, h = b.x1 - b.x0, b.y1 - b.y0
    assert int(max(b.x0.max(), b.y0.max(), w.max(), h.max())) <= 255, "a field does not fit 8 bits: this grid has no packed rectangles"
    word = (b.x0 | (b.y0 << 8) | (w << 16) | (h << 24)).astype(np.uint32)
    return np.where(b.rect_tiles > 0, word, np.uint32(0)).astype(np.uint32)


def check_invariants(b, depth_key, gx, gy):
    """What a restated binning must satisfy whatever produced its inputs: the ranges partition [0, R) in tile order, each range is
    ordered by (depth key, index), and every entry's Gaussian covers its tile."""
    key = np.asarray(depth_key).astype(np.int64)
    r = b.ranges.astype(np.int64)
    occ = np.flatnonzero(r[:, 1] > r[:, 0])
    assert not r[np.setdiff1d(np.arange(gx * gy), occ)].any(), "an empty tile's range is not (0, 0)"
    assert b.num_rendered == 0 or (r[occ[0], 0] == 0 and r[occ[-1], 1] == b.num_rendered)
    assert np.array_equal(r[occ[1:], 0], r[occ[:-1], 1]), "the ranges of the occupied tiles do not follow one another"
    assert np.array_equal(np.repeat(occ, r[occ, 1] - r[occ, 0]), b.tile_ids), "tile_ids is not what the ranges say"
    same = b.tile_ids[1:] == b.tile_ids[:-1]
    k, g = key[b.point_list], b.point_list
    assert (~same | (k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (g[1:] > g[:-1]))).all(), "a tile's list is not in (depth key, index) order"
    tx, ty = b.tile_ids % gx, b.tile_ids // gx
    assert ((b.x0[g] <= tx) & (tx < b.x1[g]) & (b.y0[g] <= ty) & (ty < b.y1[g])).all(), "an entry's Gaussian does not cover its tile"
    assert int(b.rect_tiles.sum()) == b.num_rendered == b.point_list.shape[0]


def tile_changes(b):
    """instance numbers at which the sorted list enters another tile"""
    return np.flatnonzero(b.tile_ids[1:] != b.tile_ids[:-1]) + 1


# ================================================================================================ scenes in pixel space
def sigma_for_radius(r):
    """The footprint (pixels) of an isotropic splat whose radius comes out as exactly r: ceil(3 sqrt(lambda)) with lambda = sigma^2 +
    sqrt(0.1) (forward.cu's eigenvalue of an isotropic 2D covariance: the discriminant is clamped to 0.1), aimed at r - 0.5."""
    r = np.asarray(r, np.float64)
    assert (r >= 3).all(), "radius 2 is what a point-sized splat already has"
    return np.sqrt(((r - 0.5) / 3.0) ** 2 - np.sqrt(0.1))


def pixel_scene(W, H, u, v, z, radius, seed=0):
    """Opaque isotropic Gaussians whose centres project to pixel (u, v) at view depth z (z <= 0.2: culled) with a radius of `radius` px"""
    u, v, z, radius = (np.asarray(a, np.float64).reshape(-1) for a in (u, v, z, radius))
    n = u.shape[0]
    s = make_scene(n, W, H, sh_degree=0, seed=0, kernel_size=0.0, require_coord=False, require_depth=True, near_cull_frac=0.0, filter3d=False,
                   fovx_deg=FOV_DEG, bg=(0.2, 0.4, 0.6))
    fx, fy = W / (2.0 * s.tanfovx), H / (2.0 * s.tanfovy)
    za = np.maximum(np.abs(z), 0.3)
    means = np.stack([(u - (W - 1) / 2.0) * za / fx, (v - (H - 1) / 2.0) * za / fy, z], 1)
    scales = np.repeat((sigma_for_radius(radius) * za / fx)[:, None], 3, 1)
    q = np.zeros((n, 4))
    q[:, 0] = 1.0
    shs = np.zeros((n, 16, 3))
    shs[:, 0, :] = np.random.default_rng(1000 + seed).uniform(-1.5, 1.5, (n, 3))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
    return s._replace(means3D=t(means), shs=t(shs), rotations=t(q), scales=t(scales), opacities=t(np.full((n, 1), 0.9)))


def _axis(a, n, g, r):
    """Centre coordinate of a splat of radius r that covers tiles [a, a + n) of an axis of g tiles: unclipped where r fits n tiles
    (8 n - 9 <= r <= 8 n - 2), otherwise cut by the border the interval touches."""
    assert 0 <= a and n >= 1 and a + n <= g
    if 8 * n - 9 <= r <= 8 * n - 2:
        return 16 * a + 8 * n                             # centred: p - r inside tile a, p + r + 15 inside tile a + n
    assert r > 8 * n - 2, "the radius is too small for this many tiles"
    if a + n == g:
        return 16 * a + 4 + r                             # reaches past the far border
    assert a == 0, "a rectangle narrower than its radius implies must touch a border"
    return 16 * n - 6 - r                                 # reaches past the near border


def splat_for_rect(x0, y0, w, h, gx, gy, r=None):
    """(u, v, radius) of the isotropic splat whose tile rectangle is [x0, x0 + w) x [y0, y0 + h) on a gx x gy grid"""
    r = max(8 * max(w, h) - 4, 3) if r is None else r
    return float(_axis(x0, w, gx, r)), float(_axis(y0, h, gy, r)), float(r)


def one_tile(tile, gx):
    """a radius-3 splat at the centre of a tile"""
    return 16.0 * (tile % gx) + 7.5, 16.0 * (tile // gx) + 7.5, 3.0


def _scene_from(W, H, rows, depth_order, seed):
    """rows: (u, v, radius) per splat IN DEPTH ORDER (front first); the Gaussian indices are a seeded permutation of that order, so the
    depth sort has work to do.  depth_order None: depths 2 + 0.002 k; else the depths themselves."""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, np.float64).reshape(-1, 3)
    n = rows.shape[0]
    z = 2.0 + 0.002 * np.arange(n) if depth_order is None else np.asarray(depth_order, np.float64)
    perm = rng.permutation(n)
    return pixel_scene(W, H, rows[perm, 0], rows[perm, 1], z[perm], rows[perm, 2], seed)


# ---- coop_threshold
COOP_COUNTS = (1, 2, 15, 16, 17, 63, 64, 65, 300)
_COOP_SHAPES = {1: (1, 1), 2: (2, 1), 15: (5, 3), 16: (4, 4), 17: (17, 1), 63: (9, 7), 64: (8, 8), 65: (13, 5), 300: (20, 15)}


def coop_threshold():
    """320 x 320, 20 x 20 tiles.  In depth order: wave 0 = 64 splats of 1, 2, 15, 16, 17, 63, 64, 65 and 300 tiles (most of them cut
    by the border they lean on); wave 1 = 64 splats of 25 tiles each (all cooperative); wave 2 = 64 splats of 1 .. 16 tiles (none
    cooperative); wave 3 = 40 small ones.  Every 5th Gaussian in index order is culled, so the scan gathers zero counts and the last
    waves of the emission hold invisible lanes."""
    g = 20
    rows = []
    for k in range(64):
        n = COOP_COUNTS[k % len(COOP_COUNTS)]
        w, h = _COOP_SHAPES[n]
        if k % 2:
            w, h = h, w
        far = (k // len(COOP_COUNTS)) % 2 == 1      # lean on the far borders every other round
        natural = w == h
        x0 = (k % (g - w + 1)) if natural else ((g - w) if far else 0)
        y0 = ((3 * k) % (g - h + 1)) if natural else ((g - h) if far else 0)
        rows.append(splat_for_rect(x0, y0, w, h, g, g))
    for k in range(64):
        rows.append(splat_for_rect((5 * k) % 16, (3 * k) % 16, 5, 5, g, g))
    for k in range(64):
        n = 1 + k % 4
        rows.append(splat_for_rect((7 * k) % (g - n + 1), (11 * k) % (g - n + 1), n, n, g, g))
    for k in range(40):
        rows.append(one_tile((37 * k) % (g * g), g))
    # the invisible rows take indices of their own: the visible ones keep their depth order
    s = _scene_from(320, 320, rows, None, seed=3)
    n = len(rows)
    extra = pixel_scene(320, 320, np.full(n // 4, 100.0), np.full(n // 4, 100.0), np.full(n // 4, -1.0), np.full(n // 4, 5.0), seed=4)
    rng = np.random.default_rng(5)
    where = np.sort(rng.choice(n + n // 4, n // 4, replace=False))
    keep = np.setdiff1d(np.arange(n + n // 4), where)

    def mix(a, b):
        out = torch.zeros((n + n // 4,) + tuple(a.shape[1:]), dtype=a.dtype)
        out[torch.from_numpy(keep)] = a
        out[torch.from_numpy(where)] = b
        return out

    return s._replace(**{k: mix(getattr(s, k), getattr(extra, k)) for k in ("means3D", "opacities", "scales", "rotations", "shs")})


def coop_reaches(b, depth_key):
    vis = np.flatnonzero(b.rect_tiles > 0)
    order = vis[np.lexsort((vis, np.asarray(depth_key).astype(np.int64)[vis]))]
    n = b.rect_tiles[order]
    waves = [n[k:k + 64] for k in range(0, 192, 64)]
    return {
        "every listed tile count occurs in wave 0": set(COOP_COUNTS) <= set(waves[0].tolist()),
        "16 and 17 tiles occur": (n == COOP_THRESHOLD).any() and (n == COOP_THRESHOLD + 1).any(),
        "wave 1 is all above the threshold": (waves[1] > COOP_THRESHOLD).all(),
        "wave 2 has none above it": (waves[2] <= COOP_THRESHOLD).all() and (waves[2] == COOP_THRESHOLD).any(),
        "invisible rows are mixed in": 30 < int((b.rect_tiles == 0).sum()) and (np.diff(np.flatnonzero(b.rect_tiles == 0)) > 1).any(),
        "the last wave holds invisible lanes": len(order) % 64 != 0,
        "R allows a forced redo": b.num_rendered > SPEC_SLACK + 1,
    }


def clipped_by_border(b, radii, gx, gy):
    """Gaussians whose rectangle is narrower than the radius implies (2 r + 1 pixels reach (2 r + 15) // 16 tiles at least), because the image ends"""
    w, h, need = b.x1 - b.x0, b.y1 - b.y0, (2 * np.asarray(radii).astype(np.int64) + 15) // 16
    edge = (b.x0 == 0) | (b.y0 == 0) | (b.x1 == gx) | (b.y1 == gy)
    return (b.rect_tiles > 0) & edge & ((w < need) | (h < need))


# ---- ties
TIES_W, TIES_H, TIES_TILE = 48, 32, 4


def ties(W=TIES_W, H=TIES_H):
    """200 splats in the middle tile of a 3 x 2 grid in 8 groups of 25 at ONE depth each, so the order inside a group falls to the
    index; the groups' depth keys come in pairs that differ in the lowest bit; the last pair lies beyond z = 13 107, outside the
    three-pass sort's window: the forward is redone with four passes (and remembers)."""
    z = []
    for base in (2.0, 2.5, 7.0, SORT27_Z + 100.0):
        a = F(base)
        z += [float(a), float(np.nextafter(a, F(np.inf)))]
    u, v, r = one_tile(TIES_TILE, 3)
    depths = np.repeat(np.asarray(z), 25)
    return _scene_from(W, H, [(u, v, r)] * 200, depths, seed=9)


def ties_reaches(b, depth_key):
    k = np.unique(np.asarray(depth_key).astype(np.int64)[b.rect_tiles > 0])
    return {
        "200 instances in one tile": b.num_rendered == 200 and (b.tile_ids == TIES_TILE).all(),
        "8 depth keys, 25 splats each": len(k) == 8,
        "the keys pair up one bit apart": len(k) == 8 and (k[1::2] - k[0::2] == 1).all(),
        "one pair lies beyond the three-pass window": int((k > int(F(SORT27_Z).view(np.uint32))).sum()) == 2,
        "the index order inside a group is not the depth order": (np.diff(b.point_list) < 0).sum() > 4,
    }


# ---- range_edges
RANGE_R16 = (1, 7, 8, 9, 2047, 2048, 2049, 4097)      # 16-bit keys: 8 keys per thread, 2048 per workgroup
RANGE_R32 = (1, 3, 4, 5, 1023, 1024, 1025, 2049)      # 32-bit keys: 4 per thread, 1024 per workgroup
ARRANGEMENTS = ("one_tile", "own_tile", "changes")


def range_grid(R):
    """the smallest near-square grid with a tile per instance (at least two tiles)"""
    gy = max(int(np.ceil(np.sqrt(R))), 1)
    return max(-(-R // gy), 2), gy


def range_change_points(R, per_thread, per_group):
    """where `changes` switches tile: at 8k and 8k - 1 (k = 1, 2, and around the workgroup boundary) and at the workgroup size itself"""
    V, G = per_thread, per_group
    pts = {V - 1, V, 2 * V - 1, 2 * V, G - V - 1, G - V, G - 1, G, G + V - 1, G + V, 2 * G - 1, 2 * G}
    return sorted(p for p in pts if 1 <= p <= R - 1)


def range_edges(R, arrangement, per_thread, per_group):
    """R one-tile splats, one instance each.  one_tile: all in the LAST tile of the grid; own_tile: one per tile, spread from the
    first tile to the last; changes: the sorted list changes tile exactly at range_change_points, the first segment in the first tile
    and the last in the last.  Tiles between occupied ones stay empty."""
    gx, gy = range_grid(R)
    T = gx * gy
    if arrangement == "one_tile":
        tile = np.full(R, T - 1)
    elif arrangement == "own_tile":
        tile = np.unique(np.round(np.linspace(0, T - 1, R)).astype(np.int64)) if R > 1 else np.zeros(1, np.int64)
        assert tile.shape[0] == R
    else:
        cuts = range_change_points(R, per_thread, per_group)
        seg = np.searchsorted(np.asarray(cuts), np.arange(R), "right")            # segment of every sorted position
        ids = np.unique(np.round(np.linspace(0, T - 1, len(cuts) + 1)).astype(np.int64)) if cuts else np.zeros(1, np.int64)
        assert ids.shape[0] == len(cuts) + 1
        tile = ids[seg]
    rng = np.random.default_rng(R * 3 + ARRANGEMENTS.index(arrangement))
    z = rng.uniform(2.0, 10.0, R)
    for t in np.unique(tile):                       # inside a tile the sorted position follows the depth
        z[tile == t] = np.sort(z[tile == t])
    rows = [one_tile(t, gx) for t in tile]
    return _scene_from(16 * gx, 16 * gy, rows, z, seed=R)


def range_reaches(R, arrangement, per_thread, per_group):
    def f(b, depth_key):
        gx, gy = range_grid(R)
        occ = np.unique(b.tile_ids)
        ch = tile_changes(b).tolist()
        out = {"R is the listed value": b.num_rendered == R, "one instance per splat": (b.rect_tiles == 1).all()}
        if arrangement == "one_tile":
            out["all in the last tile"] = occ.tolist() == [gx * gy - 1]
        elif arrangement == "own_tile":
            out["every instance in a tile of its own"] = len(occ) == R
            out["first and last tile occupied"] = R == 1 or (occ[0] == 0 and occ[-1] == gx * gy - 1)
        else:
            cuts = range_change_points(R, per_thread, per_group)
            out["tile changes exactly at the listed instances"] = ch == cuts
            out["first and last tile occupied"] = occ[0] == 0 and (not cuts or occ[-1] == gx * gy - 1)
            out["empty tiles between occupied ones"] = len(occ) < 3 or (np.diff(occ) > 1).all()
        return out
    return f


# ---- grids on both sides of the 8-bit rectangle and of the 16-bit key
def _small_random(rng, n, gx, gy):
    W, H = 16 * gx, 16 * gy
    return [(float(rng.uniform(0, W)), float(rng.uniform(0, H)), float(rng.integers(3, 21))) for _ in range(n)]


def thin_grid(gx, gy):
    """A grid one tile thick (gx x 1 or 1 x gy) of 255 or 256 tiles: splats in the first and the last tile, one whose rectangle spans
    the whole long axis (255 tiles fill the 8-bit width field exactly), one straddling tiles 254 | 255 and one 255 | 256 of the long
    axis (the second is cut to nothing on the 255 grid), about 300 small ones at random."""
    n = max(gx, gy)
    rng = np.random.default_rng(100 + n + (gx > gy))
    rows = [one_tile(0, gx), one_tile(gx * gy - 1, gx)]
    span = splat_for_rect(0, 0, gx, gy, gx, gy, r=8 * n - 4)
    rows.append(span)
    for edge in (255, 256):
        along, across = 16.0 * edge - 0.5, 7.5
        rows.append((along, across, 3.0) if gx > gy else (across, along, 3.0))
    rows += _small_random(rng, 300, gx, gy)
    order = rng.permutation(len(rows))
    return _scene_from(16 * gx, 16 * gy, [rows[i] for i in order], None, seed=n)


def thin_reaches(gx, gy):
    def f(b, depth_key):
        n, T = max(gx, gy), gx * gy
        w = (b.x1 - b.x0) if gx > gy else (b.y1 - b.y0)
        lo = b.x0 if gx > gy else b.y0
        return {
            "first and last tile occupied": b.tile_ids[0] == 0 and b.tile_ids[-1] == T - 1,
            "a rectangle spans the whole axis": int(w.max()) == n,
            "a splat straddles 254 | 255": ((lo == 254) & (w == (2 if n == 256 else 1))).any(),
            "a splat sits at 255 | 256": ((lo == 255) & (w == 1)).any() if n == 256 else int((b.rect_tiles == 0).sum()) >= 1,
            "hundreds of instances": b.num_rendered > 500,
        }
    return f


def big_grid(gx, gy):
    """65 535, 65 536 or 65 792 tiles: 300 small splats at random; one-tile splats in tile 0, in the last tile and in tiles 65 535 and
    65 536 where the grid has them; two splats of 25 tiles; one splat that spans the longer axis (more than 255 tiles), cut to two
    tiles across by the border.  A few hundred Gaussians: the emission grid is two workgroups and its range clear has to stride."""
    T = gx * gy
    rng = np.random.default_rng(gx * 1000 + gy)
    rows = [one_tile(t, gx) for t in (0, T - 1, 65535, 65536) if t < T]
    rows += [splat_for_rect(gx - 7, gy - 9, 5, 5, gx, gy), splat_for_rect(3, gy // 2, 5, 5, gx, gy)]
    if gx >= gy:
        rows.append(splat_for_rect(0, 0, gx, 2, gx, gy))
    else:
        rows.append(splat_for_rect(0, 0, 2, gy, gx, gy))
    rows += _small_random(rng, 300, gx, gy)
    order = rng.permutation(len(rows))
    return _scene_from(16 * gx, 16 * gy, [rows[i] for i in order], None, seed=gx + gy)


def big_reaches(gx, gy):
    def f(b, depth_key):
        T = gx * gy
        occ = set(np.unique(b.tile_ids).tolist())
        long_axis = np.maximum(b.x1 - b.x0, b.y1 - b.y0)
        return {
            "tile 0 and the last tile are occupied": 0 in occ and T - 1 in occ,
            "tiles 65 535 and 65 536 are occupied where they exist": all(t in occ for t in (65535, 65536) if t < T),
            "two splats of more than 16 tiles": int(((b.rect_tiles > COOP_THRESHOLD) & (long_axis <= 255)).sum()) >= 2,
            "one splat longer than 255 tiles": int(long_axis.max()) == max(gx, gy) > 255,
            "at most two emission workgroups": b.rect_tiles.shape[0] <= 512,
        }
    return f


# ================================================================================================ the cases
class Case(NamedTuple):
    name: str
    gx: int
    gy: int
    build: Callable
    reaches: Callable           # (Binning, depth_key) -> {what the case is named for: reached?}
    small: bool                 # runs every path and is compared with the oracle's per-Gaussian state on the GPU


def _cases():
    out = [Case("coop_threshold", 20, 20, coop_threshold, coop_reaches, True),
           Case("ties", 3, 2, ties, ties_reaches, True)]
    for bits, Rs, V, G in ((16, RANGE_R16, 8, 2048), (32, RANGE_R32, 4, 1024)):
        for R in Rs:
            for arr in ARRANGEMENTS:
                gx, gy = range_grid(R)
                out.append(Case(f"range_edges_{bits}-{R}-{arr}", gx, gy, functools.partial(range_edges, R, arr, V, G),
                                range_reaches(R, arr, V, G), True))
    for gx, gy in ((256, 1), (255, 1), (1, 256), (1, 255)):
        out.append(Case(f"grid_{gx}x{gy}", gx, gy, functools.partial(thin_grid, gx, gy), thin_reaches(gx, gy), False))
    for gx, gy in ((255, 257), (256, 256), (257, 256)):
        out.append(Case(f"grid_{gx}x{gy}", gx, gy, functools.partial(big_grid, gx, gy), big_reaches(gx, gy), False))
    return {c.name: c for c in out}


CASES = _cases()
SMALL = [n for n, c in CASES.items() if c.small]
LARGE = [n for n, c in CASES.items() if not c.small]


@functools.lru_cache(maxsize=None)
def scene(name):
    s = CASES[name].build()
    assert ((s.W + 15) // 16, (s.H + 15) // 16) == (CASES[name].gx, CASES[name].gy)
    return s


def restate_oracle(o, s):
    """the restatement computed from an Oracle's own per-Gaussian arrays after forward()"""
    P = s.means3D.shape[0]
    radii, m2, tt = o.get("radii"), o.get("means2D", (P, 2)), o.get("tiles_touched")
    key = np.where(radii > 0, o.get("depths").astype(F).view(np.uint32), np.uint32(INVISIBLE_KEY))
    return restate(radii, m2[:, 0], m2[:, 1], key, tt, (s.W + 15) // 16, (s.H + 15) // 16), key
