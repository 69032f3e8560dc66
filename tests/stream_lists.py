"""Checker for what the sub-tile entry-stream stage leaves in the image state (csrc/rg_streams.inc; test infrastructure, pure numpy).

    check_stream_state(st, truth_fn)   part B: meta words, chunk layout, list contents, block masks, blk_order, tightness
    check_contributions(st)            part C: the contribution ("history") words, blk_consumed, both planes of n_contrib

`st` is a StreamState: the arrays radegs_debug_export serves after a stream forward (tests/test_gpu_stream_lists.py), or a host stand-in
built from the oracle's lists and the host-compiled masks (tests/test_stream_lists_standin.py, which also proves that every check here
fires).  A failure names the array, the tile and the block.

The replay of part C restates the blend rule of DGR/cuda_rasterizer/forward.cu:552-573 in np.float32, one rounding per operation:
    power = -0.5 (cx dx dx + cz dy dy) - cy dx dy;  alpha = min(0.99, op exp_spec(max(power, -87)));
    ok = !(power > 0) && !(alpha < 1/255);  act = ok && !(T (1 - alpha) < 1e-4);  T <- T (1 - alpha) when ok;  T starts at 1 (0 outside)
exp_spec32 is csrc/rg_blend.h's specification in numpy.  numpy has no fma, so fma32 forms the exact product in float64 (24 + 24 bits),
adds in float64 rounded TO ODD (the sum's error from TwoSum) and rounds once to float32: 53 >= 2 * 24 + 2 bits make that the correctly
rounded fused result.  The CPU suite pins exp_spec32 bit for bit to the host build of rg_blend.h (which test_hostcheck pins to the oracle's);
the GPU machine has no compiler, and needs none for this file."""
import numpy as np

TAG = 0x53545247
CHUNK_WORDS = 48
NONE_MEDIAN = 0xFFFFFFFF     # blend_fwd_epilogue writes max_c as it stands; it starts at 0xFFFFFFFF (the reference's -1)
F = np.float32
_LOG2E, _MAGIC = F(1.44269504088896341), F(12582912.0)
_K255 = F(1.0) / F(255.0)


# ------------------------------------------------------------------------------------------------ exact float32 pieces
def fma32(a, b, c):
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                    # exact
        s = np.ascontiguousarray(p + c)
        # Rounding s once more, to float32, differs from the fused result only where s sits exactly on a float32 midpoint while p + c does
        # not (or where the float32 result is subnormal and the midpoints lie elsewhere): only there is the sum redone rounded to odd.
        flat = s.reshape(-1)
        k = np.flatnonzero(((flat.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) | (np.abs(flat) < 1.1754944e-38))
        if len(k):
            pk, ck, sk = np.broadcast_to(p, s.shape).reshape(-1)[k], np.broadcast_to(c, s.shape).reshape(-1)[k], flat[k]
            bb = sk - pk
            err = (pk - (sk - bb)) + (ck - bb)       # TwoSum: p + c == s + err exactly
            fix = (err != 0) & np.isfinite(sk) & ((sk.view(np.uint64) & np.uint64(1)) == 0)
            flat[k] = np.where(fix, np.nextafter(sk, np.where(err > 0, np.inf, -np.inf)), sk)
        return s.astype(np.float32)


def _exp_core(x):
    with np.errstate(all="ignore"):
        tm = np.ascontiguousarray(x * _LOG2E + _MAGIC)
        kf = tm - _MAGIC
        r = fma32(kf, F(-0.693359375), x)
        r = fma32(kf, F(2.12194440e-4), r)
        p = np.full(x.shape, F(1.9875691500e-4), np.float32)
        for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
            p = fma32(p, r, F(c))
        y = np.ascontiguousarray(fma32(p, r * r, r) + F(1.0))
        return (y.view(np.uint32) + (tm.view(np.uint32) << np.uint32(23))).view(np.float32)


def exp_spec32(x):
    x = np.ascontiguousarray(x, np.float32)
    return np.where(x < F(-87.0), F(0.0), _exp_core(x)).astype(np.float32)


def exp_spec_floor32(x):
    return _exp_core(np.fmax(np.ascontiguousarray(x, np.float32), F(-87.0)))


def splat_power32(cx, cy, cz, dx, dy):
    with np.errstate(all="ignore"):
        s = (cx * dx) * dx + (cz * dy) * dy
        return F(-0.5) * s - (cy * dx) * dy          # -0.5 s is exact: one rounding, like the header's fmaf(-0.5, s, -v)


def skip_threshold32(op):
    """log in float64 rounded to float32 (within 1/2 ulp of the exact logarithm, so within 1.5 ulp of any 1-ulp logf), minus the margin"""
    op = np.asarray(op, np.float32)
    with np.errstate(all="ignore"):
        q = F(1.0) / (F(255.0) * op)
        return np.log(q.astype(np.float64)).astype(np.float32) - F(1.0e-3)


def popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a, np.uint32).view(np.uint8)).sum())


# ------------------------------------------------------------------------------------------------ the state
class StreamState:
    FIELDS = ("W", "H", "ranges", "point_list", "splat_a", "rect", "tiles_touched", "blk_count", "blk_base", "blk_order", "blk_consumed",
              "stream_meta", "blk_chunks", "tile_keys_sorted", "n_contrib", "used_streams")

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw.pop(k))
        assert not kw, kw
        self.gx, self.gy = (self.W + 15) // 16, (self.H + 15) // 16
        self.tiles = self.gx * self.gy

    def copy(self):
        return StreamState(**{k: (getattr(self, k).copy() if isinstance(getattr(self, k), np.ndarray) else getattr(self, k)) for k in self.FIELDS})


def export_state(h, mask_in_key=False):
    """The arrays of a HipRun after forward_native() with entry streams."""
    import torch
    s = h.s
    W, H, P, R = s.W, s.H, h.P, int(h.state[0])
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    u = lambda name, n: h.export(name, torch.int32, n).view(np.uint32)   # noqa: E731
    meta = u("stream_meta", 4)
    nch = int(meta[1]) if int(meta[0]) == TAG and int(meta[3]) == 0 else 0
    return StreamState(
        W=W, H=H, ranges=u("ranges", 2 * tiles).reshape(tiles, 2), point_list=u("point_list", R),
        splat_a=h.export("splat_a", torch.float32, 16 * P).reshape(P, 16), rect=u("rect", P), tiles_touched=u("tiles_touched", P),
        blk_count=u("blk_count", 8 * tiles), blk_base=u("blk_base", 8 * tiles), blk_order=u("blk_order", 8 * tiles),
        blk_consumed=u("blk_consumed", 8 * tiles), stream_meta=meta,
        blk_chunks=u("blk_chunks", nch * CHUNK_WORDS).reshape(nch, CHUNK_WORDS) if nch else np.zeros((0, CHUNK_WORDS), np.uint32),
        tile_keys_sorted=u("tile_keys_sorted", R) if mask_in_key else None, n_contrib=u("n_contrib", 2 * H * W).reshape(2, H, W),
        used_streams=h.C.last_forward_used_streams())


def _fail(array, tile, blk, msg):
    raise AssertionError(f"{array}: tile {int(tile)} block {int(blk)}: {msg}")


def entries(st):
    """Every list entry in block order -> (blk, i, gid, pos): block id, index in its list, the two stored words.  Needs a sound chunk layout."""
    cnt, base = st.blk_count.astype(np.int64), st.blk_base.astype(np.int64)
    nb = cnt.shape[0]
    blk = np.repeat(np.arange(nb), cnt)
    i = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ch = base[blk] + i // 16
    if ch.size and ch.max() >= st.blk_chunks.shape[0]:
        k = int(np.argmax(ch))
        _fail("blk_base", blk[k] // 8, blk[k] % 8, f"list reaches chunk {int(ch[k])} of {st.blk_chunks.shape[0]}")
    return blk, i, st.blk_chunks[ch, 2 * (i % 16)].astype(np.int64), st.blk_chunks[ch, 2 * (i % 16) + 1].astype(np.int64)


def layout(nb, blk, gid, pos):
    """The inverse of entries() for a stand-in: flat lists in block order -> (blk_count, blk_base, zero-filled chunks with the list words)."""
    cnt = np.bincount(blk, minlength=nb).astype(np.int64)
    nch = (cnt + 15) // 16
    base = np.cumsum(nch) - nch
    chunks = np.zeros((int(nch.sum()), CHUNK_WORDS), np.uint32)
    i = np.arange(blk.shape[0]) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ch = base[blk] + i // 16
    chunks[ch, 2 * (i % 16)] = gid
    chunks[ch, 2 * (i % 16) + 1] = pos
    return cnt.astype(np.uint32), base.astype(np.uint32), chunks


def expected_order(blk_count):
    """balance_blocks' key: inside every group of 512 consecutive block ids, (count, id) descending"""
    cnt = blk_count.astype(np.int64)
    out = np.empty(cnt.shape[0], np.int64)
    for g0 in range(0, cnt.shape[0], 512):
        ids = np.arange(g0, min(g0 + 512, cnt.shape[0]))
        out[ids] = ids[np.lexsort((ids, cnt[ids]))][::-1]
    return out


def instance_tiles(st):
    """tile of every position of point_list (from ranges)"""
    R = st.point_list.shape[0]
    x, n = st.ranges[:, 0].astype(np.int64), (st.ranges[:, 1].astype(np.int64) - st.ranges[:, 0].astype(np.int64))
    assert (n >= 0).all() and int(n.sum()) == R, ("ranges do not cover point_list", int(n.sum()), R)
    t = np.repeat(np.arange(st.tiles), n)
    at = np.repeat(x, n) + (np.arange(R) - np.repeat(np.cumsum(n) - n, n))
    out = np.full(R, -1, np.int64)
    out[at] = t
    assert (out >= 0).all(), "ranges overlap"
    return out


def unpack_rect(rect):
    r = rect.astype(np.int64)
    x0, y0 = r & 255, (r >> 8) & 255
    return x0, y0, x0 + ((r >> 16) & 255), y0 + (r >> 24)


def cannot_reach(st, gid, tile, b):
    """A bound on how loose a block mask may be, for the pairs (Gaussian gid, block b of tile): True where the block provably lies outside
    anything ellipse_tile_mask may keep.  rg_blend.h keeps a block only when it meets the ellipse cx dx^2 + 2 cy dx dy + cz dy^2 <= M,
    M = -2 thr + 1e-2 + 2e-5 terms (terms: the quadratic form's magnitude at the far corner of the splat's rectangle), with extents widened
    by 2e-4 relative + 0.01 px.  Here, in float64: the block's pixel rectangle grown by 2 px misses the axis-aligned bounding box of the
    ellipse with 2 M + 1 in place of M (extents x 1.41).  Regular conics only (the others keep every block); thr > 0 keeps nothing."""
    rec = st.splat_a[gid].astype(np.float64)
    mx, my, cx, cy, cz, thr = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 6]
    x0, y0, x1, y1 = unpack_rect(st.rect[gid])
    with np.errstate(all="ignore"):
        U = np.maximum(np.abs(x0 * 16 - mx), np.abs(x1 * 16 - 1 - mx))
        V = np.maximum(np.abs(y0 * 16 - my), np.abs(y1 * 16 - 1 - my))
        det = cx * cz - cy * cy
        regular = (cx > 0) & (cz > 0) & (det > 2e-3 * cx * cz) & np.isfinite(mx + my + cx + cy + cz + thr) & (cx * cz < 1e29)
        M2 = 2.0 * (2e-5 * (cx * U * U + cz * V * V + 2 * np.abs(cy) * U * V) - 2.0 * thr + 1e-2) + 1.0
        hx, hy = np.sqrt(cz * M2 / det), np.sqrt(cx * M2 / det)
        bx = (tile % st.gx) * 16 + (b & 1) * 8 - mx
        by = (tile // st.gx) * 16 + (b >> 1) * 4 - my
        miss = (bx - 2 > hx) | (bx + 7 + 2 < -hx) | (by - 2 > hy) | (by + 3 + 2 < -hy)
    return (regular & miss) | (thr > 0)


# ------------------------------------------------------------------------------------------------ part B
def check_stream_state(st, truth_fn, tight=False):
    """truth_fn(splat_a, gid, ox, oy) -> the brute-force block mask of Gaussian gid[i] in the tile whose first pixel is (ox[i], oy[i]).
    Returns the figures (kept / reachable (entry, block) pairs)."""
    assert st.used_streams is True, f"radegs_last_forward_used_streams says {st.used_streams}: the forward did not use entry streams"
    cnt, base = st.blk_count.astype(np.int64), st.blk_base.astype(np.int64)
    nb = 8 * st.tiles
    nch = (cnt + 15) // 16
    meta = [int(v) for v in st.stream_meta]
    # 1. meta words
    assert meta[0] == TAG, f"stream_meta[0] = {meta[0]:#x}, not the stream tag"
    assert meta[3] == 0, f"stream_meta[3] = {meta[3]}: the lists did not fit"
    assert meta[1] == int(nch.sum()), f"stream_meta[1] = {meta[1]} chunks, the counts need {int(nch.sum())}"
    assert st.blk_chunks.shape[0] >= meta[1], "blk_chunks: fewer chunks exported than stream_meta[1]"
    # 2. chunk layout
    b2, n2 = base.reshape(-1, 8), nch.reshape(-1, 8)
    bad = np.argwhere(b2[:, 1:] != b2[:, :-1] + n2[:, :-1])
    if len(bad):
        t, b = bad[0]
        _fail("blk_base", t, b + 1, f"starts at chunk {b2[t, b + 1]}, block {b} ends at chunk {b2[t, b] + n2[t, b]}")
    live = np.flatnonzero(cnt > 0)
    order = live[np.argsort(base[live], kind="stable")]
    lo, hi = base[order], base[order] + nch[order]
    bad = np.flatnonzero(lo != np.concatenate([[0], hi[:-1]]))
    if len(bad):
        k = order[bad[0]]
        _fail("blk_base", k // 8, k % 8, f"chunks [{lo[bad[0]]}, {hi[bad[0]]}) do not start where the ranges before them end "
              f"({0 if bad[0] == 0 else hi[bad[0] - 1]}): overlap or gap")
    assert (hi[-1] if len(hi) else 0) == meta[1], f"blk_base: the ranges end at chunk {hi[-1] if len(hi) else 0}, stream_meta[1] = {meta[1]}"
    # 3. list contents
    blk, i, gid, pos = entries(st)
    tile, b = blk // 8, blk % 8
    r0 = st.ranges[:, 0].astype(np.int64)
    n_tile = st.ranges[:, 1].astype(np.int64) - r0
    bad = np.flatnonzero(pos >= n_tile[tile])
    if len(bad):
        k = bad[0]
        _fail("blk_chunks", tile[k], b[k], f"entry {i[k]}: pos {pos[k]} >= the tile list's length {n_tile[tile[k]]}")
    bad = np.flatnonzero((blk[1:] == blk[:-1]) & (pos[1:] <= pos[:-1]))
    if len(bad):
        k = bad[0] + 1
        _fail("blk_chunks", tile[k], b[k], f"entry {i[k]}: pos {pos[k]} after pos {pos[k - 1]}, not strictly increasing")
    pl = st.point_list.astype(np.int64)
    assert not (pl >> 24).any(), f"point_list: top byte set at index {int(np.flatnonzero(pl >> 24)[0]) if (pl >> 24).any() else 0}"
    assert (pl < st.splat_a.shape[0]).all(), "point_list: a Gaussian index past P"
    bad = np.flatnonzero(gid != pl[r0[tile] + pos])
    if len(bad):
        k = bad[0]
        _fail("blk_chunks", tile[k], b[k], f"entry {i[k]}: gid {gid[k]} but point_list[range.x + {pos[k]}] = {pl[r0[tile[k]] + pos[k]]}")
    # 4. masks
    R = pl.shape[0]
    it = instance_tiles(st)
    recon = np.zeros(R, np.uint32)
    np.bitwise_or.at(recon, r0[tile] + pos, (1 << b).astype(np.uint32))
    truth = truth_fn(st.splat_a, st.point_list, ((it % st.gx) * 16).astype(np.float32), ((it // st.gx) * 16).astype(np.float32)).astype(np.uint32)
    missed = truth & ~recon
    if missed.any():
        k = int(np.flatnonzero(missed)[0])
        mb = int(missed[k]) & -int(missed[k])
        _fail("blk_chunks", it[k], mb.bit_length() - 1, f"the list misses tile entry {k - r0[it[k]]} (Gaussian {pl[k]}), which reaches the block: "
              f"kept mask {int(recon[k]):#04x}, truth {int(truth[k]):#04x}; {int((missed != 0).sum())} entries in all")
    if st.tile_keys_sorted is not None:
        keys = st.tile_keys_sorted.astype(np.int64)
        bad = np.flatnonzero((keys & 0xFFFFFF) != it)
        assert not len(bad), f"tile_keys_sorted: index {bad[0] if len(bad) else 0} holds tile {keys[bad[0]] & 0xFFFFFF if len(bad) else 0}, ranges say {it[bad[0]] if len(bad) else 0}"
        bad = np.flatnonzero((keys >> 24) != recon)
        if len(bad):
            k = bad[0]
            d = int(keys[k] >> 24) ^ int(recon[k])
            _fail("tile_keys_sorted", it[k], (d & -d).bit_length() - 1, f"tile entry {k - r0[it[k]]}: mask {int(keys[k] >> 24):#04x} in the key, {int(recon[k]):#04x} in the lists")
    bad = np.flatnonzero(cannot_reach(st, gid, tile, b))
    if len(bad):
        k = bad[0]
        _fail("blk_chunks", tile[k], b[k], f"entry {i[k]} (Gaussian {gid[k]}, pos {pos[k]}) is kept in a block its splat cannot reach")
    # the emission itself: every visible Gaussian appears exactly once in every tile of its rectangle and nowhere else
    vis = np.flatnonzero(st.tiles_touched > 0)
    x0, y0, x1, y1 = unpack_rect(st.rect[vis])
    w, nt = x1 - x0, (x1 - x0) * (y1 - y0)
    assert np.array_equal(nt, st.tiles_touched[vis].astype(np.int64)), "rect: w * h differs from tiles_touched"
    local = np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)
    g_rep, w_rep = np.repeat(vis, nt), np.repeat(w, nt)
    want = g_rep * st.tiles + (np.repeat(y0, nt) + local // w_rep) * st.gx + np.repeat(x0, nt) + local % w_rep   # row-major in the rectangle
    assert np.array_equal(np.sort(want), np.sort(pl * st.tiles + it)), "point_list: the (Gaussian, tile) pairs are not the rectangles' tiles, each once"
    # 6. blk_order
    bo = st.blk_order.astype(np.int64)
    seen = np.bincount(bo[bo < nb], minlength=nb)
    if (bo >= nb).any() or (seen != 1).any():
        k = int(bo[bo >= nb][0]) if (bo >= nb).any() else int(np.flatnonzero(seen != 1)[0])
        _fail("blk_order", k // 8, k % 8, f"appears {int(seen[k]) if k < nb else 0} times: not a permutation of 0 .. {nb - 1}" if k < nb else f"id {k} out of range")
    exp = expected_order(st.blk_count)
    bad = np.flatnonzero(bo != exp)
    if len(bad):
        p = bad[0]
        _fail("blk_order", bo[p] // 8, bo[p] % 8, f"at position {p} (count {cnt[bo[p]]}); (count, id) descending puts block {exp[p]} (count {cnt[exp[p]]}) there")
    # 7. tightness
    kept, needed = popcount(recon), popcount(truth)
    if tight:
        assert kept <= 1.25 * needed + 100, f"blk_count: {kept} (entry, block) pairs kept, {needed} reachable: more than 1.25 x + 100"
    return dict(kept=kept, reachable=needed, ratio=kept / max(needed, 1), instances=R, entries=int(cnt.sum()))


def list_contents(st):
    """What two layouts of one scene must share: the counts and every list's (gid, pos) sequence, in block order"""
    _, _, gid, pos = entries(st)
    return st.blk_count.copy(), gid, pos


# ------------------------------------------------------------------------------------------------ part C
def block_pixels(st):
    """lane l of block (tile, b), pixel s: px [nb, 16], py [nb, 16, 2]"""
    nb = 8 * st.tiles
    tile, b, lane = (np.arange(nb) // 8)[:, None], (np.arange(nb) % 8)[:, None], np.arange(16)[None, :]
    px = (tile % st.gx) * 16 + 8 * (b & 1) + (lane & 7)
    py = (tile // st.gx) * 16 + 4 * (b >> 1) + (lane >> 3)
    return px, np.stack([py, py + 2], -1)


def replay(st):
    """-> (hist [nb, rounds, 16] uint32, consumed [nb], last [nb, 16, 2], median [nb, 16, 2]) as the rule gives them from the lists.
    An entry's record is the one its POSITION names in the tile list; its contributor number is pos + 1."""
    blk, i, _, pos = entries(st)
    cnt = st.blk_count.astype(np.int64)
    nb, maxc = cnt.shape[0], int(cnt.max()) if cnt.size else 0
    r0 = st.ranges[:, 0].astype(np.int64)
    n_tile = st.ranges[:, 1].astype(np.int64) - r0
    tile = blk // 8
    G = np.zeros((nb, max(maxc, 1)), np.int64)
    Pp = np.zeros((nb, max(maxc, 1)), np.int64)
    G[blk, i] = st.point_list.astype(np.int64)[r0[tile] + np.minimum(pos, np.maximum(n_tile[tile] - 1, 0))] & 0xFFFFFF
    Pp[blk, i] = pos
    px, py = block_pixels(st)
    inside = (px[..., None] < st.W) & (py < st.H)
    T = np.where(inside, F(1.0), F(0.0)).astype(np.float32)
    n_eff = cnt.copy()
    n_eff[~inside.reshape(nb, -1).any(1)] = 0          # a block wholly outside the image consumes nothing
    pxf, pyf = px.astype(np.float32)[..., None], py.astype(np.float32)
    hist = np.zeros((nb, (maxc + 15) // 16 + 1, 16), np.uint32)
    last = np.zeros((nb, 16, 2), np.uint32)
    med = np.full((nb, 16, 2), NONE_MEDIAN, np.uint32)
    A = st.splat_a.astype(np.float32)
    with np.errstate(all="ignore"):
        for e in range(maxc):
            ab = np.flatnonzero(e < n_eff)
            if not len(ab):
                break
            rec = A[G[ab, e]][:, None, None, :]
            dx, dy = rec[..., 0] - pxf[ab], rec[..., 1] - pyf[ab]
            power = splat_power32(rec[..., 2], rec[..., 3], rec[..., 4], dx, dy)
            alpha = np.fmin(F(0.99), rec[..., 5] * exp_spec_floor32(power))
            Tb = T[ab]
            test_T = Tb * (F(1.0) - alpha)
            ok = ~(power > F(0.0)) & ~(alpha < _K255)
            act = ok & ~(test_T < F(0.0001))
            r, j = divmod(e, 16)
            hist[ab, r] |= (act[..., 0].astype(np.uint32) << np.uint32(j)) | (act[..., 1].astype(np.uint32) << np.uint32(j + 16))
            con = (Pp[ab, e] + 1).astype(np.uint32)[:, None, None]
            last[ab] = np.where(act, con, last[ab])
            med[ab] = np.where(act & (Tb > F(0.5)), con, med[ab])
            T[ab] = np.where(ok, test_T, Tb)
            if j == 15:                                  # a block whose 32 pixels have all terminated stops consuming its list
                done = (T[ab] < F(0.0001)).reshape(len(ab), -1).all(1)
                n_eff[ab[done]] = np.minimum(n_eff[ab[done]], e + 1)
    return hist, n_eff, last, med


def write_contributions(st, rep):
    """stand-in: what the forward leaves behind, from a replay"""
    hist, n_eff, last, med = rep
    cnt, base = st.blk_count.astype(np.int64), st.blk_base.astype(np.int64)
    n_tile = st.ranges[:, 1].astype(np.int64) - st.ranges[:, 0].astype(np.int64)
    st.blk_consumed = np.where(np.repeat(n_tile, 8) > 0, n_eff, 0xFFFFFFFF).astype(np.uint32)   # not written for tiles with an empty range
    for k in np.flatnonzero(n_eff > 0):
        rounds = (int(n_eff[k]) + 15) // 16
        st.blk_chunks[base[k]:base[k] + rounds, 32:48] = hist[k, :rounds]
    for k in np.flatnonzero((cnt > 0) & (n_eff < cnt)):    # rounds the forward never reached keep whatever was there
        st.blk_chunks[base[k] + (int(n_eff[k]) + 15) // 16:base[k] + (int(cnt[k]) + 15) // 16, 32:48] = 0xFFFFFFFF


def check_contributions(st, rep=None):
    """Returns the figures (blocks that stopped early, history words compared)."""
    hist, n_eff, last, med = rep if rep is not None else replay(st)
    cnt, base = st.blk_count.astype(np.int64), st.blk_base.astype(np.int64)
    nb = cnt.shape[0]
    n_tile = np.repeat(st.ranges[:, 1].astype(np.int64) - st.ranges[:, 0].astype(np.int64), 8)
    got = st.blk_consumed.astype(np.int64)
    bad = np.flatnonzero((n_tile > 0) & (got != n_eff))
    if len(bad):
        k = bad[0]
        _fail("blk_consumed", k // 8, k % 8, f"{got[k]}, the replay consumes {n_eff[k]} of {cnt[k]} entries")
    rounds = (n_eff + 15) // 16
    blk = np.repeat(np.arange(nb), rounds)
    r = np.arange(int(rounds.sum())) - np.repeat(np.cumsum(rounds) - rounds, rounds)
    words = st.blk_chunks[base[blk] + r, 32:48]
    bad = np.argwhere(words != hist[blk, r])
    if len(bad):
        k, l = bad[0]
        _fail("blk_chunks", blk[k] // 8, blk[k] % 8, f"history word of round {r[k]}, lane {l}: {int(words[k, l]):#010x}, the replay gives "
              f"{int(hist[blk[k], r[k], l]):#010x}; {len(bad)} words differ in all")
    px, py = block_pixels(st)
    inside = (px[..., None] < st.W) & (py < st.H)
    pxb = np.broadcast_to(px[..., None], py.shape)
    for plane, name, want in ((0, "last", last), (1, "median", med)):
        have = st.n_contrib[plane][np.minimum(py, st.H - 1), np.minimum(pxb, st.W - 1)]
        bad = np.argwhere(inside & (have != want))
        if len(bad):
            k, l, s = bad[0]
            _fail("n_contrib", k // 8, k % 8, f"{name} contributor of pixel ({pxb[k, l, s]}, {py[k, l, s]}): {int(have[k, l, s])}, the contribution words give {int(want[k, l, s])}")
    return dict(stopped_early=int(((n_eff < cnt) & (n_eff > 0)).sum()), history_words=int(words.size), max_list=int(cnt.max()) if nb else 0)


# ------------------------------------------------------------------------------------------------ the scenarios
_RAGGED = dict(P=2500, W=72, H=40, sh_degree=1, mu_px=2.0, seed=81, kernel_size=0.1, pose="random")
_BIG = dict(P=600, W=104, H=72, sh_degree=1, mu_px=14.0, seed=93, kernel_size=0.1, pose="random", low_opacity=True)
# (RADEGS_SPECULATE=0 next to the mask-in-key layout: tile_keys_sorted is exported from a binning buffer laid out for exactly R instances)
SCENARIOS = {   # scene: make_scene arguments; coord: coord + depth mode instead of depth; env: switches next to RADEGS_STREAMS=1; tight: ordinary splats
    "ragged": dict(scene=_RAGGED, coord=False, env={}, tight=True, parts="BC"),
    "ragged-coord": dict(scene=_RAGGED, coord=True, env={}, tight=True, parts="BC"),
    "ragged-mask-in-key": dict(scene=_RAGGED, coord=False, env={"RADEGS_MASK_IN_KEY": "1", "RADEGS_SPECULATE": "0"}, tight=True, parts="BC"),
    "big": dict(scene=_BIG, coord=False, env={}, tight=False, parts="BC"),
    "early-stop": dict(scene=dict(_BIG, kernel_size=0.0, pose="identity", low_opacity=False), coord=False, env={}, tight=False, parts="BC"),
    # (60 Gaussians: with 300 every one of the 104 tiles has a list)
    "sparse": dict(scene=dict(P=60, W=200, H=120, sh_degree=1, mu_px=1.5, seed=3, kernel_size=0.0), coord=False, env={}, tight=True, parts="BC"),
    "two-groups": dict(scene=dict(P=4000, W=208, H=136, sh_degree=1, mu_px=2.0, seed=82, kernel_size=0.0), coord=False, env={}, tight=True, parts="B"),
}


def scenario_scene(name):
    from synth_scene import make_scene
    sc = SCENARIOS[name]
    return make_scene(**sc["scene"], require_coord=sc["coord"], require_depth=True)


def check_scenario_property(name, st):
    """The property a scenario is in the table for (asserted wherever the scenario runs: on the host stand-in and on the device)."""
    cnt, cons = st.blk_count.astype(np.int64), st.blk_consumed.astype(np.int64)
    n_tile = np.repeat(st.ranges[:, 1].astype(np.int64) - st.ranges[:, 0].astype(np.int64), 8)
    px, py = block_pixels(st)
    outside = ~((px[..., None] < st.W) & (py < st.H)).reshape(cnt.shape[0], -1).any(1)
    if name.startswith("ragged"):
        assert (st.gx, st.gy) == (5, 3) and st.W % 16 and st.H % 16
        assert (outside & (cnt > 0)).sum() > 0, "no block with a list lies wholly outside the image"
        assert (cons[outside & (n_tile > 0)] == 0).all()
    elif name == "big":
        assert (st.tiles_touched > 16).sum() > 50, int((st.tiles_touched > 16).sum())
        assert cnt.max() >= 200 and ((cnt % 16 != 0) & (cnt > 32)).sum() > 10, (int(cnt.max()),)
    elif name == "early-stop":
        assert ((cons < cnt) & (cons > 0) & (n_tile > 0)).sum() > 0, "no block stops consuming its list early"
    elif name == "sparse":
        assert (n_tile == 0).sum() > 0 and ((n_tile > 0) & (cnt == 0) & ~outside).sum() > 0 and ((cnt > 0) & (cnt < 16)).sum() > 0
    elif name == "two-groups":
        assert 512 < cnt.shape[0] < 1024 and cnt.shape[0] % 512
