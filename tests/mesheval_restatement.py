"""Mesh evaluation restated in numpy, in this project's own words: the triangle sampling, the sequential thinning loop over
brute-force radius lists, brute-force nearest neighbour, the observation / plane masks and the mesh cull of evaluate_dtu_mesh.py.  Needs
neither sklearn nor scipy.  It is checked against the fixtures the reference's code wrote (tests/test_mesheval_golden.py) and then serves as
the expectation at sizes and edge cases the fixtures do not reach (tests/test_gpu_mesheval.py)."""
import numpy as np

CHUNK = 1024


def _norm3(v):
    return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])


def sample_mesh(vertices, faces, density=0.2):
    """-> (cloud [V+M,3]: vertices then samples, counts [F]).  Samples of triangle (p0, p1, p2): the lattice points
    k = ((i + .5) / n1, (j + .5) / n2), i <= n1, j <= n2, with k0 + k1 < 1 (two divisions, one addition), i major."""
    vertices = np.asarray(vertices, np.float64)
    faces = np.asarray(faces).reshape(-1, 3)
    counts = np.zeros(faces.shape[0], np.int64)
    parts = [vertices]
    if faces.shape[0]:
        tri = vertices[faces]
        p0, v1, v2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        l1, l2 = _norm3(v1), _norm3(v2)
        cr = np.stack([v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1], v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2], v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]], 1)
        area2 = _norm3(cr)
        with np.errstate(divide="ignore", invalid="ignore"):
            thr = density * np.sqrt(l1 * l2 / area2)
            n1, n2 = np.floor(l1 / thr), np.floor(l2 / thr)
        for t in np.nonzero(area2 > 0)[0]:
            a, b = n1[t], n2[t]
            if not (a >= 1 and b >= 1):              # n = 0: the 1e-7 of max(n, 1e-7) sends every lattice point outside
                continue
            k0 = (np.arange(int(a) + 1, dtype=np.float64) + 0.5) / a
            k1 = (np.arange(int(b) + 1, dtype=np.float64) + 0.5) / b
            keep = (k0[:, None] + k1[None, :]) < 1
            ii, jj = np.nonzero(keep)                # row-major: i major, j minor
            parts.append((v1[t][None] * k0[ii][:, None] + v2[t][None] * k1[jj][:, None]) + p0[t][None])
            counts[t] = ii.shape[0]
    return np.concatenate(parts, 0), counts


def _d2(a, b):
    """[len(a), len(b)] squared distances, accumulated over x, y, z in that order"""
    d = a[:, None, 0] - b[None, :, 0]
    d *= d
    for k in (1, 2):                      # (dx^2 + dy^2) + dz^2, in place to spare the temporaries
        e = a[:, None, k] - b[None, :, k]
        e *= e
        d += e
    return d


def thin(points, radius):
    """the keep mask of eval.py's loop: walk the points in order; a point still set clears every point within d^2 <= radius^2 and stays"""
    points = np.asarray(points, np.float64)
    N, r2 = points.shape[0], radius ** 2
    mask = np.ones(N, bool)
    for s in range(0, N, CHUNK):
        near = _d2(points[s:s + CHUNK], points) <= r2
        for k in range(near.shape[0]):
            if mask[s + k]:
                mask[near[k]] = False
                mask[s + k] = True
    return mask


def thin_rounds(points, radius):
    """the same mask by the round-based definition (undecided -> removed when a lower-index neighbour is kept, -> kept when all of them are
    removed), and the number of rounds it took"""
    points = np.asarray(points, np.float64)
    N, r2 = points.shape[0], radius ** 2
    lower = []
    for s in range(0, N, CHUNK):
        near = _d2(points[s:s + CHUNK], points) <= r2
        for k in range(near.shape[0]):
            j = np.nonzero(near[k][:s + k])[0]
            lower.append(j)
    state, rounds = np.zeros(N, np.int8), 0
    while (state == 0).any():
        rounds += 1
        prev = state.copy()
        for i in np.nonzero(prev == 0)[0]:
            st = prev[lower[i]]
            if (st == 1).any():
                state[i] = 2
            elif (st == 2).all():
                state[i] = 1
    return state == 1, rounds


def nearest(cloud, queries, max_dist):
    """-> (dist [Q], index [Q]): the nearest cloud point (lowest index among equals) where dist < max_dist, else (inf, -1)"""
    cloud, queries = np.asarray(cloud, np.float64), np.asarray(queries, np.float64).reshape(-1, 3)
    dist, index = np.full(queries.shape[0], np.inf), np.full(queries.shape[0], -1, np.int64)
    for s in range(0, queries.shape[0], CHUNK):
        d2 = _d2(queries[s:s + CHUNK], cloud)
        j = np.argmin(d2, 1)
        d = np.sqrt(d2[np.arange(j.shape[0]), j])
        ok = d < max_dist
        dist[s:s + CHUNK][ok], index[s:s + CHUNK][ok] = d[ok], j[ok]
    return dist, index


SUM_THREADS, SUM_BLOCKS = 256, 1024
SUM_MAX_DIST = 10.0 ** 4.8


def _halving_tree(a):
    """the 256-wide tree over axis 1: level w adds element t + w onto element t for t < w, w = 128 .. 1 -> element 0"""
    a = a.copy()
    w = SUM_THREADS // 2
    while w > 0:
        a[:, :w] += a[:, w:2 * w]
        w >>= 1
    return a[:, 0]


def _strided_rows(x, lanes):
    """[n, K] -> [steps, lanes, K]: step j holds rows j * lanes .. ; what is past the end is 0.0, and adding it changes nothing"""
    steps = max(1, -(-x.shape[0] // lanes))
    padded = np.zeros((steps * lanes, x.shape[1]))
    padded[:x.shape[0]] = x
    return padded.reshape(steps, lanes, x.shape[1])


def fixed_order_sum(values, K, max_blocks=SUM_BLOCKS):
    """The library's two-stage fp64 sum of the [n, K] rows, addition by addition.  nb = min(ceil(n / 256), max_blocks) blocks of 256 threads:
    thread t of block b adds rows b * 256 + t, + nb * 256, ... in that order, the block's 256 values go through the halving tree; then
    thread t of one block adds the partials of blocks t, t + 256, ... and the tree runs again.  A row the kernel skips is a row of zeros."""
    x = np.asarray(values, np.float64).reshape(-1, K)
    nb = min(max(1, -(-x.shape[0] // SUM_THREADS)), max_blocks)
    acc = np.zeros((nb * SUM_THREADS, K))
    for step in _strided_rows(x, nb * SUM_THREADS):
        acc = acc + step
    partial = _halving_tree(acc.reshape(nb, SUM_THREADS, K))            # [nb, K]
    acc = np.zeros((SUM_THREADS, K))
    for step in _strided_rows(partial, SUM_THREADS):
        acc = acc + step
    return _halving_tree(acc[None])[0]


def sum_case(n):
    """The seeded distances of the sum tests: 10 ** U(-6, 6), about a tenth of them at or above SUM_MAX_DIST, a few infinite.  The seed is
    picked, not arbitrary: tree-shaped sums are accurate to a fraction of the total's last bit, so two of them differ on about one seed in
    seven only (8 of the seeds 1 .. 59 at n = 600 001), and tests/test_mesheval_restatement.py asserts that this one tells them apart."""
    rng = np.random.default_rng(8)
    d = 10.0 ** rng.uniform(-6.0, 6.0, n)
    d[rng.random(n) < 0.002] = np.inf
    return d


def sum_below(dist, max_dist):
    """mean_below's (sum, count) of dist < max_dist in the library's order"""
    below = dist < max_dist
    return fixed_order_sum(np.stack([np.where(below, dist, 0.0), below.astype(np.float64)], 1), 2)


def obs_masks(points, obs_mask, BB, Res, patch=60):
    """three full-length masks: inside the padded box; also inside the volume's index range; also ObsMask set there"""
    points = np.asarray(points, np.float64)
    BB = np.asarray(BB).astype(np.float32)
    res = float(np.asarray(Res).reshape(-1)[0])
    lo, hi = BB[:1] - patch, BB[1:] + patch * 2                       # float32, as the reference computes them
    inbound = ((points >= lo) & (points < hi)).all(1)
    g = np.rint((points[inbound] - BB[:1]) / res).astype(np.int64)    # half to even
    gin = ((g >= 0) & (g < np.asarray(obs_mask.shape)[None])).all(1)
    grid_inbound, in_obs = np.zeros_like(inbound), np.zeros_like(inbound)
    where = np.nonzero(inbound)[0]
    grid_inbound[where[gin]] = True
    gi = g[gin]
    in_obs[where[gin]] = np.asarray(obs_mask)[gi[:, 0], gi[:, 1], gi[:, 2]] != 0
    return inbound, grid_inbound, in_obs


def above_plane(points, plane):
    p, P = np.asarray(points, np.float64), np.asarray(plane, np.float64).reshape(4)
    return ((P[0] * p[:, 0] + P[1] * p[:, 1]) + P[2] * p[:, 2]) + P[3] > 0


def chamfer(vertices, faces, stl, obs_mask, BB, Res, plane, perm, density=0.2, patch=60, max_dist=20):
    """eval.py end to end with the shuffle given as a permutation; the dict tests compare stage by stage"""
    data_pcd, counts = sample_mesh(vertices, faces, density)
    shuffled = data_pcd[perm]
    keep = thin(shuffled, density)
    data_down = shuffled[keep]
    inbound, grid_inbound, in_obs = obs_masks(data_down, obs_mask, BB, Res, patch)
    data_in, data_in_obs = data_down[inbound], data_down[in_obs]
    dist_d2s, idx_d2s = nearest(stl, data_in_obs, max_dist)
    above = above_plane(stl, plane)
    dist_s2d, idx_s2d = nearest(data_in, stl[above], max_dist)
    mean_d2s, mean_s2d = dist_d2s[dist_d2s < max_dist].mean(), dist_s2d[dist_s2d < max_dist].mean()
    return dict(data_pcd=data_pcd, counts=counts, keep=keep, data_down=data_down, inbound=inbound, grid_inbound=grid_inbound, in_obs=in_obs,
                dist_d2s=dist_d2s, idx_d2s=idx_d2s, above=above, dist_s2d=dist_s2d, idx_s2d=idx_s2d, mean_d2s=mean_d2s, mean_s2d=mean_s2d,
                overall=(mean_d2s + mean_s2d) / 2)


# --------------------------------------------------------------------------- cull ---------------------------------------------------------------------------
def dilate(mask, radius=6):
    """binary dilation of mask != 0 by the disk x^2 + y^2 <= radius^2; clear outside the image"""
    m = np.asarray(mask) != 0
    H, W = m.shape
    pad = np.zeros((H + 2 * radius, W + 2 * radius), bool)
    pad[radius:radius + H, radius:radius + W] = m
    out = np.zeros((H, W), bool)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dx * dx + dy * dy <= radius * radius:
                out |= pad[radius + dy:radius + dy + H, radius + dx:radius + dx + W]
    return out


def cull_vertex_mask(vertices, cameras, dilation=6):
    """cameras: (M float32 [3,4] = rows 0-2 of K w2c, W, H, mask [H,W]).  float32 throughout, one rounding per operation.  A vertex stays
    iff for every camera it projects outside (-1, 1) on some axis or onto a set pixel of the dilated mask (nearest pixel, half to even)."""
    v = np.asarray(vertices).astype(np.float32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    keep = np.ones(v.shape[0], bool)
    f = np.float32
    for M, W, H, mask in cameras:
        M = np.asarray(M, np.float32)
        big = dilate(mask, dilation)
        row = lambda r: ((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            den = row(2) + f(1e-6)
            gx = ((row(0) / den) / f(W - 1) - f(0.5)) * f(2)
            gy = ((row(1) / den) / f(H - 1) - f(0.5)) * f(2)
            valid = (gx > -1) & (gx < 1) & (gy > -1) & (gy < 1)
            ix = np.rint(((gx + f(1)) / f(2)) * f(W - 1))
            iy = np.rint(((gy + f(1)) / f(2)) * f(H - 1))
        inside = valid & (ix >= 0) & (iy >= 0) & (ix <= W - 1) & (iy <= H - 1)
        hit = np.zeros(v.shape[0], bool)
        hit[inside] = big[iy[inside].astype(np.int64), ix[inside].astype(np.int64)]
        keep &= ~valid | hit
    return keep


def apply_vertex_mask(vertices, faces, keep):
    """update_vertices(keep) then update_faces(all three kept): kept vertices in order, faces renumbered"""
    faces = np.asarray(faces).reshape(-1, 3)
    fmask = keep[faces].all(1) if faces.shape[0] else np.zeros(0, bool)
    remap = np.cumsum(keep) - 1
    return np.asarray(vertices)[keep], remap[faces[fmask]].astype(np.int64), fmask
