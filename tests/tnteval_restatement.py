"""Tanks-and-Temples mesh evaluation restated in NumPy / SciPy, in this project's own words: the specification of
include/radegs.h ("Tanks-and-Temples evaluation") and DESIGN 11 N10, one rounding per operation in the order written there.  Neighbours come
from scipy's cKDTree.  It is checked against what the reference's own NumPy code wrote (tests/test_tnteval_restatement.py) and then serves as
the expectation of tests/test_gpu_tnteval.py.

Every decision on a threshold is checked for a MARGIN (raise Margin), so that an implementation whose arithmetic differs in the last bit
must still decide alike and the comparison can be exact.  Makers of inputs redraw what misses a margin (`redraw`); tests never skip."""
import numpy as np
from scipy.spatial import cKDTree

from mesheval_restatement import fixed_order_sum

REL = 1e-9          # distances against max_dist / tau / a bin edge, first against second neighbour, points against polygon edges and bounds
VOXEL_MARGIN = 1e-6  # of a voxel, from a voxel face
MAX_POINT_NUMBER = 4e6


class Margin(AssertionError):
    pass


def _need(ok, what):
    if not bool(np.all(ok)):
        raise Margin(what)


# ------------------------------------------------------------------------- clouds -------------------------------------------------------------------------
def mesh_points(vertices, faces):
    v, f = np.asarray(vertices, np.float64), np.asarray(faces).reshape(-1, 3)
    c = (v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]
    return np.concatenate([v, c / 3.0], 0)


def transform(points, T):
    p, T = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(T, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def axes_of(orthogonal_axis):
    return {"X": (1, 2, 0), "Y": (0, 2, 1)}.get(orthogonal_axis, (0, 1, 2))


def crop_bad(points, volume):
    """the points whose crop decision has no margin: within REL (relative) of an axis bound without being on it, level with a polygon vertex,
    or with a crossing within REL of their own u"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    u, v, w = axes_of(volume["orthogonal_axis"])
    poly = np.asarray(volume["bounding_polygon"], np.float64)
    scale = max(float(np.abs(poly).max()), 1e-300)
    bad = np.zeros(p.shape[0], bool)
    for bound in (volume["axis_min"], volume["axis_max"]):
        d = np.abs(p[:, w] - bound)
        bad |= (d != 0) & (d <= REL * max(abs(bound), scale))
    pu, pv = p[:, u], p[:, v]
    n = poly.shape[0]
    for i in range(n):
        a, b = poly[i], poly[(i + 1) % n]
        bad |= np.abs(pv - a[v]) <= REL * scale
        cross = (a[v] > pv) != (b[v] > pv)
        with np.errstate(divide="ignore", invalid="ignore"):
            node = a[u] + (pv - a[v]) / (b[v] - a[v]) * (b[u] - a[u])
        bad |= cross & (np.abs(node - pu) <= REL * np.maximum(scale, np.abs(pu)))
    return bad


def crop_mask(points, volume, check=True):
    """volume: dict(orthogonal_axis, axis_min, axis_max, bounding_polygon [n,3]).  Even-odd rule on the crossings left of the point."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if check:
        _need(~crop_bad(p, volume), "a point within the margin of the crop volume's boundary")
    u, v, w = axes_of(volume["orthogonal_axis"])
    poly = np.asarray(volume["bounding_polygon"], np.float64)
    pu, pv, pw = p[:, u], p[:, v], p[:, w]
    left = np.zeros(p.shape[0], np.int64)
    n = poly.shape[0]
    for i in range(n):
        a, b = poly[i], poly[(i + 1) % n]
        cross = (a[v] > pv) != (b[v] > pv)
        with np.errstate(divide="ignore", invalid="ignore"):
            node = a[u] + (pv - a[v]) / (b[v] - a[v]) * (b[u] - a[u])
        left += cross & (node < pu)
    return ~(pw < volume["axis_min"]) & ~(pw > volume["axis_max"]) & (left % 2 == 1)


def crop(points, volume, T=None, check=True):
    p = np.asarray(points, np.float64).reshape(-1, 3) if T is None else transform(points, T)
    keep = crop_mask(p, volume, check)
    return p[keep], keep


def voxel_bad(points, voxel):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if p.shape[0] == 0:
        return np.zeros(0, bool)
    r = (p - (p.min(0) - 0.5 * voxel)) / voxel
    return (np.abs(r - np.rint(r)) <= VOXEL_MARGIN).any(1)


def voxel_down_sample(points, voxel, check=True):
    """-> (means [M,3], counts [M], index [M,3]) ascending by (ix, iy, iz); a voxel's points are added in index order, then divided"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if p.shape[0] == 0:
        return np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros((0, 3), np.int64)
    if check:
        _need(~voxel_bad(p, voxel), "a coordinate within the margin of a voxel face")
    idx = np.floor((p - (p.min(0) - 0.5 * voxel)) / voxel).astype(np.int64)
    assert idx.min() >= 0 and idx.max() < 2 ** 21, "more than 2^21 voxels along an axis"
    order = np.lexsort((np.arange(p.shape[0]), idx[:, 2], idx[:, 1], idx[:, 0]))      # stable: index order inside a voxel
    sidx = idx[order]
    first = np.ones(p.shape[0], bool)
    first[1:] = (sidx[1:] != sidx[:-1]).any(1)
    start = np.nonzero(first)[0]
    counts = np.diff(np.append(start, p.shape[0]))
    sums = np.zeros((start.shape[0], 3))
    for k in range(int(counts.max())):                                                 # round k adds every voxel's k-th point
        has = counts > k
        sums[has] = sums[has] + p[order[start[has] + k]]
    return sums / counts[:, None].astype(np.float64), counts.astype(np.int32), sidx[start]


def uniform_down_sample(points, k):
    return np.asarray(points)[::k]


# ----------------------------------------------------------------------- neighbours -----------------------------------------------------------------------
def nearest(cloud, queries, max_dist, check=True, tree=None):
    """-> (dist [Q], index [Q]): the nearest cloud point where dist < max_dist, else (inf, -1); dist = sqrt((dx^2 + dy^2) + dz^2)"""
    cloud, q = np.asarray(cloud, np.float64).reshape(-1, 3), np.asarray(queries, np.float64).reshape(-1, 3)
    dist, index = np.full(q.shape[0], np.inf), np.full(q.shape[0], -1, np.int64)
    if cloud.shape[0] == 0 or q.shape[0] == 0:
        return dist, index
    tree = cKDTree(cloud) if tree is None else tree
    k = min(2, cloud.shape[0])
    dd, ii = tree.query(q, k=k)
    dd, ii = dd.reshape(q.shape[0], k), ii.reshape(q.shape[0], k)
    j = ii[:, 0]
    e = q - cloud[j]
    d = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    hit = d < max_dist
    if check:
        if np.isfinite(max_dist):
            _need(np.abs(d - max_dist) > REL * max_dist, "a distance within the margin of max_dist")
        if k == 2:
            _need(~hit | (dd[:, 1] - dd[:, 0] > REL * dd[:, 1]), "two neighbours at (nearly) the same distance")
    dist[hit], index[hit] = d[hit], j[hit]
    return dist, index


# ---------------------------------------------------------------------------- ICP ----------------------------------------------------------------------------
def umeyama(s, t):
    """Eigen's umeyama with scaling from the matched points themselves: t ~ c R s + b"""
    s, t = np.asarray(s, np.float64).reshape(-1, 3), np.asarray(t, np.float64).reshape(-1, 3)
    n = s.shape[0]
    if n < 3:
        return np.eye(4)
    mu_s, mu_t = s.mean(0), t.mean(0)
    ds, dt = s - mu_s, t - mu_t
    var_s = (ds * ds).sum() / n
    if not var_s > 0:
        return np.eye(4)
    U, D, Vt = np.linalg.svd(dt.T @ ds / n)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    c = (D * S).sum() / var_s
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = c * R, mu_t - c * (R @ mu_s)
    return T


def pair_sums(moved, target, index):
    """radegs_tnteval_pair_sums' 18 outputs, from the kernel comments of radegs_tnteval.hip, in the library's order of additions.  A pair is a
    query q with index[q] in [0, NT): s = moved[q], t = target[index[q]]; every other query adds nothing.
        [0, 8)   count, sum s, sum t, sum (dx dx + dy dy) + dz dz   with d = s - t
        means6 = sum s / count, sum t / count   (zeros without a pair)
        [8, 18)  sum dt[r] ds[c] by rows, sum (ds0 ds0 + ds1 ds1) + ds2 ds2   with ds = s - mean s, dt = t - mean t"""
    moved, target, index = np.asarray(moved, np.float64).reshape(-1, 3), np.asarray(target, np.float64).reshape(-1, 3), np.asarray(index, np.int64)
    pair = (index >= 0) & (index < target.shape[0])
    s, t = moved, target[np.where(pair, index, 0)]
    d = s - t
    rows = np.concatenate([np.ones((s.shape[0], 1)), s, t, ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]], 1)
    sums = fixed_order_sum(np.where(pair[:, None], rows, 0.0), 8)
    means6 = sums[1:7] / sums[0] if sums[0] > 0.0 else np.zeros(6)
    ds, dt = s - means6[:3], t - means6[3:]
    rows = np.concatenate([(dt[:, :, None] * ds[:, None, :]).reshape(-1, 9), ((ds[:, 0] * ds[:, 0] + ds[:, 1] * ds[:, 1]) + ds[:, 2] * ds[:, 2])[:, None]], 1)
    return np.concatenate([sums, fixed_order_sum(np.where(pair[:, None], rows, 0.0), 10)])


def icp(source, target, max_dist, max_iter=20, relative_fitness=1e-6, relative_rmse=1e-6, check=True):
    """Open3D's RegistrationICP from the identity; every evaluation moves the original source by the accumulated transformation"""
    source, target = np.asarray(source, np.float64).reshape(-1, 3), np.asarray(target, np.float64).reshape(-1, 3)
    T = np.eye(4)
    if source.shape[0] == 0 or target.shape[0] == 0:
        return dict(transformation=T, fitness=0.0, inlier_rmse=0.0, iterations=0, history=[dict(count=0, fitness=0.0, inlier_rmse=0.0)],
                    correspondence=np.full(source.shape[0], -1, np.int64))
    tree = cKDTree(target)

    def evaluate():
        moved = transform(source, T)
        dist, idx = nearest(target, moved, max_dist, check, tree)
        hit = idx >= 0
        n = int(hit.sum())
        rmse = float(np.sqrt((dist[hit] * dist[hit]).sum() / n)) if n else 0.0
        return moved, idx, dict(count=n, fitness=n / source.shape[0], inlier_rmse=rmse)

    moved, idx, rec = evaluate()
    history, iterations = [rec], 0
    for _ in range(max_iter):
        hit = idx >= 0
        T = umeyama(moved[hit], target[idx[hit]]) @ T
        iterations += 1
        prev = rec
        moved, idx, rec = evaluate()
        history.append(rec)
        if check:                                       # the stopping rule is a decision too (1e-3 relative: the steps carry rounding of their own)
            _need(abs(abs(prev["fitness"] - rec["fitness"]) - relative_fitness) > 1e-3 * relative_fitness, "a fitness step at the criterion")
            _need(abs(abs(prev["inlier_rmse"] - rec["inlier_rmse"]) - relative_rmse) > 1e-3 * relative_rmse, "an rmse step at the criterion")
        if abs(prev["fitness"] - rec["fitness"]) < relative_fitness and abs(prev["inlier_rmse"] - rec["inlier_rmse"]) < relative_rmse:
            break
    return dict(transformation=T, fitness=rec["fitness"], inlier_rmse=rec["inlier_rmse"], iterations=iterations, history=history, correspondence=idx)


def registration_vol_ds(source, target, init, volume, voxel, threshold, max_itr, check=True):
    s_crop, s_keep = crop(source, volume, init, check)
    t_crop, t_keep = crop(target, volume, None, check)
    s, s_counts, _ = voxel_down_sample(s_crop, voxel, check)
    t, t_counts, _ = voxel_down_sample(t_crop, voxel, check)
    reg = icp(s, t, threshold, max_itr, check=check)
    reg["transformation"] = reg["transformation"] @ np.asarray(init, np.float64)
    reg.update(s=s, t=t, s_keep=s_keep, t_keep=t_keep, s_crop=s_crop, t_crop=t_crop, s_counts=s_counts, t_counts=t_counts)
    return reg


def _uniform(p):
    n = p.shape[0]
    return uniform_down_sample(p, int(round(n / float(MAX_POINT_NUMBER)))) if n > MAX_POINT_NUMBER else p


def registration_unif(source, target, init, volume, threshold, max_itr, check=True):
    s_crop, s_keep = crop(source, volume, init, check)
    t_crop, t_keep = crop(target, volume, None, check)
    s, t = _uniform(s_crop), _uniform(t_crop)
    reg = icp(s, t, threshold, max_itr, check=check)
    reg["transformation"] = reg["transformation"] @ np.asarray(init, np.float64)
    reg.update(s=s, t=t, s_keep=s_keep, t_keep=t_keep)
    return reg


# -------------------------------------------------------------------------- the scores --------------------------------------------------------------------------
def histogram(d, edges):
    """numpy.histogram's rule over explicit edges, by search: left-closed bins, the last one closed on both sides"""
    d, edges = np.asarray(d, np.float64), np.asarray(edges, np.float64)
    inside = (d >= edges[0]) & (d <= edges[-1])
    b = np.searchsorted(edges, d[inside], side="right") - 1
    b = np.minimum(b, edges.shape[0] - 2)
    return np.bincount(b, minlength=edges.shape[0] - 1).astype(np.int64)


def scores_bad(d, threshold, edges):
    d = np.asarray(d, np.float64)
    f = d[np.isfinite(d)]
    near = np.abs(f - threshold) <= REL * threshold
    k = np.clip(np.searchsorted(edges, f), 1, edges.shape[0] - 1)
    for e in (edges[k - 1], edges[k]):
        near |= np.abs(f - e) <= REL * np.maximum(e, threshold)
    out = np.zeros(d.shape[0], bool)
    out[np.isfinite(d)] = near
    return out


def precision_recall(dist_s, dist_t, threshold, plot_stretch=5, check=True):
    d1, d2 = np.asarray(dist_s, np.float64), np.asarray(dist_t, np.float64)
    if not (len(d1) and len(d2)):
        return 0, 0, 0, np.array([0]), np.array([0]), np.array([0]), np.array([0])
    edges = np.arange(0, threshold * plot_stretch, threshold / 100)
    if check:
        _need(~scores_bad(d1, threshold, edges) & True, "a distance within the margin of tau or of a bin edge")
        _need(~scores_bad(d2, threshold, edges) & True, "a distance within the margin of tau or of a bin edge")
    recall = float(int((d2 < threshold).sum())) / float(len(d2))
    precision = float(int((d1 < threshold).sum())) / float(len(d1))
    fscore = 2 * recall * precision / (recall + precision) if recall + precision else float("nan")
    cum_source = np.cumsum(histogram(d1, edges)).astype(float) / len(d1)
    cum_target = np.cumsum(histogram(d2, edges)).astype(float) / len(d2)
    return precision, recall, fscore, edges, cum_source, edges.copy(), cum_target


def evaluate_histo(source, target, trans, volume, voxel, threshold, plot_stretch=5, check=True):
    s_crop, s_keep = crop(source, volume, trans, check)
    t_crop, t_keep = crop(target, volume, None, check)
    s, s_counts, _ = voxel_down_sample(s_crop, voxel, check)
    t, t_counts, _ = voxel_down_sample(t_crop, voxel, check)
    dist1, idx1 = nearest(t, s, np.inf, check)          # upstream's distances are unbounded
    dist2, idx2 = nearest(s, t, np.inf, check)
    names = ("precision", "recall", "fscore", "edges_source", "cum_source", "edges_target", "cum_target")
    out = dict(zip(names, precision_recall(dist1, dist2, threshold, plot_stretch, check)))
    out.update(s=s, t=t, s_keep=s_keep, t_keep=t_keep, s_crop=s_crop, t_crop=t_crop, s_counts=s_counts, t_counts=t_counts, dist1=dist1, idx1=idx1,
               dist2=dist2, idx2=idx2)
    return out


def evaluate(vertices, faces, gt_points, init, volume, tau, plot_stretch=5, check=True):
    """run.py:152-187"""
    pcd, gt = mesh_points(vertices, faces), np.asarray(gt_points, np.float64)
    r2 = registration_vol_ds(pcd, gt, init, volume, tau, tau * 80, 20, check)
    r3 = registration_vol_ds(pcd, gt, r2["transformation"], volume, tau / 2.0, tau * 20, 20, check)
    r = registration_unif(pcd, gt, r3["transformation"], volume, 2 * tau, 20, check)
    out = evaluate_histo(pcd, gt, r["transformation"], volume, tau / 2.0, tau, plot_stretch, check)
    out.update(pcd=pcd, r2=r2, r3=r3, r=r, transformation=r["transformation"])
    return out


# ------------------------------------------------------------------------ test inputs ------------------------------------------------------------------------
def redraw(points, bad_of, draw, tries=100):
    """replaces the points bad_of(points) marks by draw(count) until none is marked"""
    p = np.array(points, np.float64)
    for _ in range(tries):
        bad = bad_of(p)
        if not bad.any():
            return p
        p[bad] = draw(int(bad.sum()))
    raise Margin("no draw keeps the margins")


def volume_of(fx):
    """the crop volume of tests/golden/tnteval_pipeline.npz as the dict this module takes"""
    return dict(orthogonal_axis=str(fx["orthogonal_axis"]), axis_min=float(fx["axis_min"]), axis_max=float(fx["axis_max"]),
                bounding_polygon=np.asarray(fx["bounding_polygon"], np.float64))
