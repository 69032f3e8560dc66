"""HIP-backed Tanks-and-Temples mesh evaluation: what the reference does with the marching-tetrahedra mesh --
eval_tnt/run.py:94-108 and 152-187 with registration.py (crop, voxel / uniform thinning, three rounds of point-to-point ICP with scaling)
and evaluation.py (nearest-neighbour distances both ways, the cumulative histograms, precision / recall / F-score).  GPU only; geometry is
float64.  Nearest neighbours are mesh_eval.PointGrid.  The files (.ply / .log / _trans.txt) are read by eval_io; trajectory_alignment, which
produces `init_transform`, is ransac_correspondence below, a deterministic RANSAC in HIP, and run_evaluation goes from paths
to the scores.  estimate_normals, the coloured clouds and the plots stay with the caller; eval_tnt/cull_mesh.py is
tnt_cull."""
import ctypes
import functools
import json
import math
import os

import numpy as np
import torch

import eval_io
import geom_host as gh
from diff_gaussian_rasterization import _C
from geom_host import f64, i32, ll, pf64, sz, vp
from mesh_eval import PointGrid

MAX_POINT_NUMBER = 4e6            # registration.py:42
NN_CELLS_PER_MAX_DIST = 8         # the grids' cell = max_dist / 8 unless the caller passes one
MAX_POLYGON, MAX_EDGES = 1024, 4096

_SIGNATURES = {
    "radegs_tnteval_centroids": (i32, [ll, ll, vp, vp, vp, vp]),
    "radegs_tnteval_transform": (i32, [ll, vp, pf64, vp, vp]),
    "radegs_tnteval_crop": (i32, [ll, vp, i32, f64, f64, i32, vp, vp, vp]),
    "radegs_tnteval_voxel_bytes": (sz, [ll]),
    "radegs_tnteval_voxel_plan": (i32, [ll, vp, pf64, f64, vp, sz, vp, vp]),
    "radegs_tnteval_voxel_emit": (i32, [ll, vp, vp, ll, vp, vp, vp]),
    "radegs_tnteval_sums_bytes": (sz, []),
    "radegs_tnteval_pair_sums": (i32, [ll, vp, ll, vp, vp, vp, sz, vp, vp]),
    "radegs_tnteval_histogram": (i32, [ll, vp, i32, vp, f64, vp, vp, vp]),
    **eval_io.SIGNATURES,         # ransac_correspondence below runs on radegs_evalio_ransac; the readers are eval_io's
}


def _lib():
    return gh.bind(_SIGNATURES)


_call = functools.partial(gh.call, _SIGNATURES)


def _matrix(transform, name="transform"):
    """a finite affine 4x4 as float64 numpy, or None"""
    if transform is None:
        return None
    m = np.asarray(transform.detach().cpu() if isinstance(transform, torch.Tensor) else transform, dtype=np.float64)
    if m.shape != (4, 4) or not np.isfinite(m).all():
        raise RuntimeError(f"`{name}` must be a finite 4x4 matrix")
    if not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
        raise RuntimeError(f"`{name}` must be affine: its last row must be (0, 0, 0, 1)")
    return m


def _vector(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.float64:
        raise RuntimeError(f"`{name}` must be a float64 vector")
    _C._require_gpu(t, name)
    return t.detach().contiguous()


# --------------------------------------------------------------------- the cloud of a mesh ---------------------------------------------------------------------
@torch.no_grad()
def mesh_points(vertices, faces):
    """run.py:94-108: the vertices followed by the face centroids ((a + b) + c) / 3.  `vertices` float64 [V,3], `faces` int [F,3] -> [V+F,3]"""
    gh.faces_type(faces)
    v = gh.points(vertices, "vertices")
    f = gh.faces(faces, v.shape[0])
    gh.finite(v, "vertices")
    V, F = v.shape[0], f.shape[0]
    out = torch.empty((V + F, 3), dtype=torch.float64, device=v.device)
    out[:V].copy_(v)
    _call("radegs_tnteval_centroids", v.device, V, F, v, f, ctypes.c_void_p(out.data_ptr() + 24 * V))
    return out


@torch.no_grad()
def transform_points(points, transform):
    """T (x, y, z, 1) per point, rows evaluated as ((m0 x + m1 y) + m2 z) + m3; `transform` None returns the points themselves"""
    m = _matrix(transform)
    p = gh.points(points, "points")
    if m is None:
        return p
    out = torch.empty_like(p)
    _call("radegs_tnteval_transform", p.device, p.shape[0], p, gh.doubles(m[:3].reshape(-1)), out)
    return out


# ----------------------------------------------------------------------------- crop -----------------------------------------------------------------------------
class CropVolume:
    """Open3D's SelectionPolygonVolume: a polygon swept along `orthogonal_axis` ("X", "Y" or "Z") from axis_min to axis_max.
    `bounding_polygon`: [n,3] world points, n >= 3; only the two coordinates across the axis are used."""

    def __init__(self, orthogonal_axis, axis_min, axis_max, bounding_polygon):
        if not isinstance(orthogonal_axis, str):
            raise RuntimeError("`orthogonal_axis` must be a string")
        poly = np.asarray(bounding_polygon, dtype=np.float64)
        if poly.ndim != 2 or poly.shape[1] != 3:
            raise RuntimeError("`bounding_polygon` must have shape (n,3)")
        if poly.shape[0] < 3:
            raise RuntimeError("`bounding_polygon` needs at least three vertices")
        if poly.shape[0] > MAX_POLYGON:
            raise RuntimeError(f"`bounding_polygon` has more than {MAX_POLYGON} vertices")
        if not np.isfinite(poly).all() or not (math.isfinite(axis_min) and math.isfinite(axis_max)):
            raise RuntimeError("`bounding_polygon`, `axis_min` and `axis_max` must be finite")
        self.orthogonal_axis, self.axis_min, self.axis_max, self.bounding_polygon = orthogonal_axis, float(axis_min), float(axis_max), poly

    @property
    def axes(self):
        """(u, v, w): the polygon's two coordinates and the swept one"""
        return {"X": (1, 2, 0), "Y": (0, 2, 1)}.get(self.orthogonal_axis, (0, 1, 2))

    @classmethod
    def from_json(cls, path):
        """the file read_selection_polygon_volume reads"""
        with open(path) as f:
            d = json.load(f)
        return cls(d["orthogonal_axis"], d["axis_min"], d["axis_max"], d["bounding_polygon"])


@torch.no_grad()
def crop_points(points, volume, transform=None):
    """registration.py:120-122: applies `transform` (4x4 or None), then keeps the points inside `volume`.  Returns (kept points, keep mask
    bool [N] over the input)."""
    if not isinstance(volume, CropVolume):
        raise RuntimeError("`volume` must be a CropVolume")
    p = transform_points(points, transform)
    gh.finite(p, "points")
    N, dev = p.shape[0], p.device
    u, v, w = volume.axes
    poly = torch.from_numpy(np.ascontiguousarray(volume.bounding_polygon[:, [u, v]])).to(dev)
    keep = torch.zeros(N, dtype=torch.uint8, device=dev)
    _call("radegs_tnteval_crop", dev, N, p, w, volume.axis_min, volume.axis_max, poly.shape[0], poly, keep)
    keep = keep.bool()
    return p[keep], keep


# ------------------------------------------------------------------------- downsampling -------------------------------------------------------------------------
@torch.no_grad()
def voxel_down_sample(points, voxel):
    """Open3D's voxel_down_sample: the mean of the points of every occupied voxel of the grid with origin min - voxel / 2.  Returns (means
    float64 [M,3], counts int32 [M]), voxels ascending by (ix, iy, iz) -- Open3D's own order is that of a hash map."""
    voxel = gh.positive(voxel, "voxel")
    p = gh.points(points, "points")
    gh.finite(p, "points")
    N, dev = p.shape[0], p.device
    if N == 0:
        return torch.empty((0, 3), dtype=torch.float64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    origin = (p.amin(dim=0).cpu().numpy() - 0.5 * voxel)
    nbytes = _lib().radegs_tnteval_voxel_bytes(N)
    if nbytes == 0:
        gh.check(gh.ERR_TOO_LARGE, "voxel_down_sample")
    ws = gh.workspace(nbytes, dev)
    counts2 = torch.zeros(2, dtype=torch.int64, device=dev)
    _call("radegs_tnteval_voxel_plan", dev, N, p, gh.doubles(origin), voxel, ws, nbytes, counts2)
    M, outside = counts2.tolist()          # the one host read
    if outside:
        raise RuntimeError(f"voxel_down_sample ({gh.ERR_TOO_LARGE}): the cloud spans more than 2^21 voxels of {voxel} along an axis")
    means = torch.empty((M, 3), dtype=torch.float64, device=dev)
    counts = torch.empty(M, dtype=torch.int32, device=dev)
    _call("radegs_tnteval_voxel_emit", dev, N, p, ws, M, means, counts)
    return means, counts


@torch.no_grad()
def uniform_down_sample(points, k):
    """every k-th point, from the first"""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise RuntimeError("`k` must be a positive integer")
    return gh.points(points, "points")[::k].contiguous()


# ------------------------------------------------------------------------------ ICP ------------------------------------------------------------------------------
def umeyama(sums):
    """The similarity of TransformationEstimationPointToPoint(True) (Eigen's umeyama with scaling) from radegs_tnteval_pair_sums' 18 numbers:
    {count, sum s, sum t, sum d^2, sum (t - mt)(s - ms)^T by rows, sum |s - ms|^2}.  Host, numpy float64.  Fewer than three pairs, or a
    source of no extent, give the identity."""
    a = np.asarray(sums, dtype=np.float64).reshape(-1)
    if a.shape != (18,):
        raise RuntimeError("`sums` must hold 18 numbers")
    n = a[0]
    if n < 3 or not a[17] > 0:
        return np.eye(4)
    mu_s, mu_t, var_s, sigma = a[1:4] / n, a[4:7] / n, a[17] / n, a[8:17].reshape(3, 3) / n
    U, D, Vt = np.linalg.svd(sigma)
    S = np.array([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = U @ np.diag(S) @ Vt
    c = float(D @ S) / var_s
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = mu_t - c * (R @ mu_s)
    return T


def _cell(cell, max_dist):
    return float(max_dist) / NN_CELLS_PER_MAX_DIST if cell is None else gh.positive(cell, "cell")


@torch.no_grad()
def icp(source, target, max_dist, max_iter=20, relative_fitness=1e-6, relative_rmse=1e-6, cell=None):
    """Open3D's registration_icp from the identity with TransformationEstimationPointToPoint(True) and
    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iter).  `source`, `target` float64 [N,3] on the GPU.  Returns a dict:
    transformation (numpy [4,4]), fitness, inlier_rmse, iterations (updates applied), history (per evaluation: count, fitness, inlier_rmse),
    correspondence (int64 [|source|] indices into target, -1 without one).  Every evaluation moves the ORIGINAL source by the accumulated
    transformation."""
    max_dist = gh.positive(max_dist, "max_dist")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 0:
        raise RuntimeError("`max_iter` must be a non-negative integer")
    cell = _cell(cell, max_dist)
    src, tgt = gh.points(source, "source"), gh.points(target, "target")
    if src.device != tgt.device:
        raise RuntimeError("`source` and `target` must be on the same device")
    gh.finite(src, "source")
    Q, NT, dev = src.shape[0], tgt.shape[0], src.device
    T = np.eye(4)
    if Q == 0 or NT == 0:
        rec = dict(count=0, fitness=0.0, inlier_rmse=0.0)
        return dict(transformation=T, fitness=0.0, inlier_rmse=0.0, iterations=0, history=[rec],
                    correspondence=torch.full((Q,), -1, dtype=torch.int64, device=dev))
    grid = PointGrid(tgt, cell)                      # built once; refuses a non-finite target
    nbytes = _lib().radegs_tnteval_sums_bytes()
    ws = gh.workspace(nbytes, dev)
    out = torch.empty(18, dtype=torch.float64, device=dev)
    moved = torch.empty_like(src)
    state = {}

    def evaluate():
        _call("radegs_tnteval_transform", dev, Q, src, gh.doubles(T[:3].reshape(-1)), moved)
        _, index = grid.nearest(moved, max_dist)
        _call("radegs_tnteval_pair_sums", dev, Q, moved, NT, tgt, index, ws, nbytes, out)
        sums = out.cpu().numpy()                     # the one host read of an evaluation
        n = int(sums[0])
        state["index"] = index
        return sums, dict(count=n, fitness=n / Q, inlier_rmse=math.sqrt(sums[7] / n) if n else 0.0)

    sums, rec = evaluate()
    history, iterations = [rec], 0
    for _ in range(max_iter):
        T = umeyama(sums) @ T
        iterations += 1
        prev = rec
        sums, rec = evaluate()
        history.append(rec)
        if abs(prev["fitness"] - rec["fitness"]) < relative_fitness and abs(prev["inlier_rmse"] - rec["inlier_rmse"]) < relative_rmse:
            break
    return dict(transformation=T, fitness=rec["fitness"], inlier_rmse=rec["inlier_rmse"], iterations=iterations, history=history,
                correspondence=state["index"])


def _register(s, t, init, threshold, max_itr, cell):
    reg = icp(s, t, threshold, max_iter=max_itr, cell=cell)
    reg["transformation"] = reg["transformation"] @ init
    reg["s"], reg["t"] = s, t
    return reg


@torch.no_grad()
def registration_vol_ds(source, gt_target, init_trans, volume, voxel_size, threshold, max_itr, cell=None):
    """registration.py:166-202: crop both clouds (the source moved by `init_trans` first), voxel-thin them, ICP from the identity;
    transformation = the ICP's @ init_trans.  Returns icp()'s dict with the two thinned clouds as `s` and `t`."""
    init = _matrix(init_trans, "init_trans")
    s = voxel_down_sample(crop_points(source, volume, init)[0], voxel_size)[0]
    t = voxel_down_sample(crop_points(gt_target, volume)[0], voxel_size)[0]
    return _register(s, t, init, threshold, max_itr, cell)


def _uniform(p):
    n = p.shape[0]
    return uniform_down_sample(p, int(round(n / float(MAX_POINT_NUMBER)))) if n > MAX_POINT_NUMBER else p


@torch.no_grad()
def registration_unif(source, gt_target, init_trans, volume, threshold, max_itr, cell=None):
    """registration.py:134-163: as registration_vol_ds with every int(round(n / 4e6))-th point of a cropped cloud of more than 4e6"""
    init = _matrix(init_trans, "init_trans")
    s = _uniform(crop_points(source, volume, init)[0])
    t = _uniform(crop_points(gt_target, volume)[0])
    return _register(s, t, init, threshold, max_itr, cell)


# ---------------------------------------------------------------------------- the scores ----------------------------------------------------------------------------
def histogram_edges(threshold, plot_stretch=5):
    """evaluation.py:189, the reference's own expression"""
    return np.arange(0, threshold * plot_stretch, threshold / 100)


@torch.no_grad()
def precision_recall(dist_s, dist_t, threshold, plot_stretch=5):
    """evaluation.get_f1_score_histo2 on float64 GPU vectors (inf allowed: in no bin, not below the threshold).  Returns (precision, recall,
    fscore, edges_source, cum_source, edges_target, cum_target), the scores Python floats and the rest numpy, value for value the reference's
    -- its zeros for an empty input included."""
    threshold = gh.positive(threshold, "threshold")
    gh.positive(plot_stretch, "plot_stretch")
    d1, d2 = _vector(dist_s, "dist_s"), _vector(dist_t, "dist_t")
    if not (len(d1) and len(d2)):
        return 0, 0, 0, np.array([0]), np.array([0]), np.array([0]), np.array([0])
    edges = histogram_edges(threshold, plot_stretch)
    if not 2 <= edges.shape[0] <= MAX_EDGES:
        raise RuntimeError(f"the histogram has {edges.shape[0]} edges; between 2 and {MAX_EDGES} are supported")
    dev = d1.device
    e = torch.from_numpy(edges).to(dev)
    out = torch.empty((2, edges.shape[0]), dtype=torch.int64, device=dev)      # per side: the bins, then the count below the threshold
    for row, d in zip(out, (d1, d2)):
        _call("radegs_tnteval_histogram", dev, d.shape[0], d, edges.shape[0], e, threshold, row, ctypes.c_void_p(row.data_ptr() + 8 * (edges.shape[0] - 1)))
    h = out.cpu().numpy()                                                        # the one host read
    precision, recall = float(h[0, -1]) / float(len(d1)), float(h[1, -1]) / float(len(d2))
    fscore = 2 * recall * precision / (recall + precision) if recall + precision else float("nan")   # upstream divides by zero there
    cum_source = np.cumsum(h[0, :-1]).astype(float) / len(d1)
    cum_target = np.cumsum(h[1, :-1]).astype(float) / len(d2)
    return precision, recall, fscore, edges, cum_source, edges.copy(), cum_target


def distance_cut(threshold, plot_stretch=5):
    """The distance beyond which neither a histogram count nor the count below the threshold can change: the first double above the larger
    of the histogram's last edge and the threshold (PointGrid.nearest keeps d < max_dist)."""
    return float(np.nextafter(max(float(histogram_edges(threshold, plot_stretch)[-1]), float(threshold)), np.inf))


@torch.no_grad()
def cloud_distances(queries, cloud, cut, cell=None):
    """compute_point_cloud_distance cut at `cut`: (dist float64 [Q], index int64 [Q]), inf and -1 where the nearest point is not closer"""
    cut = gh.positive(cut, "cut")
    q, c = gh.points(queries, "queries"), gh.points(cloud, "cloud")
    if c.shape[0] == 0 or q.shape[0] == 0:
        return (torch.full((q.shape[0],), math.inf, dtype=torch.float64, device=q.device), torch.full((q.shape[0],), -1, dtype=torch.int64, device=q.device))
    return PointGrid(c, _cell(cell, cut)).nearest(q, cut)


@torch.no_grad()
def evaluate(vertices, faces, gt_points, init_transform, volume, tau, plot_stretch=5, cut=None):
    """run.py:152-187 end to end: three registrations, then EvaluateHisto.  `init_transform`: what trajectory_alignment returns.  `cut`: the
    distance at which the two nearest-neighbour passes give up (default distance_cut(tau, plot_stretch); no score depends on it).  Returns
    a dict: precision, recall, fscore, edges_source, cum_source, edges_target, cum_target, r2, r3, r (the registrations), transformation,
    s, t (the two evaluated clouds), dist1 / idx1 (s to t), dist2 / idx2 (t to s)."""
    tau = gh.positive(tau, "tau")
    gh.positive(plot_stretch, "plot_stretch")
    init = _matrix(init_transform, "init_transform")
    if init is None:
        raise RuntimeError("`init_transform` must be a 4x4 matrix")
    if not isinstance(volume, CropVolume):
        raise RuntimeError("`volume` must be a CropVolume")
    gt = gh.points(gt_points, "gt_points")
    pcd = mesh_points(vertices, faces)
    r2 = registration_vol_ds(pcd, gt, init, volume, tau, tau * 80, 20)
    r3 = registration_vol_ds(pcd, gt, r2["transformation"], volume, tau / 2.0, tau * 20, 20)
    r = registration_unif(pcd, gt, r3["transformation"], volume, 2 * tau, 20)
    out = evaluate_histo(pcd, gt, r["transformation"], volume, tau / 2.0, tau, plot_stretch, cut)
    out.update(r2=r2, r3=r3, r=r, transformation=r["transformation"])
    return out


@torch.no_grad()
def evaluate_histo(source, target, trans, volume, voxel_size, threshold, plot_stretch=5, cut=None):
    """evaluation.EvaluateHisto without its normals and files: move, crop and voxel-thin both clouds, distances both ways, the scores"""
    cut = distance_cut(threshold, plot_stretch) if cut is None else gh.positive(cut, "cut")
    s = voxel_down_sample(crop_points(source, volume, _matrix(trans, "trans"))[0], voxel_size)[0]
    t = voxel_down_sample(crop_points(target, volume)[0], voxel_size)[0]
    dist1, idx1 = cloud_distances(s, t, cut)
    dist2, idx2 = cloud_distances(t, s, cut)
    names = ("precision", "recall", "fscore", "edges_source", "cum_source", "edges_target", "cum_target")
    out = dict(zip(names, precision_recall(dist1, dist2, threshold, plot_stretch)))
    out.update(s=s, t=t, dist1=dist1, idx1=idx1, dist2=dist2, idx2=idx2)
    return out


# ------------------------------------------------------------------- the coarse alignment -------------------------------------------------------------------
def _integer(value, name, lo, hi):
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        raise RuntimeError(f"`{name}` must be an integer in [{lo}, {hi}]")
    return value


@torch.no_grad()
def ransac_correspondence(source, target, max_dist=0.2, ransac_n=6, max_iteration=100000, seed=0, with_scaling=True, return_all=False):
    """Open3D's registration_ransac_based_on_correspondence with TransformationEstimationPointToPoint(True) over the correspondence set (i, i):
    `source`, `target` float64 [N,3] on the GPU, already paired.  Hypothesis h = 0 .. max_iteration - 1 draws `ransac_n` distinct pairs from
    the counter-based generator of include/radegs.h (a function of seed, h and the draw alone), fits Eigen's umeyama to them, moves all N
    pairs and counts d < max_dist; the best is the largest count, then the smallest sqrt(sumsq / count), then the smallest h.  ALL hypotheses
    are evaluated (Open3D stops early by a confidence estimate, and its draws are unseeded): two runs give the same bits.  Returns a dict:
    transformation (numpy 4x4), fitness (count / N), inlier_rmse, hypothesis (-1 when no hypothesis has an inlier: the identity, fitness 0),
    count; with `return_all` also counts int32 [max_iteration] and sumsq float64 [max_iteration] on the GPU."""
    max_dist = gh.positive(max_dist, "max_dist")
    ransac_n = _integer(ransac_n, "ransac_n", eval_io.RANSAC_MIN_N, eval_io.RANSAC_MAX_N)
    K = _integer(max_iteration, "max_iteration", 1, 2 ** 31 - 1)
    seed = _integer(seed, "seed", 0, 2 ** 64 - 1)
    if with_scaling is not True:
        raise RuntimeError("`with_scaling` must be True: the trajectory alignment estimates a similarity (TransformationEstimationPointToPoint(True))")
    src, tgt = gh.points(source, "source"), gh.points(target, "target")
    if src.device != tgt.device or src.shape != tgt.shape:
        raise RuntimeError("`source` and `target` must be paired: the same shape on the same device")
    N, dev = src.shape[0], src.device
    if N < ransac_n:
        raise RuntimeError(f"{N} pairs are fewer than `ransac_n` = {ransac_n}")
    if N >= 2 ** 31:
        gh.check(gh.ERR_TOO_LARGE, "ransac_correspondence")
    gh.finite(src, "source")
    gh.finite(tgt, "target")
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    sumsq = torch.empty(K, dtype=torch.float64, device=dev)
    out = torch.empty(15, dtype=torch.float64, device=dev)
    _call("radegs_evalio_ransac", dev, N, src, tgt, max_dist, ransac_n, K, seed, counts, sumsq, out)
    o = out.cpu().numpy()                              # the one host read
    T = np.eye(4)
    T[:3] = o[:12].reshape(3, 4)
    count = int(o[12])
    res = dict(transformation=T, fitness=count / N, inlier_rmse=math.sqrt(o[13] / count) if count else 0.0, hypothesis=int(o[14]), count=count)
    if return_all:
        res.update(counts=counts, sumsq=sumsq)
    return res


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"tnt_eval runs on the GPU only, got device `{device}`")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _centres(traj):
    """convert_trajectory_to_pointcloud: the camera centres pose[:3, 3] of [B,4,4] poses (or of a list of CameraPose-like objects / 4x4s)"""
    if not isinstance(traj, np.ndarray):
        traj = np.array([np.asarray(getattr(p, "pose", p), dtype=np.float64) for p in traj], dtype=np.float64).reshape(-1, 4, 4)
    if traj.ndim != 3 or traj.shape[1:] != (4, 4):
        raise RuntimeError(f"a trajectory must be a stack of 4x4 poses, got shape {traj.shape}")
    return np.ascontiguousarray(traj[:, :3, 3], dtype=np.float64)


@torch.no_grad()
def trajectory_alignment(map_file, traj_to_register, gt_traj_col, gt_trans, seed=0, device="cuda"):
    """registration.py:66-110: the similarity that takes the camera centres of `traj_to_register` onto those of `gt_traj_col` moved by
    `gt_trans` (4x4 or None), pose i paired with pose i.  Trajectories are [B,4,4] arrays (eval_io.read_trajectory's) or lists of poses.
    With more than 1600 poses and a `map_file`, the sparse trajectory of eval_io.gen_sparse_trajectory is registered.  Returns numpy 4x4."""
    ref = _centres(gt_traj_col)
    m = _matrix(gt_trans, "gt_trans")
    est_traj = traj_to_register if isinstance(traj_to_register, np.ndarray) else np.array(
        [np.asarray(getattr(p, "pose", p), dtype=np.float64) for p in traj_to_register], dtype=np.float64).reshape(-1, 4, 4)
    if len(est_traj) > 1600 and map_file is not None:
        est_traj = eval_io.gen_sparse_trajectory(eval_io.read_mapping(map_file)[2], est_traj)
    est = _centres(est_traj)
    if est.shape != ref.shape:
        raise RuntimeError(f"{est.shape[0]} poses to register against {ref.shape[0]} reference poses: pose i is paired with pose i")
    dev = _device(device)
    ref_d = transform_points(torch.from_numpy(ref).to(dev), m)
    return ransac_correspondence(torch.from_numpy(est).to(dev), ref_d, 0.2, 6, 100000, seed=seed)["transformation"]


# ------------------------------------------------------------------------- from paths to the scores -------------------------------------------------------------------------
SCENES_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01,
              "Truck": 0.005}          # eval_tnt/config.py scenes_tau_dict, restated


@torch.no_grad()
def run_evaluation(dataset_dir, traj_path, ply_path, out_dir=None, seed=0, device="cuda"):
    """eval_tnt/run.py:58-196 from paths alone: the scene is the directory's name and sets dTau; reads {scene}_COLMAP_SfM.log, {scene}_trans.txt,
    {scene}.ply, {scene}.json, the trajectory to register (.npy or .log; upstream's .json branch is refused) and the mesh; runs
    trajectory_alignment (without the mapping file, as upstream, which sets it to None) and evaluate; prints upstream's report.  With
    `out_dir`, writes {scene}.recall.txt, {scene}.precision.txt and {scene}.prf_tau_plotstr.txt as EvaluateHisto's np.savetxt calls do.
    Returns evaluate's dict with `scene`, `tau` and `init_transform` added."""
    scene = os.path.basename(os.path.normpath(dataset_dir))
    if scene not in SCENES_TAU:
        raise RuntimeError(f"invalid dataset_dir `{dataset_dir}`: `{scene}` is none of {sorted(SCENES_TAU)}")
    if traj_path.endswith(".json"):
        raise RuntimeError(f"{traj_path}: the .json branch of run.py (auto_orient_and_center_poses) is not supported; pass a .npy stack or a .log file")
    tau = SCENES_TAU[scene]
    dev = _device(device)
    print("")
    print("===========================")
    print("Evaluating %s" % scene)
    print("===========================")
    vertices, faces = eval_io.read_ply_mesh(ply_path, dev)
    gt = eval_io.read_ply_points(os.path.join(dataset_dir, scene + ".ply"), dev)
    gt_trans = eval_io.load_transform(os.path.join(dataset_dir, scene + "_trans.txt"))
    traj = np.load(traj_path) if traj_path.endswith(".npy") else eval_io.read_trajectory(traj_path)[0]
    gt_traj = eval_io.read_trajectory(os.path.join(dataset_dir, scene + "_COLMAP_SfM.log"))[0]
    init = trajectory_alignment(None, np.asarray(traj, dtype=np.float64), gt_traj, gt_trans, seed=seed, device=dev)
    volume = CropVolume.from_json(os.path.join(dataset_dir, scene + ".json"))
    res = evaluate(vertices, faces, gt, init, volume, tau)
    res.update(scene=scene, tau=tau, init_transform=init)
    print("==============================")
    print("evaluation result : %s" % scene)
    print("==============================")
    print("distance tau : %.3f" % tau)
    print("precision : %.4f" % res["precision"])
    print("recall : %.4f" % res["recall"])
    print("f-score : %.4f" % res["fscore"])
    print("==============================")
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        np.savetxt(os.path.join(out_dir, scene + ".recall.txt"), res["cum_target"])
        np.savetxt(os.path.join(out_dir, scene + ".precision.txt"), res["cum_source"])
        np.savetxt(os.path.join(out_dir, scene + ".prf_tau_plotstr.txt"), np.array([res["precision"], res["recall"], res["fscore"], tau, 5]))
    return res
