"""HIP-backed Delaunay tetrahedralisation: the `cells = cpp.triangulate(points)` of mesh_extract_tetrahedra.py:63, which
upstream hands to tetranerf's CGAL Delaunay_triangulation_3.  GPU only.  Every point clips its own Voronoi cell against its neighbours
("meshless Voronoi"); a cell's vertices are the tetrahedra at that point, and a tetrahedron counts once all four of its corners found it.
All arithmetic is float64.  The input that matters, get_tetra_points' box corners, is exactly degenerate, so the coordinates are first moved
by a deterministic jitter of `jitter` x the bounding-box diagonal: the result is the Delaunay triangulation of those coordinates, a valid
tetrahedralisation of the hull of the input to 1e-9 of the scene's size.  include/radegs.h, "Delaunay", is the specification, DESIGN 11 N13
the reasoning, tests/delaunay_restatement.py the NumPy restatement."""
import ctypes
import functools
import math

import torch

import geom_host as gh
from geom_host import f64, i32, ll, sz, vp

ull = ctypes.c_ulonglong
MAX_POINTS = 2 ** 31 - 8
MAX_RECORDS = 2 ** 32 - 65537     # 4 T records through the 32-bit sort (include/radegs.h)
RETRIES = 2

SIGNATURES = {
    "radegs_delaunay_bytes": (sz, [ll, ll]),
    "radegs_delaunay_perturb": (i32, [ll, vp, f64, ull, vp, vp]),
    "radegs_delaunay_plan": (i32, [ll, vp, gh.pf64, f64, ull, ll, vp, sz, vp, vp]),
    "radegs_delaunay_emit": (i32, [ll, ll, ll, vp, sz, ll, vp, vp, vp]),
}


def _lib():
    return gh.bind(SIGNATURES)


_call = functools.partial(gh.call, SIGNATURES)


# ------------------------------------------------------------------------- arguments -------------------------------------------------------------------------
def _points(points):
    """float64 [N,3] on the GPU, finite, N >= 4: a float32 tensor is widened (exactly), anything else refused"""
    if not isinstance(points, torch.Tensor) or points.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("`points` must be a float32 or float64 tensor")
    p = gh.points(points, "points", points.dtype)
    if p.shape[0] < 4:
        raise RuntimeError(f"`points` must hold at least 4 points, got {p.shape[0]}")
    if p.shape[0] > MAX_POINTS:
        raise RuntimeError(f"`points` holds more than 2^31 - 8 points ({p.shape[0]}): beyond the 32-bit sort (include/radegs.h)")
    gh.finite(p, "points")
    return p.double()


def _jitter(jitter):
    if isinstance(jitter, bool) or not isinstance(jitter, (int, float)) or not math.isfinite(jitter) or jitter < 0:
        raise RuntimeError("`jitter` must be a non-negative finite number")
    return float(jitter)


def _seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63:
        raise RuntimeError("`seed` must be an integer in [0, 2^63)")
    return seed


def _bounds(p64):
    """([min x, y, z, max x, y, z], diagonal): one host read; the diagonal is sqrt((dx dx + dy dy) + dz dz) in float64"""
    lo, hi = p64.min(dim=0).values.tolist(), p64.max(dim=0).values.tolist()
    d = [h - l for l, h in zip(lo, hi)]
    return lo + hi, math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


# ------------------------------------------------------------------------- perturbation -------------------------------------------------------------------------
@torch.no_grad()
def perturbed(points, jitter=1e-9, seed=0):
    """The float64 [N,3] coordinates triangulate(points, jitter, seed) computes on: x + (jitter diag) (u - 0.5), diag the bounding-box
    diagonal and u in [0, 1) the top 53 bits of a splitmix64-style hash of (seed, 3 i + axis) (include/radegs.h writes it out).
    jitter = 0 returns the input widened to float64.  One host read."""
    jitter, seed = _jitter(jitter), _seed(seed)
    p = _points(points)
    if jitter == 0.0:
        return p.clone()
    _, diag = _bounds(p)
    out = torch.empty_like(p)
    _call("radegs_delaunay_perturb", p.device, p.shape[0], p, jitter * diag, seed, out)
    return out


# ------------------------------------------------------------------------- triangulation -------------------------------------------------------------------------
def _plan(p, bounds, scale, seed):
    """the cells of every point as records in a workspace: (workspace, its bytes, record capacity, [records, deferred, uncertain, overflow]);
    one host read, one more for every time the records outgrew the workspace"""
    dev, N = p.device, p.shape[0]
    counts4 = torch.zeros(4, dtype=torch.int64, device=dev)
    capacity = min(32 * N + 1024, MAX_RECORDS)          # 4 T is about 27 N on scattered points
    while True:
        nbytes = _lib().radegs_delaunay_bytes(N, capacity)
        ws = gh.workspace(nbytes, dev)
        _call("radegs_delaunay_plan", dev, N, p, gh.doubles(bounds), scale, seed, capacity, ws, nbytes, counts4)
        counts = counts4.tolist()                    # the host read that sizes the sort and the output
        if counts[0] <= capacity:
            return ws, nbytes, capacity, counts
        if counts[0] > MAX_RECORDS:
            raise RuntimeError(f"radegs_delaunay_plan: {counts[0]} records (4 T) are more than the 32-bit sort addresses (include/radegs.h)")
        del ws
        capacity = counts[0]                         # an input with more tetrahedra a point than scattered ones have


def _emit(N, ws, nbytes, capacity, records):
    """(cells int32 [ceil(records / 4), 4], distinct quadruples, inconsistent ones); one host read"""
    dev = ws.device
    rows = (records + 3) // 4
    cells = torch.empty((rows, 4), dtype=torch.int32, device=dev)
    counts2 = torch.zeros(2, dtype=torch.int64, device=dev)
    _call("radegs_delaunay_emit", dev, N, records, capacity, ws, nbytes, rows, cells, counts2)
    unique, inconsistent = counts2.tolist()
    return cells, unique, inconsistent


def _attempt(p, bounds, scale, seed):
    """one plan + emit: (cells int32 [T,4] or None, info)"""
    ws, nbytes, capacity, (records, deferred, uncertain, overflow) = _plan(p, bounds, scale, seed)
    info = dict(tets=0, inconsistent=0, uncertain=uncertain, deferred=deferred, overflow=overflow)
    if overflow:
        raise RuntimeError(f"radegs_delaunay_plan: {overflow} cells outgrew the 256 faces / 508 triangles of a cell (include/radegs.h)")
    if records == 0:
        info["inconsistent"] = 1
        return None, info
    cells, unique, inconsistent = _emit(p.shape[0], ws, nbytes, capacity, records)
    info["tets"], info["inconsistent"] = unique, inconsistent
    return (cells if inconsistent == 0 and 4 * unique == records else None), info


@torch.no_grad()
def triangulate(points, jitter=1e-9, seed=0, return_info=False):
    """The Delaunay tetrahedra of `points` (float32 or float64 [N,3] on the GPU, N >= 4): cells int32 [T,4] on the same device.  A row is
    the ascending index quadruple with the last two exchanged where needed to make it positively oriented (float64 det[b-a, c-a, d-a] > 0
    on perturbed(points, jitter, seed)); rows are unique and in lexicographic order of their ascending quadruple; two calls give the same
    bits.  With `return_info` also a dict: `tets`; `inconsistent`, the distinct tetrahedra not found by exactly four cells; `uncertain`, the
    predicate values within the forward error bound of their evaluation (an in-sphere value: of its second, about the nearest origin, too); `deferred`, the points the one-wave-per-point kernel finished;
    `overflow`, the cells too large even for that one; `retries`.  An inconsistent result is tried again with seed + 1 and ten times the
    jitter, at most twice, and then raises; with jitter = 0 nothing is tried again.  jitter = 0 is the caller's statement that the points
    are in general position: any uncertain predicate refutes it -- a tie was met and decided by the order of clipping, so whether the cells
    then happen to agree depends on the order of the points -- and raises as well.  With jitter > 0 the result is Delaunay only up to the
    jitter anyway, and a consistent tetrahedralisation is returned whatever `uncertain` says."""
    jitter, seed = _jitter(jitter), _seed(seed)
    if not isinstance(return_info, bool):
        raise RuntimeError("`return_info` must be a bool")
    p = _points(points)
    bounds, diag = _bounds(p)
    for retry in range(RETRIES + 1):
        cells, info = _attempt(p, bounds, jitter * diag, seed)
        info["retries"] = retry
        if jitter == 0.0 and info["uncertain"]:
            raise RuntimeError(f"triangulate: {info['uncertain']} predicate values are within their error bound ({info['inconsistent']} of "
                               f"{info['tets']} tetrahedra not found by exactly four cells): the points are degenerate and jitter=0 decides no tie")
        if cells is not None:
            return (cells, info) if return_info else cells
        if jitter == 0.0:
            break
        jitter, seed = jitter * 10.0, seed + 1
    raise RuntimeError(f"triangulate: {info['inconsistent']} of {info['tets']} tetrahedra were not found by exactly four cells "
                       f"({info['uncertain']} uncertain predicates, {info['retries']} retries): the points are degenerate at this jitter")
