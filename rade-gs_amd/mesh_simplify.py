"""HIP-backed mesh simplification: vertex clustering with quadric error (Lindstrom 2000), the step upstream's users take in
Open3D (simplify_vertex_clustering with SimplificationContraction.Quadric or .Average) or MeshLab once post_process_mesh has removed the
floaters.  GPU only.  `vertices` float32 or float64 [V,3], `faces` int32 or int64 [F,3] on the same device; all arithmetic is float64, every
sum runs in a fixed order, the result is rounded once to the dtype of `vertices`, and two calls return the same bits.  Open3D's rules are
written from memory (DESIGN 11 N21 marks each); include/radegs.h, "Mesh simplification", is the specification and
tests/simplify_restatement.py restates it in NumPy."""
import functools
import math

import torch

import geom_host as gh
import mesh_clean
from diff_gaussian_rasterization import _C
from geom_host import f64, i32, ll, sz, vp

CELL_BITS = 21                       # RADEGS_SIMPLIFY_CELL_BITS: a cell coordinate per axis, three of them in a 63-bit key
CONTRACTIONS = ("average", "quadric")

SIGNATURES = {
    "radegs_simplify_cells_bytes": (sz, [ll]),
    "radegs_simplify_cells": (i32, [ll, vp, f64, f64, f64, f64, ll, vp, sz, vp, vp, vp, vp, vp, vp]),
    "radegs_simplify_vertices_bytes": (sz, [ll]),
    "radegs_simplify_vertices": (i32, [ll, ll, ll, i32, vp, vp, vp, vp, vp, vp, vp, f64, f64, f64, f64, i32, vp, sz, vp, vp, vp, vp, vp]),
    "radegs_simplify_faces_bytes": (sz, [ll]),
    "radegs_simplify_faces": (i32, [ll, ll, ll, vp, vp, i32, vp, sz, vp, vp, vp]),
    "radegs_simplify_face_source": (i32, [ll, ll, vp, ll, vp, vp]),
}
_SIGNATURES = SIGNATURES


def _lib():
    return gh.bind(_SIGNATURES)


_call = functools.partial(gh.call, _SIGNATURES)


# ------------------------------------------------------------------------- arguments -------------------------------------------------------------------------
def _contraction(contraction):
    if contraction not in CONTRACTIONS:
        raise RuntimeError(f"`contraction` must be one of {CONTRACTIONS}")
    return CONTRACTIONS.index(contraction)


def _flag(value, name):
    if not isinstance(value, bool):
        raise RuntimeError(f"`{name}` must be a bool")
    return value


def _attributes(attributes, v):
    if attributes is None:
        return None
    if not isinstance(attributes, torch.Tensor) or attributes.dtype not in (torch.float32, torch.float64) or attributes.dim() != 2 or \
            attributes.shape[0] != v.shape[0]:
        raise RuntimeError("`attributes` must be a float32 or float64 tensor of shape (V,A)")
    if attributes.shape[1] > 2 ** 16:
        raise RuntimeError("`attributes` has more than 2^16 columns")
    _C._require_gpu(attributes, "attributes")
    if attributes.device != v.device:
        raise RuntimeError("`attributes` and `vertices` must be on the same device")
    a = attributes.detach().contiguous()
    gh.finite(a, "attributes")
    return a


def _origin(origin):
    if origin is None:
        return None
    if isinstance(origin, torch.Tensor):
        origin = origin.detach().cpu().tolist()
    if not isinstance(origin, (list, tuple)) or len(origin) != 3 or \
            not all(isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x) for x in origin):
        raise RuntimeError("`origin` must be three finite numbers")
    return tuple(float(x) for x in origin)


def _bounds(v):
    """(min [3], max [3]) of checked, non-empty vertices as Python floats (float64 holds a float32 exactly): one host read"""
    lo, hi = torch.aminmax(v.double(), dim=0)
    both = torch.stack([lo, hi]).tolist()
    return both[0], both[1]


def _grid(lo, hi, h, origin):
    """(origin, max_key) of the cell grid; refuses, on the bounds alone, a grid with a cell coordinate outside [0, 2^21).  x -> floor((x - o) / h)
    does not decrease with x (a difference and a quotient by h > 0, each rounded once), so the extreme vertices bound every cell."""
    if origin is None:
        origin = tuple(m - h / 2.0 for m in lo)        # Open3D's rule (from memory): the minimum bound less half a voxel
    if not all(math.isfinite(o) for o in origin):
        raise RuntimeError("the cell grid's origin is not finite")
    cmax = []
    for a in range(3):
        c0, c1 = math.floor((lo[a] - origin[a]) / h), math.floor((hi[a] - origin[a]) / h)
        if not (c0 >= 0 and c1 < 2 ** CELL_BITS):       # an infinite quotient fails here too
            raise RuntimeError(f"`voxel_size` {h} puts the vertices in cells {c0}..{c1} on axis {a}: outside [0, 2^{CELL_BITS}) "
                               "(include/radegs.h, Mesh simplification)")
        cmax.append(int(c1))
    return origin, cmax[0] << (2 * CELL_BITS) | cmax[1] << CELL_BITS | cmax[2]


def _empty(dev, *shape, dtype=torch.int64):
    return torch.empty(shape, dtype=dtype, device=dev)


# --------------------------------------------------------------------------- stages ---------------------------------------------------------------------------
class _Cells:
    """what radegs_simplify_cells leaves: vertex_cell int64 [V], order int32 [V], cell_start int32 [V+1], cell_key int64 [V], K"""


def _cells(v64, origin, h, max_key):
    """the cells of checked, non-empty vertices; the one host read is K"""
    dev, V = v64.device, v64.shape[0]
    nbytes = _lib().radegs_simplify_cells_bytes(V)
    ws = gh.workspace(nbytes, dev)
    c = _Cells()
    c.vertex_cell, c.order, c.cell_key = _empty(dev, V), _empty(dev, V, dtype=torch.int32), _empty(dev, V)
    c.cell_start = _empty(dev, V + 1, dtype=torch.int32)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    _call("radegs_simplify_cells", dev, V, v64, origin[0], origin[1], origin[2], h, max_key, ws, nbytes, c.vertex_cell, c.order, c.cell_start, c.cell_key, n)
    c.K = int(n)
    return c


def _cell_vertices(v64, f, a64, cells, origin, h, quadric):
    """(positions float64 [K,3], attributes float64 [K,A] or None, averages float64 [K,3], quadrics float64 [K,10] or None).  No host read."""
    dev, V, F, K = v64.device, v64.shape[0], f.shape[0], cells.K
    A = 0 if a64 is None else a64.shape[1]
    nbytes = _lib().radegs_simplify_vertices_bytes(F) if quadric and F else 0
    ws = gh.workspace(nbytes, dev)
    averages = _empty(dev, K, 3, dtype=torch.float64)
    attr = _empty(dev, K, A, dtype=torch.float64) if A else None
    quadrics = _empty(dev, K, 10, dtype=torch.float64) if quadric else None
    positions = _empty(dev, K, 3, dtype=torch.float64) if quadric else averages
    _call("radegs_simplify_vertices", dev, V, F, K, A, v64, f, a64, cells.vertex_cell, cells.order, cells.cell_start, cells.cell_key, origin[0], origin[1],
          origin[2], h, int(quadric), ws, nbytes, averages, attr, quadrics, positions if quadric else None)
    return positions, attr, averages, quadrics


def _cell_faces(f, V, cells, remove_duplicates):
    """(cell_faces int64 [F,3], remove uint8 [F]) of checked faces, F > 0.  No host read."""
    dev, F = f.device, f.shape[0]
    nbytes = _lib().radegs_simplify_faces_bytes(F) if remove_duplicates else 0
    ws = gh.workspace(nbytes, dev)
    cell_faces, remove = _empty(dev, F, 3), _empty(dev, F, dtype=torch.uint8)
    _call("radegs_simplify_faces", dev, V, F, cells.K, f, cells.vertex_cell, int(remove_duplicates), ws, nbytes, cell_faces, remove)
    return cell_faces, remove


def _compact_plan(K, cell_faces, remove, drop_unreferenced):
    """radegs_meshclean_compact_plan on the cells and the flagged faces: (workspace, cells kept, faces kept); the one host read is the two counts"""
    dev, F = cell_faces.device, cell_faces.shape[0]
    nbytes = mesh_clean._lib().radegs_meshclean_compact_bytes(K, F)
    ws = gh.workspace(nbytes, dev)
    counts2 = torch.zeros(2, dtype=torch.int64, device=dev)
    mesh_clean._call("radegs_meshclean_compact_plan", dev, K, F, 0, cell_faces, remove, None, None, 0, int(drop_unreferenced), ws, nbytes, counts2)
    nv, nf = counts2.tolist()
    return ws, nv, nf


def _compact_apply(K, cell_faces, ws, nv, nf):
    """(kept_cells int64 [nv], faces int64 [nf,3], face_source int64 [nf]) of a plan.  No host read."""
    dev, F = cell_faces.device, cell_faces.shape[0]
    kept, out_f, source = _empty(dev, nv), _empty(dev, nf, 3), _empty(dev, nf)
    mesh_clean._call("radegs_meshclean_compact_apply", dev, K, F, cell_faces, ws, nv, nf, kept, out_f)
    _call("radegs_simplify_face_source", dev, K, F, ws, nf, source)
    return kept, out_f, source


def _checked(vertices, faces, voxel_size, contraction, origin, attributes, remove_duplicates, drop_unreferenced):
    quadric = _contraction(contraction)
    h = gh.positive(voxel_size, "voxel_size")
    origin = _origin(origin)
    _flag(remove_duplicates, "remove_duplicates"), _flag(drop_unreferenced, "drop_unreferenced")
    v, f = mesh_clean._mesh(vertices, faces)
    return v, f, h, quadric, origin, _attributes(attributes, v)


def _count_only(v64, f, lo, hi, h, origin, remove_duplicates, drop_unreferenced):
    """(K, faces kept) at voxel size h, and what a mesh would be built from: no position is computed"""
    origin, max_key = _grid(lo, hi, h, origin)
    cells = _cells(v64, origin, h, max_key)
    cell_faces, remove = _cell_faces(f, v64.shape[0], cells, remove_duplicates)
    ws, nv, nf = _compact_plan(cells.K, cell_faces, remove, drop_unreferenced)
    return cells, origin, cell_faces, ws, nv, nf


def _build(v, v64, f, a, h, quadric, origin, cells, cell_faces, ws, nv, nf):
    dev, K = v.device, cells.K
    positions, attr, _, _ = _cell_vertices(v64, f, None if a is None else a.double(), cells, origin, h, quadric)
    kept, out_f, source = _compact_apply(K, cell_faces, ws, nv, nf)
    new_index = torch.full((K,), -1, dtype=torch.int64, device=dev)
    new_index[kept] = torch.arange(nv, dtype=torch.int64, device=dev)
    return positions[kept].to(v.dtype), out_f, new_index[cells.vertex_cell], source, None if a is None else attr[kept].to(a.dtype)


def _no_vertices(v, f, a):
    dev = v.device
    return v[:0], _empty(dev, 0, 3), torch.full((v.shape[0],), -1, dtype=torch.int64, device=dev), _empty(dev, 0), None if a is None else a[:0]


# ----------------------------------------------------------------------- the public calls -----------------------------------------------------------------------
@torch.no_grad()
def simplify_vertex_clustering(vertices, faces, voxel_size, contraction="quadric", origin=None, attributes=None, remove_duplicates=True,
                               drop_unreferenced=True):
    """Open3D's simplify_vertex_clustering.  The vertices that fall in one cell of a grid of step `voxel_size` become one vertex; `origin`
    defaults to the per-axis minimum less half a step (Open3D's rule, from memory).  contraction "average": the mean of the cell's vertices;
    "quadric": the point that minimises the summed squared distances, weighted by area, to the planes of the triangles with a corner in the
    cell, restricted to the well-conditioned directions (eigenvalues above 1e-3 of the largest, Lindstrom's cut), and the mean where that point
    is not finite or leaves the cell.  `attributes` [V,A] (colours, normals) are averaged per cell.  A face with two corners in one cell goes;
    with `remove_duplicates` so do the faces that repeat an earlier face's cells in the same orientation; with `drop_unreferenced` the cells no
    surviving face references.  Cells are numbered by ascending (x, y, z) cell coordinate, not in Open3D's hash-map order; output faces keep
    the order of their input faces and start at their smallest index.  A step that would need 2^21 or more cells along an axis is refused.
    Returns (vertices [K',3] in the input dtype, faces int64 [F',3], vertex_map int64 [V]: the output vertex of every input vertex, -1 where
    its cell was dropped, face_source int64 [F']: the input face of every output face, attributes [K',A] or None).  A mesh without vertices
    or without faces returns empty outputs (every vertex mapped to -1) and the library is not called.  Host reads: the bounds (a check), the
    number of cells and the two output sizes."""
    v, f, h, quadric, origin, a = _checked(vertices, faces, voxel_size, contraction, origin, attributes, remove_duplicates, drop_unreferenced)
    if v.shape[0] == 0 or f.shape[0] == 0:          # no face: nothing survives, and the library is not called
        return _no_vertices(v, f, a)
    v64 = v.double()
    lo, hi = _bounds(v64)
    cells, origin, cell_faces, ws, nv, nf = _count_only(v64, f, lo, hi, h, origin, remove_duplicates, drop_unreferenced)
    return _build(v, v64, f, a, h, quadric, origin, cells, cell_faces, ws, nv, nf)


@torch.no_grad()
def simplify_to_face_count(vertices, faces, target_faces, contraction="quadric", max_tries=16, **kw):
    """simplify_vertex_clustering at the finest voxel size found whose result has at most `target_faces` faces.  log(voxel_size) is bisected
    between the bounding-box diagonal and that diagonal / 2^20: the diagonal itself is tried first, then midpoints, `max_tries` sizes at the
    most, each a count-only plan (cells and faces are numbered and counted, no position is computed); the search ends early on an exact hit.
    The face count need not be monotone in the size -- a coarser grid can by chance keep more faces -- so the result is the finest size TRIED
    that qualifies, not the finest that exists.  Raises if no tried size qualifies.  Keywords as simplify_vertex_clustering's (not
    `voxel_size`).  Returns its tuple plus the voxel size used."""
    if isinstance(target_faces, bool) or not isinstance(target_faces, int) or target_faces < 1:
        raise RuntimeError("`target_faces` must be a positive integer")
    if isinstance(max_tries, bool) or not isinstance(max_tries, int) or max_tries < 1:
        raise RuntimeError("`max_tries` must be a positive integer")
    unknown = set(kw) - {"origin", "attributes", "remove_duplicates", "drop_unreferenced"}
    if unknown:
        raise RuntimeError(f"unknown arguments {sorted(unknown)}")
    remove_duplicates, drop_unreferenced = kw.get("remove_duplicates", True), kw.get("drop_unreferenced", True)
    v, f, _, quadric, origin, a = _checked(vertices, faces, 1.0, contraction, kw.get("origin"), kw.get("attributes"), remove_duplicates, drop_unreferenced)
    if v.shape[0] == 0 or f.shape[0] == 0:
        return simplify_vertex_clustering(v, f, 1.0, contraction, origin, a, remove_duplicates, drop_unreferenced) + (1.0,)
    v64 = v.double()
    lo, hi = _bounds(v64)
    diagonal = math.sqrt(sum((hi[k] - lo[k]) ** 2 for k in range(3)))
    if not (diagonal > 0.0 and math.isfinite(diagonal)):
        raise RuntimeError("the bounding box of `vertices` has no extent to bisect")
    coarse, fine = math.log(diagonal), math.log(diagonal) - 20.0 * math.log(2.0)
    best, h = None, diagonal
    for _ in range(max_tries):
        plan = _count_only(v64, f, lo, hi, h, origin, remove_duplicates, drop_unreferenced)
        if plan[-1] <= target_faces:
            best = (h, plan)                  # every size tried after the diagonal lies below the finest that qualified so far
            coarse = math.log(h)
            if plan[-1] == target_faces:
                break
        elif best is None:
            break                             # the diagonal itself leaves too many faces, and nothing coarser is tried
        else:
            fine = math.log(h)
        h = math.exp(0.5 * (coarse + fine))
    if best is None:
        raise RuntimeError(f"no voxel size tried leaves at most {target_faces} faces")
    h, (cells, origin_used, cell_faces, ws, nv, nf) = best
    return _build(v, v64, f, a, h, quadric, origin_used, cells, cell_faces, ws, nv, nf) + (h,)
