"""HIP-backed mesh clean-up: the steps of the reference that treat the mesh as a graph and that upstream hands to Open3D and
trimesh -- utils/mesh_utils.py:23-44 post_process_mesh (cluster_connected_triangles, remove_triangles_by_mask, remove_unreferenced_vertices,
remove_degenerate_triangles), eval_tnt/cull_mesh.py:186-202 Mesher.get_connected_mesh (mesh.split, areas) and mesh_extract.py:104
compute_vertex_normals.  GPU only.  `faces` is an int [F,3] GPU tensor, `vertices` float32 or float64 [V,3] on the same device; all arithmetic
is float64, every sum runs in a fixed order, and two calls return the same bits.  The rules of Open3D and trimesh are written from memory
(DESIGN 11 N12 marks each); include/radegs.h, "Mesh clean-up", is the specification and tests/meshclean_restatement.py restates it in NumPy."""
import functools

import torch

import geom_host as gh
from diff_gaussian_rasterization import _C
from geom_host import i32, ll, sz, vp

MAX_VERTICES, MAX_FACES = 2 ** 31 - 1, 2 ** 30     # 3 F edge records and their indices stay in the u32 words of the sort
ADJACENCY = ("edge", "manifold_edge")

SIGNATURES = {
    "radegs_meshclean_cluster_bytes": (sz, [ll]),
    "radegs_meshclean_cluster": (i32, [ll, ll, vp, i32, vp, sz, vp, vp, vp]),
    "radegs_meshclean_stats_bytes": (sz, [ll, ll]),
    "radegs_meshclean_stats": (i32, [ll, ll, ll, vp, vp, vp, vp, sz, vp, vp, vp, vp]),
    "radegs_meshclean_compact_bytes": (sz, [ll, ll]),
    "radegs_meshclean_compact_plan": (i32, [ll, ll, ll, vp, vp, vp, vp, i32, i32, vp, sz, vp, vp]),
    "radegs_meshclean_compact_apply": (i32, [ll, ll, vp, vp, ll, ll, vp, vp, vp]),
    "radegs_meshclean_normals_bytes": (sz, [ll]),
    "radegs_meshclean_vertex_normals": (i32, [ll, ll, vp, vp, i32, vp, sz, vp, vp]),
}
_SIGNATURES = SIGNATURES


def _lib():
    return gh.bind(_SIGNATURES)


_call = functools.partial(gh.call, _SIGNATURES)


# ------------------------------------------------------------------------- arguments -------------------------------------------------------------------------
def _faces(faces, V):
    """int64 [F,3], contiguous, every index inside [0, V): refused otherwise, before any kernel reads them"""
    gh.faces_type(faces)
    if faces.shape[0] > MAX_FACES or V > MAX_VERTICES:
        raise RuntimeError(f"the mesh has more than 2^30 faces or 2^31 - 1 vertices ({faces.shape[0]}, {V}): beyond the 32-bit sort (include/radegs.h)")
    return gh.faces(faces, V)


def _faces_alone(faces):
    """(checked faces, V) where no vertices are given: V is one past the largest index"""
    gh.faces_type(faces)
    if faces.shape[0] > MAX_FACES:
        raise RuntimeError(f"the mesh has more than 2^30 faces ({faces.shape[0]}): beyond the 32-bit sort (include/radegs.h)")
    _C._require_gpu(faces, "faces")
    V = max(int(faces.max()) + 1, 0) if faces.numel() else 0
    return _faces(faces, V), V


def _mesh(vertices, faces):
    if not isinstance(vertices, torch.Tensor) or vertices.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("`vertices` must be a float32 or float64 tensor")
    gh.faces_type(faces)
    v = gh.points(vertices, "vertices", vertices.dtype)
    f = _faces(faces, v.shape[0])
    if f.device != v.device:
        raise RuntimeError("`vertices` and `faces` must be on the same device")
    gh.finite(v, "vertices")
    return v, f


def _count(value, name):
    if isinstance(value, bool) or not isinstance(value, int) or value < 1:
        raise RuntimeError(f"`{name}` must be a positive integer")
    return value


def _adjacency(adjacency):
    if adjacency not in ADJACENCY:
        raise RuntimeError(f"`adjacency` must be one of {ADJACENCY}")
    return ADJACENCY.index(adjacency)


def _empty(dev, *shape, dtype=torch.int64):
    return torch.empty(shape, dtype=dtype, device=dev)


# -------------------------------------------------------------------------- clusters --------------------------------------------------------------------------
def _cluster(f, V, manifold):
    """(labels int64 [F], C) of checked faces, F > 0; the one host read is C"""
    dev, F = f.device, f.shape[0]
    nbytes = _lib().radegs_meshclean_cluster_bytes(F)
    ws = gh.workspace(nbytes, dev)
    labels, n = _empty(dev, F), torch.zeros(1, dtype=torch.int64, device=dev)
    _call("radegs_meshclean_cluster", dev, V, F, f, manifold, ws, nbytes, labels, n)
    return labels, int(n)


def _stats(v64, f, labels, C, areas, total=False):
    """(counts int64 [C], areas float64 [C] or None, total float64 [1] or None); v64 may be None without areas"""
    dev, F = f.device, f.shape[0]
    nbytes = _lib().radegs_meshclean_stats_bytes(F, C)
    ws = gh.workspace(nbytes, dev)
    counts = _empty(dev, C)
    area = _empty(dev, C, dtype=torch.float64) if areas else None
    tot = _empty(dev, 1, dtype=torch.float64) if total else None
    _call("radegs_meshclean_stats", dev, 0 if v64 is None else v64.shape[0], F, C, v64, f, labels, ws, nbytes, counts, area, tot)
    return counts, area, tot


@torch.no_grad()
def cluster_connected_triangles(faces, vertices=None, adjacency="edge"):
    """Open3D's TriangleMesh.cluster_connected_triangles.  Two triangles are adjacent when they share an undirected edge {a, b}, a != b, by
    vertex index; sharing only a vertex joins nothing.  adjacency "edge": all triangles on an edge are joined (Open3D's rule); "manifold_edge":
    only an edge that exactly two edge records have joins them (trimesh's face_adjacency, which mesh.split walks).  Clusters are numbered by
    ascending smallest triangle index.  Returns (triangle_clusters int64 [F], cluster_n_triangles int64 [C], cluster_area float64 [C], the sum
    of 0.5 |(b - a) x (c - a)|, or None without `vertices`).  One host read: C."""
    manifold = _adjacency(adjacency)
    if vertices is None:
        v, (f, V) = None, _faces_alone(faces)
    else:
        v, f = _mesh(vertices, faces)
        V = v.shape[0]
    dev = f.device
    if f.shape[0] == 0:
        return _empty(dev, 0), _empty(dev, 0), None if v is None else _empty(dev, 0, dtype=torch.float64)
    labels, C = _cluster(f, V, manifold)
    counts, area, _ = _stats(None if v is None else v.double(), f, labels, C, v is not None)
    return labels, counts, area


# ------------------------------------------------------------------------- compaction -------------------------------------------------------------------------
def _compact(V, f, remove=None, labels=None, cluster_keep=None, drop_degenerate=False, drop_unreferenced=True):
    """(kept_vertices int64 [V'], faces int64 [F',3]) of checked faces; the one host read is the two counts"""
    dev, F = f.device, f.shape[0]
    if V + F == 0:
        return _empty(dev, 0), _empty(dev, 0, 3)
    nbytes = _lib().radegs_meshclean_compact_bytes(V, F)
    ws = gh.workspace(nbytes, dev)
    counts2 = torch.zeros(2, dtype=torch.int64, device=dev)
    C = 0 if cluster_keep is None else cluster_keep.shape[0]
    _call("radegs_meshclean_compact_plan", dev, V, F, C, f, remove, labels, cluster_keep, int(drop_degenerate), int(drop_unreferenced), ws, nbytes, counts2)
    nv, nf = counts2.tolist()              # the host read that sizes the outputs
    kept, out_f = _empty(dev, nv), _empty(dev, nf, 3)
    _call("radegs_meshclean_compact_apply", dev, V, F, f, ws, nv, nf, kept, out_f)
    return kept, out_f


@torch.no_grad()
def remove_triangles_by_mask(vertices, faces, remove):
    """The triangles with `remove` (bool [F], on the faces' device) set go; so do the vertices no surviving triangle references (Open3D's
    remove_triangles_by_mask followed by its remove_unreferenced_vertices).  Survivors keep their relative order and are renumbered.  Returns
    (vertices, faces int64, kept_vertices int64 [V']: the old index of every new vertex).  One host read."""
    v, f = _mesh(vertices, faces)
    if not isinstance(remove, torch.Tensor) or remove.dtype != torch.bool or remove.dim() != 1 or remove.shape[0] != f.shape[0]:
        raise RuntimeError("`remove` must be a bool tensor of shape (F,)")
    if remove.device != f.device:
        raise RuntimeError("`remove` and `faces` must be on the same device")
    kept, out_f = _compact(v.shape[0], f, remove=remove.detach().contiguous().to(torch.uint8))
    return v[kept], out_f, kept


@torch.no_grad()
def remove_unreferenced_vertices(vertices, faces):
    """Open3D's remove_unreferenced_vertices: (vertices, faces int64, kept_vertices int64 [V']).  One host read."""
    v, f = _mesh(vertices, faces)
    kept, out_f = _compact(v.shape[0], f)
    return v[kept], out_f, kept


@torch.no_grad()
def remove_degenerate_triangles(faces):
    """Open3D's remove_degenerate_triangles: a triangle with two equal vertex indices goes (by index, not by area).  Returns faces int64
    [F',3] in their original order; no vertex is touched.  One host read."""
    f, V = _faces_alone(faces)
    return _compact(V, f, drop_degenerate=True, drop_unreferenced=False)[1]


# ---------------------------------------------------------------------- the two whole steps ----------------------------------------------------------------------
@torch.no_grad()
def post_process_mesh(vertices, faces, cluster_to_keep=1000, min_triangles=50):
    """utils/mesh_utils.py:23-44, post_process_mesh, in its order: cluster the triangles ("edge"), n = max(sorted(counts)[-cluster_to_keep],
    min_triangles), the triangles of the clusters with count < n go (ties at the cut stay), then the unreferenced vertices, then the degenerate
    triangles -- a vertex that only a degenerate triangle references therefore stays.  One deliberate difference: with fewer clusters than
    `cluster_to_keep` the reference raises IndexError; here the cut is then the smallest count.  The selection stays on the device.  Returns
    (vertices, faces int64, kept_vertices int64 [V']).  Two host reads: the number of clusters and the two output sizes."""
    cluster_to_keep = _count(cluster_to_keep, "cluster_to_keep")
    if isinstance(min_triangles, bool) or not isinstance(min_triangles, int) or min_triangles < 0:
        raise RuntimeError("`min_triangles` must be a non-negative integer")
    v, f = _mesh(vertices, faces)
    if f.shape[0] == 0:
        return v[:0], f, _empty(f.device, 0)
    labels, C = _cluster(f, v.shape[0], 0)
    counts, _, _ = _stats(None, f, labels, C, False)
    cut = torch.sort(counts).values[C - min(cluster_to_keep, C)].clamp(min=min_triangles)      # C values, on the device
    kept, out_f = _compact(v.shape[0], f, labels=labels, cluster_keep=(counts >= cut).to(torch.uint8), drop_degenerate=True)
    return v[kept], out_f, kept


@torch.no_grad()
def get_connected_mesh(vertices, faces, get_largest_components=False, remove_small_geometry_threshold=0.2):
    """eval_tnt/cull_mesh.py:186-202, Mesher.get_connected_mesh: the "manifold_edge" clusters (trimesh's split(only_watertight=False)); with
    `get_largest_components` the cluster of greatest area (the lowest number on a tie), otherwise the clusters whose area exceeds
    `remove_small_geometry_threshold` x the total area.  Survivors keep their original order and unreferenced vertices go; trimesh re-orders
    by component, so the result is the same mesh, not the same arrays.  Returns (vertices, faces int64, kept_vertices int64 [V']).  Two host
    reads: the number of clusters and the two output sizes."""
    if not isinstance(get_largest_components, bool):
        raise RuntimeError("`get_largest_components` must be a bool")
    thr = remove_small_geometry_threshold
    if isinstance(thr, bool) or not isinstance(thr, (int, float)) or not thr == thr or abs(thr) == float("inf"):
        raise RuntimeError("`remove_small_geometry_threshold` must be a finite number")
    v, f = _mesh(vertices, faces)
    if f.shape[0] == 0:
        return v[:0], f, _empty(f.device, 0)
    labels, C = _cluster(f, v.shape[0], 1)
    _, area, total = _stats(v.double(), f, labels, C, True, total=True)
    if get_largest_components:
        keep = torch.zeros(C, dtype=torch.uint8, device=f.device)
        keep[torch.argmax(area)] = 1                                  # the first of equal maxima
    else:
        keep = (area > float(thr) * total).to(torch.uint8)
    kept, out_f = _compact(v.shape[0], f, labels=labels, cluster_keep=keep)
    return v[kept], out_f, kept


# ------------------------------------------------------------------------ vertex normals ------------------------------------------------------------------------
@torch.no_grad()
def compute_vertex_normals(vertices, faces, normalized=True):
    """Open3D's compute_vertex_normals (mesh_extract.py:104): per vertex the sum of the unnormalised triangle normals (b - a) x (c - a) of its
    corners (area weighting), in ascending (triangle, corner) order -- np.add.at's order, no float atomics -- then normalised; a zero or
    non-finite length gives (0, 0, 1).  float64 arithmetic, rounded once to the dtype of `vertices`.  Returns [V,3].  No host read."""
    if not isinstance(normalized, bool):
        raise RuntimeError("`normalized` must be a bool")
    v, f = _mesh(vertices, faces)
    dev, V, F = v.device, v.shape[0], f.shape[0]
    out = torch.empty((V, 3), dtype=torch.float64, device=dev)
    if V:
        nbytes = _lib().radegs_meshclean_normals_bytes(F)
        ws = gh.workspace(nbytes, dev)
        _call("radegs_meshclean_vertex_normals", dev, V, F, v.double(), f, int(normalized), ws, nbytes, out)
    return out.to(v.dtype)
