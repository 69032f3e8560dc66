"""Plain NumPy float64 restatement of the mesh clean-up unit (rade-gs_amd/mesh_clean.py, csrc/radegs_meshclean.hip; include/radegs.h, "Mesh
clean-up", is the specification).  Written from the rules, not from the kernels: the connected components are an own union-find over the edge
records; the two summation orders the kernels fix are restated addition by addition -- a cluster's area (its triangles in ascending index,
consecutive groups of 256 through the 256-wide halving tree, the group sums added to 0.0 in ascending order) and a vertex normal (np.add.at
over the corners in ascending (triangle, corner) order)."""
import numpy as np

from mesheval_restatement import fixed_order_sum

ADJACENCY = ("edge", "manifold_edge")
GROUP = 256


# --------------------------------------------------------------------------- clusters ---------------------------------------------------------------------------
def edge_records(faces):
    """[3 F, 2]: record 3 f + k is the undirected edge from corner k to corner k + 1 as (smaller, larger) vertex index"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
    return np.stack([np.minimum(a, b), np.maximum(a, b)], 1)


def _find(parent, x):
    root = x
    while parent[root] != root:
        root = parent[root]
    while parent[x] != root:
        parent[x], x = root, parent[x]
    return root


def triangle_clusters(faces, adjacency="edge"):
    """(labels int64 [F], counts int64 [C]).  Records with equal ends join nothing.  "edge": the triangles of all records with one key are
    joined; "manifold_edge": only where exactly two records have the key.  Clusters are numbered by ascending smallest triangle index."""
    assert adjacency in ADJACENCY
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = f.shape[0]
    if F == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    rec = edge_records(f)
    order = np.lexsort((rec[:, 1], rec[:, 0]))                  # stable: by the smaller index, then the larger
    key = rec[order]
    new_run = np.ones(3 * F, bool)
    new_run[1:] = (key[1:] != key[:-1]).any(1)
    starts = np.flatnonzero(new_run)
    ends = np.append(starts[1:], 3 * F)
    parent = list(range(F))
    for s, e in zip(starts.tolist(), ends.tolist()):
        if e - s < 2 or key[s, 0] == key[s, 1] or (adjacency == "manifold_edge" and e - s != 2):
            continue
        tris = (order[s:e] // 3).tolist()
        for t in tris[1:]:
            a, b = _find(parent, tris[0]), _find(parent, t)
            if a != b:
                parent[max(a, b)] = min(a, b)                    # the root of a set is its smallest triangle
    root = np.array([_find(parent, t) for t in range(F)], np.int64)
    assert (root <= np.arange(F)).all()
    roots, labels = np.unique(root, return_inverse=True)         # ascending root = ascending smallest triangle index
    return labels.astype(np.int64), np.bincount(labels, minlength=roots.shape[0]).astype(np.int64)


# ---------------------------------------------------------------------------- areas ----------------------------------------------------------------------------
def triangle_normals(vertices, faces):
    """(b - a) x (c - a) per triangle, one rounding per operation: (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx)"""
    v, f = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    a = v[f[:, 0]]
    u, w = v[f[:, 1]] - a, v[f[:, 2]] - a
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def triangle_areas(vertices, faces):
    n = triangle_normals(vertices, faces)
    return 0.5 * np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])


def _halving_tree(a):
    """[g, 256] -> [g]: level w adds element t + w onto element t for t < w, w = 128 .. 1"""
    a = a.copy()
    w = GROUP // 2
    while w > 0:
        a[:, :w] += a[:, w:2 * w]
        w >>= 1
    return a[:, 0]


def ordered_sum(terms):
    """the order of a cluster's area: a function of the number of terms alone"""
    terms = np.asarray(terms, np.float64)
    groups = -(-terms.shape[0] // GROUP)
    padded = np.zeros(groups * GROUP)
    padded[:terms.shape[0]] = terms
    s = np.float64(0.0)
    for g in _halving_tree(padded.reshape(groups, GROUP)):
        s = s + g
    return s


def cluster_areas(vertices, faces, labels, C):
    area = triangle_areas(vertices, faces)
    return np.array([ordered_sum(area[labels == c]) for c in range(C)], np.float64)      # a mask keeps ascending triangle index


def total_area(vertices, faces):
    area = triangle_areas(vertices, faces)
    return np.float64(fixed_order_sum(area[:, None], 1)[0]) if area.shape[0] else np.float64(0.0)


def cluster_connected_triangles(faces, vertices=None, adjacency="edge"):
    labels, counts = triangle_clusters(faces, adjacency)
    return labels, counts, None if vertices is None else cluster_areas(vertices, faces, labels, counts.shape[0])


# -------------------------------------------------------------------------- compaction --------------------------------------------------------------------------
def _compact(vertices, faces, keep_face, drop_unreferenced=True):
    v, f = np.asarray(vertices), np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[keep_face]
    used = np.zeros(v.shape[0], bool)
    if drop_unreferenced:
        used[f.reshape(-1)] = True
    else:
        used[:] = True
    kept = np.flatnonzero(used).astype(np.int64)
    new_index = np.cumsum(used) - 1
    return v[kept], new_index[f].astype(np.int64).reshape(-1, 3), kept


def remove_triangles_by_mask(vertices, faces, remove):
    return _compact(vertices, faces, ~np.asarray(remove, bool))


def remove_unreferenced_vertices(vertices, faces):
    return _compact(vertices, faces, np.ones(np.asarray(faces).reshape(-1, 3).shape[0], bool))


def degenerate(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])


def remove_degenerate_triangles(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return f[~degenerate(f)]


def cut_count(counts, cluster_to_keep, min_triangles):
    """max(sorted(counts)[-cluster_to_keep], min_triangles); with fewer clusters than cluster_to_keep, where the reference's index raises, the
    smallest count stands in: the documented clamp"""
    ordered = sorted(int(c) for c in counts)
    return max(ordered[-min(cluster_to_keep, len(ordered))], min_triangles)


def post_process_mesh(vertices, faces, cluster_to_keep=1000, min_triangles=50, clusters=None):
    """mesh_utils.py:31-41 in its order: by mask, then unreferenced vertices, then degenerate triangles (whose vertices therefore stay).
    `clusters`: the (labels, counts, ...) of "edge" where the caller has them already."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return np.asarray(vertices)[:0], f, np.zeros(0, np.int64)
    labels, counts = triangle_clusters(f, "edge") if clusters is None else clusters[:2]
    remove = counts[labels] < cut_count(counts, cluster_to_keep, min_triangles)
    v1, f1, kept = remove_triangles_by_mask(vertices, f, remove)
    return v1, remove_degenerate_triangles(f1), kept


def get_connected_mesh(vertices, faces, get_largest_components=False, remove_small_geometry_threshold=0.2, clusters=None):
    """`clusters`: the (labels, counts, areas) of "manifold_edge" where the caller has them already"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return np.asarray(vertices)[:0], f, np.zeros(0, np.int64)
    labels, counts, area = cluster_connected_triangles(f, vertices, "manifold_edge") if clusters is None else clusters
    if get_largest_components:
        keep = np.zeros(counts.shape[0], bool)
        keep[int(np.argmax(area))] = True                          # the first of equal maxima
    else:
        keep = area > np.float64(remove_small_geometry_threshold) * total_area(vertices, f)
    return _compact(vertices, f, keep[labels])


# ------------------------------------------------------------------------ vertex normals ------------------------------------------------------------------------
def compute_vertex_normals(vertices, faces, normalized=True):
    v, f = np.asarray(vertices), np.asarray(faces, np.int64).reshape(-1, 3)
    acc = np.zeros((v.shape[0], 3))
    np.add.at(acc, f.reshape(-1), np.repeat(triangle_normals(v, f), 3, axis=0))           # ascending (triangle, corner)
    if normalized:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            length = np.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
            ok = (length > 0.0) & np.isfinite(length)
            acc = np.where(ok[:, None], acc / length[:, None], np.array([0.0, 0.0, 1.0]))
    return acc.astype(v.dtype)
