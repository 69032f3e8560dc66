"""The seeded meshes of the mesh clean-up tests, each the smallest input at which one step can go wrong.  All are well-shaped: vertices sit
on a unit grid with a jitter below a quarter of the step, so that no triangle area is a cancellation residue.  CASES maps a name to
(vertices float64 [V,3], faces int64 [F,3]); the restatement's results are computed once per case and shared (reference())."""
import functools

import numpy as np

import meshclean_restatement as mr

JITTER = 0.2          # of a grid step of 1: below a quarter
PIECES = (1, 63, 64, 65, 255, 256, 257)


def _jitter(rng, v):
    return v + rng.uniform(-JITTER, JITTER, v.shape)


def strip(n, rng, origin=(0.0, 0.0, 0.0)):
    """a strip of n triangles over n + 2 vertices in two rows: triangle i is (i, i + 1, i + 2), adjacent to i - 1 and i + 1"""
    i = np.arange(n + 2)
    v = np.stack([(i // 2).astype(np.float64), (i % 2).astype(np.float64), np.zeros(n + 2)], 1)
    t = np.arange(n)
    return _jitter(rng, v) + np.asarray(origin), np.stack([t, t + 1, t + 2], 1).astype(np.int64)


def sheet(nx, ny, rng, origin=(0.0, 0.0, 0.0)):
    """an nx x ny grid of quads, two triangles each, counter-clockwise seen from +z"""
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    v = np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros(gx.size)], 1).astype(np.float64)
    q = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([q, q + 1, q + nx + 2], 1), np.stack([q, q + nx + 2, q + nx + 1], 1)])
    return _jitter(rng, v) + np.asarray(origin), f.astype(np.int64)


def tetrahedron(rng, origin):
    """a closed surface of 4 triangles, oriented outwards"""
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)
    return _jitter(rng, v) + np.asarray(origin), f


def join(*parts):
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + base)
        base += v.shape[0]
    return np.concatenate(vs), np.concatenate(fs)


def _points(rng, n):
    """n well separated points for the hand-written small cases"""
    i = np.arange(n)
    return _jitter(rng, np.stack([(i % 3) * 1.0, (i // 3) * 1.0, (i % 2) * 1.0], 1))


def _build():
    rng = np.random.default_rng(12)
    I = lambda rows: np.array(rows, np.int64).reshape(-1, 3)
    c = {}
    c["single"] = (_points(rng, 3), I([[0, 1, 2]]))
    c["shared_edge"] = (_points(rng, 4), I([[0, 1, 2], [2, 1, 3]]))
    c["bow_tie"] = (_points(rng, 5), I([[0, 1, 2], [2, 3, 4]]))                                 # one shared vertex: two clusters
    c["three_on_an_edge"] = (_points(rng, 5), I([[0, 1, 2], [1, 0, 3], [0, 1, 4]]))             # "edge": 1 cluster, "manifold_edge": 3
    c["duplicate"] = (_points(rng, 4), I([[0, 1, 2], [0, 1, 2], [1, 0, 3]]))
    c["degenerate_alone"] = (_points(rng, 5), I([[0, 0, 1], [2, 3, 4]]))
    sv, sf = sheet(4, 4, rng)
    c["degenerate_on_sheet"] = (sv, np.concatenate([sf, I([[0, 0, 1], [1, 6, 1]])]))             # (a, a, b) on a boundary edge of the sheet
    v, f = sheet(3, 3, rng)
    c["unused_vertex"] = (np.concatenate([v[:5], _points(rng, 1) + 20.0, v[5:]]), np.where(f >= 5, f + 1, f))
    v, f = strip(4097, rng)                                                                     # long parent chains; crosses 64 and 256
    c["strip"] = (v, f)
    c["strip_reversed"] = (v, f[::-1].copy())
    c["strip_shuffled"] = (v, f[np.random.default_rng(5).permutation(f.shape[0])])
    pieces = join(*[strip(n, rng, (0.0, 3.0 * k, 0.0)) for k, n in enumerate(PIECES)])          # the area sum's group boundaries
    c["strip_pieces"] = pieces
    c["strip_pieces_shuffled"] = (pieces[0], pieces[1][np.random.default_rng(6).permutation(pieces[1].shape[0])])
    c["sheet_64"] = sheet(64, 64, rng)                                                          # 8192 triangles
    c["floaters_49_50_51"] = join(sheet(8, 8, rng), strip(49, rng, (0, 20, 0)), strip(50, rng, (0, 30, 0)), strip(51, rng, (0, 40, 0)))
    c["tie_at_the_cut"] = join(sheet(8, 8, rng), strip(60, rng, (0, 20, 0)), strip(30, rng, (0, 30, 0)), strip(60, rng, (0, 40, 0)))
    c["tetrahedra_1000"] = join(*[tetrahedron(rng, (3.0 * (k % 32), 3.0 * (k // 32), 0.0)) for k in range(1000)])
    v, f = join(sheet(187, 187, rng), strip(49, rng, (0, 200, 0)), strip(120, rng, (0, 210, 0)))  # 70 107 triangles, 210 k edge records: many blocks of the sort and the scan
    c["large_shuffled"] = (v, f[np.random.default_rng(7).permutation(f.shape[0])])
    return c


CASES = _build()
NAMES = tuple(CASES)
# (a case, the case whose faces it permutes): the partitions must agree as sets of triangles
PERMUTED = (("strip_reversed", "strip"), ("strip_shuffled", "strip"), ("strip_pieces_shuffled", "strip_pieces"))


def cluster_to_keep_values(C):
    """1, C - 1, C, C + 1 and 1000, without repeats and without values below 1"""
    return tuple(sorted({k for k in (1, C - 1, C, C + 1, 1000) if k >= 1}))


@functools.lru_cache(maxsize=None)
def reference(name, adjacency="edge"):
    """the restatement's (labels, counts, areas) of a case: computed once, shared, not to be written to"""
    v, f = CASES[name]
    out = mr.cluster_connected_triangles(f, v, adjacency)
    for a in out:
        a.setflags(write=False)
    return out
