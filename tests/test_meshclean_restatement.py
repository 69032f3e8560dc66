"""CPU tier of the mesh clean-up: the NumPy restatement the GPU tests compare with is itself checked -- its clusters against
scipy.sparse.csgraph.connected_components over an adjacency built another way, its numbering rule, its fixed-order areas against math.fsum, its
normals on a closed surface, and the documented clamp where the reference raises IndexError."""
import math
from collections import defaultdict

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import mesh_clean
import meshclean_cases as mc
import meshclean_restatement as mr


def _first_occurrence(labels):
    """labels renumbered in the order of their first occurrence: equal arrays iff equal partitions"""
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse]


def _scipy_labels(faces, adjacency):
    """connected components over an adjacency gathered in a dict of undirected edges, triangle by triangle: no sort, no union-find"""
    on_edge = defaultdict(list)
    for t, (a, b, c) in enumerate(faces.tolist()):
        for p, q in ((a, b), (b, c), (c, a)):
            if p != q:
                on_edge[(min(p, q), max(p, q))].append(t)
    rows, cols = [], []
    for tris in on_edge.values():
        if len(tris) < 2 or (adjacency == "manifold_edge" and len(tris) != 2):
            continue
        rows += tris[:-1]
        cols += tris[1:]
    F = faces.shape[0]
    graph = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(F, F)).tocsr()
    return connected_components(graph, directed=False)[1]


@pytest.mark.parametrize("adjacency", mr.ADJACENCY)
@pytest.mark.parametrize("name", mc.NAMES)
def test_clusters_equal_scipy_components_and_follow_the_numbering_rule(name, adjacency):
    _, f = mc.CASES[name]
    labels, counts, _ = mc.reference(name, adjacency)
    assert np.array_equal(_first_occurrence(_scipy_labels(f, adjacency)), labels)
    # numbered by ascending smallest triangle index: the first triangle of cluster c comes after that of c - 1, and triangle 0 is in cluster 0
    first = np.array([np.flatnonzero(labels == c)[0] for c in range(counts.shape[0])])
    assert labels[0] == 0 and (np.diff(first) > 0).all()
    assert np.array_equal(counts, np.bincount(labels)) and counts.sum() == f.shape[0]


def test_the_small_cases_have_the_clusters_the_rules_give():
    assert mr.ADJACENCY == mesh_clean.ADJACENCY
    n = lambda name, adj: mc.reference(name, adj)[1].tolist()
    assert n("single", "edge") == [1] and n("shared_edge", "edge") == [2] and n("shared_edge", "manifold_edge") == [2]
    assert n("bow_tie", "edge") == [1, 1]                                                     # a shared vertex joins nothing
    assert n("three_on_an_edge", "edge") == [3] and n("three_on_an_edge", "manifold_edge") == [1, 1, 1]
    assert n("duplicate", "edge") == [3] and n("duplicate", "manifold_edge") == [2, 1]         # the twins share two two-record edges
    assert n("degenerate_alone", "edge") == [1, 1]
    assert n("degenerate_on_sheet", "edge") == [34] and n("degenerate_on_sheet", "manifold_edge") == [32, 1, 1]
    assert n("strip", "edge") == [4097] and sorted(n("strip_pieces", "edge")) == sorted(mc.PIECES)
    assert n("tetrahedra_1000", "manifold_edge") == [4] * 1000
    assert sorted(n("floaters_49_50_51", "edge")) == [49, 50, 51, 128] and sorted(n("tie_at_the_cut", "edge")) == [30, 60, 60, 128]
    assert mc.CASES["large_shuffled"][1].shape[0] > 70000 and sorted(n("large_shuffled", "edge")) == [49, 120, 2 * 187 * 187]


@pytest.mark.parametrize("permuted, base", mc.PERMUTED)
def test_a_permutation_of_the_faces_keeps_the_partition(permuted, base):
    (_, fp), (_, fb) = mc.CASES[permuted], mc.CASES[base]
    key = lambda f: {tuple(r): i for i, r in enumerate(f.tolist())}
    at = key(fb)
    to_base = np.array([at[tuple(r)] for r in fp.tolist()])
    lp, lb = mc.reference(permuted)[0], mc.reference(base)[0]
    assert np.array_equal(_first_occurrence(lb[to_base]), lp)


@pytest.mark.parametrize("adjacency", mr.ADJACENCY)
@pytest.mark.parametrize("name", mc.NAMES)
def test_cluster_areas_are_within_the_bound_of_the_exact_sum(name, adjacency):
    v, f = mc.CASES[name]
    labels, counts, area = mc.reference(name, adjacency)
    terms = mr.triangle_areas(v, f)
    for c in range(counts.shape[0]):
        exact = math.fsum(terms[labels == c].tolist())
        assert abs(float(area[c]) - exact) <= (int(counts[c]) + 16) * 2.0 ** -53 * exact, (c, float(area[c]), exact)
    exact = math.fsum(terms.tolist())
    assert abs(float(mr.total_area(v, f)) - exact) <= (f.shape[0] + 16) * 2.0 ** -53 * exact


def test_the_area_order_depends_on_the_count_alone_and_pads_with_zero():
    rng = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 600):
        t = rng.uniform(0.5, 1.5, n)
        groups = [t[i:i + 256] for i in range(0, n, 256)]
        by_hand = np.float64(0.0)
        for g in groups:
            a = np.zeros(256)
            a[:g.shape[0]] = g
            for w in (128, 64, 32, 16, 8, 4, 2, 1):
                a[:w] = a[:w] + a[w:2 * w]
            by_hand = by_hand + a[0]
        assert mr.ordered_sum(t) == by_hand


def test_normals_of_a_closed_outward_tetrahedron_point_outward():
    v, f = mc.tetrahedron(np.random.default_rng(1), (0.0, 0.0, 0.0))
    n = mr.compute_vertex_normals(v, f)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-15)
    assert ((n * (v - v.mean(0))).sum(1) > 0).all()
    raw = mr.compute_vertex_normals(v, f, normalized=False)
    assert np.array_equal(raw / np.linalg.norm(raw, axis=1)[:, None] > 0, n > 0)
    lonely = mr.compute_vertex_normals(np.concatenate([v, [[9.0, 9.0, 9.0]]]), f)
    assert lonely[-1].tolist() == [0.0, 0.0, 1.0]                                              # no triangle: zero length
    assert mr.compute_vertex_normals(v.astype(np.float32), f).dtype == np.float32


def test_the_reference_index_error_is_the_documented_clamp():
    counts = [128, 49, 50, 51]
    with pytest.raises(IndexError):
        sorted(counts)[-5]                                                                     # what mesh_utils.py:34 does with 4 clusters
    assert mr.cut_count(counts, 5, 0) == 49 and mr.cut_count(counts, 1000, 50) == 50           # the smallest count stands in
    assert mr.cut_count(counts, 4, 0) == 49 and mr.cut_count(counts, 1, 50) == 128 and mr.cut_count(counts, 2, 50) == 51
    v, f = mc.CASES["floaters_49_50_51"]
    _, f1, kept = mr.post_process_mesh(v, f)                                                   # defaults: 1000 > 4 clusters, floor 50
    assert f1.shape[0] == 128 + 50 + 51 and kept.shape[0] == v.shape[0] - 51
    v, f = mc.CASES["tie_at_the_cut"]
    assert mr.post_process_mesh(v, f, cluster_to_keep=2, min_triangles=0)[1].shape[0] == 128 + 60 + 60      # ties at the cut stay


def test_post_process_keeps_a_vertex_only_a_degenerate_triangle_references():
    v, f = mc.CASES["degenerate_alone"]
    v1, f1, kept = mr.post_process_mesh(v, f, min_triangles=0)
    assert f1.tolist() == [[2, 3, 4]] and kept.tolist() == [0, 1, 2, 3, 4] and np.array_equal(v1, v)
    v2, f2, kept2 = mr.remove_unreferenced_vertices(v, mr.remove_degenerate_triangles(f))
    assert kept2.tolist() == [2, 3, 4] and f2.tolist() == [[0, 1, 2]]
    v, f = mc.CASES["unused_vertex"]
    _, f3, kept3 = mr.remove_unreferenced_vertices(v, f)
    assert kept3.tolist() == [i for i in range(v.shape[0]) if i != 5] and f3.max() == v.shape[0] - 2


def test_get_connected_mesh_selects_by_area():
    v, f = mc.CASES["floaters_49_50_51"]
    _, f1, _ = mr.get_connected_mesh(v, f, get_largest_components=True)
    assert f1.shape[0] == 128
    _, f2, _ = mr.get_connected_mesh(v, f, remove_small_geometry_threshold=0.15)               # the sheet is ~64 of ~139 units, a strip ~25
    assert f2.shape[0] == 128 + 49 + 50 + 51
    _, f3, _ = mr.get_connected_mesh(v, f)
    assert f3.shape[0] == 128
