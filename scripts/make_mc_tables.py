"""Generates rade-gs_amd/csrc/rg_mc_tables.h, the marching-cubes case table of the TSDF extraction.

    python scripts/make_mc_tables.py            writes the header, prints the maximum triangle count of a case
    python scripts/make_mc_tables.py --check    exits 1 when the committed header differs from what this script generates

Nothing here is typed from a published table; every row follows from one rule.

Corner i of a cell sits at offset (i & 1, (i >> 1) & 1, (i >> 2) & 1) from the cell's lowest corner.  Bit i of the case index is set
when corner i is negative (inside).  Edge e = 4 * axis + a + 2 * b runs along `axis` from the corner whose other two coordinates (in
ascending axis order) are (a, b); that corner's voxel owns the edge.  An edge is cut when its two corners differ in sign.

Per case: on each of the six faces connect the cut edges -- two cuts: one segment; four cuts (diagonal corners alike): the two
segments that cut off each NEGATIVE corner by itself.  The rule reads the face's four signs only, so the two cells that share a face
always draw the same segments on it.  Every cut edge then lies on exactly two segments: the segments chain into closed loops.  Each
segment is directed so that, seen from outside the cell, the positive corners lie to its left; the loops are then counter-clockwise
seen from the positive side (the normal points outside the surface).  A loop is rotated to start at its lowest-numbered edge and
fan-triangulated from there; the loops of a case are ordered by their lowest edge."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "rade-gs_amd", "csrc", "rg_mc_tables.h")

CORNERS = [(i & 1, (i >> 1) & 1, (i >> 2) & 1) for i in range(8)]


def corner_index(c):
    return c[0] | (c[1] << 1) | (c[2] << 2)


def edge_ends(e):
    """(owner corner, far corner) of edge e as corner indices"""
    axis, a, b = e // 4, e & 1, (e >> 1) & 1
    lo = [0, 0, 0]
    others = [k for k in range(3) if k != axis]
    lo[others[0]], lo[others[1]] = a, b
    hi = list(lo)
    hi[axis] = 1
    return corner_index(lo), corner_index(hi)


EDGES = [edge_ends(e) for e in range(12)]
EDGE_OF = {frozenset(p): e for e, p in enumerate(EDGES)}
# [e] = (dx, dy, dz, axis): the owning voxel's offset from the cell's lowest corner, and the edge's direction
EDGE_INFO = [CORNERS[EDGES[e][0]] + (e // 4,) for e in range(12)]


def faces():
    """the six faces as (outward normal, its four corners in cyclic order)"""
    out = []
    for axis in range(3):
        u, v = [k for k in range(3) if k != axis]
        for side in (0, 1):
            ring = []
            for a, b in ((0, 0), (1, 0), (1, 1), (0, 1)):
                c = [0, 0, 0]
                c[axis], c[u], c[v] = side, a, b
                ring.append(corner_index(c))
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            out.append((tuple(n), ring))
    return out


FACES = faces()


def negative(case, corner):
    return (case >> corner) & 1 == 1


def edge_mask(case):
    return sum(1 << e for e, (a, b) in enumerate(EDGES) if negative(case, a) != negative(case, b))


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def midpoint2(e):
    """twice the midpoint of edge e (integers)"""
    a, b = CORNERS[EDGES[e][0]], CORNERS[EDGES[e][1]]
    return tuple(a[k] + b[k] for k in range(3))


def direct(seg, cut_off, normal):
    """the segment (e0, e1) directed so that, seen against `normal`, the negative corner `cut_off` lies to its right"""
    p, q = midpoint2(seg[0]), midpoint2(seg[1])
    d = tuple(q[k] - p[k] for k in range(3))
    c = CORNERS[cut_off]
    to_positive = tuple((p[k] + q[k]) - 4 * c[k] for k in range(3))      # 4 * (segment midpoint - corner)
    s = sum(cross(d, to_positive)[k] * normal[k] for k in range(3))
    assert s != 0
    return seg if s > 0 else (seg[1], seg[0])


def face_segments(case):
    """the directed segments of a case, face by face: a list of six lists of (edge from, edge to)"""
    out = []
    for normal, ring in FACES:
        ring_edges = [EDGE_OF[frozenset((ring[k], ring[(k + 1) % 4]))] for k in range(4)]    # ring_edges[k] joins ring[k], ring[k + 1]
        cut = [k for k in range(4) if negative(case, ring[k]) != negative(case, ring[(k + 1) % 4])]
        segs = []
        if len(cut) == 2:
            neg = [c for c in ring if negative(case, c)][0]
            segs.append(direct((ring_edges[cut[0]], ring_edges[cut[1]]), neg, normal))
        elif len(cut) == 4:
            for k in range(4):
                if negative(case, ring[k]):
                    segs.append(direct((ring_edges[(k - 1) % 4], ring_edges[k]), ring[k], normal))
        else:
            assert not cut
        out.append(segs)
    return out


def loops(case):
    nxt = {}
    for segs in face_segments(case):
        for a, b in segs:
            assert a not in nxt, (case, a)
            nxt[a] = b
    mask = edge_mask(case)
    assert sorted(nxt) == [e for e in range(12) if mask >> e & 1] == sorted(nxt.values()), case
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3, case
        out.append(loop)                    # starts at its lowest edge: `start` ascends
    return out


def triangles(case):
    tris = []
    for loop in loops(case):
        for k in range(1, len(loop) - 1):
            tris.append((loop[0], loop[k], loop[k + 1]))
    return tris


def tables():
    tri = [triangles(c) for c in range(256)]
    return tri, max(len(t) for t in tri)


def render():
    tri, most = tables()
    width = 3 * most + 1
    lines = ["// rg_mc_tables.h -- GENERATED by scripts/make_mc_tables.py; do not edit.  The marching-cubes case table of radegs_tsdf.hip.",
             "// Corner i at offset (i & 1, (i >> 1) & 1, (i >> 2) & 1); case bit i = corner i negative; edge e = 4 * axis + a + 2 * b.",
             "// kMcTriTable[case]: edge triples, -1 ends the row.  kMcNumTris[case].  kMcEdgeMask[case]: bit e = edge e is cut.",
             "// kMcEdgeInfo[e] = {dx, dy, dz, axis}: the voxel that owns edge e, relative to the cell, and the edge's direction.",
             "#pragma once",
             "#if defined(__HIPCC__)",
             "#define RG_MC_TABLE static __device__ const",
             "#else",
             "#define RG_MC_TABLE static const",
             "#endif",
             "#define RG_MC_MAX_TRIS %d" % most,
             "#define RG_MC_ROW %d" % width,
             "",
             "RG_MC_TABLE signed char kMcEdgeInfo[12][4] = {"]
    lines += ["  {%d, %d, %d, %d}," % EDGE_INFO[e] for e in range(12)]
    lines += ["};", "", "RG_MC_TABLE unsigned short kMcEdgeMask[256] = {"]
    for r in range(0, 256, 16):
        lines.append("  " + ", ".join("0x%03x" % edge_mask(c) for c in range(r, r + 16)) + ",")
    lines += ["};", "", "RG_MC_TABLE unsigned char kMcNumTris[256] = {"]
    for r in range(0, 256, 32):
        lines.append("  " + ", ".join("%d" % len(tri[c]) for c in range(r, r + 32)) + ",")
    lines += ["};", "", "RG_MC_TABLE signed char kMcTriTable[256][RG_MC_ROW] = {"]
    for c in range(256):
        row = [e for t in tri[c] for e in t]
        row += [-1] * (width - len(row))
        lines.append("  {" + ", ".join("%2d" % v for v in row) + "},")
    lines += ["};", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        with open(HEADER) as fh:
            sys.exit(0 if fh.read() == text else 1)
    with open(HEADER, "w") as fh:
        fh.write(text)
    print("maximum triangles per case:", tables()[1])
    print("wrote", os.path.relpath(HEADER, ROOT))
