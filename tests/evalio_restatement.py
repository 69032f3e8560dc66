"""Evaluation from files restated in NumPy, in this project's own words: the specification of include/radegs.h ("Evaluation
from files") and DESIGN 11 N18.  Three parts: the correspondence RANSAC (generator, per-sample umeyama, counts, choice), a PLY reader over
NumPy structured dtypes with the writers the tests build their files with, and merge_vertices over np.unique.  It is checked on the CPU
(tests/test_evalio_restatement.py) and then serves as the expectation of tests/test_gpu_evalio.py and tests/test_gpu_evalio_files.py.

Every decision on a threshold is checked for a MARGIN (raise Margin), as tests/tnteval_restatement.py does: an implementation whose SVD
differs in the last bits must still decide alike, so counts can be compared exactly.  Makers of inputs redraw from the next seed what misses
a margin; the margin is never narrowed and tests never skip."""
import struct

import numpy as np

from tnteval_restatement import Margin, transform

MARGIN = 1e-9            # |d - max_dist| over all hypotheses and pairs; relative rmse gap between the winner and a runner-up of its count
SCOPE = 1e-3             # sigma_2 / sigma_1 of a sample's covariance above which its rotation is well determined
U64 = np.uint64
_M = (1 << 64) - 1


# ------------------------------------------------------------------------- the generator -------------------------------------------------------------------------
def draw_u32(seed, h, k):
    """the high 32 bits of mix(seed A + h B + k C + D), 64-bit wrapping; h may be an array"""
    h = np.asarray(h, dtype=U64)
    with np.errstate(over="ignore"):
        z = (U64((int(seed) * 0x9E3779B97F4A7C15) & _M) + h * U64(0xD1B54A32D192ED03) + U64((int(k) * 0x8CB92BA72F3D8DD7) & _M)
             + U64(0x2545F4914F6CDD1D))
        z ^= z >> U64(30)
        z *= U64(0xBF58476D1CE4E5B9)
        z ^= z >> U64(27)
        z *= U64(0x94D049BB133111EB)
        z ^= z >> U64(31)
    return z >> U64(32)


def sample_indices(seed, K, n, N):
    """[K,n] int64: draw k of hypothesis h is the r-th index of [0, N) that no earlier draw took, r = (u (N - k)) >> 32"""
    out = np.zeros((K, n), np.int64)
    h = np.arange(K, dtype=U64)
    for k in range(n):
        r = ((draw_u32(seed, h, k) * U64(N - k)) >> U64(32)).astype(np.int64)
        taken = np.sort(out[:, :k], axis=1)
        for j in range(k):
            r += r >= taken[:, j]
        out[:, k] = r
    return out


# ------------------------------------------------------------------------ the similarity ------------------------------------------------------------------------
def sample_sums(s, t):
    """radegs_tnteval_pair_sums' 18 numbers for the pairs (s[i], t[i]) in the order given ([..., n, 3] arrays): what tnt_eval.umeyama takes"""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    n = s.shape[-2]
    ss, st = np.zeros(s.shape[:-2] + (3,)), np.zeros(s.shape[:-2] + (3,))
    for k in range(n):
        ss, st = ss + s[..., k, :], st + t[..., k, :]
    ms, mt = ss / n, st / n
    sig, var, d2 = np.zeros(s.shape[:-2] + (3, 3)), np.zeros(s.shape[:-2]), np.zeros(s.shape[:-2])
    for k in range(n):
        ds, dt, d = s[..., k, :] - ms, t[..., k, :] - mt, s[..., k, :] - t[..., k, :]
        sig = sig + dt[..., :, None] * ds[..., None, :]
        var = var + ((ds[..., 0] * ds[..., 0] + ds[..., 1] * ds[..., 1]) + ds[..., 2] * ds[..., 2])
        d2 = d2 + ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    count = np.full(s.shape[:-2] + (1,), float(n))
    return np.concatenate([count, ss, st, d2[..., None], sig.reshape(s.shape[:-2] + (9,)), var[..., None]], -1)


def umeyama_batch(sums):
    """Eigen's umeyama with scaling from [K,18] sums -> (T [K,4,4], ok [K], ratio [K] = sigma_2 / sigma_1).  ok False: no extent, or not finite."""
    a = np.asarray(sums, np.float64).reshape(-1, 18)
    n = a[:, 0]
    T = np.tile(np.eye(4), (a.shape[0], 1, 1))
    ok = a[:, 17] > 0
    with np.errstate(all="ignore"):
        mu_s, mu_t, var_s, sigma = a[:, 1:4] / n[:, None], a[:, 4:7] / n[:, None], a[:, 17] / n, a[:, 8:17].reshape(-1, 3, 3) / n[:, None, None]
        sigma = np.where(np.isfinite(sigma), sigma, 0.0)
        U, D, Vt = np.linalg.svd(sigma)
        S = np.ones((a.shape[0], 3))
        S[:, 2] = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0)
        R = np.einsum("kij,kj,kjl->kil", U, S, Vt)
        c = (D * S).sum(1) / var_s
        T[:, :3, :3] = c[:, None, None] * R
        T[:, :3, 3] = mu_t - c[:, None] * np.einsum("kij,kj->ki", R, mu_s)
        ratio = np.where(D[:, 0] > 0, D[:, 1] / np.where(D[:, 0] > 0, D[:, 0], 1.0), 0.0)
    ok &= np.isfinite(T).all((1, 2))
    T[~ok] = np.eye(4)
    return T, ok, ratio


def better(count_a, rmse_a, h_a, count_b, rmse_b, h_b):
    """the rule of the choice: more inliers; then the smaller rmse; then the smaller h"""
    if count_a != count_b:
        return count_a > count_b
    if rmse_a != rmse_b:
        return rmse_a < rmse_b
    return h_a < h_b


def ransac(source, target, max_dist=0.2, ransac_n=6, max_iteration=100000, seed=0, check=True, block=8192):
    """-> dict(samples [K,n], T [K,4,4], ok [K], scope [K], counts int32 [K], sumsq [K], hypothesis, count, transformation, fitness,
    inlier_rmse).  Pair i ascending: p = T s_i, d2 = (dx dx + dy dy) + dz dz, an inlier where sqrt(d2) < max_dist; sumsq adds d2 in that order."""
    s, t = np.asarray(source, np.float64).reshape(-1, 3), np.asarray(target, np.float64).reshape(-1, 3)
    N, K = s.shape[0], int(max_iteration)
    assert s.shape == t.shape and N >= ransac_n and 3 <= ransac_n <= 8
    samples = sample_indices(seed, K, ransac_n, N)
    T, ok, ratio = umeyama_batch(sample_sums(s[samples], t[samples]))
    counts, sumsq, closest = np.zeros(K, np.int32), np.zeros(K), np.inf
    for b in range(0, K, block):
        Tb = T[b:b + block]
        d2 = None
        diff = []
        for r in range(3):
            p = ((Tb[:, r, 0, None] * s[None, :, 0] + Tb[:, r, 1, None] * s[None, :, 1]) + Tb[:, r, 2, None] * s[None, :, 2]) + Tb[:, r, 3, None]
            diff.append(p - t[None, :, r])
        d2 = (diff[0] * diff[0] + diff[1] * diff[1]) + diff[2] * diff[2]
        d = np.sqrt(d2)
        live = ok[b:b + block, None]
        inl = (d < max_dist) & live
        if live.any():
            closest = min(closest, float(np.abs(d - max_dist)[np.broadcast_to(live, d.shape)].min()))
        counts[b:b + block] = inl.sum(1)
        acc = np.zeros(Tb.shape[0])
        for i in range(N):                              # ascending pair order
            acc = np.where(inl[:, i], acc + d2[:, i], acc)
        sumsq[b:b + block] = acc
    if check and closest < MARGIN:
        raise Margin(f"a distance within {MARGIN} of max_dist ({closest})")
    with np.errstate(all="ignore"):
        rmse = np.where(counts > 0, np.sqrt(sumsq / np.maximum(counts, 1)), np.inf)
    best = int(counts.max())
    out = dict(samples=samples, T=T, ok=ok, scope=ok & (ratio > SCOPE), ratio=ratio, counts=counts, sumsq=sumsq, rmse=rmse, closest=closest)
    if best == 0:
        out.update(hypothesis=-1, count=0, transformation=np.eye(4), fitness=0.0, inlier_rmse=0.0)
        return out
    top = np.nonzero(counts == best)[0]
    order = top[np.lexsort((top, rmse[top]))]
    w = int(order[0])
    if check and order.shape[0] > 1:
        gap = rmse[order[1]] - rmse[w]
        if gap < MARGIN * rmse[order[1]]:
            raise Margin(f"the winner's rmse is within {MARGIN} relative of the runner-up's")
    out.update(hypothesis=w, count=best, transformation=T[w], fitness=best / N, inlier_rmse=float(rmse[w]))
    return out


# --------------------------------------------------------------------------- fixtures ---------------------------------------------------------------------------
def similarity(rng, scale=None):
    """a random similarity 4x4: scale in [0.5, 2], a proper rotation, a shift of a few units"""
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 2] *= -1
    T = np.eye(4)
    T[:3, :3] = (rng.uniform(0.5, 2.0) if scale is None else scale) * q
    T[:3, 3] = rng.uniform(-2, 2, 3)
    return T


def noisy_pairs(N, seed, outliers=0.22, noise=0.015):
    """(source, target, known): a uniform cloud in [-3,3]^3, its image under a known similarity plus noise, a share of outliers"""
    rng = np.random.default_rng(seed)
    known = similarity(rng)
    src = rng.uniform(-3, 3, (N, 3))
    tgt = transform(src, known) + noise * rng.standard_normal((N, 3))
    bad = rng.permutation(N)[:int(round(outliers * N))]
    tgt[bad] = rng.uniform(-6, 6, (bad.shape[0], 3))
    return src, tgt, known


def fixture(N, K, ransac_n=6, seed=0, first_seed=100, tries=50, **kw):
    """noisy_pairs redrawn from the next seed until ransac() keeps its margins -> (source, target, known, restatement's result)"""
    for attempt in range(tries):
        src, tgt, known = noisy_pairs(N, first_seed + attempt, **kw)
        try:
            return src, tgt, known, ransac(src, tgt, 0.2, ransac_n, K, seed)
        except Margin:
            continue
    raise Margin("no draw keeps the margins")


# ------------------------------------------------------------------------------ PLY ------------------------------------------------------------------------------
TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4",
         "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
NAMES = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float", "f8": "double"}
FMT = {"i1": "b", "u1": "B", "i2": "h", "u2": "H", "i4": "i", "u4": "I", "f4": "f", "f8": "d"}
ENDIAN = {"binary_little_endian": "<", "binary_big_endian": ">"}


def write_ply(path, elements, fmt="binary_little_endian", version="1.0", cut=None):
    """elements: [(name, [(property, code) | (property, ("list", count code, item code))], columns)], `columns` one sequence per property
    (a list property: one sequence of items per row, of any length).  `cut`: drop that many bytes from the end (a truncated file)."""
    head = ["ply", f"format {fmt} {version}", "comment written by the tests"]
    for name, props, cols in elements:
        head.append(f"element {name} {len(cols[0]) if cols else 0}")
        for p, t in props:
            head.append(f"property list {NAMES[t[1]]} {NAMES[t[2]]} {p}" if isinstance(t, tuple) else f"property {NAMES[t]} {p}")
    data = ("\n".join(head) + "\nend_header\n").encode("ascii")
    body = []
    for name, props, cols in elements:
        for r in range(len(cols[0]) if cols else 0):
            if fmt == "ascii":
                words = []
                for (p, t), c in zip(props, cols):
                    items = [len(c[r])] + list(c[r]) if isinstance(t, tuple) else [c[r]]
                    kinds = [t[1]] + [t[2]] * len(c[r]) if isinstance(t, tuple) else [t]
                    words += [repr(float(v)) if k[0] == "f" else str(int(v)) for v, k in zip(items, kinds)]
                body.append((" ".join(words) + "\n").encode("ascii"))
            else:
                e = ENDIAN[fmt]
                for (p, t), c in zip(props, cols):
                    if isinstance(t, tuple):
                        body.append(struct.pack(e + FMT[t[1]], len(c[r])) + struct.pack(e + FMT[t[2]] * len(c[r]), *[int(v) for v in c[r]]))
                    else:
                        body.append(struct.pack(e + FMT[t], float(c[r]) if t[0] == "f" else int(c[r])))
    data += b"".join(body)
    with open(path, "wb") as f:
        f.write(data if not cut else data[:-cut])


def read_ply(path):
    """{element: structured array}: a header parser of its own and one NumPy structured dtype per element; a list property is read as a
    length and three items (`name` and `name_n`), which is right iff every list has three -- the caller checks `name_n`"""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    fmt, elements = None, []
    for line in raw[:end].decode("ascii").split("\n")[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info", "end_header"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property" and w[1] == "list":
            elements[-1][2] += [(w[4] + "_n", TYPES[w[2]]), (w[4], TYPES[w[3]], (3,))]
        else:
            elements[-1][2].append((w[2], TYPES[w[1]]))
    out, at = {}, end
    tokens = raw[end:].split() if fmt == "ascii" else None
    for name, count, fields in elements:
        if fmt == "ascii":
            width = sum(int(np.prod(f[2])) if len(f) == 3 else 1 for f in fields)
            table = np.array(tokens[at - end:at - end + count * width]).reshape(count, width)
            arr, col = np.zeros(count, np.dtype([(f[0], "<" + f[1]) + tuple(f[2:]) for f in fields])), 0
            for f in fields:
                k = int(np.prod(f[2])) if len(f) == 3 else 1
                vals = table[:, col:col + k].astype(np.float64) if f[1][0] == "f" else np.array([[int(v) for v in row] for row in table[:, col:col + k]], np.int64).reshape(count, k)
                arr[f[0]] = vals.reshape(arr[f[0]].shape)
                col += k
            at += count * width
        else:
            dt = np.dtype([(f[0], ENDIAN[fmt] + f[1]) + tuple(f[2:]) for f in fields])
            arr = np.frombuffer(raw, dtype=dt, count=count, offset=at)
            at += count * dt.itemsize
        out[name] = arr
    assert fmt == "ascii" or at == len(raw), "the structured dtypes do not cover the file"
    return out


def ply_points(path):
    v = read_ply(path)["vertex"]
    return np.stack([v["x"].astype(np.float64), v["y"].astype(np.float64), v["z"].astype(np.float64)], 1)


def ply_mesh(path):
    el = read_ply(path)
    face = el["face"]
    name = [n for n in face.dtype.names if n.endswith("_n")][0][:-2]
    assert (face[name + "_n"] == 3).all()
    return ply_points(path), face[name].astype(np.int64).reshape(-1, 3)


def mesh_data(V, F, seed):
    """(vertices float64 [V,3] with more digits than a float holds, faces int64 [F,3])"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-5, 5, (V, 3)) * [1.0, 1e-3, 1e3], rng.integers(0, V, (F, 3))


def _xyz(v, t):
    return [("x", t), ("y", t), ("z", t)], [v[:, 0], v[:, 1], v[:, 2]]


def _f32(v):
    return v.astype(np.float32).astype(np.float64)


def _layout_tetmesh(v, f):                      # tetmesh.write_ply; trimesh's writer has the same layout
    p, c = _xyz(v, "f4")
    return [("vertex", p, c), ("face", [("vertex_indices", ("list", "u1", "i4"))], [f])], _f32(v), f


def _layout_coloured(v, f):                     # tsdf.write_ply(colors=, normals=), mesh_clean's and unbounded_mesh's: normals, then colours
    p, c = _xyz(v, "f4")
    n = len(v)
    extra = [("nx", "f4"), ("ny", "f4"), ("nz", "f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]
    cols = [np.linspace(-1, 1, n)] * 3 + [np.arange(n) % 256, np.arange(n) * 7 % 256, np.arange(n) * 13 % 256]
    return [("vertex", p + extra, c + cols), ("face", [("vertex_indices", ("list", "u1", "i4"))], [f])], _f32(v), f


def _layout_open3d(v, f):                       # double x y z, list uchar uint
    p, c = _xyz(v, "f8")
    return [("vertex", p, c), ("face", [("vertex_indices", ("list", "u1", "u4"))], [f])], v, f


def _layout_cloud(v, f):                        # a vertex-only cloud with normals and colours (the ground truth of both benchmarks)
    elements, exp, _ = _layout_coloured(v, f)
    return elements[:1], exp, None


def _layout_xyz_last(v, f):                     # x y z not first, of three different types, and an odd record size
    n = len(v)
    vi = np.round(v[:, 2]).astype(np.int64)
    props = [("flag", "u1"), ("quality", "f8"), ("z", "i2"), ("id", "u2"), ("y", "f8"), ("x", "f4")]
    cols = [np.arange(n) % 2, np.linspace(0, 1, n), vi, np.arange(n) % 60000, v[:, 1], v[:, 0]]
    exp = np.stack([_f32(v[:, 0]), v[:, 1], vi.astype(np.float64)], 1)
    faces = [("material", "i2"), ("vertex_index", ("list", "i4", "i4")), ("area", "f4"), ("tag", "u1")]      # scalars before and after the list
    m = len(f)
    return [("vertex", props, cols), ("face", faces, [np.arange(m) % 100 - 50, f, np.linspace(0, 2, m), np.arange(m) % 200])], exp, f


def _layout_middle_element(v, f):               # fixed-size elements before, between and after
    p, c = _xyz(v, "f8")
    cam = ("camera", [("cx", "f4"), ("n", "u1")], [np.arange(3.0), np.arange(3)])
    edge = ("edge", [("a", "i4"), ("b", "i4"), ("w", "u1")], [np.arange(5), np.arange(5) + 1, np.arange(5)])
    return [cam, ("vertex", p, c), edge, ("face", [("vertex_indices", ("list", "u2", "u4"))], [f]), cam], v, f


LAYOUTS = {"tetmesh": _layout_tetmesh, "coloured": _layout_coloured, "open3d": _layout_open3d, "cloud": _layout_cloud, "xyz_last": _layout_xyz_last,
           "middle_element": _layout_middle_element}


# ------------------------------------------------------------------------ merge_vertices ------------------------------------------------------------------------
def merge_vertices(vertices, faces, digits=8):
    """drop non-finite vertices and their faces; weld rows equal after round(v 10^digits) (np.unique over rows); keep referenced vertices, in
    first-occurrence order, the first of a group standing for it; faces renumbered, in order"""
    v, f = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    fin = np.isfinite(v).all(1)
    f = f[fin[f].all(1)]
    idx = np.nonzero(fin)[0]
    if f.shape[0] == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    _, first, inverse = np.unique(np.round(v[idx] * 10.0 ** digits), axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    rep = np.full(v.shape[0], -1, np.int64)
    rep[idx] = idx[first][inverse]                      # every finite vertex -> the first vertex of its group
    fr = rep[f]
    kept = np.unique(fr)                                # ascending original index = first-occurrence order
    new = np.full(v.shape[0], -1, np.int64)
    new[kept] = np.arange(kept.shape[0])
    return v[kept], new[fr]
