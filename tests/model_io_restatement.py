"""NumPy-only restatement of the model state I/O (include/radegs.h, "Model state"): the header writer and reader, the
payload as a structured dtype, the init formulas in float32 and reset_opacity in float64 on the float32 inputs.  Nothing here imports the
package under test: the GPU tests compare rade-gs_amd/model_io.py against this file, and tests/test_model_io_api.py compares this file
against what the reference's own code produced (tests/golden/g_model_io.npz)."""
import numpy as np

C0 = np.float32(0.28209479177387814)
NAMES_OF_TYPE = {"i1": ("char", "int8"), "u1": ("uchar", "uint8"), "i2": ("short", "int16"), "u2": ("ushort", "uint16"), "i4": ("int", "int32"),
                 "u4": ("uint", "uint32"), "f4": ("float", "float32"), "f8": ("double", "float64")}
TYPE_OF_NAME = {n: t for t, names in NAMES_OF_TYPE.items() for n in names}


# ----------------------------------------------------------------------------- header -----------------------------------------------------------------------------
def attribute_names(n_rest, with_filter=True):
    """construct_list_of_attributes for n_rest = 3 K"""
    out = ["x", "y", "z", "nx", "ny", "nz"] + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(n_rest)] + ["opacity"]
    out += ["scale_%d" % i for i in range(3)] + ["rot_%d" % i for i in range(4)]
    if with_filter:
        out.append("filter_3D")
    return out


def write_header(count, properties, fmt="binary_little_endian", spelling=0, newline="\n", comments=()):
    """properties: [(name, numpy code)]; spelling 0: float / uchar ..., 1: float32 / uint8 ..."""
    lines = ["ply", "format %s 1.0" % fmt] + ["comment " + c for c in comments] + ["element vertex %d" % count]
    lines += ["property %s %s" % (NAMES_OF_TYPE[t][spelling], n) for n, t in properties] + ["end_header"]
    return (newline.join(lines) + newline).encode("ascii")


def parse_header(data):
    """(format, [(element, count, [(name, numpy code)])], data offset) of a file's bytes; scalar properties only"""
    end = data.index(b"end_header")
    offset = data.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:end].decode("ascii").splitlines()[1:]:
        w = line.split()
        if not w or w[0] == "comment":
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            elements[-1][2].append((w[2], TYPE_OF_NAME[w[1]]))
    return fmt, elements, offset


# ----------------------------------------------------------------------------- payload -----------------------------------------------------------------------------
def record_dtype(properties, endian="<"):
    return np.dtype([(n, endian + t) for n, t in properties])


def model_columns(xyz, f_dc, f_rest, opacity, scaling, rotation, filter_3D=None):
    """[P, C] float32: upstream's np.concatenate((xyz, normals, f_dc, f_rest, opacities, scale, rotation, filter_3D), axis=1)"""
    P = xyz.shape[0]
    parts = [xyz, np.zeros_like(xyz), f_dc.transpose(0, 2, 1).reshape(P, 3), f_rest.transpose(0, 2, 1).reshape(P, 3 * f_rest.shape[1]), opacity, scaling,
             rotation]
    if filter_3D is not None:
        parts.append(filter_3D)
    return np.ascontiguousarray(np.concatenate(parts, axis=1), dtype=np.float32)


def model_file(xyz, f_dc, f_rest, opacity, scaling, rotation, filter_3D=None):
    """the bytes of save_ply's file"""
    table = model_columns(xyz, f_dc, f_rest, opacity, scaling, rotation, filter_3D)
    names = attribute_names(3 * f_rest.shape[1], filter_3D is not None)
    assert table.shape[1] == len(names)
    rec = np.empty(table.shape[0], dtype=record_dtype([(n, "f4") for n in names]))
    for j, n in enumerate(names):
        rec[n] = table[:, j]
    return write_header(table.shape[0], [(n, "f4") for n in names]) + rec.tobytes()


def read_vertex(data):
    """(structured array of the vertex element, properties) of a binary little-endian file's bytes"""
    fmt, elements, offset = parse_header(data)
    assert fmt == "binary_little_endian" and elements[0][0] == "vertex"
    _, count, props = elements[0]
    return np.frombuffer(data, dtype=record_dtype(props), count=count, offset=offset), props


def model_from_file(data):
    """upstream's load_ply on a file's bytes: (xyz, f_dc, f_rest, opacity, scaling, rotation, filter_3D or None), float32; every value goes
    through float64 as upstream's np.zeros tables do"""
    rec, props = read_vertex(data)
    names = [n for n, _ in props]
    P = rec.shape[0]
    num = lambda prefix: sorted([n for n in names if n.startswith(prefix)], key=lambda n: int(n.split("_")[-1]))   # noqa: E731
    col = lambda ns: np.stack([rec[n].astype(np.float64) for n in ns], axis=1).astype(np.float32) if ns else np.zeros((P, 0), np.float32)   # noqa: E731
    rest = num("f_rest_")
    K = len(rest) // 3
    f_rest = np.ascontiguousarray(col(rest).reshape(P, 3, K).transpose(0, 2, 1))
    f_dc = np.ascontiguousarray(col(["f_dc_0", "f_dc_1", "f_dc_2"]).reshape(P, 3, 1).transpose(0, 2, 1))
    filt = col(["filter_3D"]) if "filter_3D" in names else None
    return col(["x", "y", "z"]), f_dc, f_rest, col(["opacity"]), col(num("scale_")), col(num("rot")), filt


POINTS3D = [("x", "f4"), ("y", "f4"), ("z", "f4"), ("nx", "f4"), ("ny", "f4"), ("nz", "f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]


def points3d_file(xyz, rgb, normals=None):
    """storePly's file: 27-byte records"""
    rec = np.zeros(xyz.shape[0], dtype=record_dtype(POINTS3D))
    for j, n in enumerate(("x", "y", "z")):
        rec[n] = xyz[:, j]
    if normals is not None:
        for j, n in enumerate(("nx", "ny", "nz")):
            rec[n] = normals[:, j]
    for j, n in enumerate(("red", "green", "blue")):
        rec[n] = np.asarray(rgb[:, j]).astype(np.uint8)
    return write_header(xyz.shape[0], POINTS3D) + rec.tobytes()


def fetch_points3d(data):
    """fetchPly followed by create_from_pcd's .float(): (points, colours / 255 in float64 rounded once to float32, normals)"""
    rec, _ = read_vertex(data)
    pts = np.stack([rec["x"], rec["y"], rec["z"]], axis=1)
    col = (np.stack([rec["red"], rec["green"], rec["blue"]], axis=1) / 255.0).astype(np.float32)
    nrm = np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=1)
    return pts, col, nrm


# ----------------------------------------------------------------------------- the two steps -----------------------------------------------------------------------------
def rgb2sh(rgb):
    """utils/sh_utils.py RGB2SH in float32"""
    return ((np.asarray(rgb, dtype=np.float32) - np.float32(0.5)) / C0).astype(np.float32)


def initial_opacity():
    p = np.float32(0.1)
    return np.log(p / (np.float32(1.0) - p), dtype=np.float32)


def init_state(points, colors, dist2, sh_degree):
    """create_from_pcd after the kNN step, float32; scaling's float64 value is returned last for the tolerance"""
    P, K = points.shape[0], (sh_degree + 1) ** 2 - 1
    d = np.maximum(np.asarray(dist2, dtype=np.float32), np.float32(0.0000001))
    s64 = np.log(np.sqrt(d.astype(np.float64)))
    scaling = np.repeat(np.log(np.sqrt(d), dtype=np.float32)[:, None], 3, axis=1)
    rotation = np.zeros((P, 4), np.float32)
    rotation[:, 0] = 1
    return dict(xyz=np.asarray(points, np.float32), features_dc=rgb2sh(colors).reshape(P, 1, 3), features_rest=np.zeros((P, K, 3), np.float32),
                opacity=np.full((P, 1), initial_opacity(), np.float32), scaling=scaling, rotation=rotation, scaling64=np.repeat(s64[:, None], 3, axis=1))


def reset_opacity64(opacity_raw, scaling_raw, filter_3D):
    """reset_opacity (gaussian_model.py:495-510) in float64 on the float32 inputs: (new raw opacity [P,1], x, kappa = 1 / (1 - x))"""
    with np.errstate(all="ignore"):
        o, s, f = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (opacity_raw, scaling_raw, filter_3D))
        q = np.square(np.exp(s))
        coef = np.sqrt(q.prod(axis=1) / (q + np.square(f)).prod(axis=1))[:, None]
        cur = 1.0 / (1.0 + np.exp(-o)) * coef
        x = np.where(np.isnan(cur), cur, np.minimum(cur, 0.01)) / coef
        return np.log(x / (1.0 - x)), x, 1.0 / (1.0 - x)


def reset_recipe():
    """the inputs of the golden's reset case (tests/golden/make_golden_model_io.py records what the reference made of them)"""
    rng = np.random.default_rng(5)
    P = 4096
    o = rng.uniform(-8, 8, (P, 1)).astype(np.float32)
    s = rng.uniform(-7, -1, (P, 3)).astype(np.float32)
    f = rng.uniform(0.001, 0.05, (P, 1)).astype(np.float32)
    f[::7] = 0
    return o, s, f


def reset_edges():
    """named edge rows: (names, opacity_raw, scaling_raw, filter_3D)"""
    rows = [("o=+30", 30.0, (-3, -3, -3), 0.01), ("o=-30", -30.0, (-3, -3, -3), 0.01), ("filter 0", 2.0, (-4, -2, -3), 0.0),
            ("filter 0, low", -9.0, (-4, -2, -3), 0.0), ("coef < 0.01", 6.0, (-7, -7, -7), 0.05), ("coef < 0.01, low", -6.0, (-7, -7, -7), 0.05),
            ("scale e^8", 1.0, (8, 8, 8), 0.02), ("scale e^8, one axis", 1.0, (8, -3, -3), 0.02),
            # x = 1 exactly: +inf; sigmoid = 0: -inf; det1 = det2 = inf: NaN
            ("coef < 0.01, o=+30", 30.0, (-7, -7, -7), 0.05), ("o=-200", -200.0, (-3, -3, -3), 0.01), ("scale e^30", 1.0, (30, 30, 30), 0.02)]
    names = [r[0] for r in rows]
    o = np.array([[r[1]] for r in rows], np.float32)
    s = np.array([r[2] for r in rows], np.float32)
    f = np.array([[r[3]] for r in rows], np.float32)
    return names, o, s, f
