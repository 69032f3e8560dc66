"""HIP-backed Gaussian model state I/O: what train.py, render.py and the two mesh routes do with a model on disk and that
upstream hands to plyfile and a dozen eager kernels each -- scene/gaussian_model.py:301-328 create_from_pcd, 379-397 save_ply, 495-513
reset_opacity, 515-559 load_ply, and scene/dataset_readers.py:156-189 fetchPly / storePly.  GPU only.  Tensors are float32, contiguous and
on the GPU in the model's own shapes; a wrong dtype, shape or device is refused, nothing is converted silently.  include/radegs.h, "Model
state", is the specification of the four kernels and tests/model_io_restatement.py restates them in NumPy.  plyfile is never imported: the
header it writes is restated from memory (DESIGN 11 N15 marks it)."""
import collections
import os
import re

import numpy as np
import torch

import geom_host as gh
from diff_gaussian_rasterization import _C
from geom_host import f32, i32, ll, vp

SIGNATURES = {
    "radegs_modelio_pack": (i32, [ll, ll, ll, i32] + [vp] * 9),
    "radegs_modelio_unpack": (i32, [ll, i32, vp, i32, vp, vp]),
    "radegs_modelio_reset_opacity": (i32, [ll] + [vp] * 7),
    "radegs_modelio_init": (i32, [ll, i32, vp, vp, f32] + [vp] * 6),
}
_SIGNATURES = SIGNATURES
MAX_REST, MAX_RECORD, MAX_COLUMNS = 79, 768, 256      # RADEGS_MODELIO_MAX_* (include/radegs.h)
DEFAULT_CHUNK_ROWS = 1 << 18                          # 66 MB of SH3 records per pinned buffer

# both spellings of a PLY scalar type -> (numpy code, RADEGS_MODELIO_* of the unpack kernel)
PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
             "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
TYPE_CODES = {"i1": 0, "u1": 1, "i2": 2, "u2": 3, "i4": 4, "u4": 5, "f4": 6, "f8": 7}
FORMATS = ("binary_little_endian", "binary_big_endian", "ascii")
_COLUMN = np.dtype([("dst", "<u8"), ("stride", "<i8"), ("elem", "<i4"), ("offset", "<i4"), ("type", "<i4"), ("scale", "<i4")])

PlyElement = collections.namedtuple("PlyElement", "name count properties")       # properties: [(name, numpy code)] or (name, ("list", c, t))
PlyHeader = collections.namedtuple("PlyHeader", "format elements data_offset")
GaussianState = collections.namedtuple("GaussianState", "xyz features_dc features_rest opacity scaling rotation filter_3D")
PointCloud = collections.namedtuple("PointCloud", "points colors normals")


def _lib():
    return gh.bind(_SIGNATURES)


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"model_io runs on the GPU only, got device `{device}`")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _rows(t, name, P, tail, dev=None):
    """a tensor as the kernels address it: float32, on the GPU, contiguous, exactly (P, *tail); anything else is refused"""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"`{name}` must be a tensor")
    _C._require_gpu(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"`{name}` must be float32, got {str(t.dtype).replace('torch.', '')}")
    if tuple(t.shape) != (P,) + tuple(tail):
        raise RuntimeError(f"`{name}` must have shape {(P,) + tuple(tail)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"`{name}` must be contiguous")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"`{name}` must be on {dev}, like the other tensors")
    return t.detach()


# ----------------------------------------------------------------------------- header -----------------------------------------------------------------------------
def attribute_names(n_rest, with_filter=True):
    """GaussianModel.construct_list_of_attributes (gaussian_model.py:363-377) for `n_rest` = 3 K rest coefficients"""
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(n_rest)] + ["opacity"]
    names += [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
    return names + ["filter_3D"] if with_filter else names


def ply_header(count, properties, fmt="binary_little_endian"):
    """The header plyfile writes for one `vertex` element: properties [(name, numpy code)], each spelled with the C-style type name."""
    spell = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float", "f8": "double"}
    lines = ["ply", f"format {fmt} 1.0", f"element vertex {count}"] + [f"property {spell[t]} {n}" for n, t in properties] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def read_ply_header(path):
    """PlyHeader(format, elements, data_offset) of a PLY file: both spellings of every type name, comment and obj_info lines, "\\n" or "\\r\\n"
    line ends.  A list property in the `vertex` element or in an element before it is refused by name: its records have no fixed size."""
    with open(path, "rb") as f:
        head = f.read(1 << 20)
    end = re.search(rb"(^|\n)end_header\r?\n", head)
    if not head.startswith(b"ply") or end is None:
        raise RuntimeError(f"{path}: not a PLY file (no `ply` ... `end_header` within the first MiB)")
    fmt, elements = None, []
    for raw in head[:end.start() + 1].decode("ascii", "replace").split("\n")[1:]:
        words = raw.strip().split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "format" and len(words) == 3:
            fmt = words[1]
        elif words[0] == "element" and len(words) == 3:
            elements.append(PlyElement(words[1], int(words[2]), []))
        elif words[0] == "property" and elements and len(words) == 3 and words[1] in PLY_TYPES:
            elements[-1].properties.append((words[2], PLY_TYPES[words[1]]))
        elif words[0] == "property" and elements and len(words) == 5 and words[1] == "list" and words[2] in PLY_TYPES and words[3] in PLY_TYPES:
            elements[-1].properties.append((words[4], ("list", PLY_TYPES[words[2]], PLY_TYPES[words[3]])))
        else:
            raise RuntimeError(f"{path}: header line not understood: `{raw.strip()}`")
    if fmt not in FORMATS:
        raise RuntimeError(f"{path}: format `{fmt}` is none of {FORMATS}")
    for el in elements:
        for name, t in el.properties:
            if isinstance(t, tuple):
                raise RuntimeError(f"{path}: list property `{name}` of element `{el.name}`: the records up to the end of `vertex` must have a fixed size")
        if el.name == "vertex":
            break
    else:
        raise RuntimeError(f"{path}: no `vertex` element")
    return PlyHeader(fmt, elements, end.end())


def _vertex(header):
    """(the vertex element, scalar values in the elements before it, their bytes)"""
    skip_values = skip_bytes = 0
    for el in header.elements:
        if el.name == "vertex":
            return el, skip_values, skip_bytes
        skip_values += el.count * len(el.properties)
        skip_bytes += el.count * sum(np.dtype(t).itemsize for _, t in el.properties)


def _read_records(path, header):
    """(records: a uint8 host tensor padded to a multiple of 4 and by 4 more, pinned where there is a GPU so that the file is read straight
    into the memory the upload starts from; P; S; {name: (byte offset, numpy code)}): the vertex element as little-endian records; a
    big-endian or ascii file is turned into them here, on the host."""
    el, skip_values, skip_bytes = _vertex(header)
    P, props = el.count, el.properties
    if len({n for n, _ in props}) != len(props):
        raise RuntimeError(f"{path}: a property name occurs twice in `vertex`")
    little = np.dtype([(n, "<" + t) for n, t in props]) if props else np.dtype([])
    S = little.itemsize
    layout = {n: (little.fields[n][1], t) for n, t in props}
    if header.format != "ascii":
        have = os.path.getsize(path) - header.data_offset - skip_bytes
        if have < P * S:
            raise RuntimeError(f"{path}: short payload: {max(have, 0)} bytes after the header, {P} records of {S} bytes need {P * S}")
    records = torch.empty((P * S + 3) // 4 * 4 + 4, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    buf = records.numpy()
    buf[P * S:] = 0
    if header.format == "ascii":
        with open(path, "rb") as f:
            f.seek(header.data_offset)
            tokens = f.read().split()
        need = P * len(props)
        if len(tokens) < skip_values + need:
            raise RuntimeError(f"{path}: short payload: {len(tokens) - skip_values} values after the header, `vertex` needs {need}")
        table = np.array(tokens[skip_values:skip_values + need]).reshape(P, len(props))
        rec = np.zeros(P, dtype=little)
        for j, (n, t) in enumerate(props):
            rec[n] = table[:, j].astype(np.float64).astype(t) if t[0] == "f" else np.array([int(v) for v in table[:, j]], dtype=np.int64).astype(t)
        buf[:P * S] = rec.view(np.uint8).reshape(-1)
        return records, P, S, layout
    with open(path, "rb") as f:
        f.seek(header.data_offset + skip_bytes)
        got = f.readinto(memoryview(buf)[:P * S])
    if got != P * S:
        raise RuntimeError(f"{path}: short payload: read {got} of {P * S} bytes")
    if header.format == "binary_big_endian" and P:
        big = np.dtype([(n, ">" + t) for n, t in props])
        buf[:P * S] = buf[:P * S].view(big).astype(little).view(np.uint8)
    return records, P, S, layout


# ----------------------------------------------------------------------------- unpack -----------------------------------------------------------------------------
def _unpack(records, P, S, columns, dev):
    """records: uint8 GPU tensor (padded); columns: [(dst tensor, float within its row, byte offset, numpy code, scale)]"""
    if P == 0 or not columns:
        return
    _launch_unpack(records, P, S, len(columns), _column_table(S, columns, dev), dev)


def _column_table(S, columns, dev):
    """the descriptors as RadegsModelioColumn records on the device, ordered by destination so that neighbouring lanes store to neighbouring floats"""
    if S > MAX_RECORD or len(columns) > MAX_COLUMNS:
        raise RuntimeError(f"a record of {S} bytes / {len(columns)} columns is beyond the unpack kernel's {MAX_RECORD} / {MAX_COLUMNS} (include/radegs.h)")
    table = np.zeros(len(columns), dtype=_COLUMN)
    for k, (dst, elem, offset, code, scale) in enumerate(sorted(columns, key=lambda c: (c[0].data_ptr(), c[1]))):
        table[k] = (dst.data_ptr(), dst.stride(0), elem, offset, TYPE_CODES[code], int(bool(scale)))
    return torch.from_numpy(table.view(np.uint8)).to(dev)


def _launch_unpack(records, P, S, D, table, dev):
    gh.call(_SIGNATURES, "radegs_modelio_unpack", dev, P, S, records, D, table)


def _upload(records, dev):
    return records.to(dev, non_blocking=True)


@torch.no_grad()
def read_vertex_columns(path, names, scale=None, device="cuda"):
    """float32 [P, len(names)]: the named properties of the `vertex` element, whatever their type and place in the record; properties not
    asked for are skipped.  scale: None, or one bool per name: the value divided by 255 in float64 before the one rounding to float32."""
    header = read_ply_header(path)
    el = _vertex(header)[0]
    have = dict(el.properties)
    for n in names:
        if n not in have:
            raise RuntimeError(f"{path}: `vertex` has no property `{n}`")
    scale = [False] * len(names) if scale is None else list(scale)
    if len(scale) != len(names):
        raise RuntimeError("`scale` must have one entry per name")
    buf, P, S, layout = _read_records(path, header)
    dev = _device(device)
    out = torch.empty((P, len(names)), dtype=torch.float32, device=dev)
    _unpack(_upload(buf, dev), P, S, [(out, j, layout[n][0], layout[n][1], scale[j]) for j, n in enumerate(names)], dev)
    return out


# ------------------------------------------------------------------------------ model ------------------------------------------------------------------------------
def _state(xyz, features_dc, features_rest, opacity, scaling, rotation, filter_3D):
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2:
        raise RuntimeError("`xyz` must be a tensor of shape (P,3)")
    if not isinstance(features_rest, torch.Tensor) or features_rest.dim() != 3:
        raise RuntimeError("`features_rest` must be a tensor of shape (P,K,3)")
    P, K = xyz.shape[0], features_rest.shape[1]
    if K > MAX_REST:
        raise RuntimeError(f"`features_rest` has {K} coefficients, the pack kernel takes at most {MAX_REST} (include/radegs.h)")
    x = _rows(xyz, "xyz", P, (3,))
    dev = x.device
    t = [x, _rows(features_dc, "features_dc", P, (1, 3), dev), _rows(features_rest, "features_rest", P, (K, 3), dev),
         _rows(opacity, "opacity", P, (1,), dev), _rows(scaling, "scaling", P, (3,), dev), _rows(rotation, "rotation", P, (4,), dev),
         None if filter_3D is None else _rows(filter_3D, "filter_3D", P, (1,), dev)]
    return t, P, K, dev


def _pack(t, P, K, begin, end, out, dev):
    gh.call(_SIGNATURES, "radegs_modelio_pack", dev, P, begin, end, K, *t, out)


@torch.no_grad()
def pack_records(xyz, features_dc, features_rest, opacity, scaling, rotation, filter_3D=None, row_begin=0, row_end=None):
    """float32 [row_end - row_begin, C] on the device: the records of save_ply's payload for those rows, C = 17 + 3 K (+ 1 with the filter)"""
    t, P, K, dev = _state(xyz, features_dc, features_rest, opacity, scaling, rotation, filter_3D)
    row_end = P if row_end is None else row_end
    if not (0 <= row_begin <= row_end <= P):
        raise RuntimeError(f"rows [{row_begin}, {row_end}) are outside the {P} rows")
    out = torch.empty((row_end - row_begin, 17 + 3 * K + (filter_3D is not None)), dtype=torch.float32, device=dev)
    _pack(t, P, K, row_begin, row_end, out, dev)
    return out


def _mkdir_p(path):
    folder = os.path.dirname(path)
    if folder:
        os.makedirs(folder, exist_ok=True)


@torch.no_grad()
def save_ply(path, xyz, features_dc, features_rest, opacity, scaling, rotation, filter_3D=None, chunk_rows=None):
    """GaussianModel.save_ply: the file plyfile writes for upstream's structured array -- one `vertex` element of float properties in
    construct_list_of_attributes' order, binary little-endian.  Packed on the device `chunk_rows` rows at a time, copied into one of two
    pinned buffers and written while the next chunk is packed."""
    t, P, K, dev = _state(xyz, features_dc, features_rest, opacity, scaling, rotation, filter_3D)
    chunk_rows = DEFAULT_CHUNK_ROWS if chunk_rows is None else chunk_rows
    if isinstance(chunk_rows, bool) or not isinstance(chunk_rows, int) or chunk_rows < 1:
        raise RuntimeError("`chunk_rows` must be a positive integer")
    C = 17 + 3 * K + (filter_3D is not None)
    _mkdir_p(path)
    with open(path, "wb") as f:
        f.write(ply_header(P, [(n, "f4") for n in attribute_names(3 * K, filter_3D is not None)]))
        if P == 0:
            return
        rows = min(chunk_rows, P)
        device_buf = [torch.empty((rows, C), dtype=torch.float32, device=dev) for _ in range(2)]
        pinned = [torch.empty((rows, C), dtype=torch.float32, pin_memory=True) for _ in range(2)]
        ready = [torch.cuda.Event() for _ in range(2)]
        pending = None
        with torch.cuda.device(dev):
            for k, begin in enumerate(range(0, P, rows)):
                b, n = k & 1, min(rows, P - begin)
                _pack(t, P, K, begin, begin + n, device_buf[b], dev)
                pinned[b][:n].copy_(device_buf[b][:n], non_blocking=True)
                ready[b].record()
                if pending is not None:
                    ready[pending[0]].synchronize()
                    f.write(pinned[pending[0]].numpy()[:pending[1]])
                pending = (b, n)
            ready[pending[0]].synchronize()
            f.write(pinned[pending[0]].numpy()[:pending[1]])


def _numbered(have, prefix, path):
    names = [n for n in have if n.startswith(prefix)]
    try:
        return sorted(names, key=lambda n: int(n.split("_")[-1]))
    except ValueError:
        raise RuntimeError(f"{path}: a `{prefix}*` property without a numeric suffix among {names}") from None


@torch.no_grad()
def load_ply(path, max_sh_degree=None, require_filter=True, device="cuda"):
    """GaussianModel.load_ply: GaussianState of the seven tensors in the model's own shapes, every value written to its final place by the
    unpack kernel.  f_rest_*, scale_* and rot_* are ordered by their numeric suffix; the f_rest count must be 3 (d + 1)^2 - 3 for
    `max_sh_degree` = d, or, without one, for some integer d.  With require_filter=False a file without `filter_3D` gives filter_3D None."""
    header = read_ply_header(path)
    have = dict(_vertex(header)[0].properties)
    for n in ("x", "y", "z", "opacity", "f_dc_0", "f_dc_1", "f_dc_2"):
        if n not in have:
            raise RuntimeError(f"{path}: `vertex` has no property `{n}`")
    with_filter = "filter_3D" in have
    if require_filter and not with_filter:
        raise RuntimeError(f"{path}: `vertex` has no property `filter_3D` (pass require_filter=False to load without it)")
    rest, scales, rots = _numbered(have, "f_rest_", path), _numbered(have, "scale_", path), _numbered(have, "rot", path)
    n_rest = len(rest)
    if max_sh_degree is None:
        d = int(round(((n_rest + 3) / 3) ** 0.5)) - 1
        if d < 0 or 3 * (d + 1) ** 2 - 3 != n_rest:
            raise RuntimeError(f"{path}: {n_rest} f_rest_* properties are not 3 (d + 1)^2 - 3 for any SH degree d")
    elif 3 * (max_sh_degree + 1) ** 2 - 3 != n_rest:
        raise RuntimeError(f"{path}: {n_rest} f_rest_* properties, SH degree {max_sh_degree} needs {3 * (max_sh_degree + 1) ** 2 - 3}")
    if len(scales) != 3 or len(rots) != 4:
        raise RuntimeError(f"{path}: {len(scales)} scale_* and {len(rots)} rot_* properties, the model has 3 and 4")
    K = n_rest // 3
    buf, P, S, layout = _read_records(path, header)
    dev = _device(device)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
    st = GaussianState(new(P, 3), new(P, 1, 3), new(P, K, 3), new(P, 1), new(P, 3), new(P, 4), new(P, 1) if with_filter else None)
    cols = [(st.xyz, j, n) for j, n in enumerate("xyz")] + [(st.features_dc, j, f"f_dc_{j}") for j in range(3)] + [(st.opacity, 0, "opacity")]
    cols += [(st.features_rest, (j % K) * 3 + j // K, n) for j, n in enumerate(rest)]         # f_rest_j -> [j % K][j // K]
    cols += [(st.scaling, j, n) for j, n in enumerate(scales)] + [(st.rotation, j, n) for j, n in enumerate(rots)]
    if with_filter:
        cols.append((st.filter_3D, 0, "filter_3D"))
    _unpack(_upload(buf, dev), P, S, [(dst, elem) + layout[n] + (False,) for dst, elem, n in cols], dev)
    return st


# --------------------------------------------------------------------------- point clouds ---------------------------------------------------------------------------
_POINTS3D = [("x", "f4"), ("y", "f4"), ("z", "f4"), ("nx", "f4"), ("ny", "f4"), ("nz", "f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]


@torch.no_grad()
def fetch_ply(path, device="cuda"):
    """dataset_readers.py:156-162 fetchPly: PointCloud(points, colors = colours / 255, normals), float32 [P,3] each on the device.  The
    quotient is taken in float64 and rounded once, as upstream's float64 colours are when create_from_pcd makes them float."""
    names = [n for n, _ in _POINTS3D]
    t = read_vertex_columns(path, names[:3] + names[6:] + names[3:6], scale=[False] * 3 + [True] * 3 + [False] * 3, device=device)
    return PointCloud(t[:, 0:3].contiguous(), t[:, 3:6].contiguous(), t[:, 6:9].contiguous())


def store_ply(path, xyz, rgb):
    """dataset_readers.py:174-189 storePly: x y z, zero normals, red green blue as 27-byte records.  A host routine, as upstream's: the file
    is written once per scene.  `rgb`: uint8, or floats in [0, 256), truncated as numpy's cast to u1 truncates; anything else is refused."""
    xyz = np.asarray(xyz.detach().cpu() if isinstance(xyz, torch.Tensor) else xyz)
    rgb = np.asarray(rgb.detach().cpu() if isinstance(rgb, torch.Tensor) else rgb)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.dtype.kind != "f" or rgb.shape != xyz.shape:
        raise RuntimeError("`xyz` must be a float array of shape (P,3) and `rgb` have the same shape")
    if rgb.dtype != np.uint8:
        if rgb.dtype.kind != "f" or not bool(np.all((rgb >= 0) & (rgb < 256))):
            raise RuntimeError("`rgb` must be uint8, or floats in [0, 256)")
        rgb = rgb.astype(np.uint8)
    rec = np.zeros(xyz.shape[0], dtype=np.dtype([(n, "<" + t) for n, t in _POINTS3D]))
    for j, n in enumerate("xyz"):
        rec[n] = xyz[:, j]
    for j, n in enumerate(("red", "green", "blue")):
        rec[n] = rgb[:, j]
    with open(path, "wb") as f:
        f.write(ply_header(xyz.shape[0], _POINTS3D))
        f.write(rec.tobytes())


# ----------------------------------------------------------------------- the two per-Gaussian steps -----------------------------------------------------------------------
def initial_opacity():
    """inverse_sigmoid(0.1 * ones) in float32, computed once on the host"""
    p = np.float32(0.1) * np.float32(1.0)
    return float(np.log(p / (np.float32(1.0) - p), dtype=np.float32))


@torch.no_grad()
def init_from_points(points, colors, max_sh_degree, dist2=None):
    """create_from_pcd after the upload (gaussian_model.py:305-327): GaussianState (filter_3D None) from points [P,3] and colors [P,3] in
    [0, 1].  dist2 [P]: distCUDA2's result, computed here when None."""
    if isinstance(max_sh_degree, bool) or not isinstance(max_sh_degree, int) or max_sh_degree < 0 or (max_sh_degree + 1) ** 2 - 1 > MAX_REST:
        raise RuntimeError(f"`max_sh_degree` must be an integer with at most {MAX_REST} rest coefficients")
    if not isinstance(points, torch.Tensor) or points.dim() != 2:
        raise RuntimeError("`points` must be a tensor of shape (P,3)")
    P, K = points.shape[0], (max_sh_degree + 1) ** 2 - 1
    pts = _rows(points, "points", P, (3,))
    dev = pts.device
    col = _rows(colors, "colors", P, (3,), dev)
    if dist2 is None:
        from simple_knn._C import distCUDA2
        dist2 = distCUDA2(pts)
    d2 = _rows(dist2, "dist2", P, (), dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
    st = GaussianState(pts.clone(), new(P, 1, 3), new(P, K, 3), new(P, 1), new(P, 3), new(P, 4), None)
    gh.call(_SIGNATURES, "radegs_modelio_init", dev, P, K, col, d2, initial_opacity(), st.features_dc, st.features_rest, st.opacity, st.scaling, st.rotation)
    return st


@torch.no_grad()
def reset_opacity(opacity_raw, scaling_raw, filter_3D, zero_moments=False):
    """GaussianModel.reset_opacity's new raw opacity [P,1] (gaussian_model.py:495-510) in one pass.  zero_moments: also returns two
    zero-filled tensors of the same shape, written by the same kernel (the opacity's Adam moments after the reset)."""
    if not isinstance(opacity_raw, torch.Tensor) or opacity_raw.dim() != 2:
        raise RuntimeError("`opacity_raw` must be a tensor of shape (P,1)")
    P = opacity_raw.shape[0]
    op = _rows(opacity_raw, "opacity_raw", P, (1,))
    dev = op.device
    sc, f3 = _rows(scaling_raw, "scaling_raw", P, (3,), dev), _rows(filter_3D, "filter_3D", P, (1,), dev)
    out = torch.empty_like(op)
    m, v = (torch.empty_like(op), torch.empty_like(op)) if zero_moments else (None, None)
    gh.call(_SIGNATURES, "radegs_modelio_reset_opacity", dev, P, op, sc, f3, out, m, v)
    return (out, m, v) if zero_moments else out


# ----------------------------------------------------------------- GaussianModel's methods, by upstream's names -----------------------------------------------------------------
_PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def _set_parameters(model, st):
    for attr, t in zip(_PARAMS, st[:6]):
        setattr(model, attr, torch.nn.Parameter(t.requires_grad_(True)))


def save_model_ply(model, path):
    """GaussianModel.save_ply(path)"""
    save_ply(path, model._xyz, model._features_dc, model._features_rest, model._opacity, model._scaling, model._rotation, model.filter_3D)


def load_model_ply(model, path):
    """GaussianModel.load_ply(path): the six Parameters, filter_3D, and active_sh_degree = max_sh_degree"""
    st = load_ply(path, max_sh_degree=model.max_sh_degree)
    _set_parameters(model, st)
    model.filter_3D = st.filter_3D
    model.active_sh_degree = model.max_sh_degree


def create_from_pcd(model, pcd, spatial_lr_scale):
    """GaussianModel.create_from_pcd(pcd, spatial_lr_scale): pcd has `points` and `colors` (or `_xyz` and `_rgb`, as upstream's other branch),
    arrays or tensors; what is not already a float32 GPU tensor is uploaded as upstream's torch.tensor(np.asarray(.)).float().cuda() does."""
    model.spatial_lr_scale = spatial_lr_scale
    points, colors = (pcd.points, pcd.colors) if hasattr(pcd, "points") else (pcd._xyz, pcd._rgb)

    def up(a):
        return a if isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 else torch.tensor(np.asarray(a)).float().cuda()
    points = up(points).contiguous()
    print("Number of points at initialisation : ", points.shape[0])
    st = init_from_points(points, up(colors).contiguous(), model.max_sh_degree)
    _set_parameters(model, st)
    model.max_radii2D = torch.zeros((points.shape[0]), device=points.device)


def reset_model_opacity(model):
    """GaussianModel.reset_opacity(): the `opacity` optimizer group gets a new Parameter and its state moves to it with zeroed moments
    (replace_tensor_to_optimizer, gaussian_model.py:561-576)."""
    new, m, v = reset_opacity(model._opacity, model._scaling, model.filter_3D, zero_moments=True)
    for group in model.optimizer.param_groups:
        if group["name"] == "opacity":
            old = group["params"][0]
            state = model.optimizer.state.get(old, None)
            state["exp_avg"], state["exp_avg_sq"] = m, v
            del model.optimizer.state[old]
            group["params"][0] = torch.nn.Parameter(new.requires_grad_(True))
            model.optimizer.state[group["params"][0]] = state
            model._opacity = group["params"][0]
