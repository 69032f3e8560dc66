"""Evaluation from files: the step from the files of a geometry evaluation to the tensors tnt_eval, tnt_cull and mesh_eval
take.  Geometry PLYs (what upstream hands to o3d.io.read_point_cloud and trimesh.load) go to float64 / int64 GPU tensors through two HIP
kernels; the small text files (trajectories, the mapping, _trans.txt, the DTU calibration) are read on the host into numpy float64, value
for value as the reference's own readers return them (tests/test_evalio_restatement.py holds them to the reference's output).  include/radegs.h,
"Evaluation from files", is the specification of the kernels and tests/evalio_restatement.py restates them in NumPy.  Open3D, trimesh and cv2
are never imported: their rules are restated, those from memory are marked in DESIGN 11 N18."""
import ctypes
import os
import re

import numpy as np
import torch

import geom_host as gh
import model_io
from diff_gaussian_rasterization import _C
from geom_host import f64, i32, ll, vp

SIGNATURES = {
    "radegs_evalio_unpack_points": (i32, [ll, i32, vp, ll, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), vp, vp]),
    "radegs_evalio_unpack_faces": (i32, [ll, i32, vp, ll, i32, i32, i32, i32, ll, vp, vp, vp]),
    "radegs_evalio_ransac": (i32, [ll, vp, vp, f64, i32, ll, ctypes.c_ulonglong, vp, vp, vp, vp]),
}
_SIGNATURES = SIGNATURES
MAX_RECORD = model_io.MAX_RECORD                      # RADEGS_MODELIO_MAX_RECORD: the unpack kernels' record size
RANSAC_CHUNK, RANSAC_MIN_N, RANSAC_MAX_N = 256, 3, 8  # RADEGS_EVALIO_RANSAC_* (include/radegs.h)
FACE_LISTS = ("vertex_indices", "vertex_index")
_INTS3 = ctypes.c_int * 3


def _lib():
    return gh.bind(_SIGNATURES)


# ------------------------------------------------------------------------- PLY layout -------------------------------------------------------------------------
def _size(t):
    return np.dtype(t).itemsize


def _is_list(t):
    return isinstance(t, tuple)


def _header(path):
    """model_io.read_ply_header, and the version of the `format` line, which that reader does not look at"""
    header = model_io.read_ply_header(path)
    with open(path, "rb") as f:
        head = f.read(header.data_offset)
    line = re.search(rb"(?:^|\n)\s*format[ \t]+(\S+)[ \t]+(\S+)[ \t]*\r?\n", head)
    if line is None or line.group(2) != b"1.0":
        raise RuntimeError(f"{path}: its `format` line is none of the three of PLY 1.0 ({', '.join(f + ' 1.0' for f in model_io.FORMATS)})")
    return header


def _vertex_layout(path, header):
    """(index of `vertex` among the elements, {x, y, z: (byte offset, numpy code)}, record size)"""
    k = [el.name for el in header.elements].index("vertex")
    props = header.elements[k].properties
    have = dict(props)
    for n in "xyz":
        if n not in have:
            raise RuntimeError(f"{path}: `vertex` has no property `{n}`")
    offsets, at = {}, 0
    for n, t in props:
        offsets[n] = (at, t)
        at += _size(t)
    if at > MAX_RECORD:
        raise RuntimeError(f"{path}: a `vertex` record of {at} bytes is beyond the unpack kernel's {MAX_RECORD} (include/radegs.h)")
    return k, {n: offsets[n] for n in "xyz"}, at


def _skipped(path, el):
    """(bytes, values) of an element that is stepped over"""
    for n, t in el.properties:
        if _is_list(t):
            raise RuntimeError(f"{path}: list property `{n}` of element `{el.name}`, which must be skipped: its records have no fixed size")
    return el.count * sum(_size(t) for _, t in el.properties), el.count * len(el.properties)


def _face_layout(path, header, kv):
    """(index of `face`, record size, byte offset and numpy code of the list length, byte offset and numpy code of the three indices)"""
    names = [el.name for el in header.elements]
    if "face" not in names[kv + 1:]:
        raise RuntimeError(f"{path}: no `face` element after `vertex`")
    kf = names.index("face", kv + 1)
    lists = [(n, t) for n, t in header.elements[kf].properties if _is_list(t)]
    if len(lists) != 1 or lists[0][0] not in FACE_LISTS:
        raise RuntimeError(f"{path}: `face` must hold exactly one list property, named one of {FACE_LISTS}; it holds {[n for n, _ in lists]}")
    _, (_, ct, it) = lists[0]
    if ct[0] == "f" or ct == "f8":
        raise RuntimeError(f"{path}: the list length of `{lists[0][0]}` is of type {ct}, not an integer")
    if it not in ("i4", "u4"):
        raise RuntimeError(f"{path}: the indices of `{lists[0][0]}` are of type {it}; int32 and uint32 are read")
    at, count_offset = 0, None
    for n, t in header.elements[kf].properties:
        if _is_list(t):
            count_offset = at
            at += _size(ct) + 3 * 4
        else:
            at += _size(t)
    if at > MAX_RECORD:
        raise RuntimeError(f"{path}: a `face` record of {at} bytes is beyond the unpack kernel's {MAX_RECORD} (include/radegs.h)")
    return kf, at, count_offset, ct, count_offset + _size(ct), it


def _pinned(nbytes):
    """a host buffer the kernels' reads stay inside: padded to a multiple of 4 and by 8 more, the padding zeroed"""
    t = torch.empty((nbytes + 3) // 4 * 4 + 8, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    t.numpy()[nbytes:] = 0
    return t


def _read_bytes(path, begin, nbytes):
    buf = _pinned(nbytes)
    with open(path, "rb") as f:
        f.seek(begin)
        got = f.readinto(memoryview(buf.numpy())[:nbytes]) if nbytes else 0
    if got != nbytes:
        raise RuntimeError(f"{path}: truncated: read {got} of {nbytes} bytes")
    return buf


# --------------------------------------------------------------------------- kernels ---------------------------------------------------------------------------
def unpack_points(buffer, byte_offset, N, S, columns):
    """radegs_evalio_unpack_points: `buffer` a uint8 GPU tensor holding N records of S bytes from `byte_offset`, padded as the header asks;
    `columns` three (byte offset, numpy code).  Returns float64 [N,3]."""
    _C._require_gpu(buffer, "buffer")
    if buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous():
        raise RuntimeError("`buffer` must be a contiguous uint8 vector")
    if N < 0 or S < 1 or byte_offset < 0 or (byte_offset + N * S + 3) // 4 * 4 > buffer.numel():
        raise RuntimeError(f"{N} records of {S} bytes from byte {byte_offset} leave the buffer of {buffer.numel()} bytes (padded to a multiple of 4)")
    if len(columns) != 3 or any(t not in model_io.TYPE_CODES or o < 0 or o + _size(t) > S for o, t in columns):
        raise RuntimeError("`columns` must be three (offset, type) pairs inside the record")
    dev = buffer.device
    out = torch.empty((N, 3), dtype=torch.float64, device=dev)
    gh.call(_SIGNATURES, "radegs_evalio_unpack_points", dev, N, S, buffer, byte_offset, _INTS3(*[o for o, _ in columns]),
            _INTS3(*[model_io.TYPE_CODES[t] for _, t in columns]), out)
    return out


def unpack_faces(buffer, byte_offset, F, S, count_offset, count_type, index_offset, index_type, V):
    """radegs_evalio_unpack_faces.  Returns (faces int64 [F,3], bad): `bad` a one-element int32 GPU tensor, the number of refused records."""
    _C._require_gpu(buffer, "buffer")
    if buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous():
        raise RuntimeError("`buffer` must be a contiguous uint8 vector")
    if F < 0 or S < 1 or byte_offset < 0 or (byte_offset + F * S + 3) // 4 * 4 > buffer.numel():
        raise RuntimeError(f"{F} records of {S} bytes from byte {byte_offset} leave the buffer of {buffer.numel()} bytes (padded to a multiple of 4)")
    if count_type not in ("i1", "u1", "i2", "u2", "i4", "u4") or index_type not in ("i4", "u4"):
        raise RuntimeError("the list length must be an integer of up to 32 bits and the indices int32 or uint32")
    if count_offset < 0 or count_offset + _size(count_type) > S or index_offset < 0 or index_offset + 12 > S:
        raise RuntimeError("the list leaves the record")
    dev = buffer.device
    faces = torch.empty((F, 3), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    gh.call(_SIGNATURES, "radegs_evalio_unpack_faces", dev, F, S, buffer, byte_offset, count_offset, model_io.TYPE_CODES[count_type], index_offset,
            model_io.TYPE_CODES[index_type], V, faces, bad)
    return faces, bad


# --------------------------------------------------------------------------- readers ---------------------------------------------------------------------------
@torch.no_grad()
def read_ply_points(path, device="cuda"):
    """o3d.io.read_point_cloud(path).points: float64 [N,3] on the GPU, `x y z` of the `vertex` element whatever their type and place in the
    record; every other property and every later element is ignored.  float is widened exactly, double copied bit for bit."""
    header = _header(path)
    kv, xyz, S = _vertex_layout(path, header)
    N = header.elements[kv].count
    if header.format != "binary_little_endian":
        records, N, S, layout = model_io._read_records(path, header)     # the host decode of ascii and big-endian files
        return unpack_points(records.to(model_io._device(device), non_blocking=True), 0, N, S, [layout[n] for n in "xyz"])
    begin = header.data_offset + sum(_skipped(path, el)[0] for el in header.elements[:kv])
    if os.path.getsize(path) - begin < N * S:
        raise RuntimeError(f"{path}: truncated: {max(os.path.getsize(path) - begin, 0)} bytes where {N} `vertex` records of {S} bytes need {N * S}")
    buf = _read_bytes(path, begin, N * S)
    return unpack_points(buf.to(model_io._device(device), non_blocking=True), 0, N, S, [xyz[n] for n in "xyz"])


def _host_faces(path, header, kv, kf, F, S, ct, it):
    """the `face` element of a big-endian or ascii file as little-endian records of the same layout"""
    face = header.elements[kf]
    fields = lambda e: [(f"p{j}", e + t) if not _is_list(t) else (f"p{j}", [("n", e + ct), ("v", e + it, (3,))])   # noqa: E731
                        for j, (_, t) in enumerate(face.properties)]
    little = np.dtype(fields("<"))
    assert little.itemsize == S
    before = [_skipped(path, el) for el in header.elements[:kf]]
    after = [_skipped(path, el) for el in header.elements[kf + 1:]]
    if header.format == "binary_big_endian":
        begin = header.data_offset + sum(b for b, _ in before)
        have = os.path.getsize(path) - begin - sum(b for b, _ in after)
        _face_bytes(path, have, F, S)
        with open(path, "rb") as f:
            f.seek(begin)
            rec = np.frombuffer(f.read(F * S), dtype=np.dtype(fields(">"))).astype(little)
    else:
        with open(path, "rb") as f:
            f.seek(header.data_offset)
            tokens = f.read().split()
        per = len(face.properties) + 3
        skip, tail = sum(v for _, v in before), sum(v for _, v in after)
        have = len(tokens) - skip - tail
        if have != F * per:
            raise RuntimeError(f"{path}: the `face` element holds {max(have, 0)} values where {F} triangles need {F * per}: the file is truncated "
                               "or a face is not a triangle")
        table = np.array(tokens[skip:skip + F * per]).reshape(F, per)
        rec, col = np.zeros(F, dtype=little), 0
        for j, (_, t) in enumerate(face.properties):
            if _is_list(t):
                rec[f"p{j}"]["n"] = _ascii_column(table[:, col], ct)
                for k in range(3):
                    rec[f"p{j}"]["v"][:, k] = _ascii_column(table[:, col + 1 + k], it)
                col += 4
            else:
                rec[f"p{j}"] = _ascii_column(table[:, col], t)
                col += 1
    buf = _pinned(F * S)
    buf.numpy()[:F * S] = rec.view(np.uint8).reshape(-1)
    return buf


def _ascii_column(column, t):
    return column.astype(np.float64).astype(t) if t[0] == "f" else np.array([int(v) for v in column], dtype=np.int64).astype(t)


def _face_bytes(path, have, F, S):
    if have < F * S:
        raise RuntimeError(f"{path}: truncated: the `face` element holds {max(have, 0)} bytes where {F} triangles of {S} bytes need {F * S}")
    if have != F * S:
        raise RuntimeError(f"{path}: the `face` element holds {have} bytes where {F} triangles of {S} bytes need {F * S}: a face is not a triangle")


@torch.no_grad()
def read_ply_mesh(path, device="cuda"):
    """trimesh.load(path, process=False): (vertices float64 [V,3], faces int64 [F,3]) on the GPU.  A binary little-endian file is uploaded
    once and decoded there: the faces are read as records of one fixed size (the list length, three indices, and whatever scalar properties
    stand before and after), which holds iff every face is a triangle -- the host checks that the element has exactly F such records'
    bytes and the kernel that every length is 3 and every index in [0, V).  Anything else is a RuntimeError."""
    header = _header(path)
    kv, xyz, Sv = _vertex_layout(path, header)
    kf, Sf, count_offset, ct, index_offset, it = _face_layout(path, header, kv)
    V, F = header.elements[kv].count, header.elements[kf].count
    els = header.elements
    if header.format == "binary_little_endian":
        sizes = [V * Sv if k == kv else F * Sf if k == kf else _skipped(path, el)[0] for k, el in enumerate(els)]
        payload = os.path.getsize(path) - header.data_offset
        begin_v, begin_f = sum(sizes[:kv]), sum(sizes[:kf])
        if payload < begin_v + V * Sv:
            raise RuntimeError(f"{path}: truncated: {max(payload - begin_v, 0)} bytes where {V} `vertex` records of {Sv} bytes need {V * Sv}")
        _face_bytes(path, payload - begin_f - sum(sizes[kf + 1:]), F, Sf)
        buf = _read_bytes(path, header.data_offset, payload).to(model_io._device(device), non_blocking=True)        # the one upload
        vertices = unpack_points(buf, begin_v, V, Sv, [xyz[n] for n in "xyz"])
        faces, bad = unpack_faces(buf, begin_f, F, Sf, count_offset, ct, index_offset, it, V)
    else:
        for el in els[kv + 1:kf] + els[kf + 1:]:
            _skipped(path, el)
        records, V, Sv, layout = model_io._read_records(path, header)
        face_records = _host_faces(path, header, kv, kf, F, Sf, ct, it)
        dev = model_io._device(device)
        vertices = unpack_points(records.to(dev, non_blocking=True), 0, V, Sv, [layout[n] for n in "xyz"])
        faces, bad = unpack_faces(face_records.to(dev, non_blocking=True), 0, F, Sf, count_offset, ct, index_offset, it, V)
    n_bad = int(bad.item())                          # the one host read
    if n_bad:
        raise RuntimeError(f"{path}: {n_bad} of the {F} `face` records are not a triangle of indices in [0, {V}): a list length other than 3 "
                           "(the records then have no fixed size) or an index outside the vertices")
    return vertices, faces


@torch.no_grad()
def merge_vertices(vertices, faces, digits=8):
    """trimesh.load(process=True) followed by merge_vertices(): drops the vertices with a non-finite coordinate and their faces, welds the
    vertices whose round(v 10^digits) rows are equal (the first of them stays), keeps the referenced vertices only and renumbers the faces,
    which keep their order.  Vertices come out in first-occurrence order (trimesh: by a hash).  torch plumbing: not a hot path."""
    if isinstance(digits, bool) or not isinstance(digits, int) or not 0 <= digits <= 15:
        raise RuntimeError("`digits` must be an integer in [0, 15]")
    v = gh.points(vertices, "vertices")
    gh.faces_type(faces)
    f = gh.faces(faces, v.shape[0])
    if f.device != v.device:
        raise RuntimeError("`vertices` and `faces` must be on the same device")
    dev, V = v.device, v.shape[0]
    finite = torch.isfinite(v).all(dim=1)
    f = f[finite[f].all(dim=1)] if f.shape[0] else f
    index = finite.nonzero().squeeze(1)
    if f.shape[0] == 0:                                # no face: no referenced vertex
        return torch.empty((0, 3), dtype=torch.float64, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev)
    keys = torch.round(v[index] * float(10 ** digits))
    _, inverse = torch.unique(keys, dim=0, return_inverse=True)
    G = int(inverse.max()) + 1
    first = torch.full((G,), V, dtype=torch.int64, device=dev).scatter_reduce(0, inverse, index, "amin")
    group = torch.full((V,), -1, dtype=torch.int64, device=dev)
    group[index] = inverse
    fg = group[f]
    used = torch.zeros(G, dtype=torch.bool, device=dev)
    used[fg.reshape(-1)] = True
    kept = used.nonzero().squeeze(1)
    kept = kept[torch.argsort(first[kept])]
    new = torch.full((G,), -1, dtype=torch.int64, device=dev)
    new[kept] = torch.arange(kept.numel(), dtype=torch.int64, device=dev)
    return v[first[kept]].contiguous(), new[fg].contiguous()


# ------------------------------------------------------------------- trajectories and small files -------------------------------------------------------------------
def _row(line, n, path):
    try:
        row = np.array(line.split(), dtype=np.float64)
    except ValueError:
        row = None
    if row is None or row.shape != (n,):
        raise RuntimeError(f"{path}: a row of {n} numbers expected, got `{line.strip()}`")
    return row


def read_trajectory(path):
    """trajectory_io.read_trajectory: (poses float64 [B,4,4], metadata: one list of ints per pose) of a .log file -- per pose one line of
    integers, then four rows of four numbers"""
    poses, meta = [], []
    with open(path, "r") as f:
        head = f.readline()
        while head:
            try:
                meta.append([int(w) for w in head.split()])
            except ValueError:
                raise RuntimeError(f"{path}: a line of integers expected before a pose, got `{head.strip()}`") from None
            poses.append(np.stack([_row(f.readline(), 4, path) for _ in range(4)]))
            head = f.readline()
    return np.array(poses, dtype=np.float64).reshape(-1, 4, 4), meta


def read_mapping(path):
    """registration.read_mapping: (n_sampled_frames, n_total_frames, mapping float64 [n_sampled_frames,2])"""
    with open(path, "r") as f:
        try:
            n_sampled, n_total = int(f.readline()), int(f.readline())
        except ValueError:
            raise RuntimeError(f"{path}: two lines with one integer each expected first") from None
        mapping = np.zeros((n_sampled, 2))
        for k in range(n_sampled):
            words = f.readline().split()
            try:
                mapping[k, :] = [int(w) for w in words]
            except ValueError:
                raise RuntimeError(f"{path}: two integers expected for frame {k}, got `{' '.join(words)}`") from None
    return n_sampled, n_total, mapping


def gen_sparse_trajectory(mapping, traj):
    """registration.gen_sparse_trajectory: the poses traj[mapping[:, 1] - 1]"""
    traj = np.asarray(traj)
    idx = np.array([int(m[1] - 1) for m in np.asarray(mapping)], dtype=np.int64)
    if idx.size and (idx.min() < -traj.shape[0] or idx.max() >= traj.shape[0]):
        raise RuntimeError(f"the mapping names frame {int(idx.max()) + 1} of a trajectory of {traj.shape[0]} poses")
    return traj[idx]


def get_traj(path):
    """cull_mesh.get_traj: camera-to-world poses [B,4,4] from a .npy stack or a .log file, each rounded through float32 as upstream's
    `.float()` does (returned as float64); a 3x4 pose gets the row (0, 0, 0, 1).  Upstream's .json branch (auto_orient_and_center_poses) is
    not restated and is refused."""
    if path.endswith(".json"):
        raise RuntimeError(f"{path}: the .json branch of get_traj (auto_orient_and_center_poses) is not supported; pass a .npy stack or a .log file")
    if path.endswith(".npy"):
        poses = np.load(path)
    else:
        poses = read_trajectory(path)[0]
    poses = np.asarray(poses)
    if poses.ndim != 3 or poses.shape[1:] not in ((4, 4), (3, 4)):
        raise RuntimeError(f"{path}: a stack of 4x4 or 3x4 poses expected, got shape {poses.shape}")
    poses = poses.astype(np.float32)
    if poses.shape[1] == 3:
        poses = np.concatenate([poses, np.broadcast_to(np.array([[0, 0, 0, 1]], np.float32), (poses.shape[0], 1, 4))], axis=1)
    return poses.astype(np.float64)


def load_transform(path):
    """run.py:114: the 4x4 of a `_trans.txt`"""
    m = np.loadtxt(path)
    if m.shape != (4, 4):
        raise RuntimeError(f"{path}: a 4x4 matrix expected, got shape {m.shape}")
    return m


def dtu_camera_centres(calib_dir, n=64):
    """The camera centres load_dtu_camera keeps (evaluate_dtu_mesh.py:60-76): of calib_dir/pos_001.txt .. pos_{n}.txt, each a 3x4 projection
    P = [M | p4] read as float32, the centre -M^-1 p4 -- what cv2.decomposeProjectionMatrix returns as t[:3] / t[3], without its RQ
    decomposition -- computed in float64 and rounded to float32, the precision upstream's pose holds it in.  Returns float32 [n,3]."""
    out = np.empty((n, 3), dtype=np.float32)
    for i in range(1, n + 1):
        fname = os.path.join(calib_dir, f"pos_{i:03d}.txt")
        P = np.loadtxt(fname, dtype=np.float32)
        if P.shape != (3, 4):
            raise RuntimeError(f"{fname}: a 3x4 projection matrix expected, got shape {P.shape}")
        P = P.astype(np.float64)
        try:
            out[i - 1] = -np.linalg.solve(P[:, :3], P[:, 3])
        except np.linalg.LinAlgError:
            raise RuntimeError(f"{fname}: the camera is at infinity (its left 3x3 block is singular)") from None
    return out


def best_fit_transform(A, B):
    """evaluate_dtu_mesh.py:16-57: (T, R, t) of the rigid motion that takes the points A [N,m] onto B in the least-squares sense"""
    A, B = np.asarray(A), np.asarray(B)
    if A.shape != B.shape or A.ndim != 2:
        raise RuntimeError("`A` and `B` must be two (N,m) arrays of the same shape")
    m = A.shape[1]
    centroid_A, centroid_B = np.mean(A, axis=0), np.mean(B, axis=0)
    H = np.dot((A - centroid_A).T, B - centroid_B)
    U, _, Vt = np.linalg.svd(H)
    R = np.dot(Vt.T, U.T)
    if np.linalg.det(R) < 0:
        Vt[m - 1, :] *= -1
        R = np.dot(Vt.T, U.T)
    t = centroid_B.T - np.dot(R, centroid_A.T)
    T = np.identity(m + 1)
    T[:m, :m], T[:m, m] = R, t
    return T, R, t


def dtu_alignment(points, gt_points):
    """evaluate_dtu_mesh.py:157-164: (scale, R, t) with scale = mean |gt - mean gt| / mean |p - mean p| written as upstream applies it --
    x -> (x scale_gt / scale_points) @ R.T + t.  Returns (scale_gt_points, scale_points, R, t); gt_points is cut to len(points)."""
    points, gt_points = np.asarray(points), np.asarray(gt_points)[:len(points)]
    scale_points = np.linalg.norm(points - points.mean(axis=0), axis=1).mean()
    scale_gt_points = np.linalg.norm(gt_points - gt_points.mean(axis=0), axis=1).mean()
    _, r, t = best_fit_transform(points * scale_gt_points / scale_points, gt_points)
    return scale_gt_points, scale_points, r, t


def load_dtu_masks(dataset_dir, scan):
    """dtu_eval/eval.py:98-99, 126: (ObsMask, BB, Res, P) of dataset_dir/ObsMask/ObsMask{scan}_10.mat and Plane{scan}.mat"""
    try:
        from scipy.io import loadmat
    except ImportError:
        raise RuntimeError("load_dtu_masks reads MATLAB files with scipy.io.loadmat and scipy is not installed: load ObsMask, BB, Res and the "
                           "plane P yourself and pass them to mesh_eval.dtu_chamfer") from None
    obs = loadmat(os.path.join(dataset_dir, "ObsMask", f"ObsMask{scan}_10.mat"))
    plane = loadmat(os.path.join(dataset_dir, "ObsMask", f"Plane{scan}.mat"))["P"]
    return obs["ObsMask"], obs["BB"], obs["Res"], plane
