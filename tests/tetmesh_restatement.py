"""Numpy restatement of the mesh-extraction steps as this library implements them (include/radegs.h, "Mesh extraction"), written
from that specification: marching tetrahedra as ONE sort over the crossing edges, get_tetra_points, one view of the cull-alpha
accumulation, one bisection step and the vertex / face filter.  CPU tier: against the fixtures the reference's own code wrote
(tests/golden/make_golden_tetmesh.py); GPU tier: what the kernels are compared with at sizes the fixtures do not reach.
All floating-point work is done in float32, one rounding per operation, in the order the header states."""
import numpy as np

# upstream's 16 x 6 triangle table and the six edges of a tet (utils/tetmesh.py:23-43), as data
TRIANGLE_TABLE = np.array([[-1, -1, -1, -1, -1, -1], [1, 0, 2, -1, -1, -1], [4, 0, 3, -1, -1, -1], [1, 4, 2, 1, 3, 4], [3, 1, 5, -1, -1, -1],
                           [2, 3, 0, 2, 5, 3], [1, 4, 0, 1, 5, 4], [4, 2, 5, -1, -1, -1], [4, 5, 2, -1, -1, -1], [4, 1, 0, 4, 5, 1],
                           [3, 2, 0, 3, 5, 2], [1, 3, 5, -1, -1, -1], [4, 1, 2, 4, 3, 1], [3, 0, 4, -1, -1, -1], [2, 0, 1, -1, -1, -1],
                           [-1, -1, -1, -1, -1, -1]], dtype=np.int64)
NUM_TRIANGLES = np.array([0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0], dtype=np.int64)
EDGE_A, EDGE_B = np.array([0, 0, 0, 1, 1, 2]), np.array([1, 2, 3, 2, 3, 3])
f32 = np.float32


def marching(vertices, tets, sdf, scales):
    """(end_points[NV,2,3], end_sdf[NV,2,1], end_scales[NV,2,1], faces int64[NF,3], interp_v int64[NV,2])"""
    vertices, sdf, scales = np.asarray(vertices, f32), np.asarray(sdf, f32).reshape(-1), np.asarray(scales, f32).reshape(-1)
    tets = np.asarray(tets).astype(np.int64).reshape(-1, 4)
    V = vertices.shape[0]
    occ = sdf > 0
    o = occ[tets] if tets.size else np.zeros((0, 4), bool)
    code = (o * np.array([1, 2, 4, 8])).sum(1)
    a, b = tets[:, EDGE_A], tets[:, EDGE_B]
    cross = o[:, EDGE_A] != o[:, EDGE_B]
    key = np.minimum(a, b) * V + np.maximum(a, b)          # ascending key = ascending lexicographic (lo, hi)
    uniq, inv = np.unique(key[cross], return_inverse=True)
    vid = np.full(tets.shape[:1] + (6,), -1, dtype=np.int64)
    vid[cross] = inv.reshape(-1)
    interp_v = np.stack([uniq // max(V, 1), uniq % max(V, 1)], axis=1).astype(np.int64).reshape(-1, 2)
    nt = NUM_TRIANGLES[code]
    one, two = nt == 1, nt == 2
    faces = np.concatenate([np.take_along_axis(vid[one], TRIANGLE_TABLE[code[one]][:, :3], axis=1).reshape(-1, 3),
                            np.take_along_axis(vid[two], TRIANGLE_TABLE[code[two]][:, :6], axis=1).reshape(-1, 3)], axis=0)
    return (vertices[interp_v.reshape(-1)].reshape(-1, 2, 3), sdf[interp_v.reshape(-1)].reshape(-1, 2, 1),
            scales[interp_v.reshape(-1)].reshape(-1, 2, 1), faces, interp_v)


BOX_CORNERS = np.array([[(1 if j & 4 else -1), (1 if j & 2 else -1), (1 if j & 1 else -1)] for j in range(8)], dtype=f32)


def tetra_points(xyz, scales3, rotation_raw):
    """(points[9P,3], scale[9P,1])"""
    xyz, s, q = np.asarray(xyz, f32), np.asarray(scales3, f32) * f32(3.0), np.asarray(rotation_raw, f32)
    norm = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    r, x, y, z = (q[:, k] / norm for k in range(4))
    one, two = f32(1.0), f32(2.0)
    R = np.stack([np.stack([one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)], 1),
                  np.stack([two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)], 1),
                  np.stack([two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)], 1)], 1)     # [P,3,3]
    box = BOX_CORNERS[None, :, :] * s[:, None, :]                                                                   # [P,8,3]
    corners = ((R[:, None, :, 0] * box[:, :, None, 0] + R[:, None, :, 1] * box[:, :, None, 1]) + R[:, None, :, 2] * box[:, :, None, 2]) + xyz[:, None, :]
    smax = np.maximum(np.maximum(s[:, 0], s[:, 1]), s[:, 2])
    return (np.concatenate([corners.reshape(-1, 3), xyz], 0).astype(f32), np.concatenate([np.repeat(smax, 8), smax]).reshape(-1, 1).astype(f32))


def sample_mask(coord, mask):
    """grid_sample(bilinear, align_corners=False, zero padding) of mask[H,W] at pixel coordinates coord[PN,2], as the header states it"""
    H, W = mask.shape
    mask = np.asarray(mask, f32)
    px, py = np.asarray(coord, f32)[:, 0], np.asarray(coord, f32)[:, 1]
    one, two = f32(1.0), f32(2.0)
    gx, gy = (px * two + one) / f32(W - 1) - one, (py * two + one) / f32(H - 1) - one
    ix, iy = ((gx + one) * f32(W) - one) / two, ((gy + one) * f32(H) - one) / two
    fx, fy = np.floor(ix), np.floor(iy)

    def at(x, y):
        ok = (x >= 0) & (y >= 0) & (x < W) & (y < H)
        xi, yi = np.where(ok, x, 0).astype(np.int64), np.where(ok, y, 0).astype(np.int64)
        return np.where(ok, mask[yi, xi], f32(0.0)).astype(f32)
    x1, y1 = fx + one, fy + one
    nw, ne, sw, se = (x1 - ix) * (y1 - iy), (ix - fx) * (y1 - iy), (x1 - ix) * (iy - fy), (ix - fx) * (iy - fy)
    inside = (fx >= -1) & (fy >= -1) & (fx <= W) & (fy <= H)
    fxc, fyc = np.where(inside, fx, -1), np.where(inside, fy, -1)
    p = at(fxc, fyc) * nw
    p = p + at(fxc + 1, fyc) * ne
    p = p + at(fxc, fyc + 1) * sw
    p = p + at(fxc + 1, fyc + 1) * se
    return np.where(inside, p, f32(0.0)).astype(f32)


def cull_alpha_accumulate(final_sdf, weight, alpha, coord, mask, gt_mask=None, extra=None):
    """one view: returns the new (final_sdf, weight); the masks are multiplied, then sampled"""
    m = np.asarray(mask, f32)
    if gt_mask is not None:
        m = m * np.asarray(gt_mask, f32).reshape(m.shape)
    if extra is not None:
        m = m * np.asarray(extra, f32).reshape(m.shape)
    valid = sample_mask(coord, m) > f32(0.5)
    return (np.where(valid, np.minimum(np.asarray(alpha, f32), final_sdf), final_sdf).astype(f32), np.where(valid, weight + 1, weight).astype(np.int32))


def cull_alpha_finish(final_sdf, weight):
    return np.where(weight > 0, f32(0.5) - final_sdf, f32(-100.0)).astype(f32)


def bisect(left_pts, right_pts, left_sdf, right_sdf, mid_sdf):
    """one step: returns the new (left_pts, right_pts, left_sdf, right_sdf, next mid-points)"""
    m, l = np.asarray(mid_sdf, f32).reshape(-1), left_sdf
    low = ((m < 0) & (l < 0)) | ((m > 0) & (l > 0))
    mid = (left_pts + right_pts) / f32(2.0)
    nl, nr = np.where(low[:, None], mid, left_pts).astype(f32), np.where(low[:, None], right_pts, mid).astype(f32)
    return nl, nr, np.where(low, m, left_sdf).astype(f32), np.where(low, right_sdf, m).astype(f32), ((nl + nr) / f32(2.0)).astype(f32)


def keep_vertices(end_points, end_scales):
    e, s = np.asarray(end_points, f32), np.asarray(end_scales, f32).reshape(-1, 2)
    d = e[:, 0, :] - e[:, 1, :]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= s[:, 0] + s[:, 1]


def apply_masks(points, faces, vmask, fmask):
    """trimesh's update_vertices(vmask) followed by update_faces(fmask), for fmask = all three vertices kept"""
    remap = np.cumsum(vmask) - 1
    return np.asarray(points, f32)[vmask], remap[np.asarray(faces, np.int64)[fmask]].reshape(-1, 3)


def filter_mesh(end_points, end_scales, points, faces):
    vmask = keep_vertices(end_points, end_scales)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return apply_masks(points, faces, vmask, vmask[faces].all(axis=1) if faces.size else np.zeros(0, bool))


def driver(points, points_scale, cells, evaluate_sdf, n_binary_steps=8):
    """marching_tetrahedra_with_binary_search on numpy arrays"""
    ep, es, esc, faces, _ = marching(points, cells, evaluate_sdf(points), points_scale)
    l, r, ls, rs = ep[:, 0].copy(), ep[:, 1].copy(), es[:, 0, 0].copy(), es[:, 1, 0].copy()
    mid = (l + r) / f32(2.0)
    for _ in range(n_binary_steps):
        l, r, ls, rs, mid = bisect(l, r, ls, rs, evaluate_sdf(mid))
    return filter_mesh(ep, esc, mid, faces)


def random_case(V, T, seed):
    """random topology for sizes no fixture reaches: corners base, base + cumsum(randint(1, 40, 3)) mod V, shuffled per row; sdf normal with
    60 % at -100 and five exact zeros.  Returns (vertices[V,3], tets int32[T,4], sdf[V], scales[V,1])"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, V, (T, 1))
    tets = np.concatenate([base, base + np.cumsum(rng.integers(1, 40, (T, 3)), axis=1)], axis=1) % V
    tets = np.take_along_axis(tets, np.argsort(rng.random((T, 4)), axis=1), axis=1).astype(np.int32)
    sdf = rng.standard_normal(V).astype(f32)
    sdf[rng.random(V) < 0.6] = -100.0
    sdf[rng.choice(V, 5, replace=False)] = 0.0
    return rng.standard_normal((V, 3)).astype(f32), tets, sdf, rng.random((V, 1)).astype(f32)


def marching_unique_torch(vertices, tets, sdf, scales):
    """The REFERENCE's formulation of one chunk in eager torch, device-agnostic (what scripts/gpu_tetmesh_bench.py times the kernels
    against): torch.unique over all six edges of every crossing tet, the non-crossing edges dropped afterwards.  Same five outputs."""
    import torch
    dev = vertices.device
    tets = tets.long()
    occ = sdf.reshape(-1) > 0
    o = occ[tets.reshape(-1)].reshape(-1, 4)
    inside = o.sum(1)
    crossing_tet = (inside > 0) & (inside < 4)
    vt, vo = tets[crossing_tet], o[crossing_tet]
    ea, eb = torch.as_tensor(EDGE_A, device=dev), torch.as_tensor(EDGE_B, device=dev)
    a, b = vt[:, ea].reshape(-1), vt[:, eb].reshape(-1)
    uniq, inv = torch.unique(torch.stack([torch.minimum(a, b), torch.maximum(a, b)], 1), dim=0, return_inverse=True)
    crossing = occ[uniq[:, 0]] != occ[uniq[:, 1]]
    number = torch.cumsum(crossing.long(), 0) - 1
    number[~crossing] = -1
    vid = number[inv].reshape(-1, 6)
    interp_v = uniq[crossing]
    code = (vo.long() * torch.tensor([1, 2, 4, 8], device=dev)).sum(1)
    nt = torch.as_tensor(NUM_TRIANGLES, device=dev)[code]
    table = torch.as_tensor(TRIANGLE_TABLE, device=dev)
    one, two = nt == 1, nt == 2
    faces = torch.cat([torch.gather(vid[one], 1, table[code[one]][:, :3]).reshape(-1, 3), torch.gather(vid[two], 1, table[code[two]]).reshape(-1, 3)], 0)
    flat = interp_v.reshape(-1)
    return (vertices[flat].reshape(-1, 2, 3), sdf.reshape(-1)[flat].reshape(-1, 2, 1), scales.reshape(-1)[flat].reshape(-1, 2, 1), faces, interp_v)
