"""Generates tests/golden/mesheval_chamfer.npz and mesheval_cull.npz from the REFERENCE's own code run on the CPU (/root/reference:
dtu_eval/eval.py and evaluate_dtu_mesh.cull_mesh).  Build container only (needs sklearn and scipy).

The reference's code is RUN, not copied:
  * dtu_eval/eval.py is a script: it is executed with runpy under __main__ with sys.argv set.  `open3d` is a stub whose reads hand out the
    fixture mesh and the ground-truth cloud and whose writes record; scipy.io.loadmat hands out a synthetic ObsMask / BB / Res / P;
    np.random.default_rng returns a seeded shuffler that also records the permutation it applies; sklearn's NearestNeighbors is wrapped to
    record what is fitted, asked and answered; multiprocessing.Pool is serial (and records the number of samples per triangle).  The
    expected values are those recordings, the script's own variables (runpy returns its globals) and the results.json it writes.
  * evaluate_dtu_mesh.cull_mesh is imported with the usual stubs (scene, cv2, arguments, gaussian_renderer, trimesh) and `.cuda()` routed
    to the CPU, as make_golden_tetmesh.py does, and called on a recording mesh object.
  * `skimage` is absent: skimage.morphology.binary_dilation and disk are stood in by scipy.ndimage.binary_dilation over the footprint
    x^2 + y^2 <= r^2.  The stand-in is UNVERIFIED against skimage (its documentation describes disk() as that footprint and
    binary_dilation as zero-padded).

Every decision on a threshold is ASSERTED to keep a margin, so that tests can demand exact equality from implementations whose arithmetic
differs in the last bit (the lattice test k0 + k1 < 1 is the exception: its ties are part of the contract).  On a failed assertion change
the seed, never the margin."""
import json
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import mesheval_restatement as mr  # noqa: E402  (only for the number of rounds the thinning takes)


def stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules.setdefault(name, m)
    return sys.modules[name]


def save(name, **data):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **data)
    size = os.path.getsize(path)
    assert size < 1_000_000, (name, size)
    print(name, size, "bytes;", {k: tuple(np.shape(v)) for k, v in data.items()})


def uv_sphere(nlat, nlon, radius, centre, bump, rng):
    """a closed bumpy sphere: 2 nlon (nlat - 1) triangles"""
    verts = [[0.0, 0.0, 1.0]]
    for a in range(1, nlat):
        th = np.pi * a / nlat
        for b in range(nlon):
            ph = 2 * np.pi * (b + 0.37 * a) / nlon
            verts.append([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    verts.append([0.0, 0.0, -1.0])
    verts = np.array(verts)
    verts = verts * (radius * (1.0 + bump * rng.standard_normal((verts.shape[0], 1)))) + np.asarray(centre)[None]
    faces, ring = [], lambda a, b: 1 + (a - 1) * nlon + (b % nlon)
    for b in range(nlon):
        faces.append([0, ring(1, b), ring(1, b + 1)])
        faces.append([verts.shape[0] - 1, ring(nlat - 1, b + 1), ring(nlat - 1, b)])
    for a in range(1, nlat - 1):
        for b in range(nlon):
            faces.append([ring(a, b), ring(a + 1, b), ring(a + 1, b + 1)])
            faces.append([ring(a, b), ring(a + 1, b + 1), ring(a, b + 1)])
    return verts, np.array(faces, np.int64)


# ------------------------------------------------------------------------ chamfer ------------------------------------------------------------------------
def chamfer_fixture(seed):
    rng = np.random.default_rng(seed)
    centre, R = np.array([118.0, -83.0, 641.0]), 6.0
    verts, faces = uv_sphere(13, 24, R, centre, 0.03, rng)
    extra_v, extra_f = [], []

    def add_tri(p0, e1, e2):
        k = verts.shape[0] + len(extra_v)
        extra_v.extend([p0, p0 + e1, p0 + e2])
        extra_f.append([k, k + 1, k + 2])
    for n, leg in ((2, 0.5), (3, 0.7), (5, 1.1), (2, 0.55), (3, 0.75), (5, 1.15)):           # right isosceles: thr = density, n1 = n2 = floor(leg / 0.2)
        o = centre + rng.standard_normal(3) * 2.0
        a = rng.standard_normal(3)
        a /= np.linalg.norm(a)
        b = np.cross(a, rng.standard_normal(3))
        b /= np.linalg.norm(b)
        add_tri(o, a * leg, b * leg)
    for _ in range(4):                                                                         # smaller than thr: no samples
        add_tri(centre + rng.standard_normal(3) * 3.0, rng.standard_normal(3) * 0.05, rng.standard_normal(3) * 0.05)
    verts = np.concatenate([verts, np.array(extra_v)], 0).astype(np.float32).astype(np.float64)   # as a PLY would hold them
    faces = np.concatenate([faces, np.array(extra_f, np.int64), np.array([[5, 5, 30]], np.int64)], 0)   # and one zero-area triangle
    faces = faces[rng.permutation(faces.shape[0])]

    n_near, n_far = 7000, 1000
    d = rng.standard_normal((n_near, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    stl = np.concatenate([centre + d * (R + 0.3 * rng.standard_normal((n_near, 1))),
                          centre + np.array([45.0, 10.0, 20.0]) + rng.standard_normal((n_far, 3)) * 4.0], 0)
    stl = stl[rng.permutation(stl.shape[0])].astype(np.float32).astype(np.float64)

    res = 0.5
    BB = np.array([centre + [-125.0, -8.0, -3.0], centre + [-118.0, 40.0, 40.0]])              # hi = BB[1] + 120 cuts the sphere along x
    gx, gy, gz = np.meshgrid(np.arange(250), np.arange(40), np.arange(40), indexing="ij")
    obs = (((gy + 2 * gz) % 9 < 6) & (gy < 30)).astype(np.uint8)                               # the volume cuts through the surface
    normal = np.array([0.1, 0.2, 1.0]) / np.linalg.norm([0.1, 0.2, 1.0])
    P = np.concatenate([normal, [-(normal @ (centre + [0.0, 0.0, 1.0]))]]).reshape(1, 4)
    mats = {"ObsMask": dict(ObsMask=np.asfortranarray(obs), BB=BB, Res=np.array([[res]])), "Plane": dict(P=P)}

    rec = dict(fit=[], radius=[], knn=[], written=[], tri_counts=[], perm=None)

    class Shuffler:
        def __init__(self):
            self.rng = rng.spawn(1)[0] if hasattr(rng, "spawn") else np.random.Generator(np.random.PCG64(seed + 1))

        def shuffle(self, x, axis=0):
            perm = self.rng.permutation(x.shape[0])
            rec["perm"] = perm
            x[:] = x[perm]

    class FakePool:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def map(self, fn, it, chunksize=None):
            out = [fn(x) for x in it]
            rec["tri_counts"] = [o.shape[0] for o in out]
            return out

    import multiprocessing
    import scipy.io
    import sklearn.neighbors as skln

    class Recorder(skln.NearestNeighbors):
        def fit(self, X, y=None):
            rec["fit"].append(np.array(X))
            return super().fit(X, y)

        def radius_neighbors(self, X=None, radius=None, return_distance=True, sort_results=False):
            out = super().radius_neighbors(X, radius=radius, return_distance=return_distance, sort_results=sort_results)
            rec["radius"].append((np.array(X), radius, out))
            return out

        def kneighbors(self, X=None, n_neighbors=None, return_distance=True):
            out = super().kneighbors(X, n_neighbors=n_neighbors, return_distance=return_distance)
            rec["knn"].append((np.array(X), out[0].copy(), out[1].copy()))
            return out

    io = types.SimpleNamespace(read_triangle_mesh=lambda p: types.SimpleNamespace(vertices=verts.copy(), triangles=faces.copy()),
                               read_point_cloud=lambda p: types.SimpleNamespace(points=stl.copy()),
                               write_point_cloud=lambda f, pcd: rec["written"].append((f, np.array(pcd.points), np.array(pcd.colors))))
    sys.modules["open3d"] = types.SimpleNamespace(io=io, geometry=types.SimpleNamespace(PointCloud=lambda: types.SimpleNamespace()),
                                                  utility=types.SimpleNamespace(Vector3dVector=lambda a: np.asarray(a)))
    try:
        import tqdm  # noqa: F401
    except ImportError:
        stub("tqdm", tqdm=lambda **k: types.SimpleNamespace(update=lambda n: None, set_description=lambda s: None, close=lambda: None))
    saved = (scipy.io.loadmat, np.random.default_rng, skln.NearestNeighbors, multiprocessing.Pool, sys.argv)
    out_dir = tempfile.mkdtemp(prefix="mesheval_golden_")
    scipy.io.loadmat = lambda path, *a, **k: mats["Plane" if "Plane" in os.path.basename(path) else "ObsMask"]
    np.random.default_rng = lambda *a, **k: Shuffler()
    skln.NearestNeighbors = Recorder
    multiprocessing.Pool = FakePool
    sys.argv = ["eval.py", "--data", "fixture.ply", "--scan", "1", "--mode", "mesh", "--dataset_dir", "DTU", "--vis_out_dir", out_dir]
    try:
        g = runpy.run_path(os.path.join(REF, "dtu_eval", "eval.py"), run_name="__main__")
    finally:
        scipy.io.loadmat, np.random.default_rng, skln.NearestNeighbors, multiprocessing.Pool, sys.argv = saved
    results = json.load(open(os.path.join(out_dir, "results.json")))

    # ---- what ran ----
    density, max_dist, patch = g["thresh"], g["max_dist"], g["patch"]
    assert (density, max_dist, patch) == (0.2, 20, 60)
    perm = rec["perm"]
    data_pcd = np.concatenate([verts, g["new_pts"]], 0)
    shuffled = rec["fit"][0]
    assert np.array_equal(shuffled, data_pcd[perm]) and len(rec["fit"]) == 3 and len(rec["knn"]) == 2 and len(rec["radius"]) == 1
    counts = np.zeros(faces.shape[0], np.int64)
    counts[g["non_zero_area"]] = rec["tri_counts"]
    assert counts.sum() == g["new_pts"].shape[0] and (~g["non_zero_area"]).sum() == 1
    keep, data_down = g["mask"], g["data_down"]
    where_in = np.nonzero(g["inbound"])[0]
    inbound = g["inbound"]
    grid_inbound, in_obs = np.zeros_like(inbound), np.zeros_like(inbound)
    grid_inbound[where_in[g["grid_inbound"]]] = True
    in_obs[where_in[g["grid_inbound"]][g["in_obs"]]] = True
    assert np.array_equal(rec["fit"][2], data_down[inbound]) and np.array_equal(rec["knn"][0][0], data_down[in_obs])
    assert np.array_equal(rec["fit"][1], stl) and np.array_equal(rec["knn"][1][0], stl[g["above"]])
    assert np.array_equal(rec["written"][0][1], data_down)

    def cut(dist, idx):                                           # the contract's form: inf and -1 at max_dist or beyond
        dist, idx = dist[:, 0].copy(), idx[:, 0].astype(np.int64)
        far = ~(dist < max_dist)
        dist[far], idx[far] = np.inf, -1
        return dist, idx
    dist_d2s, idx_d2s = cut(rec["knn"][0][1], rec["knn"][0][2])
    dist_s2d, idx_s2d = cut(rec["knn"][1][1], rec["knn"][1][2])

    # ---- margins ----
    n_by_k = {k: int(((g["n1"][:, 0] == k) & (g["n2"][:, 0] == k)).sum()) for k in (2, 3, 5)}
    print("triangles:", faces.shape[0], "points:", data_pcd.shape[0], "equal subdivisions n1 = n2:", n_by_k,
          "; without samples:", int((counts == 0).sum()))
    assert all(v >= 1 for v in n_by_k.values()) and (counts[g["non_zero_area"]] == 0).sum() >= 4
    for l, name in ((g["l1"], "l1"), (g["l2"], "l2")):
        q = (l / g["thr"])[:, 0]
        gap = np.abs(q - np.rint(q)) / np.maximum(q, 1.0)
        assert gap.min() > 1e-9, (name, gap.min())
    r2, worst = density ** 2, np.inf
    for s in range(0, shuffled.shape[0], 1024):
        d2 = mr._d2(shuffled[s:s + 1024], shuffled)
        worst = min(worst, float(np.abs(d2 - r2).min() / r2))
    assert worst > 1e-9, worst
    keep_rounds, rounds = mr.thin_rounds(shuffled, density)
    print("thinning: kept", int(keep.sum()), "of", keep.shape[0], "in", rounds, "rounds; smallest |d2 - r2| / r2:", worst)
    assert np.array_equal(keep_rounds, keep) and rounds >= 4
    bb32 = BB.astype(np.float32)
    lo, hi = (bb32[:1] - patch).astype(np.float64), (bb32[1:] + patch * 2).astype(np.float64)
    assert (np.abs(data_down - lo) > 1e-9 * np.abs(lo)).all() and (np.abs(data_down - hi) > 1e-9 * np.abs(hi)).all()
    cell = (data_down[inbound] - bb32[:1]) / res
    assert np.abs(cell - np.floor(cell) - 0.5).min() > 1e-6
    print("masks: inbound", int(inbound.sum()), "grid_inbound", int(grid_inbound.sum()), "in_obs", int(in_obs.sum()), "of", inbound.shape[0])
    assert 0 < in_obs.sum() < grid_inbound.sum() < inbound.sum() < inbound.shape[0]
    hom = np.abs(stl) @ np.abs(P[0, :3]) + abs(P[0, 3])
    side = stl @ P[0, :3] + P[0, 3]
    assert (np.abs(side) > 1e-9 * hom).all() and 0 < g["above"].sum() < stl.shape[0]
    for cloud, queries, dist, tag in ((stl, data_down[in_obs], rec["knn"][0][1][:, 0], "d2s"), (data_down[inbound], stl[g["above"]], rec["knn"][1][1][:, 0], "s2d")):
        for s in range(0, queries.shape[0], 1024):
            d = np.sqrt(np.sort(mr._d2(queries[s:s + 1024], cloud), 1)[:, :2])
            assert ((d[:, 1] - d[:, 0]) > 1e-9 * d[:, 1]).all(), tag
            assert np.allclose(d[:, 0], dist[s:s + 1024], rtol=1e-12, atol=0), tag
        assert (np.abs(dist - max_dist) > 1e-9 * max_dist).all()
        print(tag, "queries", queries.shape[0], "beyond max_dist", int((dist >= max_dist).sum()))
    assert (dist_s2d == np.inf).sum() > 100
    assert results["mean_d2s"] == float(dist_d2s[dist_d2s < max_dist].mean())

    save("mesheval_chamfer.npz", vertices=verts.astype(np.float32), faces=faces.astype(np.int32), stl=stl.astype(np.float32), obs_mask=obs,
         BB=BB, Res=np.asarray(res), plane=P, perm=perm.astype(np.int32), density=np.asarray(density), max_dist=np.asarray(float(max_dist)),
         patch=np.asarray(float(patch)), data_pcd=data_pcd, counts=counts.astype(np.int32), keep=keep, inbound=inbound, grid_inbound=grid_inbound,
         in_obs=in_obs, dist_d2s=dist_d2s, idx_d2s=idx_d2s.astype(np.int32), above=g["above"], dist_s2d=dist_s2d, idx_s2d=idx_s2d.astype(np.int32),
         mean_d2s=np.asarray(results["mean_d2s"]), mean_s2d=np.asarray(results["mean_s2d"]), overall=np.asarray(results["overall"]),
         rounds=np.asarray(rounds))


# -------------------------------------------------------------------------- cull --------------------------------------------------------------------------
class FakeMesh:
    def __init__(self, vertices, faces):
        self.vertices, self.faces, self.vmask, self.fmask = vertices, faces, None, None

    def update_vertices(self, mask):
        self.vmask = np.array(mask)

    def update_faces(self, mask):
        self.fmask = np.array(mask)


def look_at(eye, target):
    """world-to-camera, +z forward"""
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z], 0)
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = Rm, -Rm @ eye
    return w2c


def cull_fixture(seed):
    import scipy.ndimage as ndi
    rng = np.random.default_rng(seed)
    dilations = []

    def binary_dilation(image, footprint):
        out = ndi.binary_dilation(np.asarray(image) != 0, structure=footprint)
        dilations.append(out.copy())
        return out

    def disk(radius):
        y, x = np.mgrid[-radius:radius + 1, -radius:radius + 1]
        return (x * x + y * y) <= radius * radius
    stub("skimage")
    stub("skimage.morphology", binary_dilation=binary_dilation, disk=disk)
    stub("cv2")
    stub("trimesh")
    stub("gaussian_renderer", GaussianModel=None)
    stub("arguments", ModelParams=None, PipelineParams=None, get_combined_args=None)
    pkg = types.ModuleType("scene")
    pkg.__path__ = []
    pkg.Scene = None
    sys.modules["scene"] = pkg
    sys.path.insert(0, REF)
    import evaluate_dtu_mesh as edm
    torch.Tensor.cuda = lambda self, *a, **k: self

    verts, faces = uv_sphere(13, 24, 1.0, [0.2, -0.1, 0.3], 0.05, rng)
    verts = verts.astype(np.float32).astype(np.float64)
    sizes = ((97, 61), (64, 80), (50, 50), (40, 30))
    eyes = ([3.0, 0.5, 0.4], [-0.4, 2.6, 1.0], [0.3, -0.2, 4.0], [0.0, 6.0, 0.3])
    targets = ([0.2, -0.1, 0.3], [0.5, -0.1, 0.3], [0.2, 0.4, 0.3], [0.0, 12.0, 0.3])     # the last camera looks away: every vertex is behind it
    cams, store = [], {}
    for i, ((W, H), eye, target) in enumerate(zip(sizes, eyes, targets)):
        w2c = look_at(np.array(eye), np.array(target)).astype(np.float32)
        yy, xx = np.mgrid[0:H, 0:W]
        blob = ((xx - W * (0.45 + 0.1 * i)) / (0.33 * W)) ** 2 + ((yy - H * 0.5) / (0.42 * H)) ** 2 < 1
        mask = (blob * 255).astype(np.uint8)
        mask[0, :3] = 255                                                                    # set pixels on the border
        fovx, fovy = 0.9 + 0.1 * i, 0.8
        cams.append(types.SimpleNamespace(world_view_transform=torch.from_numpy(w2c).T.contiguous(), gt_mask=torch.from_numpy(mask)[None].float(),
                                          FoVx=fovx, FoVy=fovy, image_width=W, image_height=H))
        store.update({f"mask{i}": mask, f"size{i}": np.asarray([W, H]), f"fov{i}": np.asarray([fovx, fovy])})
    real_inverse, real_gs = torch.inverse, torch.nn.functional.grid_sample
    # With a few thousand projected coordinates some always fall within 1e-3 px of a half: the vertices that do are redrawn (a seed change
    # for those vertices, never a narrower margin) and the reference is run again, until every coordinate keeps the margin.
    for attempt in range(50):
        inverses, grids = [], []
        del dilations[:]

        def rec_inverse(t):
            out = real_inverse(t)
            inverses.append(out.numpy().copy())
            return out

        def rec_gs(inp, grid, **k):
            grids.append(grid.numpy().reshape(-1, 2).copy())
            return real_gs(inp, grid, **k)
        torch.inverse, edm.F.grid_sample = rec_inverse, rec_gs
        mesh = FakeMesh(verts.copy(), faces.copy())
        try:
            edm.cull_mesh(cams, mesh)
        finally:
            torch.inverse, edm.F.grid_sample = real_inverse, real_gs
        assert len(inverses) == len(cams) and len(grids) == len(cams) and len(dilations) == len(cams)   # Tensor.inverse() is not torch.inverse
        bad = np.zeros(verts.shape[0], bool)
        for cam, grid in zip(cams, grids):
            size = np.array([cam.image_width - 1, cam.image_height - 1])
            px = (grid.astype(np.float64) + 1) / 2 * size
            with np.errstate(invalid="ignore"):
                ok = (np.abs(px - np.floor(px) - 0.5) > 1e-3) & (np.abs(px) > 1e-3) & (np.abs(px - size) > 1e-3)
            bad |= ~ok.all(1) & np.isfinite(grid).all(1)
        if not bad.any():
            break
        print("attempt", attempt, ":", int(bad.sum()), "vertices within 1e-3 px of a half or a border, redrawn")
        verts[bad] = (verts[bad] + 0.01 * rng.standard_normal((int(bad.sum()), 3))).astype(np.float32).astype(np.float64)
    assert not bad.any(), "a pixel coordinate within 1e-3 px of a half or of the (-1, 1) borders: change the seed"
    for i, (cam, w2c, grid, big) in enumerate(zip(cams, inverses, grids, dilations)):
        valid = ((grid > -1) & (grid < 1)).all(1)
        print("camera", i, "valid", int(valid.sum()), "of", grid.shape[0], "; dilated pixels", int(big.sum()))
        store.update({f"w2c{i}": w2c.astype(np.float32), f"dilated{i}": big})
    assert 0 < mesh.vmask.sum() < verts.shape[0] and 0 < mesh.fmask.sum() < faces.shape[0]
    remap = np.cumsum(mesh.vmask) - 1
    print("cull: vertices kept", int(mesh.vmask.sum()), "of", verts.shape[0], "; faces kept", int(mesh.fmask.sum()), "of", faces.shape[0])
    save("mesheval_cull.npz", vertices=verts.astype(np.float32), faces=faces.astype(np.int32), ncam=np.asarray(len(cams)), vertex_mask=mesh.vmask,
         face_mask=mesh.fmask, out_vertices=verts[mesh.vmask].astype(np.float32), out_faces=remap[faces[mesh.fmask]].astype(np.int64), **store)


if __name__ == "__main__":
    chamfer_fixture(seed=31)
    cull_fixture(seed=32)
