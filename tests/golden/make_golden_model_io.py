"""Generates tests/golden/g_model_io.npz from the REFERENCE's own code run on the CPU (/root/reference/scene/gaussian_model.py:
construct_list_of_attributes 363-377, reset_opacity 495-513 with replace_tensor_to_optimizer 561-576, create_from_pcd 301-328, and
utils/sh_utils.py RGB2SH).  Build container only.

The module's unavailable imports are stubbed and the object is created without __init__, as make_golden_densify.py does; `device="cuda"`
factory calls are routed to the CPU and Tensor.cuda() returns the tensor itself.  create_from_pcd's `device="cuda"` literals are neutralised
the same way, so it IS the reference's code that runs, with distCUDA2 bound to oracle/knn_oracle.py (float64 k-d tree, rounded to float32).

reset_K is the reference's own float32 error on the reset recipe against tests/model_io_restatement.py's float64 value, in units of
2^-24 (kappa + |f64|), kappa = 1 / (1 - x): the GPU test allows twice that.  The script asserts that the reference is finite on every row
of the recipe, so the comparison leaves out no element."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import model_io_restatement as mr  # noqa: E402
from oracle import knn_oracle  # noqa: E402

for name, attrs in {"plyfile": ("PlyData", "PlyElement"), "simple_knn": (), "simple_knn._C": ("distCUDA2",), "trimesh": (), "cv2": ()}.items():
    m = types.ModuleType(name)
    for a in attrs:
        setattr(m, a, None)
    sys.modules.setdefault(name, m)
sys.path.insert(0, "/root/reference")
pkg = types.ModuleType("scene")            # keep scene/__init__.py (dataset readers, PIL, ...) from running
pkg.__path__ = ["/root/reference/scene"]
sys.modules["scene"] = pkg
import scene.gaussian_model as gmod  # noqa: E402
from scene.gaussian_model import GaussianModel  # noqa: E402
from utils.graphics_utils import BasicPointCloud  # noqa: E402
from utils.sh_utils import RGB2SH  # noqa: E402

for fn in ("zeros", "ones", "empty", "full", "tensor", "rand", "randn"):   # device="cuda" -> CPU
    def _route(*a, __f=getattr(torch, fn), **k):
        if str(k.get("device", "")).startswith("cuda"):
            k.pop("device")
        return __f(*a, **k)
    setattr(torch, fn, _route)
torch.Tensor.cuda = lambda self, *a, **k: self
gmod.distCUDA2 = lambda pts: torch.from_numpy(knn_oracle.mean_dist2_3nn(pts.numpy()).astype(np.float32))

GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"), ("scaling", "_scaling"),
          ("rotation", "_rotation"))
data = {}

# ---- the property order ----
for d in (0, 1, 3):
    gm = object.__new__(GaussianModel)
    K = (d + 1) ** 2 - 1
    gm._features_dc, gm._features_rest, gm._scaling, gm._rotation = torch.zeros(2, 1, 3), torch.zeros(2, K, 3), torch.zeros(2, 3), torch.zeros(2, 4)
    data[f"names_sh{d}_filter"] = np.array(gm.construct_list_of_attributes())
    data[f"names_sh{d}_plain"] = np.array(gm.construct_list_of_attributes(exclude_filter=True))

# ---- RGB2SH ----
rgb = np.random.default_rng(11).random((512, 3)).astype(np.float32)
rgb[:4] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [0.1, 0.9, 0.5]]
data["rgb"], data["rgb2sh"] = rgb, RGB2SH(torch.from_numpy(rgb)).numpy()


# ---- reset_opacity ----
def reset(o, s, f, rng):
    gm = object.__new__(GaussianModel)
    gm.setup_functions()
    P = o.shape[0]
    init = dict(_xyz=np.zeros((P, 3)), _features_dc=np.zeros((P, 1, 3)), _features_rest=np.zeros((P, 3, 3)), _opacity=o, _scaling=s, _rotation=np.ones((P, 4)))
    for k, v in init.items():
        setattr(gm, k, torch.nn.Parameter(torch.from_numpy(np.asarray(v, dtype=np.float32))))
    gm.filter_3D = torch.from_numpy(f)
    gm.optimizer = torch.optim.Adam([{"params": [getattr(gm, a)], "lr": 0.0, "name": n} for n, a in GROUPS], lr=0.0, eps=1e-15)
    for _ in range(2):                      # two steps at lr 0: non-zero moments, step = 2, parameters unchanged
        for _, a in GROUPS:
            p = getattr(gm, a)
            p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32))
        gm.optimizer.step()
    gm.optimizer.zero_grad(set_to_none=True)
    assert np.array_equal(gm._opacity.detach().numpy(), o)
    old = gm._opacity
    before = {k: (v.numpy().copy() if torch.is_tensor(v) and v.dim() else np.asarray(float(v))) for k, v in gm.optimizer.state[old].items()}
    with torch.no_grad():
        gm.reset_opacity()
    group = [g for g in gm.optimizer.param_groups if g["name"] == "opacity"][0]
    assert group["params"][0] is gm._opacity and gm._opacity is not old and old not in gm.optimizer.state
    assert isinstance(gm._opacity, torch.nn.Parameter) and gm._opacity.requires_grad
    st = gm.optimizer.state[gm._opacity]
    return gm._opacity.detach().numpy().copy(), before, st


o, s, f = mr.reset_recipe()
rng = np.random.default_rng(6)
new, before, st = reset(o, s, f, rng)
f64, x, kappa = mr.reset_opacity64(o, s, f)
assert np.isfinite(new).all() and np.isfinite(f64).all(), "the recipe must be finite on every row"
K_err = float(np.max(np.abs(new.astype(np.float64) - f64) / (2.0 ** -24 * (kappa + np.abs(f64)))))
print("reset: max x", float(x.max()), "reset_K", K_err)
data.update(reset_new=new, reset_K=np.asarray(K_err), reset_before_exp_avg=before["exp_avg"], reset_before_exp_avg_sq=before["exp_avg_sq"],
            reset_before_step=before["step"], reset_after_exp_avg=st["exp_avg"].numpy().copy(), reset_after_exp_avg_sq=st["exp_avg_sq"].numpy().copy(),
            reset_after_step=np.asarray(float(st["step"])))
names, eo, es, ef = mr.reset_edges()
with np.errstate(all="ignore"):
    enew, _, _ = reset(eo, es, ef, rng)
print("edges:", dict(zip(names, enew[:, 0].tolist())))
data.update(edge_names=np.array(names), edge_new=enew)

# ---- create_from_pcd ----
rng = np.random.default_rng(12)
P = 500
pts = rng.standard_normal((P, 3)).astype(np.float32)
pts[10] = pts[11] = pts[12] = pts[13]                 # four coincident points: dist2 = 0, the clamp at 1e-7
col = rng.random((P, 3)).astype(np.float32)
gm = object.__new__(GaussianModel)
gm.max_sh_degree = 3
gm.create_from_pcd(BasicPointCloud(points=pts, colors=col, normals=np.zeros_like(pts)), 2.5)
assert gm.spatial_lr_scale == 2.5 and all(isinstance(getattr(gm, a), torch.nn.Parameter) and getattr(gm, a).requires_grad for _, a in GROUPS)
data.update(pcd_points=pts, pcd_colors=col, pcd_dist2=knn_oracle.mean_dist2_3nn(pts).astype(np.float32),
            **{"pcd" + a: getattr(gm, a).detach().numpy().copy() for _, a in GROUPS}, pcd_max_radii2D=gm.max_radii2D.numpy().copy())
assert float(np.abs(data["pcd_features_rest"]).sum()) == 0.0 and np.array_equal(data["pcd_xyz"], pts)
del data["pcd_features_rest"], data["pcd_xyz"]         # zeros [P,15,3] and the points themselves: nothing more to record than that
data["pcd_features_rest_shape"] = np.asarray(gm._features_rest.shape)

path = os.path.join(HERE, "g_model_io.npz")
np.savez_compressed(path, **data)
print(os.path.basename(path), os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 200_000
