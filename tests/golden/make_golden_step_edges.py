"""Generates tests/golden/step_edges_*.npz by running the REFERENCE's own Python on the CPU, with torch autograd for the gradients, on
the inputs of tests/step_edge_cases.py:

    utils/graphics_utils.py   depth_double_to_normal, point_double_to_normal + the loss expression of train.py:152-155
    utils/loss_utils.py       l1_loss, ssim, combined as in train.py:159
    scene/gaussian_model.py   GaussianModel.get_scaling_n_opacity_with_3D_filter, GaussianModel.compute_3D_filter
    torch.optim.Adam          as scene/gaussian_model.py:338-349 builds it

Run where the reference's sources are (the GPU box has none):   python tests/golden/make_golden_step_edges.py
Only data is written.  The reference hard-codes `.cuda()` and imports modules that are not installed; both are neutralised as in the
other generators of this directory."""
import importlib.util
import os
import sys
import types
from collections import namedtuple

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import step_edge_cases as sec  # noqa: E402

for name, attrs in {"plyfile": ("PlyData", "PlyElement"), "simple_knn": (), "simple_knn._C": ("distCUDA2",), "trimesh": (), "cv2": ()}.items():
    m = types.ModuleType(name)
    for a in attrs:
        setattr(m, a, None)
    sys.modules.setdefault(name, m)
torch.Tensor.cuda = lambda self, *a, **k: self


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


View = namedtuple("View", "image_width image_height FoVx FoVy")
T = torch.from_numpy


def normals():
    gu = _load("ref_graphics_utils", "utils/graphics_utils.py")
    out = {}
    for cname, c in (("holes", sec.normals_holes()), ("empty", sec.normals_all_empty())):
        view = View(c["W"], c["H"], c["fovx"], c["fovy"])
        for mode in ("depth", "points"):
            keys = ("depth1", "depth2") if mode == "depth" else ("points1", "points2")
            fn = gu.depth_double_to_normal if mode == "depth" else gu.point_double_to_normal
            for variant in ("a", "b"):
                if f"rn_{variant}" not in c:
                    continue
                m1, m2 = (T(c[k].copy()).requires_grad_(True) for k in keys)
                rn = T(c[f"rn_{variant}"].copy()).requires_grad_(True)
                nm = fn(view, m1, m2)
                err = 1 - (rn.unsqueeze(0) * nm).sum(dim=1)                                   # train.py:152-155
                loss = (1 - sec.DEPTH_RATIO) * err[0].mean() + sec.DEPTH_RATIO * err[1].mean()
                loss.backward()
                tag = f"{cname}_{mode}_{variant}"
                out.update({f"{tag}_normals": nm.detach().numpy(), f"{tag}_loss": np.float32(loss.item()), f"{tag}_g1": m1.grad.numpy(),
                            f"{tag}_g2": m2.grad.numpy(), f"{tag}_g_rendered": rn.grad.numpy()})
            m1, m2 = (T(c[k].copy()).requires_grad_(True) for k in keys)
            (fn(view, m1, m2) * T(c["cot"])).sum().backward()
            out.update({f"{cname}_{mode}_c1": m1.grad.numpy(), f"{cname}_{mode}_c2": m2.grad.numpy()})
        for k in ("depth1", "depth2", "points1", "points2"):
            out[f"{cname}_{k}"] = c[k]
    np.savez_compressed(os.path.join(HERE, "step_edges_normals.npz"), **out)
    print("normals", {k: float(np.abs(v).max()) for k, v in out.items() if k.endswith("_b_g1")})


def losses():
    lu = _load("ref_loss_utils", "utils/loss_utils.py")
    out = {}
    for C in (3, 1):
        img, gt = sec.photometric_masked(C)
        for tag, a in ((f"masked_C{C}", img), (f"identical_C{C}", gt)):
            image, gt_image = T(a.copy()).requires_grad_(True), T(gt)
            l1 = lu.l1_loss(image, gt_image)
            s = lu.ssim(image, gt_image.unsqueeze(0))
            loss = (1.0 - 0.2) * l1 + 0.2 * (1.0 - s)                                         # train.py:159
            loss.backward()
            out.update({f"{tag}_l1": np.float32(l1.item()), f"{tag}_ssim": np.float32(s.item()), f"{tag}_loss": np.float32(loss.item()),
                        f"{tag}_grad": image.grad.numpy()})
        image = T(img.copy()).requires_grad_(True)
        lu.l1_loss(image, T(gt)).backward()
        out[f"masked_C{C}_grad_l1"] = image.grad.numpy()
        out[f"masked_C{C}_img"], out[f"masked_C{C}_gt"] = img, gt
    np.savez_compressed(os.path.join(HERE, "step_edges_losses.npz"), **out)
    print("losses", {k: float(v) for k, v in out.items() if v.ndim == 0})


def filter3d():
    sys.path.insert(0, REF)
    pkg = types.ModuleType("scene")            # keep scene/__init__.py (dataset readers, PIL, ...) from running
    pkg.__path__ = [os.path.join(REF, "scene")]
    sys.modules["scene"] = pkg
    from scene.gaussian_model import GaussianModel
    gm = object.__new__(GaussianModel)
    gm.setup_functions()
    out = {}

    def activations(tag, c):
        for path in ("both", "scales", "opacity"):
            gm._scaling = T(c["scaling_raw"].copy()).requires_grad_(True)
            gm._opacity = T(c["opacity_raw"].copy()).requires_grad_(True)
            gm.filter_3D = T(c["filter_3D"].copy())
            scales, opacity = gm.get_scaling_n_opacity_with_3D_filter
            obj = 0
            if path != "opacity":
                obj = obj + (scales * T(c["cot_scales"])).sum()
            if path != "scales":
                obj = obj + (opacity * T(c["cot_opacity"])).sum()
            obj.backward()
            zero = lambda t, like: np.zeros_like(like) if t is None else t.numpy()
            out.update({f"{tag}_{path}_g_scaling_raw": zero(gm._scaling.grad, c["scaling_raw"]),
                        f"{tag}_{path}_g_opacity_raw": zero(gm._opacity.grad, c["opacity_raw"])})
        out.update({f"{tag}_scales": scales.detach().numpy(), f"{tag}_opacity": opacity.detach().numpy()})
        for k in ("scaling_raw", "opacity_raw", "filter_3D"):
            out[f"{tag}_{k}"] = c[k]

    activations("act", sec.activation_case(257))
    activations("zero", sec.activation_zero_over_zero())

    g = np.load(os.path.join(HERE, "filter3d.npz"))
    cams12 = sec.cameras_from_rows(g["cams"])

    def run(xyz, cams):
        gm._xyz = T(xyz)
        gm.compute_3D_filter(cams)
        return gm.filter_3D.numpy()

    out["random_filter"] = run(sec.filter_random_xyz(), sec.cameras_cycled(cams12))
    out["one_seen_filter"] = run(*sec.filter_scene_one_seen())
    try:
        run(*sec.filter_scene_none_seen())
        out["none_seen_raises"] = np.array(False)
    except RuntimeError as e:                    # .max() of an empty selection
        out["none_seen_raises"] = np.array(True)
        print("none seen:", str(e).splitlines()[0])
    np.savez_compressed(os.path.join(HERE, "step_edges_filter3d.npz"), **out)
    print("filter3d ok")


def adam():
    out = {}
    layout = [t for t in sec.adam_layout() if t.has_grad and t.numel]
    for phase in (0, 1):
        data = {t.name: sec.adam_data(t, phase) for t in layout}
        params = {t.name: torch.nn.Parameter(T(data[t.name][0].copy())) for t in layout}
        groups = [dict(params=[params[t.name]], lr=t.lr, **sec.ADAM_GROUPS[t.group]) for t in layout]
        for gr in groups:
            gr["betas"] = tuple(gr["betas"])
        opt = torch.optim.Adam(groups, lr=0.0)
        if phase == 1:
            for t in layout:
                opt.state[params[t.name]] = {"step": torch.tensor(999.0), "exp_avg": T(data[t.name][2].copy()),
                                             "exp_avg_sq": T(data[t.name][3].copy())}
        for t in layout:
            params[t.name].grad = T(data[t.name][1].copy())
        opt.step()
        tag = "s1" if phase == 0 else "s1000"
        for t in layout:
            out[f"{tag}_{t.name}"] = params[t.name].detach().numpy().copy()
        if phase == 0:
            for t in layout:
                params[t.name].grad = T(sec.adam_second_grad(t))
            opt.step()
            for t in layout:
                out[f"s2_{t.name}"] = params[t.name].detach().numpy().copy()
                if t.numel <= 1100:
                    out[f"m2_{t.name}"] = opt.state[params[t.name]]["exp_avg"].numpy().copy()
                    out[f"v2_{t.name}"] = opt.state[params[t.name]]["exp_avg_sq"].numpy().copy()
    np.savez_compressed(os.path.join(HERE, "step_edges_adam.npz"), **out)
    print("adam ok")


if __name__ == "__main__":
    normals()
    losses()
    filter3d()
    adam()
