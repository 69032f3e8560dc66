"""Generates tests/golden/activations_sh{0,1,2,3}.npz, trainer_schedule.npz and trainer_defaults.json from the REFERENCE's own code
(/root/reference/scene/gaussian_model.py: the activation properties 112-166, training_setup / update_learning_rate 331-361, capture 71-87;
utils/general_utils.py:31-64 get_expon_lr_func; arguments/__init__.py: the three parameter groups) run on the CPU.  Build container only.

The module's unavailable imports are stubbed, the object is created without __init__ and `device="cuda"` factory calls are routed to the
CPU, as make_golden_densify.py does.

activations_sh*.npz: P = 257 rows (four full tiles of 64 and a tail of one), raw parameters, the four property outputs, recorded cotangents
and the reference autograd's gradients of the five parameters the activations read (xyz passes through render() untouched).  Rotation norms
lie in [0.5, 2] and the cotangents are O(1): the reference's normalize sums its squares in another order than the stated chain
(tests/activation_restatement.py), a relative 1e-7 that the backward's g - y (g.y) must not amplify past the 1e-5 / 1e-4 band.  filter_3D
holds exact zeros among its rows."""
import json
import os
import sys
import types
from argparse import ArgumentParser

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

for name, attrs in {"plyfile": ("PlyData", "PlyElement"), "simple_knn": (), "simple_knn._C": ("distCUDA2",), "trimesh": (), "cv2": ()}.items():
    m = types.ModuleType(name)
    for a in attrs:
        setattr(m, a, None)
    sys.modules.setdefault(name, m)
sys.path.insert(0, "/root/reference")
pkg = types.ModuleType("scene")            # keep scene/__init__.py (dataset readers, PIL, ...) from running
pkg.__path__ = ["/root/reference/scene"]
sys.modules["scene"] = pkg
from arguments import ModelParams, OptimizationParams, PipelineParams  # noqa: E402
from scene.appearance_network import AppearanceNetwork  # noqa: E402
from scene.gaussian_model import GaussianModel  # noqa: E402
from utils.general_utils import get_expon_lr_func  # noqa: E402

for fn in ("zeros", "ones", "empty", "full", "tensor", "rand", "randn"):   # device="cuda" -> CPU
    def _route(*a, __f=getattr(torch, fn), **k):
        if str(k.get("device", "")).startswith("cuda"):
            k.pop("device")
        return __f(*a, **k)
    setattr(torch, fn, _route)

PARAMS = ("_features_dc", "_features_rest", "_rotation", "_scaling", "_opacity")
STEPS = (0, 1, 2, 100, 15000, 29999, 30000, 30001)


def bare_model(P, sh_degree, rng):
    gm = object.__new__(GaussianModel)
    gm.setup_functions()
    K = (sh_degree + 1) ** 2 - 1
    direction = rng.standard_normal((P, 4))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    init = dict(_xyz=rng.standard_normal((P, 3)), _features_dc=rng.standard_normal((P, 1, 3)), _features_rest=0.2 * rng.standard_normal((P, K, 3)),
                _rotation=direction * rng.uniform(0.5, 2.0, (P, 1)), _scaling=np.log(0.04) + 1.2 * rng.standard_normal((P, 3)),
                _opacity=2.0 * rng.standard_normal((P, 1)))
    for k, v in init.items():
        setattr(gm, k, torch.nn.Parameter(torch.from_numpy(v.astype(np.float32))))
    return gm


def activation_fixture(path, P, sh_degree, seed):
    rng = np.random.default_rng(seed)
    gm = bare_model(P, sh_degree, rng)
    f3 = (0.02 * np.exp(0.5 * rng.standard_normal((P, 1)))).astype(np.float32)
    f3[rng.random(P) < 0.15] = 0.0
    f3[[0, 63, 64, P - 1]] = [[0.0], [0.03], [0.0], [0.01]]
    gm.filter_3D = torch.from_numpy(f3)
    norms = np.linalg.norm(gm._rotation.detach().numpy().astype(np.float64), axis=1)
    assert norms.min() >= 0.5 - 1e-6 and norms.max() <= 2.0 + 1e-6
    shs, rotations = gm.get_features, gm.get_rotation
    scales, opacity = gm.get_scaling_n_opacity_with_3D_filter
    outs = dict(shs=shs, rotations=rotations, scales=scales, opacity=opacity)
    cot = {k: torch.from_numpy(rng.standard_normal(tuple(v.shape)).astype(np.float32)) for k, v in outs.items()}
    torch.autograd.backward(list(outs.values()), [cot[k] for k in outs])
    data = {a[1:]: getattr(gm, a).detach().numpy() for a in PARAMS}
    data["filter_3D"] = f3
    data.update({"out_" + k: v.detach().numpy() for k, v in outs.items()})
    data.update({"g_" + k: v.numpy() for k, v in cot.items()})
    data.update({"grad_" + a[1:]: getattr(gm, a).grad.numpy() for a in PARAMS})
    data["sh_degree"] = np.asarray(sh_degree)
    np.savez_compressed(path, **data)
    assert os.path.getsize(path) < (1 << 20)
    print(os.path.basename(path), P, "rows, K =", (sh_degree + 1) ** 2 - 1, ";", os.path.getsize(path), "bytes")


def defaults():
    """{group: {"defaults": {name: value}, "shorthands": [names with a one-letter flag]}} as the reference's classes declare them"""
    out = {}
    for cls in (ModelParams, PipelineParams, OptimizationParams):
        g = cls(ArgumentParser())
        out[cls.__name__] = {"defaults": {k.lstrip("_"): v for k, v in vars(g).items()}, "shorthands": [k[1:] for k in vars(g) if k.startswith("_")]}
    return out


def schedule_fixture(path):
    opt = OptimizationParams(ArgumentParser())
    gm = bare_model(5, 1, np.random.default_rng(0))
    gm.spatial_lr_scale = 3.7
    gm.appearance_network = AppearanceNetwork(3 + 64, 3)
    gm._appearance_embeddings = torch.nn.Parameter(torch.zeros(2048, 64))
    gm.training_setup(opt)
    data = {"steps": np.asarray(STEPS, dtype=np.int64), "spatial_lr_scale": np.asarray(3.7),
            "xyz_schedule": np.asarray([gm.xyz_scheduler_args(s) for s in STEPS], dtype=np.float64),
            "group_names": np.asarray([g["name"] for g in gm.optimizer.param_groups]),
            "group_lrs": np.asarray([g["lr"] for g in gm.optimizer.param_groups], dtype=np.float64),
            "group_sizes": np.asarray([len(g["params"]) for g in gm.optimizer.param_groups], dtype=np.int64),
            "adam_eps": np.asarray(gm.optimizer.defaults["eps"]), "adam_lr": np.asarray(gm.optimizer.defaults["lr"])}
    data["lr_after_update_100"] = np.asarray(gm.update_learning_rate(100), dtype=np.float64)
    gm.active_sh_degree, gm.max_radii2D = 0, torch.zeros(5)
    data["capture_fields"] = np.asarray(len(gm.capture()))
    # get_expon_lr_func on its own: (lr_init, lr_final, lr_delay_steps, lr_delay_mult, max_steps)
    cases = np.asarray([[1.6e-4, 1.6e-6, 0, 0.01, 30000], [1.6e-4, 1.6e-6, 500, 0.01, 30000], [2e-3, 5e-5, 2000, 0.1, 7000], [0.0, 0.0, 0, 1.0, 30000],
                        [0.0, 0.0, 100, 0.5, 30000]], dtype=np.float64)
    steps = np.asarray((-5, -1) + STEPS, dtype=np.int64)
    vals = np.empty((len(cases), len(steps)), dtype=np.float64)
    for i, (a, b, d, m, n) in enumerate(cases):
        f = get_expon_lr_func(lr_init=float(a), lr_final=float(b), lr_delay_steps=int(d), lr_delay_mult=float(m), max_steps=int(n))
        vals[i] = [f(int(s)) for s in steps]
    data.update(expon_cases=cases, expon_steps=steps, expon_values=vals)
    np.savez_compressed(path, **data)
    print(os.path.basename(path), dict(zip(data["group_names"].tolist(), data["group_lrs"].tolist())), "; capture fields", int(data["capture_fields"]))


if __name__ == "__main__":
    for d in range(4):
        activation_fixture(os.path.join(HERE, f"activations_sh{d}.npz"), 257, d, seed=190 + d)
    schedule_fixture(os.path.join(HERE, "trainer_schedule.npz"))
    with open(os.path.join(HERE, "trainer_defaults.json"), "w") as f:
        json.dump(defaults(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("trainer_defaults.json written")
