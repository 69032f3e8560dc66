"""Writes tests/golden/appearance_*.npz from the reference's own code (run where /root/reference exists; the tests never read it).

    python tests/golden/make_golden_appearance.py [reference root]

The network is the reference's scene/appearance_network.py loaded as a module from its file; the loss is the one function
`L1_loss_appearance` taken out of the parsed train.py and executed with the reference's own utils/loss_utils.l1_loss (importing train.py
whole needs packages a test machine does not have).  Nothing of the reference's text is written anywhere: only inputs drawn here and the
numbers its code returns, in float32 and float64.

    appearance_weights.<n>.npz     one state dict with default initialisation (float32) and `names`, the parameter names in its order
    appearance_<case>.<n>.npz      image, gt, embedding (the row of the view), and for p in (f32, f64): loss_p, F_p (up4's output), down_p (the
                                   first three channels of conv1's input), dimage_p, dembedding_p, dF_p, dW2_p, db2_p, dW3_p, db3_p;
                                   case 37x45 also dtrunk.<parameter>_f32
Arrays are spread over numbered parts (<stem>.<n>.npz) because no committed file of this repository may exceed 1 MiB -- the rule
make_golden_densify.py splits its fixtures for; a single appearance_99x167.npz would be 1.7 MB.  tests/appearance_restatement.load_parts
puts the parts together."""
import ast
import glob
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PART_BYTES = 900_000
CASES = {"37x45": (37, 45, 11), "63x95": (63, 95, 12), "70x101": (70, 101, 13), "99x167": (99, 167, 14), "zeros64x64": (64, 64, 15)}
VIEW, VIEWS = 2, 4


def load_module(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_loss_function(ref):
    tree = ast.parse(open(os.path.join(ref, "train.py")).read())
    node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "L1_loss_appearance"]
    assert len(node) == 1
    ns = {"torch": torch, "l1_loss": load_module("ref_loss_utils", os.path.join(ref, "utils", "loss_utils.py")).l1_loss}
    exec(compile(ast.Module(body=node, type_ignores=[]), os.path.join(ref, "train.py"), "exec"), ns)
    return ns["L1_loss_appearance"]


class Gaussians:
    def __init__(self, net, table):
        self.appearance_network, self._appearance_embeddings = net, table

    def get_apperance_embedding(self, idx):
        return self._appearance_embeddings[idx]


def write_parts(stem, arrays):
    for old in glob.glob(os.path.join(HERE, stem + ".*.npz")):
        os.remove(old)
    parts, size = [{}], 0
    for k, v in arrays.items():
        v = np.ascontiguousarray(v)
        if size and size + v.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    for n, part in enumerate(parts):
        path = os.path.join(HERE, f"{stem}.{n}.npz")
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
        print(path, os.path.getsize(path))


def inputs_of(case):
    h, w, seed = CASES[case]
    rng = np.random.default_rng(seed)
    image = rng.random((3, h, w), dtype=np.float32)
    gt = np.clip(0.7 * image + 0.3 * rng.random((3, h, w), dtype=np.float32) + 0.05 * rng.standard_normal((3, h, w)).astype(np.float32), 0, 1)
    if case.startswith("zeros"):
        image[:, 10:30, 20:50] = 0.0
        gt[:, 10:30, 20:50] = 0.0
    table = (0.5 * rng.standard_normal((VIEWS, 64))).astype(np.float32)
    return image, gt.astype(np.float32), table


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    net_mod = load_module("ref_appearance_network", os.path.join(ref, "scene", "appearance_network.py"))
    loss_fn = reference_loss_function(ref)
    torch.manual_seed(20240)
    net0 = net_mod.AppearanceNetwork(3 + 64, 3)
    state = {k: v.detach().clone() for k, v in net0.state_dict().items()}
    names = list(state)
    assert names == [n for n, _ in net0.named_parameters()]
    write_parts("appearance_weights", {"names": np.array(names), **{k: v.numpy() for k, v in state.items()}})
    for case in CASES:
        image, gt, table = inputs_of(case)
        out = {"image": image, "gt": gt, "embedding": table[VIEW].copy()}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            net = net_mod.AppearanceNetwork(3 + 64, 3)
            net.load_state_dict(state, strict=True)
            net = net.to(dtype)
            seen = {}

            def keep_features(module, args, output):
                output.retain_grad()
                seen["F"] = output

            def keep_input(module, args):
                seen["x"] = args[0]

            net.up4.register_forward_hook(keep_features)
            net.conv1.register_forward_pre_hook(keep_input)
            img = torch.from_numpy(image).to(dtype).requires_grad_(True)
            tab = torch.from_numpy(table).to(dtype).requires_grad_(True)
            loss = loss_fn(img, torch.from_numpy(gt).to(dtype), Gaussians(net, tab), VIEW)
            loss.backward()
            assert float(tab.grad[[i for i in range(VIEWS) if i != VIEW]].abs().max()) == 0.0
            rec = {"loss": loss, "F": seen["F"][0], "down": seen["x"][0, :3], "dimage": img.grad, "dembedding": tab.grad[VIEW], "dF": seen["F"].grad[0],
                   "dW2": net.conv2.weight.grad, "db2": net.conv2.bias.grad, "dW3": net.conv3.weight.grad, "db3": net.conv3.bias.grad}
            for k, v in rec.items():
                out[f"{k}_{tag}"] = v.detach().numpy().copy()
            if case == "37x45" and tag == "f32":
                for n, p in net.named_parameters():
                    if not n.startswith(("conv2", "conv3")):
                        out[f"dtrunk.{n}_f32"] = p.grad.numpy().copy()
        write_parts("appearance_" + case, out)


if __name__ == "__main__":
    main()
