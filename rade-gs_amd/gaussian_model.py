"""The Gaussian model every route shares: the class upstream's scripts build first (`GaussianModel(sh_degree)`,
scene/gaussian_model.py) with upstream's attribute, property and method names, wired from this project's ops -- model_io for the state
on disk, gaussian_model_ops for the 3D filter, the densification and the activations, tetmesh for the tetrahedra points, fused_adam for
the optimizer, appearance_network for the per-view CNN.  No plyfile, no trimesh, no simple_knn build.

`activations()` is what render() reads: the rasterizer's four per-Gaussian inputs from the raw parameters, as ONE HIP launch each way
(gaussian_model_ops.model_activations) or as the eager composition torch.cat / F.normalize / scaling_n_opacity_with_3D_filter.

`device="cpu"` builds a model on which everything that launches no kernel works (the schedule, the optimizer groups, capture / restore,
the eager properties): the host-side tests use it.  Not built: get_truc_tetra_points, compute_partial_3D_filter (nothing upstream calls
them)."""
import os
import sys

import numpy as np
import torch
from torch import nn

# module default of GaussianModel.activations(fused=None): the fused launch or the eager composition.  RADEGS_FUSED_ACTIVATIONS=0 / 1
# overrides it for a process; DESIGN.md 11 N19 has the measurement the default follows.
FUSED_ACTIVATIONS = os.environ.get("RADEGS_FUSED_ACTIVATIONS", "1") != "0"


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """utils/general_utils.py:31-64: log-linear interpolation from lr_init (step 0) to lr_final (step max_steps), optionally eased in over
    lr_delay_steps from lr_init * lr_delay_mult.  The same NumPy float64 operations in the same order as upstream's, so the two agree to
    the last bit wherever the libraries do.  A negative step, or both rates zero, gives 0.0."""
    def helper(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        if lr_delay_steps > 0:
            delay_rate = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
        else:
            delay_rate = 1.0
        t = np.clip(step / max_steps, 0, 1)
        log_lerp = np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)
        return delay_rate * log_lerp
    return helper


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def build_rotation(r):
    """[P,4] quaternions (w, x, y, z; normalised here) -> [P,3,3] rotation matrices"""
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = (1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y))
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def build_covariance_from_scaling_rotation(scaling, scaling_modifier, rotation):
    """the six upper-triangle entries (xx xy xz yy yz zz) of (R S)(R S)^T, [P,6]"""
    L = build_rotation(rotation) * (scaling_modifier * scaling)[:, None, :]
    cov = L @ L.transpose(1, 2)
    return torch.stack((cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]), dim=1)


class GaussianModel:
    def __init__(self, sh_degree: int, device="cuda"):
        from appearance_network import AppearanceNetwork
        self.device = torch.device(device)
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self._xyz = torch.empty(0)
        self._features_dc = torch.empty(0)
        self._features_rest = torch.empty(0)
        self._scaling = torch.empty(0)
        self._rotation = torch.empty(0)
        self._opacity = torch.empty(0)
        self.max_radii2D = torch.empty(0)
        self.xyz_gradient_accum = torch.empty(0)
        self.xyz_gradient_accum_abs = torch.empty(0)
        self.xyz_gradient_accum_abs_max = torch.empty(0)
        self.denom = torch.empty(0)
        self.filter_3D = torch.empty(0)
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.scaling_activation, self.scaling_inverse_activation = torch.exp, torch.log
        self.covariance_activation = build_covariance_from_scaling_rotation
        self.opacity_activation, self.inverse_opacity_activation = torch.sigmoid, inverse_sigmoid
        self.rotation_activation = torch.nn.functional.normalize
        self.appearance_network = AppearanceNetwork(3 + 64, 3).to(self.device)
        self._appearance_embeddings = nn.Parameter(torch.empty(2048, 64, device=self.device))
        self._appearance_embeddings.data.normal_(0, 1e-4)

    # ---- checkpoints: upstream's 14 fields in upstream's order ----
    def capture(self):
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity,
                self.max_radii2D, self.xyz_gradient_accum, self.denom, self.optimizer.state_dict(), self.spatial_lr_scale,
                self.appearance_network.state_dict(), self._appearance_embeddings)

    def restore(self, model_args, training_args):
        (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity,
         self.max_radii2D, xyz_gradient_accum, denom, opt_dict, self.spatial_lr_scale, app_dict, _appearance_embeddings) = model_args
        # (upstream assigns the embeddings after training_setup, which leaves the optimizer group on the Parameter it replaced; here the
        # group is built on the restored one)
        self._appearance_embeddings = _appearance_embeddings
        self.training_setup(training_args)
        self.xyz_gradient_accum = xyz_gradient_accum
        self.denom = denom
        self.optimizer.load_state_dict(opt_dict)
        self.appearance_network.load_state_dict(app_dict)

    # ---- activations ----
    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_scaling(self):
        return self.scaling_activation(self._scaling)

    @property
    def get_rotation(self):
        return self.rotation_activation(self._rotation)

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return self.opacity_activation(self._opacity)

    @property
    def get_scaling_with_3D_filter(self):
        return self.get_scaling_n_opacity_with_3D_filter[0]

    @property
    def get_opacity_with_3D_filter(self):
        return self.get_scaling_n_opacity_with_3D_filter[1]

    @property
    def get_scaling_n_opacity_with_3D_filter(self):
        if self._scaling.is_cuda:
            import gaussian_model_ops
            return gaussian_model_ops.scaling_n_opacity_with_3D_filter(self._scaling, self._opacity, self.filter_3D)
        scales_square = torch.square(self.get_scaling)
        scales_after_square = scales_square + torch.square(self.filter_3D)
        coef = torch.sqrt(scales_square.prod(dim=1) / scales_after_square.prod(dim=1))
        return torch.sqrt(scales_after_square), self.get_opacity * coef[..., None]

    def activations(self, fused=None):
        """(shs, rotations, scales, opacity): get_features, get_rotation and get_scaling_n_opacity_with_3D_filter, the rasterizer's four
        per-Gaussian inputs.  fused=True: one HIP launch forward and one backward (gaussian_model_ops.model_activations); False: the eager
        composition; None: the module default FUSED_ACTIVATIONS."""
        if FUSED_ACTIVATIONS if fused is None else fused:
            import gaussian_model_ops
            return gaussian_model_ops.model_activations(self._features_dc, self._features_rest, self._rotation, self._scaling, self._opacity,
                                                        self.filter_3D)
        scales, opacity = self.get_scaling_n_opacity_with_3D_filter
        return self.get_features, self.get_rotation, scales, opacity

    def get_apperance_embedding(self, idx):
        return self._appearance_embeddings[idx]

    def get_covariance(self, scaling_modifier=1):
        return self.covariance_activation(self.get_scaling, scaling_modifier, self._rotation)

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---- the 3D filter ----
    @torch.no_grad()
    def reset_3D_filter(self):
        xyz = self.get_xyz
        self.filter_3D = torch.zeros([xyz.shape[0], 1], device=xyz.device)

    @torch.no_grad()
    def compute_3D_filter(self, cameras):
        import gaussian_model_ops
        self.filter_3D = gaussian_model_ops.compute_3D_filter(self.get_xyz, cameras)

    # ---- state on disk ----
    def create_from_pcd(self, pcd, spatial_lr_scale: float):
        import model_io
        model_io.create_from_pcd(self, pcd, spatial_lr_scale)

    def save_ply(self, path):
        import model_io
        model_io.save_model_ply(self, path)

    def load_ply(self, path):
        import model_io
        model_io.load_model_ply(self, path)

    def reset_opacity(self):
        import model_io
        model_io.reset_model_opacity(self)

    @torch.no_grad()
    def get_tetra_points(self):
        import tetmesh
        return tetmesh.get_tetra_points(self)

    # ---- optimisation ----
    def training_setup(self, training_args):
        import fused_adam
        dev = self.get_xyz.device
        P = self.get_xyz.shape[0]
        self.percent_dense = training_args.percent_dense
        self.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
        self.xyz_gradient_accum_abs = torch.zeros((P, 1), device=dev)
        self.xyz_gradient_accum_abs_max = torch.zeros((P, 1), device=dev)
        self.denom = torch.zeros((P, 1), device=dev)
        groups = [
            {"params": [self._xyz], "lr": training_args.position_lr_init * self.spatial_lr_scale, "name": "xyz"},
            {"params": [self._features_dc], "lr": training_args.feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": training_args.feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": training_args.opacity_lr, "name": "opacity"},
            {"params": [self._scaling], "lr": training_args.scaling_lr, "name": "scaling"},
            {"params": [self._rotation], "lr": training_args.rotation_lr, "name": "rotation"},
            {"params": [self._appearance_embeddings], "lr": training_args.appearance_embeddings_lr, "name": "appearance_embeddings"},
            {"params": self.appearance_network.parameters(), "lr": training_args.appearance_network_lr, "name": "appearance_network"},
        ]
        self.optimizer = fused_adam.Adam(groups, lr=0.0, eps=1e-15)
        self.xyz_scheduler_args = get_expon_lr_func(lr_init=training_args.position_lr_init * self.spatial_lr_scale,
                                                    lr_final=training_args.position_lr_final * self.spatial_lr_scale,
                                                    lr_delay_mult=training_args.position_lr_delay_mult,
                                                    max_steps=training_args.position_lr_max_steps)

    def update_learning_rate(self, iteration):
        """the position group's rate for this step; returns it"""
        for param_group in self.optimizer.param_groups:
            if param_group["name"] == "xyz":
                lr = self.xyz_scheduler_args(iteration)
                param_group["lr"] = lr
                return lr

    def add_densification_stats(self, viewspace_point_tensor, update_filter, radii=None):
        """upstream's two arguments; with `radii` the same launch also does train.py:187's max_radii2D update"""
        import gaussian_model_ops
        gaussian_model_ops.add_densification_stats(self, viewspace_point_tensor, update_filter, radii)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
        import gaussian_model_ops
        return gaussian_model_ops.densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size)


def install():
    """Registers this module as `scene.gaussian_model`, so that upstream's `from scene.gaussian_model import GaussianModel` resolves to it
    (with scene_io.install(), `from scene import Scene, GaussianModel` too).  Opt-in: nothing calls it."""
    sys.modules["scene.gaussian_model"] = sys.modules[__name__]
    return sys.modules[__name__]
