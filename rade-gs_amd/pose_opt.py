"""Camera pose refinement: the gradient of the loss with respect to a camera's pose and the pose step, both in
HIP (csrc/radegs_pose.hip; include/radegs.h, "Camera pose refinement", is the specification).

The pose is six numbers on SE(3).  Moving the camera by a rigid motion is moving every Gaussian by that motion, so the pose gradient is a
fixed linear functional of the gradients the rasterizer's backward already returns for means3D, rotations and (for the view direction of
the SH colour) shs.  `tap` sits between the model's activations and the rasterizer, sees exactly those cotangents and hands the six-vector
to `delta`; nothing in the rasterizer changes.

    poses = CameraPoses(cameras, lr_translation=1e-3, lr_rotation=1e-3)
    out = gaussian_render.render(cam, gaussians, pipe, bg, kernel_size, pose=poses);  loss(out).backward();  poses.step(cam.uid)

The gradient is linear in what the backward returns: with the reference's argument slip left on (the default) it inherits the slip, which
kernel_size > 0 makes visible.  Not covered: intrinsics, integrate(), view_parallel."""
import numpy as np
import torch

import geom_host as gh
from diff_gaussian_rasterization import _C

KEEP_LAST = False   # test hook: when True the tap's backward leaves what it saw in LAST
LAST = None


def _lib():
    return _C.library()


def _rows(t, name, cols, P=None):
    _C._require_gpu(t, name)
    if t.dtype != torch.float32 or t.dim() < 2 or tuple(t.shape[1:]) != cols or (P is not None and t.shape[0] != P):
        raise RuntimeError(f"pose_gradient: `{name}` must be float32 of shape ({'P' if P is None else P}, {', '.join(map(str, cols))}), got "
                           f"{str(t.dtype).replace('torch.', '')} {tuple(t.shape)}")
    return t.detach().contiguous()


def pose_gradient(means3D, rotations, shs, sh_degree, campos, viewmatrix, dL_dmeans3D, dL_drotations, dL_dsh):
    """radegs_pose_gradient on tensors: float64 [12] on the inputs' device, g_xi (world-frame twist; translation then rotation) and g_tau
    (camera-frame twist).  Two launches on the current stream, no atomics, nothing read back; two calls give the same bits."""
    sh_degree = int(sh_degree)
    if not 0 <= sh_degree <= 3:
        raise RuntimeError(f"pose_gradient: sh_degree {sh_degree} is outside 0 .. 3")
    if not isinstance(shs, torch.Tensor) or shs.dim() != 3 or shs.shape[2] != 3 or not (sh_degree + 1) ** 2 <= shs.shape[1] <= 16:
        raise RuntimeError(f"pose_gradient: `shs` must be (P, M, 3) with {(sh_degree + 1) ** 2} <= M <= 16 for degree {sh_degree}")
    means3D = _rows(means3D, "means3D", (3,))
    P, M, dev = means3D.shape[0], shs.shape[1], means3D.device
    rotations, shs = _rows(rotations, "rotations", (4,), P), _rows(shs, "shs", (M, 3), P)
    gm, gr, gs = _rows(dL_dmeans3D, "dL_dmeans3D", (3,), P), _rows(dL_drotations, "dL_drotations", (4,), P), _rows(dL_dsh, "dL_dsh", (M, 3), P)
    for t, name, n in ((campos, "campos", 3), (viewmatrix, "viewmatrix", 16)):
        _C._require_gpu(t, name)
        if t.dtype != torch.float32 or t.numel() != n:
            raise RuntimeError(f"pose_gradient: `{name}` must hold {n} float32 values")
    if any(t.device != dev for t in (rotations, shs, gm, gr, gs, campos, viewmatrix)):
        raise RuntimeError("pose_gradient: the tensors are on different devices")
    campos, viewmatrix = campos.detach().contiguous(), viewmatrix.detach().contiguous()
    nbytes = _lib().radegs_pose_gradient_bytes(P)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(12, dtype=torch.float64, device=dev)
    gh.call(_C._SIGNATURES, "radegs_pose_gradient", dev, P, M, sh_degree, means3D, rotations, shs, campos, viewmatrix, gm, gr, gs, work, nbytes, out)
    return out


class _Tap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, rotations, shs, delta, camera, sh_degree):
        ctx.save_for_backward(means3D, rotations, shs)
        ctx.camera, ctx.sh_degree, ctx.delta_like = camera, int(sh_degree), (delta.dtype, delta.device)
        return means3D, rotations, shs

    @staticmethod
    def backward(ctx, g_means3D, g_rotations, g_shs):
        global LAST
        means3D, rotations, shs = ctx.saved_tensors
        g_delta = None
        if ctx.needs_input_grad[3]:
            zeros = lambda g, like: torch.zeros_like(like) if g is None else g
            gm, gr, gs = zeros(g_means3D, means3D), zeros(g_rotations, rotations), zeros(g_shs, shs)
            cam = ctx.camera
            out = pose_gradient(means3D, rotations, shs, ctx.sh_degree, cam.camera_center, cam.world_view_transform, gm, gr, gs)
            g_delta = out[6:].to(dtype=ctx.delta_like[0], device=ctx.delta_like[1])
            if KEEP_LAST:
                LAST = {"means3D": means3D.detach(), "rotations": rotations.detach(), "shs": shs.detach(), "dL_dmeans3D": gm.detach().clone(),
                        "dL_drotations": gr.detach().clone(), "dL_dsh": gs.detach().clone(), "out12": out}
        return g_means3D, g_rotations, g_shs, g_delta, None, None


def tap(means3D, rotations, shs, delta, camera, sh_degree):
    """Returns (means3D, rotations, shs) unchanged -- no launch in the forward -- for the rasterizer to read.  In the backward their
    cotangents pass through untouched and `delta` (a six-vector whose value is not read) receives g_tau, the gradient with respect to the
    camera-frame twist of `camera` (world_view_transform and camera_center are read at backward time)."""
    if shs is None or means3D is None or rotations is None:
        raise RuntimeError("pose tap: means3D, rotations and shs are needed -- the pose gradient is formed from their cotangents")
    if not isinstance(delta, torch.Tensor) or delta.numel() != 6:
        raise RuntimeError("pose tap: `delta` must be a six-vector")
    return _Tap.apply(means3D, rotations, shs, delta, camera, sh_degree)


class CameraPoses:
    """The refinable poses of `cameras` (scene_io.Camera or anything with uid, R, T, world_view_transform, projection_matrix,
    full_proj_transform, camera_center): a float64 master of every world-to-camera matrix, Adam moments [N, 6] and a step count per camera.
    step(uid) rewrites that camera's three tensors IN PLACE, so every holder of the camera sees the refined pose; the host-side R / T (what
    compute_3D_filter, camera_to_JSON and checkpoints read) follow at sync(), the one host read."""

    def __init__(self, cameras, lr_translation=1e-3, lr_rotation=1e-3, betas=(0.9, 0.999), eps=1e-15):
        self.cameras = list(cameras)
        if not self.cameras:
            raise RuntimeError("CameraPoses: no cameras")
        self.lr_translation, self.lr_rotation, self.betas, self.eps = float(lr_translation), float(lr_rotation), (float(betas[0]), float(betas[1])), float(eps)
        self.index = {}
        for i, cam in enumerate(self.cameras):
            if cam.uid in self.index:
                raise RuntimeError(f"CameraPoses: uid {cam.uid} appears twice")
            if float(getattr(cam, "scale", 1.0)) != 1.0 or np.any(np.asarray(getattr(cam, "trans", 0.0)) != 0.0):
                raise RuntimeError(f"CameraPoses: camera {cam.uid} has a scene translation / scale; its pose is not (R, T) alone")
            for name, n in (("world_view_transform", 16), ("projection_matrix", 16), ("full_proj_transform", 16), ("camera_center", 3)):
                t = getattr(cam, name)
                _C._require_gpu(t, name)
                if t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
                    raise RuntimeError(f"CameraPoses: camera {cam.uid}: `{name}` must be {n} contiguous float32 values")
            self.index[cam.uid] = i
        dev = self.device = self.cameras[0].world_view_transform.device
        n = len(self.cameras)
        # the master starts from the float32 matrix the rasterizer has been reading, so that the first step moves the pose by the step alone
        self.master = torch.stack([c.world_view_transform.detach().reshape(4, 4).t().double() for c in self.cameras]).contiguous()
        self.exp_avg = torch.zeros(n, 6, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, 6, dtype=torch.float32, device=dev)
        self.steps = [0] * n
        self._delta = {}

    def delta(self, uid):
        """a fresh zero six-vector for `uid`'s next backward; step(uid) reads its .grad"""
        d = torch.zeros(6, dtype=torch.float64, device=self.device, requires_grad=True)
        self._delta[uid] = d
        return d

    def grad(self, uid):
        d = self._delta.get(uid)
        return None if d is None else d.grad

    @torch.no_grad()
    def step(self, uid):
        """Adam on the camera-frame twist and w2c <- Exp(tau) w2c, one launch; the gradient is consumed"""
        i, g = self.index[uid], self.grad(uid)
        if g is None:
            raise RuntimeError(f"CameraPoses.step: camera {uid} has no pose gradient -- render it with pose= and run the backward first")
        cam = self.cameras[i]
        self.steps[i] += 1
        gh.call(_C._SIGNATURES, "radegs_pose_step", self.device, self.master[i], g, self.exp_avg[i], self.exp_avg_sq[i], float(self.steps[i]),
                self.lr_translation, self.lr_rotation, self.betas[0], self.betas[1], self.eps, cam.projection_matrix, cam.world_view_transform,
                cam.full_proj_transform, cam.camera_center)
        del self._delta[uid]

    def world_to_camera(self):
        """[N, 4, 4] float64 on the host: the one read-back"""
        return self.master.cpu().numpy()

    def sync(self):
        """refreshes every camera's host-side R (stored transposed, as upstream's) and T from the masters"""
        w2c = self.world_to_camera()
        for i, cam in enumerate(self.cameras):
            cam.R, cam.T = np.ascontiguousarray(w2c[i, :3, :3].T), w2c[i, :3, 3].copy()
        return w2c

    def state_dict(self):
        c = lambda name: torch.stack([getattr(cam, name).detach().reshape(-1) for cam in self.cameras]).clone()
        return {"uids": [cam.uid for cam in self.cameras], "master": self.master.clone(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "steps": list(self.steps), "world_view_transform": c("world_view_transform"), "full_proj_transform": c("full_proj_transform"),
                "camera_center": c("camera_center")}

    @torch.no_grad()
    def load_state_dict(self, state):
        """restores the masters, the Adam state and -- bit for bit, as the step kernel left them -- every camera's three tensors, then sync()"""
        if list(state["uids"]) != [cam.uid for cam in self.cameras]:
            raise RuntimeError("CameraPoses.load_state_dict: the state belongs to another set of cameras")
        self.master.copy_(state["master"])
        self.exp_avg.copy_(state["exp_avg"])
        self.exp_avg_sq.copy_(state["exp_avg_sq"])
        self.steps = [int(s) for s in state["steps"]]
        for i, cam in enumerate(self.cameras):
            for name in ("world_view_transform", "full_proj_transform", "camera_center"):
                t = getattr(cam, name)
                t.copy_(state[name][i].to(t.device).reshape(t.shape))
        self._delta = {}
        self.sync()
