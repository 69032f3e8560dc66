"""Camera pose refinement on the GPU (csrc/radegs_pose.hip, pose_opt.py, gaussian_render.render(pose=...)) against tests/pose_restatement.py.

1. radegs_pose_gradient alone, bit for bit against the restatement (whose sum order is mesheval_restatement.fixed_order_sum): P at the block
   edges and at the switch to the grid-stride loop (kSumBlocks x 256 = 262144), degrees 0-3, synthetic cotangents with zero-DC rows and
   all-zero rows, workspace and outputs poisoned, two runs with identical bits.
2. End to end on the four fixture scenes (tests/golden/pose_*.npz, P = 300, 64 x 48): delta.grad equals the restatement fed the very
   tensors the tap saw, bit for bit, and lies within the fixture's band of the float64 oracle's value.  The band is measured, not chosen
   (tests/golden/make_golden_pose.py): per triple of g_tau, the Euclidean deviation of the float32 ORACLE's pose gradient from the float64
   one, maximum over the four scenes, times 4 = 0.475 (translation) and 1.335 (rotation), next to triples of norm 42 .. 286 and
   137 .. 1013: 1e-3 of the gradient.  Measured: the HIP path's distances equal the float32 oracle's own to three digits (a quarter of the
   band at most).
3. The tap changes nothing else: under the deterministic backward, images and all parameter gradients are bit-identical with and without pose=.
4. radegs_pose_step against its restatement: Adam moments bit for bit, the float64 master within 16 x 2^-52 x max|entry| (the device's sin at
   <= 2 ulp and three-term dot products), the float32 tensors within 1 ulp, written in place (data_ptr).  Measured: all equal.
5. Recovery: P = 2000, 96 x 64, six jittered views, targets from the true poses, every camera off by 0.5 degrees about a random axis and 0.01
   in translation, Gaussians frozen, 200 pose steps each: every camera's rotation error and centre error end below half their start
   (measured on the MI355X at a learning rate of 1e-3, a tenth of the perturbation per step: worst ratios 0.033 for the rotation and 0.067
   for the centre; at 2e-4 the same run ends at 0.26 and 0.57 and misses).  On the same degree-3 scene the gradient without the SH correction
   term differs from the kernel's.
6. Refusals of render(pose=...) raise before anything is launched."""
import math
import os
import types

import numpy as np
import pytest
import torch

import pose_restatement as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [1, 63, 64, 255, 256, 257, 1000, 262144, 262145, 262401]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if np.asarray(a).dtype == np.float64 else np.int32)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------------
def synthetic(P, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    m = (rng.standard_normal((P, 3)) * 3.0).astype(f)
    q = rng.standard_normal((P, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f)
    sh = np.concatenate([rng.standard_normal((P, 1, 3)), 0.3 * rng.standard_normal((P, 15, 3))], 1).astype(f)
    g, gq, dsh = rng.standard_normal((P, 3)).astype(f), rng.standard_normal((P, 4)).astype(f), rng.standard_normal((P, 16, 3)).astype(f)
    kind = rng.random(P)
    dsh[kind < 0.3, 0, :] = 0.0                       # zero DC cotangent, the rest of the row alive: c_i is defined as zero
    dead = kind > 0.7                                 # an invisible Gaussian: every cotangent zero
    g[dead], gq[dead], dsh[dead] = 0.0, 0.0, 0.0
    if P > 2:
        dsh[2, 0, :] = (0.0, 0.0, 0.25)               # one DC entry alone keeps the row alive
    campos = np.array([0.3, -0.2, 7.5], f)            # outside the cloud's bulk; no direction of length 0
    R = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    vm = np.eye(4)
    vm[:3, :3], vm[3, :3] = R.T, rng.standard_normal(3)
    return m, q, sh, campos, vm.astype(f), g, gq, dsh


def call_kernel(L, C, P, deg, dev_arrays, poison):
    m, q, sh, campos, vm, g, gq, dsh = dev_arrays
    nbytes = L.radegs_pose_gradient_bytes(P)
    assert nbytes == max(1, min(-(-P // 256), 1024)) * 48
    work = torch.full((nbytes // 8,), poison, dtype=torch.float64, device=DEV)
    out = torch.full((12,), poison, dtype=torch.float64, device=DEV)
    rc = L.radegs_pose_gradient(P, 16, deg, C._ptr(m), C._ptr(q), C._ptr(sh), C._ptr(campos), C._ptr(vm), C._ptr(g), C._ptr(gq), C._ptr(dsh),
                                C._ptr(work), nbytes, C._ptr(out), C._stream(torch.device(DEV)))
    assert rc == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("P", SIZES)
def test_kernel_equals_the_restatement_bit_for_bit(P):
    import diff_gaussian_rasterization._C as C
    import pose_opt
    L = C.library()
    host = synthetic(P, 1000 + P % 997)
    dev_arrays = [torch.from_numpy(a).to(DEV) for a in host]
    m, q, sh, campos, vm, g, gq, dsh = host
    for deg in range(4):
        want = np.concatenate(pr.pose_gradient(m, q, sh, deg, campos, vm, g, gq, dsh))
        assert np.isfinite(want).all() and (P < 63 or np.abs(want).min() > 0)
        first = call_kernel(L, C, P, deg, dev_arrays, float("nan"))
        second = call_kernel(L, C, P, deg, dev_arrays, 1e300)
        assert np.array_equal(bits(first), bits(second)), (P, deg)
        assert np.array_equal(bits(first), bits(want)), (P, deg, first, want)
    wrapped = pose_opt.pose_gradient(*dev_arrays[:3], 3, *dev_arrays[3:]).cpu().numpy()
    assert np.array_equal(bits(wrapped), bits(first))


def test_no_gaussians_gives_zeros_and_bad_arguments_are_refused():
    import diff_gaussian_rasterization._C as C
    import pose_opt
    e = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    out = pose_opt.pose_gradient(e(0, 3), e(0, 4), e(0, 16, 3), 3, e(3), torch.eye(4, device=DEV), e(0, 3), e(0, 4), e(0, 16, 3))
    assert out.shape == (12,) and not out.any()
    with pytest.raises(RuntimeError, match="sh_degree"):
        pose_opt.pose_gradient(e(2, 3), e(2, 4), e(2, 16, 3), 4, e(3), e(4, 4), e(2, 3), e(2, 4), e(2, 16, 3))
    with pytest.raises(RuntimeError, match="shs"):
        pose_opt.pose_gradient(e(2, 3), e(2, 4), e(2, 4, 3), 3, e(3), e(4, 4), e(2, 3), e(2, 4), e(2, 4, 3))
    with pytest.raises(RuntimeError, match="dL_drotations"):
        pose_opt.pose_gradient(e(2, 3), e(2, 4), e(2, 16, 3), 3, e(3), e(4, 4), e(2, 3), e(3, 4), e(2, 16, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        pose_opt.pose_gradient(e(2, 3).cpu(), e(2, 4), e(2, 16, 3), 3, e(3), e(4, 4), e(2, 3), e(2, 4), e(2, 16, 3))
    L = C.library()
    w = torch.zeros(6, dtype=torch.float64, device=DEV)
    o = torch.zeros(12, dtype=torch.float64, device=DEV)
    args = [C._ptr(t) for t in (e(2, 3), e(2, 4), e(2, 16, 3), e(3), e(4, 4), e(2, 3), e(2, 4), e(2, 16, 3))]
    assert L.radegs_pose_gradient(2, 16, 3, *args, C._ptr(w), 47, C._ptr(o), None) == -1          # workspace one byte short
    assert L.radegs_pose_gradient(-1, 16, 3, *args, C._ptr(w), 48, C._ptr(o), None) == -1
    assert L.radegs_pose_gradient(2, 9, 3, *args, C._ptr(w), 48, C._ptr(o), None) == -1           # M below (deg + 1)^2
    assert L.radegs_pose_gradient(2, 16, 3, *args[:7], None, C._ptr(w), 48, C._ptr(o), None) == -1


# ---- 2, 3 ------------------------------------------------------------------------------------------------------------------------------------
PIPE = types.SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


class FixtureModel:
    """what gaussian_render.render reads of a model, over the fixture's already-activated tensors"""

    def __init__(self, z, requires_grad=True):
        t = lambda k: torch.from_numpy(z[k]).to(DEV).requires_grad_(requires_grad)
        self.xyz, self.rot, self.shs, self.scales, self.opacity = t("means3D"), t("rotations"), t("shs"), t("scales"), t("opacities")
        self.active_sh_degree = int(z["sh_degree"])

    @property
    def get_xyz(self):
        return self.xyz

    def activations(self, fused=None):
        return self.shs, self.rot, self.scales, self.opacity

    def leaves(self):
        return {"xyz": self.xyz, "rot": self.rot, "shs": self.shs, "scales": self.scales, "opacity": self.opacity}


def fixture_camera(z, uid=0):
    g = lambda k: torch.from_numpy(z[k]).to(DEV).contiguous()
    w2c = z["viewmatrix"].astype(np.float64).T
    return types.SimpleNamespace(uid=uid, FoVx=2 * math.atan(float(z["tanfovx"])), FoVy=2 * math.atan(float(z["tanfovy"])), image_width=int(z["W"]),
                                 image_height=int(z["H"]), world_view_transform=g("viewmatrix"), full_proj_transform=g("projmatrix"),
                                 camera_center=g("campos"), projection_matrix=g("proj"), R=w2c[:3, :3].T.copy(), T=w2c[:3, 3].copy())


def fixture_loss(z, out):
    L = 0.0
    for key, cot in (("render", "color"), ("expected_coord", "coord"), ("median_coord", "mcoord"), ("expected_depth", "depth"),
                     ("median_depth", "mdepth"), ("mask", "alpha"), ("normal", "normal")):
        c = z["cot_" + cot]
        if c.any():
            L = L + (out[key] * torch.from_numpy(c).to(DEV)).sum()
    return L


def run_fixture(z, with_pose):
    import gaussian_render
    import pose_opt
    model, cam = FixtureModel(z), fixture_camera(z)
    poses = pose_opt.CameraPoses([cam]) if with_pose else None
    out = gaussian_render.render(cam, model, PIPE, torch.from_numpy(z["bg"]).to(DEV), float(z["kernel_size"]), require_coord=bool(z["require_coord"]),
                                 require_depth=bool(z["require_depth"]), pose=poses)
    fixture_loss(z, out).backward()
    torch.cuda.synchronize()
    return model, out, poses


@pytest.mark.parametrize("name", ["plain", "depth", "coord", "both"])
def test_end_to_end_gradient_on_the_fixture_scenes(name, monkeypatch, capsys):
    import pose_opt
    z = np.load(os.path.join(GOLDEN, f"pose_{name}.npz"))
    monkeypatch.setattr(pose_opt, "KEEP_LAST", True)
    _, _, poses = run_fixture(z, True)
    got = poses.grad(0).cpu().numpy()
    saw = {k: v.cpu().numpy() for k, v in pose_opt.LAST.items()}
    want = pr.pose_gradient(saw["means3D"], saw["rotations"], saw["shs"], 3, z["campos"], z["viewmatrix"], saw["dL_dmeans3D"], saw["dL_drotations"],
                            saw["dL_dsh"])[1]
    assert got.dtype == np.float64 and np.array_equal(bits(got), bits(want)) and np.array_equal(bits(saw["out12"][6:]), bits(want))
    dev = got - z["g_tau_64"]
    d = np.array([np.linalg.norm(dev[:3]), np.linalg.norm(dev[3:])])
    with capsys.disabled():
        print(f"\npose_{name}: |delta.grad - float64 oracle| = {d[0]:.3e} (translation), {d[1]:.3e} (rotation); band {z['band_tau'][0]:.3e}, "
              f"{z['band_tau'][1]:.3e}; the float32 oracle: {np.linalg.norm((z['g_tau_32'] - z['g_tau_64'])[:3]):.3e}, "
              f"{np.linalg.norm((z['g_tau_32'] - z['g_tau_64'])[3:]):.3e}")
    assert np.all(d <= z["band_tau"]), (d, z["band_tau"])


def test_the_tap_changes_nothing_else(monkeypatch):
    import diff_gaussian_rasterization._C as C
    monkeypatch.setenv("RADEGS_STREAMS", "0")
    monkeypatch.setenv("RADEGS_DETERMINISTIC", "1")
    C.reload_env()
    z = np.load(os.path.join(GOLDEN, "pose_both.npz"))
    plain, out_plain, _ = run_fixture(z, False)
    tapped, out_tapped, poses = run_fixture(z, True)
    assert poses.grad(0) is not None and bool(poses.grad(0).abs().sum() > 0)
    for k in out_plain:
        a, b = out_plain[k], out_tapped[k]
        if k == "viewspace_points":
            a, b = a.grad, b.grad
        assert torch.equal(a.detach().view(torch.int32) if a.dtype == torch.float32 else a, b.detach().view(torch.int32) if b.dtype == torch.float32 else b), k
    for (k, a), b in zip(plain.leaves().items(), tapped.leaves().values()):
        assert a.grad is not None and bool(a.grad.abs().sum() > 0) and torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32)), k


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------------
def ulp32(want):
    return np.spacing(np.abs(np.asarray(want, np.float32)))


@pytest.mark.parametrize("case,scale_t,scale_r,steps", [("ordinary", 1e-3, 1e-3, 7), ("large", 0.2, 0.5, 5), ("no rotation", 1e-3, 0.0, 3)])
def test_pose_step_against_its_restatement(case, scale_t, scale_r, steps, capsys):
    import pose_opt
    rng = np.random.default_rng(len(case))
    z = np.load(os.path.join(GOLDEN, "pose_depth.npz"))
    cam = fixture_camera(z)
    poses = pose_opt.CameraPoses([cam], lr_translation=scale_t, lr_rotation=scale_r)
    ptrs = [t.data_ptr() for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
    master = poses.master[0].cpu().numpy().copy()
    assert np.array_equal(master, z["viewmatrix"].astype(np.float64).T)
    m, v = np.zeros(6, np.float32), np.zeros(6, np.float32)
    worst_master, worst_ulp = 0.0, 0.0
    for step in range(1, steps + 1):
        grad = rng.standard_normal(6) * np.array([30.0] * 3 + [200.0] * 3)
        poses.delta(0).grad = torch.from_numpy(grad).to(DEV)
        poses.step(0)
        master, m, v, view, full, center = pr.pose_step(master, grad, m, v, step, scale_t, scale_r, z["proj"])
        got_master = poses.master[0].cpu().numpy()
        assert np.array_equal(bits(poses.exp_avg[0].cpu().numpy()), bits(m)) and np.array_equal(bits(poses.exp_avg_sq[0].cpu().numpy()), bits(v)), step
        err = np.abs(got_master - master).max() / np.abs(master).max()
        worst_master = max(worst_master, err)
        assert err <= 16 * 2.0 ** -52, (step, err)
        assert np.array_equal(got_master[3], [0.0, 0.0, 0.0, 1.0])
        for got, want in ((cam.world_view_transform, view), (cam.full_proj_transform, full), (cam.camera_center, center)):
            got = got.cpu().numpy().reshape(want.shape)
            worst_ulp = max(worst_ulp, float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp32(want)).max()))
            assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp32(want)), (step, got, want)
        master = got_master     # the next step starts from the device's master: its sin is not the host's
    assert ptrs == [t.data_ptr() for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
    assert poses.steps == [steps] and not np.array_equal(cam.world_view_transform.cpu().numpy(), z["viewmatrix"])
    w2c = poses.sync()[0]
    assert np.array_equal(cam.R, w2c[:3, :3].T) and np.array_equal(cam.T, w2c[:3, 3]) and np.abs(w2c[:3, :3].T @ w2c[:3, :3] - np.eye(3)).max() < 1e-13
    with capsys.disabled():
        print(f"\npose step `{case}`: master off by {worst_master / 2.0 ** -52:.2f} x 2^-52 x max|entry| at worst, float32 tensors by {worst_ulp:.2f} ulp")


def test_state_dict_round_trip_restores_the_cameras_bit_for_bit():
    import pose_opt
    z = np.load(os.path.join(GOLDEN, "pose_depth.npz"))
    cam = fixture_camera(z)
    poses = pose_opt.CameraPoses([cam], 1e-3, 1e-3)
    poses.delta(0).grad = torch.arange(1.0, 7.0, dtype=torch.float64, device=DEV)
    poses.step(0)
    state = poses.state_dict()
    other_cam = fixture_camera(z)
    other = pose_opt.CameraPoses([other_cam], 1e-3, 1e-3)
    other.load_state_dict(state)
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert torch.equal(getattr(cam, name), getattr(other_cam, name)) and not torch.equal(getattr(cam, name), fixture_camera(z).__dict__[name])
    poses.sync()
    assert torch.equal(poses.master, other.master) and other.steps == [1] and np.array_equal(other_cam.R, cam.R) and np.array_equal(other_cam.T, cam.T)
    with pytest.raises(RuntimeError, match="no pose gradient"):
        poses.step(0)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------------
def test_perturbed_poses_are_recovered(monkeypatch, capsys):
    import gaussian_render
    import pose_opt
    from synth_scene import jittered_view, make_scene, projection_matrix
    base = make_scene(2000, 96, 64, sh_degree=3, mu_px=3.0, seed=271, kernel_size=0.0, require_coord=False, require_depth=False)
    proj = np.float32(projection_matrix(0.01, 100.0, 2 * math.atan(base.tanfovx), 2 * math.atan(base.tanfovy)).T)
    z = {"means3D": base.means3D.numpy(), "rotations": base.rotations.numpy(), "shs": base.shs.numpy(), "scales": base.scales.numpy(),
         "opacities": base.opacities.numpy(), "sh_degree": 3}
    model = FixtureModel(z, requires_grad=False)                       # the Gaussians are frozen
    bg = torch.zeros(3, device=DEV)
    rng = np.random.default_rng(5)

    def camera(w2c, uid):
        vm = np.float32(w2c.T)
        zz = {"viewmatrix": vm, "projmatrix": np.float32(vm.astype(np.float64) @ proj.astype(np.float64)), "campos": np.float32(-w2c[:3, :3].T @ w2c[:3, 3]),
              "proj": proj, "tanfovx": base.tanfovx, "tanfovy": base.tanfovy, "W": 96, "H": 64}
        return fixture_camera(zz, uid)

    def render(cam, poses=None):
        return gaussian_render.render(cam, model, PIPE, bg, 0.0, require_coord=False, require_depth=False, pose=poses)["render"]

    true_w2c, cams, targets = [], [], []
    for v in range(6):
        w2c = jittered_view(base, v, angle_deg=6.0, shift=0.6).viewmatrix.double().numpy().T
        with torch.no_grad():
            targets.append(render(camera(w2c, v)).clone())
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        shift = rng.standard_normal(3)
        off = pr.se3_exp(np.concatenate([0.01 * shift / np.linalg.norm(shift), math.radians(0.5) * axis]))
        true_w2c.append(w2c)
        cams.append(camera(off @ w2c, v))
    # Adam moves a component by about its learning rate per step: a tenth of the perturbation (8.7e-3 rad, 0.01) per step
    poses = pose_opt.CameraPoses(cams, lr_translation=1e-3, lr_rotation=1e-3)

    def errors():
        now = poses.world_to_camera()
        rot, cen = [], []
        for a, b in zip(now, true_w2c):
            rot.append(math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(a[:3, :3] @ b[:3, :3].T) - 1.0) / 2.0)))))
            cen.append(float(np.linalg.norm(-a[:3, :3].T @ a[:3, 3] + b[:3, :3].T @ b[:3, 3])))
        return np.array(rot), np.array(cen)

    rot0, cen0 = errors()
    monkeypatch.setattr(pose_opt, "KEEP_LAST", True)
    for it in range(200):
        for v, cam in enumerate(cams):
            loss = ((render(cam, poses) - targets[v]) ** 2).mean()
            loss.backward()
            if it == 0 and v == 0:                                     # the SH correction term is exercised on this degree-3 scene
                saw = {k: t.cpu().numpy() for k, t in pose_opt.LAST.items()}
                args = (saw["means3D"], saw["rotations"], saw["shs"], 3, cam.camera_center.cpu().numpy(), cam.world_view_transform.cpu().numpy(),
                        saw["dL_dmeans3D"], saw["dL_drotations"], saw["dL_dsh"])
                full, bare = pr.pose_gradient(*args)[1], pr.pose_gradient(*args, sh_term=False)[1]
                assert np.array_equal(bits(poses.grad(0).cpu().numpy()), bits(full))
                assert np.linalg.norm((full - bare)[3:]) > 1e-3 * np.linalg.norm(full[3:]), (full, bare)
                monkeypatch.setattr(pose_opt, "KEEP_LAST", False)
            poses.step(cam.uid)
    rot1, cen1 = errors()
    with capsys.disabled():
        print("\npose recovery, 200 steps: rotation error (degrees) " + ", ".join(f"{a:.3f}->{b:.4f}" for a, b in zip(rot0, rot1)) +
              "; centre error " + ", ".join(f"{a:.4f}->{b:.5f}" for a, b in zip(cen0, cen1)) +
              f"; worst ratios {np.max(rot1 / rot0):.3f} (rotation), {np.max(cen1 / cen0):.3f} (centre)")
    assert np.all(np.abs(rot0 - 0.5) < 1e-3)
    assert np.all(rot1 < 0.5 * rot0) and np.all(cen1 < 0.5 * cen0), (rot0, rot1, cen0, cen1)


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["compute_cov3D_python", "convert_SHs_python"])
def test_render_with_pose_refuses_what_the_tap_cannot_see(flag):
    import gaussian_render
    import pose_opt

    class Untouchable:
        active_sh_degree = 3

        @property
        def get_xyz(self):
            raise AssertionError("the refusal must come before the model is read")

        def activations(self, fused=None):
            raise AssertionError("the refusal must come before anything is launched")

    z = np.load(os.path.join(GOLDEN, "pose_plain.npz"))
    cam = fixture_camera(z)
    poses = pose_opt.CameraPoses([cam])
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=flag == "compute_cov3D_python", convert_SHs_python=flag == "convert_SHs_python")
    with pytest.raises(RuntimeError, match=flag):
        gaussian_render.render(cam, Untouchable(), pipe, torch.zeros(3, device=DEV), 0.0, pose=poses)
    with pytest.raises(RuntimeError, match="shs"):
        pose_opt.tap(torch.zeros(1, 3, device=DEV), torch.zeros(1, 4, device=DEV), None, torch.zeros(6, device=DEV), cam, 3)
