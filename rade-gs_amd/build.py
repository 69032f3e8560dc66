"""Builds libradegs_hip.so (the C-ABI HIP library, include/radegs.h) for gfx950, in-tree.

    python rade-gs_amd/build.py [--force]

hipcc cross-compiles without a GPU.  Flags that matter:
  -ffp-contract=off        one rounding per fp32 op; fma only where the source spells fmaf().  This is
                           what makes radii / tile rects / depth keys / blend decisions bit-identical to
                           the CPU oracle (see csrc/rg_math.h, csrc/rg_blend.h).
  -munsafe-fp-atomics      global_atomic_add_f32 in hardware (no CAS loop) for the gradient accumulators.
  -fno-slp-vectorize       keeps clang from fusing the two pixels' (or any two independent) fp32 chains into v_pk_* instructions:
                           packed fp32 issues as two passes on gfx950 (no throughput gain, scripts/ubench/valu_rates.hip) and the
                           fused chains lose the instruction-level parallelism of two independent ones -- measured on C2: forward
                           blend 0.36 -> 0.32 ms, backward 0.60 -> 0.57, preprocess_bwd 0.21 -> 0.18.
  (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt stays on: IEEE divide/sqrt.)
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "diff_gaussian_rasterization")
OBJ_DIR = os.path.join(HERE, "build")
LIB = os.path.join(OUT_DIR, "libradegs_hip.so")
CHECK_LIB = os.path.join(OUT_DIR, "libradegs_prims_check.so")   # test-only: rocPRIM cross-check of the hand-written sorts
# test-only: C entry points over radegs_sort.hip's primitives with the instantiation override (tests/test_gpu_sort_scan.py); sortcheck.o +
# radegs_sort.o in a shared object of its own, next to the rocPRIM cross-check -- never linked into the product, not package data
SORT_CHECK_SRC = os.path.join(CSRC, "radegs_sort_check.hip")
SORT_CHECK_LIB = os.path.join(OUT_DIR, "libradegs_sort_check.so")
# test-only: the device build of rg_blend.h's decision pieces behind C entry points (tests/test_gpu_stream_lists.py); same FLAGS as the
# product, a shared object of its own -- never linked into the product, not package data
BLEND_CHECK_SRC = os.path.join(CSRC, "radegs_blend_check.hip")
BLEND_CHECK_LIB = os.path.join(OUT_DIR, "libradegs_blend_check.so")
# test-only: the host fmaf-chain restatement of the image-evaluation convolution (tests/imageeval_restatement.py), g++ over the header the
# kernel states its K order in; -ffp-contract=off so that fmaf() stays the only fused step -- never linked into the product, not package data
CONV_CHAIN_CHECK_SRC = os.path.join(CSRC, "radegs_conv_chain_check.cpp")
CONV_CHAIN_CHECK_LIB = os.path.join(OUT_DIR, "libradegs_conv_chain_check.so")
ARCH = "gfx950"   # the only target: kernels use gfx950's 160 KB LDS (radegs_sort.hip's 32-item scatter needs 70 KB per workgroup), its DPP /
                  # bank-mask forms and wave64 tilings -- changing this does not give a working gfx90a / gfx942 library
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
         "-fno-slp-vectorize", "-Wno-unused-value", "-I", CSRC]
UNITS = {
    "radegs_prims": ["radegs_prims.hip"],
    "radegs_sort": ["radegs_sort.hip", "rg_prims.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_kernels": ["radegs_kernels.hip", "rg_launch.inc", "rg_streams.inc", "rg_integrate.inc", "rg_per_gaussian.inc", "rg_blend_bwd_body.inc", "rg_math.h", "rg_blend.h", "rg_preprocess.h", "rg_preprocess_bwd.h",
                       "rg_layout.h", "rg_prims.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_normals": ["radegs_normals.hip", "rg_reduce.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_filter3d": ["radegs_filter3d.hip", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_activate": ["radegs_activate.hip", "rg_activate.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_photometric": ["radegs_photometric.hip", "rg_reduce.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_adam": ["radegs_adam.hip", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_densify": ["radegs_densify.hip", "rg_prims.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_knn": ["radegs_knn.hip", "rg_prims.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_tetmesh": ["radegs_tetmesh.hip", "rg_filter.h", "rg_prims.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_mesheval": ["radegs_mesheval.hip", "rg_prims.h", "rg_reduce.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_tsdf": ["radegs_tsdf.hip", "rg_mc_tables.h", "rg_prims.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_tnteval": ["radegs_tnteval.hip", "rg_prims.h", "rg_reduce.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_tntcull": ["radegs_tntcull.hip", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_meshclean": ["radegs_meshclean.hip", "rg_filter.h", "rg_prims.h", "rg_reduce.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_delaunay": ["radegs_delaunay.hip", "rg_delaunay_cell.h", "rg_prims.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_appearance": ["radegs_appearance.hip", "rg_reduce.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    "radegs_imageeval": ["radegs_imageeval.hip", "rg_conv_chain.h", "rg_reduce.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    # no entry in UNIT_FLAGS: the default -ffp-contract=off and IEEE divide / sqrt are what reset_opacity and the init state in the header
    "radegs_modelio": ["radegs_modelio.hip", os.path.join("..", "..", "include", "radegs.h")],
    # default FLAGS too: -ffp-contract=off keeps the composite's float64 products and sums apart, as NumPy computes them
    "radegs_sceneio": ["radegs_sceneio.hip", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    # default FLAGS: the unit is held to tests/unbounded_restatement.py bit for bit, which needs -ffp-contract=off and IEEE divide / sqrt
    "radegs_unbounded": ["radegs_unbounded.hip", "rg_mc_tables.h", "rg_prims.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    # default FLAGS: the RANSAC's per-pair decisions are held to tests/evalio_restatement.py, one rounding per operation, IEEE divide / sqrt
    "radegs_evalio": ["radegs_evalio.hip", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
    # default FLAGS: the pose gradient is held to tests/pose_restatement.py bit for bit, one rounding per fp64 operation, IEEE divide / sqrt
    "radegs_pose": ["radegs_pose.hip", "rg_pose.h", "rg_reduce.h", os.path.join("..", "..", "include", "radegs.h")],
    # default FLAGS: the quadrics and the Jacobi solve are held to tests/simplify_restatement.py bit for bit, one rounding per fp64 operation
    "radegs_meshsimplify": ["radegs_meshsimplify.hip", "rg_filter.h", "rg_prims.h", "rg_workspace.h", os.path.join("..", "..", "include", "radegs.h")],
}
# Units outside the rasterizer's decision chain have no bit-exactness contract with the oracle: let them contract to fma.
# radegs_filter3d calls expf: under `fast` the compiler also contracts INSIDE expf's expansion (x*log2e - round(x*log2e) becomes one fma and
# the rounding residue of the product is then added a second time), which costs 0.4 ulp per unit of |x|: sigmoid(-30) was 12 ulps off.
# `on` contracts within the source's own expressions only (this also changes which products of compute_3D_filter's kernels fuse: same
# formulas, last-bit differences).  radegs_photometric calls exp on the host only; radegs_appearance still calls expf under `fast`: known,
# not covered by a test of this kind yet.
# radegs_activate restates radegs_filter3d's scale / opacity expressions (csrc/rg_activate.h) and is held to its bits: the same flag.
UNIT_FLAGS = {"radegs_normals": ["-ffp-contract=fast"], "radegs_filter3d": ["-ffp-contract=on"], "radegs_activate": ["-ffp-contract=on"],
              "radegs_photometric": ["-ffp-contract=fast"], "radegs_appearance": ["-ffp-contract=fast"]}


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "hipcc")
    os.makedirs(OBJ_DIR, exist_ok=True)
    objs = []
    for name, files in UNITS.items():
        deps = [os.path.join(CSRC, f) for f in files] + [os.path.abspath(__file__)]
        obj = os.path.join(OBJ_DIR, name + ".o")
        if force or _stale(obj, deps):
            cmd = [hipcc] + FLAGS + UNIT_FLAGS.get(name, []) + ["-c", os.path.join(CSRC, files[0]), "-o", obj]
            if verbose:
                print("[radegs build]", " ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        if name == "radegs_prims":   # never linked into the product: its own shared object, loaded on demand (RADEGS_PRIMS=rocprim)
            if force or _stale(CHECK_LIB, [obj]):
                cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", CHECK_LIB, obj]
                if verbose:
                    print("[radegs build]", " ".join(cmd), flush=True)
                subprocess.check_call(cmd)
            continue
        objs.append(obj)
    check_obj = os.path.join(OBJ_DIR, "radegs_sort_check.o")
    if force or _stale(check_obj, [SORT_CHECK_SRC, os.path.join(CSRC, "rg_prims.h"), os.path.abspath(__file__)]):
        cmd = [hipcc] + FLAGS + ["-c", SORT_CHECK_SRC, "-o", check_obj]
        if verbose:
            print("[radegs build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    sort_obj = os.path.join(OBJ_DIR, "radegs_sort.o")
    if force or _stale(SORT_CHECK_LIB, [check_obj, sort_obj]):
        cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", SORT_CHECK_LIB, check_obj, sort_obj]
        if verbose:
            print("[radegs build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    blend_obj = os.path.join(OBJ_DIR, "radegs_blend_check.o")
    if force or _stale(blend_obj, [BLEND_CHECK_SRC, os.path.join(CSRC, "rg_blend.h"), os.path.join(CSRC, "rg_math.h"), os.path.abspath(__file__)]):
        cmd = [hipcc] + FLAGS + ["-c", BLEND_CHECK_SRC, "-o", blend_obj]
        if verbose:
            print("[radegs build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    if force or _stale(BLEND_CHECK_LIB, [blend_obj]):
        cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", BLEND_CHECK_LIB, blend_obj]
        if verbose:
            print("[radegs build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    if force or _stale(CONV_CHAIN_CHECK_LIB, [CONV_CHAIN_CHECK_SRC, os.path.join(CSRC, "rg_conv_chain.h"), os.path.abspath(__file__)]):
        cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, CONV_CHAIN_CHECK_SRC, "-o", CONV_CHAIN_CHECK_LIB]
        if verbose:
            print("[radegs build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    if force or _stale(LIB, objs + [os.path.abspath(__file__)]):
        cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print("[radegs build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


TORCH_BINDING_SRC = os.path.join(CSRC, "torch_binding", "radegs_torch_binding.cpp")
TORCH_BINDING_NAME = "_C_torch"


def torch_binding_path():
    import sysconfig
    return os.path.join(OUT_DIR, TORCH_BINDING_NAME + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))


def build_torch_binding(force=False, verbose=True):
    """diff_gaussian_rasterization/_C_torch*.so: the reference's pybind `_C` module (DGR/ext.cpp:15-19 -- rasterize_gaussians,
    rasterize_gaussians_backward, mark_visible, integrate_gaussians_to_points with torch::Tensor arguments) as HOST C++ over the C ABI
    of libradegs_hip.so.  No device code in it: g++ against the torch / pybind11 / HIP runtime headers, linked to the library next to it
    ($ORIGIN rpath).  `RADEGS_BINDING=torch` makes the operator package use it instead of the ctypes binding."""
    import sysconfig

    import torch
    from torch.utils import cpp_extension as ce
    lib = build(force=False, verbose=verbose)
    out = torch_binding_path()
    header = os.path.join(HERE, "..", "include", "radegs.h")
    if not (force or _stale(out, [TORCH_BINDING_SRC, header, lib, os.path.abspath(__file__)])):
        return out
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    inc = ce.include_paths() + [os.path.join(rocm, "include"), sysconfig.get_paths()["include"], os.path.join(HERE, "..", "include")]
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-deprecated-declarations", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           "-DTORCH_EXTENSION_NAME=" + TORCH_BINDING_NAME, "-DTORCH_API_INCLUDE_EXTENSION_H",
           "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI)]
    for i in inc:
        cmd += ["-isystem", i]
    cmd += [TORCH_BINDING_SRC, "-o", out, "-L" + tlib, "-L" + OUT_DIR, "-L" + os.path.join(rocm, "lib"), "-lradegs_hip", "-lc10", "-lc10_hip", "-ltorch_cpu",
            "-ltorch_hip", "-ltorch", "-ltorch_python", "-lamdhip64", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + tlib, "-Wl,-rpath," + os.path.join(rocm, "lib")]
    if verbose:
        print("[radegs build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
    if "--torch-binding" in sys.argv:
        print(build_torch_binding(force="--force" in sys.argv))
