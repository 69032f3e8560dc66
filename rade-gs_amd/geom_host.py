"""The host layer of every module that calls libradegs_hip.so outside the rasterizer's own entry points (diff_gaussian_rasterization/_C.py):
binding a module's table of C signatures to the library, call() -- the one routine through which a launching entry point is reached -- the
return-code check, the workspace buffer, and the argument checks that refuse rather than convert."""
import ctypes
import math

import torch

from diff_gaussian_rasterization import _C

ERR_TOO_LARGE = -6   # RADEGS_ERR_TOO_LARGE (include/radegs.h)
# the C types of the signature tables
vp, ll, i32, sz, f32, f64 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_double
pf32, pf64 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
bind = _C.bind   # sets a module's table {"radegs_x": (restype, [argtypes...]), ...} on the library, once, and returns the library


def check(rc, what):
    if rc == ERR_TOO_LARGE:
        raise RuntimeError(f"{what}: the input is larger than the 32-bit sort / scan primitives address (include/radegs.h)")
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc})")


def call(signatures, name, dev, *args):
    """One launching native call, the only way a module reaches an `int radegs_x(..., void* stream)` entry point: `name` with the prototype
    the module's table `signatures` declares for it, under `dev`'s device context, on `dev`'s current stream (appended as the last
    argument), the return code through check().  A tensor stands for its device pointer, None for NULL; every other value goes to ctypes as
    it is.  A tensor that is not contiguous, or lies on another GPU than `dev`, is refused before anything is called (host tensors pass:
    pinned buffers are handed over on purpose); nothing is converted or copied.  `args` keeps the tensors alive for the call."""
    lib = bind(signatures)
    if name not in signatures:
        raise RuntimeError(f"{name} is not in the calling module's table of signatures")
    restype, argtypes = signatures[name]
    if restype is not ctypes.c_int or not argtypes or argtypes[-1] is not ctypes.c_void_p:
        raise RuntimeError(f"{name} is not declared as `int {name}(..., void* stream)`")
    if len(args) + 1 != len(argtypes):
        raise RuntimeError(f"{name} takes {len(argtypes) - 1} arguments before the stream, got {len(args)}")
    dev = torch.device(dev)
    if dev.index is None:       # plain "cuda" means the current device, as it does to torch
        dev = torch.device(dev.type, torch.cuda.current_device())
    values = []
    for i, a in enumerate(args):
        if isinstance(a, torch.Tensor):
            if not a.is_contiguous():
                raise RuntimeError(f"{name}: argument {i} is a tensor that is not contiguous")
            if a.is_cuda and a.device != dev:
                raise RuntimeError(f"{name}: argument {i} is a tensor on {a.device}, the call runs on {dev}")
            a = a.data_ptr()
        values.append(a)
    with torch.cuda.device(dev):
        check(getattr(lib, name)(*values, torch.cuda.current_stream(dev).cuda_stream), name)


def workspace(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def doubles(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def positive(value, name):
    if not (isinstance(value, (int, float)) and not isinstance(value, bool) and math.isfinite(value) and value > 0):
        raise RuntimeError(f"`{name}` must be a positive finite number")
    return float(value)


def points(t, name, dtype=torch.float64):
    """a contiguous [N,3] GPU tensor of the kernels' type; anything else is refused, nothing is converted silently"""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.size(1) != 3:
        raise RuntimeError(f"`{name}` must be a tensor of shape (N,3)" + (f", got {tuple(t.shape)}" if isinstance(t, torch.Tensor) else ""))
    if t.dtype != dtype:
        raise RuntimeError(f"`{name}` must be {str(dtype).replace('torch.', '')}, got {str(t.dtype).replace('torch.', '')}")
    _C._require_gpu(t, name)
    return t.detach().contiguous()


def finite(t, name):
    if t.numel() and not bool(torch.isfinite(t).all()):
        raise RuntimeError(f"`{name}` holds non-finite values")


def faces_type(faces):
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.size(1) != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise RuntimeError("`faces` must be an int32 or int64 tensor of shape (F,3)")


def faces(faces, V):
    faces_type(faces)
    _C._require_gpu(faces, "faces")
    if faces.numel():
        lo, hi = torch.aminmax(faces)
        lo, hi = int(lo), int(hi)
        if lo < 0 or hi >= V:
            raise RuntimeError(f"`faces` holds indices in [{lo}, {hi}], outside the {V} vertices")
    return faces.detach().to(torch.int64).contiguous()
