"""`simple_knn._C` -- `distCUDA2(points)`: mean squared distance of every point to its 3 nearest neighbours, as the reference
uses it to initialise the Gaussian scales (scene/gaussian_model.py:315).  The reference's own implementation lives in the
un-vendored `simple-knn` submodule (CUDA); this one calls libradegs_hip.so (radegs_knn_mean_dist2).  GPU only."""
import ctypes

import torch

import geom_host as gh
from diff_gaussian_rasterization import _C as _radegs

_SIGNATURES = {"radegs_knn_scratch_bytes": (ctypes.c_size_t, [ctypes.c_int]),
               "radegs_knn_mean_dist2": (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 4)}


def _lib():
    return _radegs.bind(_SIGNATURES)


def distCUDA2(points):
    _radegs._require_gpu(points, "points")
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.float32:
        raise RuntimeError("points must be a float32 tensor of shape (P,3)")
    pts = points.contiguous()
    P = int(pts.size(0))
    out = torch.empty(P, dtype=torch.float32, device=pts.device)
    if P == 0:
        return out
    scratch = gh.workspace(_lib().radegs_knn_scratch_bytes(P), pts.device)
    gh.call(_SIGNATURES, "radegs_knn_mean_dist2", pts.device, P, pts, scratch, out)
    return out
