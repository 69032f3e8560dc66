"""The Delaunay fixtures (tests/golden/make_golden_delaunay.py wrote them from scipy.spatial.Delaunay), shared by the CPU and GPU tiers."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name: (points, tetrahedra); the jittered cases are the exactly degenerate ones
CASES = {"random4": (4, 1), "random5": (5, 3), "random8": (8, 10), "random64": (64, 296), "random65": (65, 296), "random200": (200, 1133),
         "random1000": (1000, 6380), "sphere120": (120, 343), "shell151": (151, 296), "clusters120": (120, 643), "grid64": (64, 308),
         "boxes270": (270, 1591)}
JITTERED = ("grid64", "boxes270")
_cache = {}


def load(name):
    """the fixture as a dict of arrays; loaded once, never modified"""
    if name not in _cache:
        with np.load(os.path.join(GOLDEN, f"delaunay_{name}.npz")) as z:
            fx = {k: z[k] for k in z.files}
        for v in fx.values():
            v.setflags(write=False)
        assert fx["points"].shape == (CASES[name][0], 3) and fx["cells"].shape == (CASES[name][1], 4), name
        assert (float(fx["jitter"]) > 0) == (name in JITTERED)
        _cache[name] = fx
    return _cache[name]
