"""Drop-in for `from tetranerf.utils.extension import cpp` (mesh_extract_tetrahedra.py:18): `cpp.triangulate(points)` is tetranerf's CGAL
Delaunay_triangulation_3 binding upstream (py_binding.cpp:26-43) and delaunay.triangulate here -- the same signature, int32 [T,4] on
`points.device`, computed on the GPU."""
from . import cpp

__all__ = ["cpp"]
