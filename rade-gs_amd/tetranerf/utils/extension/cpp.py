"""`cpp.triangulate(points)`: see the package."""
import delaunay


def triangulate(points):
    """The Delaunay tetrahedra of `points` [N,3] as int32 [T,4] on `points.device` (delaunay.triangulate with its defaults)."""
    return delaunay.triangulate(points)
