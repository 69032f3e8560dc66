"""Drop-in for the part of the `tetranerf` package the reference imports (mesh_extract_tetrahedra.py:18): `tetranerf.utils.extension.cpp`."""
