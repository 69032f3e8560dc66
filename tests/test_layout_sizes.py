"""The sizes of the state buffers and of the ordered backward's scratch, as literal numbers recorded from the library BEFORE the rasterizer's
layouts moved to the shared carver (csrc/rg_workspace.h): a layout change that moves an array shows up here without a GPU.
The arguments put array ends on, just below and just above a 256-byte boundary and include the empty arrays.  PointState has no size
function; tests/test_gpu_integrate.py covers it."""
import pytest

N = (0, 1, 255, 256, 257, 1000, 1000003)

GEOMETRY = {(0, 0): 6144, (0, 1): 6144, (1, 0): 10752, (1, 1): 11008, (255, 0): 34048, (255, 1): 46336, (256, 0): 34048, (256, 1): 46336,
            (257, 0): 36608, (257, 1): 49152, (1000, 0): 110080, (1000, 1): 158208, (1000003, 0): 102010112, (1000003, 1): 150010368}
BINNING = {0: 5888, 1: 9216, 255: 14080, 256: 14080, 257: 15360, 1000: 32512, 1000003: 25008640}
IMAGE = {(1, 1): 11008, (16, 16): 17152, (17, 31): 25344, (640, 360): 6585088, (1920, 1080): 59179264, (4120, 40): 4728832}
# (R, coord): the size does not depend on P
ORDERED = {(0, 0): 5632, (0, 1): 5632, (1, 0): 8704, (1, 1): 8704, (255, 0): 28160, (255, 1): 44544, (256, 0): 28160, (256, 1): 44544,
           (257, 0): 29184, (257, 1): 45568, (1000, 0): 88064, (1000, 1): 152064, (1000003, 0): 81008128, (1000003, 1): 145008384}


@pytest.fixture(scope="module")
def L():
    import diff_gaussian_rasterization._C as C
    return C.library()


def test_the_tables_cover_the_cases():
    assert set(GEOMETRY) == {(P, c) for P in N for c in (0, 1)} and set(BINNING) == set(N) and set(ORDERED) == {(R, c) for R in N for c in (0, 1)}
    assert set(IMAGE) == {(1, 1), (16, 16), (17, 31), (640, 360), (1920, 1080), (4120, 40)}


def test_geometry_bytes(L):
    assert {k: int(L.radegs_geometry_bytes(*k)) for k in GEOMETRY} == GEOMETRY


def test_binning_bytes(L):
    assert {R: int(L.radegs_binning_bytes(R)) for R in BINNING} == BINNING


def test_image_bytes(L):
    assert {k: int(L.radegs_image_bytes(*k)) for k in IMAGE} == IMAGE


def test_backward_ordered_scratch_bytes(L):
    for P in N:
        assert {k: int(L.radegs_backward_ordered_scratch_bytes(P, *k)) for k in ORDERED} == ORDERED, P
