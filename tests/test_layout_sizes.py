"""The sizes of the state buffers and of the ordered backward's scratch, as literal numbers recorded from the library BEFORE the rasterizer's
layouts moved to the shared carver (csrc/rg_workspace.h): a layout change that moves an array shows up here without a GPU.
The arguments put array ends on, just below and just above a 256-byte boundary and include the empty arrays.  POINT, the point state of
integrate (radegs_point_bytes), was recorded from the layout it has had since it was written."""
import pytest

N = (0, 1, 255, 256, 257, 1000, 1000003)

GEOMETRY = {(0, 0): 6144, (0, 1): 6144, (1, 0): 10752, (1, 1): 11008, (255, 0): 34048, (255, 1): 46336, (256, 0): 34048, (256, 1): 46336,
            (257, 0): 36608, (257, 1): 49152, (1000, 0): 110080, (1000, 1): 158208, (1000003, 0): 102010112, (1000003, 1): 150010368}
BINNING = {0: 5888, 1: 9216, 255: 14080, 256: 14080, 257: 15360, 1000: 32512, 1000003: 25008640}
IMAGE = {(1, 1): 11008, (16, 16): 17152, (17, 31): 25344, (640, 360): 6585088, (1920, 1080): 59179264, (4120, 40): 4728832}
# (R, coord): the size does not depend on P
ORDERED = {(0, 0): 5632, (0, 1): 5632, (1, 0): 8704, (1, 1): 8704, (255, 0): 28160, (255, 1): 44544, (256, 0): 28160, (256, 1): 44544,
           (257, 0): 29184, (257, 1): 45568, (1000, 0): 88064, (1000, 1): 152064, (1000003, 0): 81008128, (1000003, 1): 145008384}
# (P, PN, W, H): inte_rec ends at 32 P (P = 7, 8, 9), p2d at 8 PN (31, 32, 33), pdepth / ppix / pt_sorted at 4 PN (64), the per-pixel arrays at 4 W H (8 x 8)
POINT = {(0, 0, 1, 1): 3072, (0, 0, 16, 16): 6400, (1, 1, 8, 8): 4608, (8, 0, 16, 16): 6656, (0, 64, 16, 16): 7680, (8, 32, 8, 8): 4608,
         (9, 33, 8, 8): 5120, (7, 31, 8, 8): 4608, (8, 64, 17, 31): 12800, (1000, 1000, 64, 48): 103936, (257, 255, 61, 45): 59904,
         (1000003, 4000001, 1920, 1080): 145205248}


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


def test_point_bytes(L):
    assert {k: int(L.radegs_point_bytes(*k)) for k in POINT} == POINT
    assert any(k[0] == 0 for k in POINT) and any(k[1] == 0 for k in POINT)
