"""CPU tier of the Delaunay unit: the library exports the entry points and include/radegs.h declares them, the size function and the
argument checks of the C entry points run without a device, delaunay.py has the call surface and refuses bad arguments before any launch,
the tetranerf shim imports under the reference's name, and the cell arithmetic compiled for the HOST gives scipy's cells."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import delaunay
from delaunay_cases import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("radegs_delaunay_bytes", "radegs_delaunay_perturb", "radegs_delaunay_plan", "radegs_delaunay_emit")
INVALID, TOO_LARGE = -1, -6


def _library():
    import diff_gaussian_rasterization._C as C
    return C, delaunay._lib()


def test_library_exports_and_header_declares_the_entry_points():
    C, L = _library()
    header = open(os.path.join(ROOT, "include", "radegs.h")).read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in C.EXPORTED_SYMBOLS, sym
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % sym, header), sym
    assert "SURVEY.md 8f N13" in header
    assert set(delaunay.SIGNATURES) == set(SYMBOLS)


def test_sizes_and_argument_checks_run_without_a_device():
    _, L = _library()
    fake = 0x1000
    box = (ctypes.c_double * 6)(0, 0, 0, 1, 1, 1)
    assert L.radegs_delaunay_bytes(3, 100) == 0 and L.radegs_delaunay_bytes(4, 0) == 0 and L.radegs_delaunay_bytes(2 ** 31 - 7, 100) == 0
    assert L.radegs_delaunay_bytes(4, 2 ** 32 - 65536) == 0
    small, large = L.radegs_delaunay_bytes(4, 16), L.radegs_delaunay_bytes(1_000_000, 32_000_000)
    assert 0 < small < 256 * 1024 and small % 256 == 0
    assert 72 * 32_000_000 <= large <= 100 * 32_000_000 + 80 * 1_000_000       # 18 words a record, the sort's temp, 72 B a point
    assert L.radegs_delaunay_bytes(2 ** 27, 2 ** 32 - 65537) > 2 ** 38          # a size_t: not cut to 32 bits

    def perturb(N=8, p=fake, scale=1e-9, seed=0, out=fake):
        return L.radegs_delaunay_perturb(N, p, scale, seed, out, None)
    assert perturb(N=0) == 0                                                     # nothing to do: no launch
    assert perturb(N=-1) == INVALID and perturb(scale=-1.0) == INVALID and perturb(scale=float("nan")) == INVALID and perturb(scale=float("inf")) == INVALID
    assert perturb(p=None) == INVALID and perturb(out=None) == INVALID and perturb(N=2 ** 31) == TOO_LARGE

    def plan(N=8, p=fake, b=box, scale=0.0, seed=0, cap=64, ws=fake, nbytes=1 << 40, counts=fake):
        return L.radegs_delaunay_plan(N, p, b, scale, seed, cap, ws, nbytes, counts, None)
    assert plan(N=3) == INVALID and plan(p=None) == INVALID and plan(b=None) == INVALID and plan(counts=None) == INVALID and plan(cap=0) == INVALID
    assert plan(scale=-1.0) == INVALID and plan(scale=float("nan")) == INVALID
    assert plan(b=(ctypes.c_double * 6)(0, 0, 0, 1, float("inf"), 1)) == INVALID
    assert plan(N=2 ** 31 - 7) == TOO_LARGE and plan(cap=2 ** 32 - 65536) == TOO_LARGE
    assert plan(ws=None) == INVALID and plan(ws=fake + 4) == INVALID and plan(nbytes=L.radegs_delaunay_bytes(8, 64) - 1) == INVALID

    def emit(N=8, records=40, cap=64, ws=fake, nbytes=1 << 40, rows=10, cells=fake, counts=fake):
        return L.radegs_delaunay_emit(N, records, cap, ws, nbytes, rows, cells, counts, None)
    assert emit(N=3) == INVALID and emit(records=0) == INVALID and emit(records=65) == INVALID and emit(rows=-1) == INVALID
    assert emit(cells=None) == INVALID and emit(counts=None) == INVALID and emit(cap=2 ** 32 - 65536, records=1) == TOO_LARGE
    assert emit(ws=None) == INVALID and emit(ws=fake + 8) == INVALID and emit(nbytes=L.radegs_delaunay_bytes(8, 64) - 1) == INVALID


def test_call_surface():
    sig = inspect.signature(delaunay.triangulate)
    assert list(sig.parameters) == ["points", "jitter", "seed", "return_info"]
    assert [p.default for p in sig.parameters.values()][1:] == [1e-9, 0, False]
    assert list(inspect.signature(delaunay.perturbed).parameters) == ["points", "jitter", "seed"]
    import tetmesh
    assert tetmesh.triangulate is delaunay.triangulate
    assert list(inspect.signature(tetmesh.marching_tetrahedra_with_binary_search).parameters)[:3] == ["points", "points_scale", "cells"]


def test_arguments_are_refused_before_any_launch():
    ok = torch.zeros(8, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        delaunay.triangulate(ok)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        delaunay.perturbed(ok.double())
    for bad, what in ((torch.zeros(8, 4), r"\(N,3\)"), (torch.zeros(8), r"\(N,3\)"), (torch.zeros(8, 3, dtype=torch.float16), "float32 or float64"),
                      (torch.zeros(8, 3, dtype=torch.int64), "float32 or float64"), (np.zeros((8, 3)), "float32 or float64"), (None, "float32 or float64")):
        with pytest.raises(RuntimeError, match=what):
            delaunay.triangulate(bad)
    for kw, what in ((dict(jitter=-1e-9), "jitter"), (dict(jitter=float("nan")), "jitter"), (dict(jitter="1e-9"), "jitter"), (dict(jitter=True), "jitter"),
                     (dict(seed=-1), "seed"), (dict(seed=1.5), "seed"), (dict(seed=2 ** 63), "seed"), (dict(return_info=1), "return_info")):
        with pytest.raises(RuntimeError, match=what):
            delaunay.triangulate(ok, **kw)


def test_packaging_lists_the_module_and_the_shim():
    setup = open(os.path.join(ROOT, "rade-gs_amd", "setup.py")).read()
    assert '"delaunay"' in re.search(r"py_modules=\[([^\]]*)\]", setup).group(1)
    packages = re.search(r"packages=\[([^\]]*)\]", setup).group(1)
    for name in ("tetranerf", "tetranerf.utils", "tetranerf.utils.extension"):
        assert f'"{name}"' in packages
    build = open(os.path.join(ROOT, "rade-gs_amd", "build.py")).read()
    assert '"radegs_delaunay.hip"' in build and '"rg_delaunay_cell.h"' in build


def test_the_shim_imports_under_the_reference_name():
    from tetranerf.utils.extension import cpp
    assert list(inspect.signature(cpp.triangulate).parameters) == ["points"]
    with pytest.raises(RuntimeError, match="GPU tensor"):
        cpp.triangulate(torch.zeros(8, 3))


HOST_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "rg_delaunay_cell.h"
using namespace rgdl;
struct HostData : NoTriangleData {
  const double* P;
  V3 xi;
  V3 rel(int, uint32_t g) const { return V3{P[3 * g] - xi.x, P[3 * g + 1] - xi.y, P[3 * g + 2] - xi.z}; }
};
template <int F, int T>
void run(const std::vector<double>& P, uint32_t N) {
  unsigned uncertain = 0, overflow = 0;
  for (uint32_t i = 0; i < N; i++) {
    static uint32_t face[F];
    static uint8_t tri[3 * T];
    Cell<F, T, 1> c;
    c.init(face, tri, N);
    HostData d;
    d.P = P.data(), d.xi = V3{P[3 * i], P[3 * i + 1], P[3 * i + 2]};
    for (uint32_t p = 0; p < N && !c.overflow; p++)
      if (p != i) c.clip(p, d.rel(0, p), d, uncertain);
    if (c.overflow) { overflow++; continue; }
    for (int t = 0; t < c.nt; t++) {
      const uint32_t a = c.id(c.corner(t, 0)), b = c.id(c.corner(t, 1)), e = c.id(c.corner(t, 2));
      if (a < N && b < N && e < N) printf("%u %u %u %u\n", i, a, b, e);
    }
  }
  printf("# %u %u\n", uncertain, overflow);
}
int main(int argc, char** argv) {
  std::vector<double> P;
  double v;
  while (fread(&v, 8, 1, stdin) == 1) P.push_back(v);
  if (argc > 1) run<48, 92>(P, (uint32_t)(P.size() / 3)); else run<256, 508>(P, (uint32_t)(P.size() / 3));
  return 0;
}
"""


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """csrc/rg_delaunay_cell.h -- the predicates, the cell and the clip the kernels run -- compiled as plain C++ for the host"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("delaunay_host")
    src, exe = d / "cell.cpp", d / "cell"
    src.write_text(HOST_PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "rade-gs_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def _host_cells(exe, X, small=False):
    out = subprocess.run([exe] + (["small"] if small else []), input=np.ascontiguousarray(X, dtype=np.float64).tobytes(), capture_output=True, check=True).stdout.decode()
    lines = out.strip().split("\n")
    uncertain, overflow = (int(x) for x in lines[-1][1:].split())
    rec = np.sort(np.array([[int(x) for x in l.split()] for l in lines[:-1]], dtype=np.int64).reshape(-1, 4), axis=1)
    uniq, found = np.unique(rec, axis=0, return_counts=True)
    return uniq, found, uncertain, overflow


@pytest.mark.parametrize("name", ["random8", "random200", "sphere120", "shell151", "clusters120", "grid64", "boxes270"])
def test_cell_arithmetic_on_the_host_equals_scipy(host_program, name):
    fx = load(name)
    uniq, found, uncertain, overflow = _host_cells(host_program, fx["perturbed"])
    assert uncertain == 0 and overflow == 0 and (found == 4).all()
    assert np.array_equal(uniq, fx["cells"])


def test_fast_cell_capacity_on_the_host(host_program):
    """the 48-face / 92-triangle cell of the fast kernel: enough for scattered points, outgrown by the centre of the shell (a deferral on
    the GPU), and an outgrown cell is reported, not written past"""
    fx = load("random200")
    uniq, found, uncertain, overflow = _host_cells(host_program, fx["perturbed"], small=True)
    assert overflow == 0 and uncertain == 0 and (found == 4).all() and np.array_equal(uniq, fx["cells"])
    assert _host_cells(host_program, load("shell151")["perturbed"], small=True)[3] == 1


def test_unperturbed_box_corners_are_uncertain_on_the_host(host_program):
    uniq, found, uncertain, overflow = _host_cells(host_program, load("boxes270")["points"].astype(np.float64))
    assert uncertain > 0 and (found != 4).any()


SECOND_LOOK_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "rg_delaunay_cell.h"
using namespace rgdl;
struct HostData : NoTriangleData {
  const double* P;
  V3 xi;
  bool look;
  V3 at(uint32_t g) const { return V3{P[3 * g], P[3 * g + 1], P[3 * g + 2]}; }
  V3 rel(int, uint32_t g) const { return at(g) - xi; }
  int second_look(uint32_t ia, uint32_t ib, uint32_t ic, uint32_t iq, V3 a, V3 b, V3 c, V3 q) const {
    return look ? in_sphere_recentred(xi, at(ia), at(ib), at(ic), at(iq), a, b, c, q) : -1;
  }
};
int main(int argc, char**) {
  std::vector<double> P;
  double v;
  while (fread(&v, 8, 1, stdin) == 1) P.push_back(v);
  const uint32_t N = (uint32_t)(P.size() / 3);
  unsigned uncertain = 0, overflow = 0;
  for (uint32_t i = 0; i < N; i++) {
    static uint32_t face[256];
    static uint8_t tri[3 * 508];
    Cell<256, 508, 1> c;
    c.init(face, tri, N);
    HostData d;
    d.P = P.data(), d.xi = d.at(i), d.look = argc > 1;
    for (uint32_t p = 0; p < N && !c.overflow; p++)
      if (p != i) c.clip(p, d.rel(0, p), d, uncertain);
    if (c.overflow) { overflow++; continue; }
    for (int t = 0; t < c.nt; t++) {
      const uint32_t a = c.id(c.corner(t, 0)), b = c.id(c.corner(t, 1)), e = c.id(c.corner(t, 2));
      if (a < N && b < N && e < N) printf("%u %u %u %u\n", i, a, b, e);
    }
  }
  printf("# %u %u\n", uncertain, overflow);
  return 0;
}
"""


@pytest.fixture(scope="module")
def second_look_program(tmp_path_factory):
    """the same cell code with a Data that answers second_look from absolute coordinates, as the two kernels' do (any argument: on)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("delaunay_second_look")
    src, exe = d / "cell.cpp", d / "cell"
    src.write_text(SECOND_LOOK_PROGRAM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "rade-gs_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def test_second_look_decides_what_a_twin_a_jitter_apart_leaves_uncertain(second_look_program):
    """100 points each listed twice, parted by the default jitter alone: with x_i as the only origin thousands of in-sphere values of a
    candidate against a triangle that holds its twin are within their bound and the cells disagree; about the nearest origin every one is
    decided, exactly: the cells agree and pass the exact certificate.  What is exactly tied stays uncertain, and what was certain stays
    the same."""
    import delaunay_certificate as cert
    import delaunay_restatement as dr
    from delaunay_cases import cloud
    X = dr.perturbed(cloud("dup200"), 1e-9, 0)
    uniq, found, uncertain, overflow = _host_cells(second_look_program, X)
    assert uncertain > 1000 and (found != 4).any() and overflow == 0                 # 6 130 and 1 865 of 2 655 when this was written
    uniq, found, uncertain, overflow = _host_cells(second_look_program, X, small=True)
    assert uncertain == 0 and (found == 4).all() and overflow == 0
    assert cert.defects(cert.certify(X, dr.orient(X, uniq))) == {}
    box = load("boxes270")
    for coords in (box["points"].astype(np.float64), box["perturbed"], load("random200")["perturbed"]):
        off, on = _host_cells(second_look_program, coords), _host_cells(second_look_program, coords, small=True)
        assert off[2] == on[2] and np.array_equal(off[0], on[0]) and np.array_equal(off[1], on[1])
    assert _host_cells(second_look_program, box["points"].astype(np.float64), small=True)[2] > 0     # exact ties are not decided by moving the origin
