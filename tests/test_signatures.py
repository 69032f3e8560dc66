"""Every exported symbol gets its C signature from exactly one kind of place, a module's `_SIGNATURES` table handed to `_C.bind`: together the
tables cover `_C.EXPORTED_SYMBOLS`, and no function that returns something other than `int` is left with ctypes' default (a `size_t` called
unbound comes back truncated to 32 bits)."""
import ctypes
import importlib
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ("diff_gaussian_rasterization._C", "graphics_utils", "loss_utils", "gaussian_model_ops", "fused_adam", "simple_knn._C",
           "tetmesh", "mesh_eval", "tsdf", "tnt_eval", "tnt_cull")
WIDE = {"size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p, "long long": ctypes.c_longlong}


def _module(name):
    m = importlib.import_module(name)
    if getattr(m, "__file__", None) is None:   # a stand-in that tests/test_dropin_reference_caller.py left in sys.modules: load the file itself
        spec = importlib.util.spec_from_file_location("the_real_" + name.replace(".", "_"), os.path.join(ROOT, "rade-gs_amd", *name.split(".")) + ".py")
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    return m


def _modules():
    return [_module(m) for m in MODULES]


def test_the_signature_tables_cover_the_exported_symbols():
    mods = _modules()
    union = set()
    for m in mods:
        assert m._SIGNATURES, m.__name__
        union |= set(m._SIGNATURES)
    assert union == set(mods[0].EXPORTED_SYMBOLS)
    for m in mods:      # a name that two modules bind has one signature
        for other in mods:
            for name in set(m._SIGNATURES) & set(other._SIGNATURES):
                assert m._SIGNATURES[name] == other._SIGNATURES[name], (name, m.__name__, other.__name__)


def test_every_wide_return_type_of_the_header_is_bound():
    mods = _modules()
    L = mods[0].library()
    for m in mods[1:]:
        assert m._lib() is L
    hdr = open(os.path.join(ROOT, "include", "radegs.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    wide = re.findall(r"^\s*(size_t|const char\s*\*|long long)\s*(radegs_[a-z0-9_]+)\s*\(", hdr, flags=re.M)
    assert len(wide) >= 20, wide      # the header declares more than twenty of them: the pattern still reads it
    for ret, name in wide:
        assert getattr(L, name).restype is WIDE[re.sub(r"\s*\*", "*", ret)], (name, ret)
    for m in mods:
        for name, (restype, argtypes) in m._SIGNATURES.items():
            fn = getattr(L, name)
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
