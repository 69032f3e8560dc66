"""geom_host.call, the one routine through which the package's modules reach a launching entry point, against a recording stand-in for the
library: what arrives (pointers, NULL, the other values unchanged, the stream last), what a return code becomes, and what is refused
before the library is touched.  No GPU: the device context and the stream lookup are stand-ins too."""
import contextlib
import ctypes

import pytest
import torch

import geom_host as gh

STREAM = 0x5EED0
DEV = torch.device("cuda", 0)
I, VP, F64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
TABLE = {
    "radegs_fake": (I, [I, VP, VP, F64, ctypes.POINTER(ctypes.c_double), VP, VP]),
    "radegs_fake_bytes": (ctypes.c_size_t, [I]),
    "radegs_fake_no_stream": (I, [I, I]),
}


class FakeLibrary:
    def __init__(self, rc=0):
        self.rc, self.calls, self.entered = rc, [], []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args, list(self.entered)))
            return self.rc
        return fn


@pytest.fixture
def lib(monkeypatch):
    fake = FakeLibrary()

    @contextlib.contextmanager
    def device(dev):
        fake.entered.append(dev)
        yield
        fake.entered.pop()

    class Stream:
        cuda_stream = STREAM

    monkeypatch.setattr(gh, "bind", lambda table: fake)
    monkeypatch.setattr(gh.torch.cuda, "device", device)
    monkeypatch.setattr(gh.torch.cuda, "current_stream", lambda dev=None: Stream())
    return fake


def test_arguments_arrive_as_pointers_null_and_themselves_with_the_stream_last(lib):
    a, b = torch.arange(6, dtype=torch.float32), torch.zeros((2, 3), dtype=torch.float64)
    doubles = gh.doubles([1.0, 2.0])
    explicit = ctypes.c_void_p(b.data_ptr() + 24)
    assert gh.call(TABLE, "radegs_fake", DEV, 7, a, None, 0.5, doubles, explicit) is None
    (name, args, entered), = lib.calls
    assert name == "radegs_fake"
    assert args[0] == 7 and type(args[0]) is int
    assert args[1] == a.data_ptr() and type(args[1]) is int
    assert args[2] is None
    assert args[3] == 0.5 and type(args[3]) is float
    assert args[4] is doubles and args[5] is explicit
    assert args[6] == STREAM and len(args) == 7
    assert entered == [DEV]                        # called inside the device context of `dev`
    assert lib.entered == []


def test_a_nonzero_code_raises_with_the_functions_name_and_the_code(lib):
    lib.rc = -3
    with pytest.raises(RuntimeError) as e:
        gh.call(TABLE, "radegs_fake", DEV, 1, None, None, 0.0, None, None)
    assert "radegs_fake" in str(e.value) and "-3" in str(e.value)
    assert len(lib.calls) == 1


def test_too_large_raises_checks_sentence(lib):
    lib.rc = gh.ERR_TOO_LARGE
    assert gh.ERR_TOO_LARGE == -6
    with pytest.raises(RuntimeError) as e:
        gh.call(TABLE, "radegs_fake", DEV, 1, None, None, 0.0, None, None)
    with pytest.raises(RuntimeError) as expected:
        gh.check(-6, "radegs_fake")
    assert str(e.value) == str(expected.value)
    assert "larger than the 32-bit sort / scan primitives address" in str(e.value)


@pytest.mark.parametrize("name, args", [
    ("radegs_not_declared", (1, None)),                                      # not in the module's table
    ("radegs_fake", (1, None, None, 0.0, None)),                             # one argument short
    ("radegs_fake", (1, None, None, 0.0, None, None, None)),                 # one too many: ctypes would take it silently on a cdecl function
    ("radegs_fake_bytes", ()),                                               # restype is not c_int (and it takes no stream)
    ("radegs_fake_no_stream", (1,)),                                         # the last parameter is not the void* stream
    ("radegs_fake", (1, torch.zeros((4, 3)).t(), None, 0.0, None, None)),    # a tensor that is not contiguous
])
def test_refused_before_the_library_is_called(lib, name, args):
    with pytest.raises(RuntimeError):
        gh.call(TABLE, name, DEV, *args)
    assert lib.calls == [] and lib.entered == []


def test_host_tensors_pass_whatever_the_device(lib):
    pinned_like = torch.zeros(16, dtype=torch.uint8)
    gh.call(TABLE, "radegs_fake", torch.device("cuda", 3), 1, pinned_like, None, 0.0, None, None)
    assert lib.calls[0][1][1] == pinned_like.data_ptr()
