"""geom_host.call on the GPU, through real entry points: the library's own refusals surface as check() writes them, the call runs on the
current stream of its device and inside that device's context, and the tensors call() refuses never reach the library.  Nothing here
provokes a fault: every refusal is raised in Python or returned by the library's argument checks before any launch."""
import pytest
import torch

import geom_host as gh
import tnt_eval

pytestmark = pytest.mark.gpu
EYE = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


class Recorder:
    """the real library, with the arguments and the current device of every call written down"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def wrapped(*args):
            self.calls.append((name, args, torch.cuda.current_device()))
            return fn(*args)
        return wrapped


@pytest.fixture
def recorder(monkeypatch):
    rec = Recorder(tnt_eval._lib())
    monkeypatch.setattr(gh, "bind", lambda table: rec)
    return rec


def _cloud(n, dev):
    g = torch.Generator().manual_seed(7)
    return torch.rand((n, 3), dtype=torch.float64, generator=g).to(dev)


def test_the_librarys_refusals_surface_with_the_functions_name():
    dev = torch.device("cuda", 0)
    p = _cloud(8, dev)
    out = torch.empty_like(p)
    with pytest.raises(RuntimeError) as e:       # N < 0: RADEGS_ERR_INVALID_ARG, returned before a pointer is read
        gh.call(tnt_eval._SIGNATURES, "radegs_tnteval_transform", dev, -1, p, gh.doubles(EYE), out)
    assert "radegs_tnteval_transform" in str(e.value) and "(-1)" in str(e.value)
    ws, counts = gh.workspace(4096, dev), torch.zeros(2, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError) as e:       # N = 2^32: RADEGS_ERR_TOO_LARGE, likewise
        gh.call(tnt_eval._SIGNATURES, "radegs_tnteval_voxel_plan", dev, 2 ** 32, p, gh.doubles([0.0, 0.0, 0.0]), 1.0, ws, 4096, counts)
    assert str(e.value) == "radegs_tnteval_voxel_plan: the input is larger than the 32-bit sort / scan primitives address (include/radegs.h)"
    torch.cuda.synchronize(dev)
    assert counts.tolist() == [0, 0]


def test_the_call_runs_on_the_current_stream_of_its_device(recorder):
    dev = torch.device("cuda", 0)
    p = _cloud(1000, dev)
    T = torch.tensor([[0.5, -0.25, 0.0, 1.0], [0.25, 0.5, 0.125, -2.0], [0.0, 0.375, 1.5, 0.5], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)
    default = tnt_eval.transform_points(p, T)
    torch.cuda.synchronize(dev)
    assert recorder.calls[-1][1][-1] == torch.cuda.current_stream(dev).cuda_stream
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        on_side = tnt_eval.transform_points(p, T)
        expected = torch.cuda.current_stream(dev).cuda_stream
    torch.cuda.synchronize(dev)
    assert expected == side.cuda_stream and expected != torch.cuda.current_stream(dev).cuda_stream
    name, args, _ = recorder.calls[-1]
    assert name == "radegs_tnteval_transform" and args[-1] == expected
    assert args[0] == 1000 and args[1] == p.data_ptr() and args[3] == on_side.data_ptr()
    assert bytes(on_side.cpu().numpy().data) == bytes(default.cpu().numpy().data)
    assert not torch.equal(default, p)


def test_a_transposed_tensor_is_refused_before_the_library_is_called(recorder):
    dev = torch.device("cuda", 0)
    transposed = torch.zeros((3, 4), dtype=torch.float64, device=dev).t()
    assert tuple(transposed.shape) == (4, 3) and not transposed.is_contiguous()
    with pytest.raises(RuntimeError):
        gh.call(tnt_eval._SIGNATURES, "radegs_tnteval_transform", dev, 4, transposed, gh.doubles(EYE), torch.empty((4, 3), dtype=torch.float64, device=dev))
    assert recorder.calls == []


def _two_devices():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    return torch.device("cuda", 0), torch.device("cuda", 1)


def test_a_tensor_on_another_device_is_refused(recorder):
    dev0, dev1 = _two_devices()
    p, out = _cloud(8, dev0), torch.empty((8, 3), dtype=torch.float64, device=dev1)
    with pytest.raises(RuntimeError):
        gh.call(tnt_eval._SIGNATURES, "radegs_tnteval_transform", dev0, 8, p, gh.doubles(EYE), out)
    assert recorder.calls == []


def test_the_call_runs_inside_the_context_of_its_device(recorder):
    _, dev1 = _two_devices()
    assert torch.cuda.current_device() == 0
    p = _cloud(8, dev1)
    out = tnt_eval.transform_points(p, torch.eye(4, dtype=torch.float64))
    torch.cuda.synchronize(dev1)
    assert recorder.calls[-1][2] == dev1.index and torch.cuda.current_device() == 0
    assert torch.equal(out, p)
