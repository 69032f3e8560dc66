"""_C._ScratchCache, the cache of the backward's scratch buffers, on CPU tensors: the class does not care about the device type.
What must hold: a lease owns the module lock until it ends, so a second thread neither receives a buffer in use nor one that was dropped;
clear() waits for a lease; at most 8 buffers are kept; a buffer only grows, and the ordered cache lets go of the smaller one first.

A thread is known to be blocked without any sleeping: the module lock is replaced by one that sets an event when an acquire finds it held."""
import threading
import weakref

import pytest
import torch

KEY = (0, 1234)


class _WatchedLock:
    def __init__(self):
        self._lock = threading.RLock()
        self.contended = threading.Event()

    def __enter__(self):
        if not self._lock.acquire(blocking=False):
            self.contended.set()
            self._lock.acquire()
        return self

    def __exit__(self, *exc):
        self._lock.release()


@pytest.fixture
def C(monkeypatch):
    import diff_gaussian_rasterization._C as C
    monkeypatch.setattr(C, "_SCRATCH_LOCK", _WatchedLock())
    return C


@pytest.mark.parametrize("zeroed", [True, False])
def test_a_second_thread_waits_for_the_lease_and_never_sees_a_dropped_buffer(C, zeroed):
    cache = C._ScratchCache(zeroed=zeroed)
    log, got = [], []

    def second():
        with cache.lease(KEY, 64, "cpu") as t:
            log.append("second has a buffer")
            got.append(t)

    with cache.lease(KEY, 64, "cpu") as mine:
        mine.fill_(7)
        b = threading.Thread(target=second)
        b.start()
        assert C._SCRATCH_LOCK.contended.wait(10), "the second thread never asked for the lock"
        assert not log                      # it is waiting: the lock is held by this lease
        cache.drop(KEY)                     # the call "failed": nobody may receive this buffer again
        log.append("first leaves")
    b.join(10)
    assert not b.is_alive() and log == ["first leaves", "second has a buffer"]
    assert got[0] is not mine and got[0].numel() >= 64
    if zeroed:
        assert int(torch.count_nonzero(got[0])) == 0
    assert cache.values()[0] is got[0] and len(cache) == 1


def test_clear_from_a_second_thread_returns_only_after_the_lease_ends(C):
    cache = C._ScratchCache(zeroed=True)
    cleared = threading.Event()

    def second():
        cache.clear()
        cleared.set()

    with cache.lease(KEY, 16, "cpu"):
        b = threading.Thread(target=second)
        b.start()
        assert C._SCRATCH_LOCK.contended.wait(10), "the second thread never asked for the lock"
        assert not cleared.is_set() and len(cache) == 1
    b.join(10)
    assert not b.is_alive() and cleared.is_set() and len(cache) == 0


@pytest.mark.parametrize("zeroed", [True, False])
def test_the_ninth_key_empties_the_cache_before_it_is_stored(C, zeroed):
    cache = C._ScratchCache(zeroed=zeroed)
    for k in range(8):
        with cache.lease((0, k), 16, "cpu"):
            pass
    assert len(cache) == 8
    with cache.lease((0, 3), 16, "cpu"):     # a key it has: nothing is evicted
        pass
    assert len(cache) == 8
    with cache.lease((0, 8), 16, "cpu") as ninth:
        assert len(cache) == 1 and cache.values()[0] is ninth
    assert len(cache) == 1


def test_a_larger_request_gets_a_new_zero_buffer_and_a_smaller_one_the_same_object(C):
    cache = C._ScratchCache(zeroed=True)
    with cache.lease(KEY, 100, "cpu") as first:
        assert first.dtype == torch.uint8 and first.numel() >= 100 and int(torch.count_nonzero(first)) == 0
    with cache.lease(KEY, 40, "cpu") as again:
        assert again is first
    with cache.lease(KEY, 100, "cpu") as again:
        assert again is first
        again.fill_(9)                       # whatever a failed call left behind must not leak into the larger buffer
    with cache.lease(KEY, 101, "cpu") as larger:
        assert larger is not first and larger.numel() >= 101 and int(torch.count_nonzero(larger)) == 0
    assert len(cache) == 1
    with cache.lease(KEY, 0, "cpu") as empty_request:
        assert empty_request is larger


def test_the_ordered_cache_releases_the_smaller_buffer_before_it_allocates_the_larger(C):
    cache = C._ScratchCache(zeroed=False)
    with cache.lease(KEY, 64, "cpu") as small:
        small_ref = weakref.ref(small)
    del small
    assert small_ref() is not None           # cached
    seen = []

    def recorder(n, **kw):
        seen.append((n, small_ref() is None, len(cache)))
        return torch.empty(n, **kw)

    cache._alloc = recorder
    with cache.lease(KEY, 128, "cpu") as large:
        assert large.numel() == 128
    assert seen == [(128, True, 0)]          # at the time of the allocation the smaller tensor was gone, and so was its entry
    with cache.lease(KEY, 128, "cpu") as again:
        assert again is large
    assert len(seen) == 1
