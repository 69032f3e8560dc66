"""The hand-written device-wide primitives of csrc/radegs_sort.hip, called directly (csrc/radegs_sort_check.hip ->
libradegs_sort_check.so, built by rade-gs_amd/build.py) with the instantiation forced, against exact host references:

    sort   d = ((key - key_base) mod 2^32) & (2^end_bit - 1);  perm = np.argsort(d, kind="stable")
           keys_out == keys_in[perm] (the whole key, bits above end_bit included), vals_out == vals_in[perm] (perm itself without vals_in)
    order  of (major, minor) word pairs:  perm = np.lexsort((minor & mask_minor, major & mask_major))
           perm_out == perm, major_sorted == major[perm] (the whole word)
    scan   c = vals[idx] (w * h of the packed word in the packed form);  out == cumsum(c) in uint64 cast to uint32,
           packed_out == vals[idx],  *sq_sum == sum(c^2) as an exact uint64

Integer code on both sides: every comparison is bit for bit.  Each output buffer and the temp buffer lies between two 64 KiB guards inside
one allocation; temp is exactly *_temp_bytes(n) bytes and is filled with 0xA5 before every call.  After every call: return code, guards,
inputs unchanged.  The test id names the instantiation, the entry point with its end_bit, and the key pattern or the size; a failing
assertion adds the remaining parameters."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "rade-gs_amd", "diff_gaussian_rasterization", "libradegs_sort_check.so")
DEV = "cuda:0"
GUARD = 64 * 1024
GUARD_BYTE, OUT_BYTE, TEMP_BYTE = 0x5C, 0xEE, 0xA5
HIP_ERROR_INVALID_VALUE = 1

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        assert os.path.exists(LIB_PATH), LIB_PATH + " is missing: build it with `python rade-gs_amd/build.py`"
        L = ctypes.CDLL(LIB_PATH)
        vp, sz, ci, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
        for f in (L.sortcheck_sort_temp_bytes, L.sortcheck_scan_temp_bytes):
            f.restype, f.argtypes = sz, [sz]
        for f in (L.sortcheck_sort_u32, L.sortcheck_sort_u16):   # temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, end_bit, stream, n_dev, items
            f.restype, f.argtypes = ci, [vp, sz, vp, vp, vp, vp, sz, ci, vp, vp, ci]
        L.sortcheck_sort_u32_27.restype = ci                     # ..., n, key_base, stream, items
        L.sortcheck_sort_u32_27.argtypes = [vp, sz, vp, vp, vp, vp, sz, u32, vp, ci]
        L.sortcheck_sort_2xu32.restype = ci                      # temp, temp_bytes, minor, major, major_sorted, perm, s0, s1, s2, n, end bits, stream, n_dev
        L.sortcheck_sort_2xu32.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, vp, vp]
        L.sortcheck_sort_2xu32_joined.restype = ci               # the same and joined
        L.sortcheck_sort_2xu32_joined.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, vp, sz, ci, ci, vp, vp, vp]
        L.sortcheck_scan.restype = ci                            # temp, temp_bytes, vals, idx, out, n, stream, packed_out, sq_sum, items
        L.sortcheck_scan.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, vp, ci]
        _LIB = L
    return _LIB


def _depth_key_base():
    src = open(os.path.join(ROOT, "rade-gs_amd", "csrc", "radegs_kernels.hip")).read()
    return int(re.search(r"kDepthKeyBase\s*=\s*(0x[0-9A-Fa-f]+)u", src).group(1), 16)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if DEV != "cpu" else None


class Guarded:
    """`nbytes` bytes filled with `fill` between two guards, all in one allocation."""

    def __init__(self, nbytes, fill):
        self.nbytes = nbytes
        self.raw = torch.full((2 * GUARD + nbytes,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.raw[GUARD:GUARD + nbytes] = fill
        self.ptr = self.raw.data_ptr() + GUARD

    def host(self, dtype=np.uint8):
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == GUARD_BYTE).all()) and bool((self.raw[GUARD + self.nbytes:] == GUARD_BYTE).all())


def _upload(a):
    """numpy uint32 / uint16 -> a torch int32 / int16 tensor on the device (None stays None)"""
    if a is None:
        return None
    return torch.from_numpy(a.view({2: np.int16, 4: np.int32}[a.dtype.itemsize]).copy()).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _unchanged(t, a):
    return t is None or np.array_equal(t.cpu().numpy().view(a.dtype), a)


# ---------------------------------------------------------------- sort ----------------------------------------------------------------

ENTRIES = [("u32", e) for e in (1, 8, 9, 13, 17, 30, 32)] + [("u16", e) for e in (1, 7, 13, 15, 16)] + [("u32_27", 27)]
LARGE_ENTRIES = [("u32", 30), ("u16", 13), ("u32_27", 27)]     # the 258-block size: one end_bit per entry point
PATTERNS = ["uniform", "equal_ones", "equal_zero", "two_hot", "ascending", "descending", "ties8", "runs"]


def _entry_id(e):
    return e[0] if e[0] == "u32_27" else "%s_bits%d" % e


def _key_bits(entry):
    return 16 if entry == "u16" else 32


def _digit_width(entry, end_bit):
    digit_bits = 9 if entry == "u32_27" else 8
    passes = (end_bit + digit_bits - 1) // digit_bits
    return (end_bit + passes - 1) // passes, passes


def make_keys(pattern, entry, end_bit, n, rng):
    """Keys of width 16 / 32 bits.  Patterns are laid out in the space the sort looks at, (key - key_base), then shifted by key_base."""
    bits = _key_bits(entry)
    base = _depth_key_base() if entry == "u32_27" else 0
    full = (1 << bits) - 1
    if pattern == "uniform":
        if entry == "u32_27":
            # float bits of depths: inside the three-pass window [0.2, 13107), a few percent below 0.2 (key - base wraps) and above it
            z = np.exp(rng.uniform(np.log(0.2), np.log(13107.0), n))
            sel = rng.random(n)
            z = np.where(sel < 0.04, rng.uniform(0.01, 0.2, n), z)
            z = np.where(sel > 0.96, rng.uniform(13108.0, 1.0e6, n), z)
            k = z.astype(np.float32).view(np.uint32).astype(np.uint64)
            k[::97] = base                      # 0.2f itself: difference 0
            return k.astype(np.uint32)
        k = rng.integers(0, full + 1, n, dtype=np.uint64)               # every bit, those above end_bit too
    elif pattern == "equal_ones":                                       # every digit of every pass all ones; u32 / u16: the high bits too
        k = np.full(n, ((1 << end_bit) - 1) if entry == "u32_27" else full, dtype=np.uint64)
    elif pattern == "equal_zero":
        k = np.zeros(n, dtype=np.uint64)
    elif pattern == "two_hot":                                          # digits d and d ^ 1 in EVERY pass: the two halves of one LDS word
        width, passes = _digit_width(entry, end_bit)
        a = int(rng.integers(0, 1 << (27 if entry == "u32_27" else bits)))
        flip = sum(1 << (p * width) for p in range(passes))
        k = np.where(rng.random(n) < 0.5, a, a ^ flip).astype(np.uint64)
    elif pattern == "ascending":
        k = np.arange(n, dtype=np.uint64)
    elif pattern == "descending":
        k = np.arange(n, dtype=np.uint64)[::-1].copy()
    elif pattern == "ties8":                                            # long ties: stability is what orders them
        k = rng.integers(0, 1 << (27 if entry == "u32_27" else bits), 8, dtype=np.uint64)[rng.integers(0, 8, n)]
    elif pattern == "runs":                                             # short ascending runs, as the instance emission writes tile ids
        starts = rng.integers(0, 1 << min(end_bit, bits), n, dtype=np.uint64)
        length = rng.integers(1, 9, n)
        first = np.zeros(n, dtype=np.int64)
        pos = np.cumsum(length)
        pos = pos[pos < n]
        first[pos] = pos
        first = np.maximum.accumulate(first)                            # index of the run's first item
        k = starts[first] + (np.arange(n) - first).astype(np.uint64)
    else:
        raise AssertionError(pattern)
    return ((k + base) & full).astype(np.uint16 if bits == 16 else np.uint32)


def make_vals(n, rng):
    v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    v[::7] = 0xFFFFFFFF
    return v


def ref_perm(keys, entry, end_bit):
    base = _depth_key_base() if entry == "u32_27" else 0
    d = keys.astype(np.uint32) - np.uint32(base)          # array arithmetic: wraps mod 2^32
    if end_bit < 32:
        d = d & np.uint32((1 << end_bit) - 1)
    if end_bit <= 16:
        d = d.astype(np.uint16)
    return np.argsort(d, kind="stable")


def call_sort(entry, items, keys, vals, end_bit, n=None, m=None, temp_short=0):
    """One call.  keys / vals: host arrays of the capacity `n` (default: their length); m: the device-side count (n_dev) or None.
    Returns (rc, keys_out, vals_out, temp) as host arrays after asserting guards and untouched inputs."""
    L = _lib()
    n = len(keys) if n is None else n
    ksize = keys.dtype.itemsize
    d_keys, d_vals = _upload(keys), _upload(vals)
    d_m = None if m is None else torch.tensor([m], dtype=torch.int64).to(torch.int32).to(DEV)
    temp_bytes = L.sortcheck_sort_temp_bytes(n) - temp_short
    temp = Guarded(temp_bytes, TEMP_BYTE)
    k_out, v_out = Guarded(len(keys) * ksize, OUT_BYTE), Guarded(len(keys) * 4, OUT_BYTE)
    if entry == "u32_27":
        assert m is None and end_bit == 27
        rc = L.sortcheck_sort_u32_27(temp.ptr, temp_bytes, _ptr(d_keys), k_out.ptr, _ptr(d_vals), v_out.ptr, n, _depth_key_base(), _stream(), items)
    else:
        fn = L.sortcheck_sort_u32 if entry == "u32" else L.sortcheck_sort_u16
        rc = fn(temp.ptr, temp_bytes, _ptr(d_keys), k_out.ptr, _ptr(d_vals), v_out.ptr, n, end_bit, _stream(), _ptr(d_m), items)
    if DEV != "cpu":
        torch.cuda.synchronize()
    assert temp.guards_intact(), "temp guards overwritten"
    assert k_out.guards_intact(), "keys_out guards overwritten"
    assert v_out.guards_intact(), "vals_out guards overwritten"
    assert _unchanged(d_keys, keys), "keys_in modified"
    assert _unchanged(d_vals, vals), "vals_in modified"
    assert d_m is None or int(d_m.cpu()[0]) == np.int32(np.uint32(m)), "n_dev modified"
    return rc, k_out.host(keys.dtype), v_out.host(np.uint32), temp


def check_sort(entry, items, keys, vals, end_bit, perm, m=None):
    rc, k_out, v_out, _ = call_sort(entry, items, keys, vals, end_bit, m=m)
    assert rc == 0, "hip error %d" % rc
    cnt = len(perm)
    bad = np.flatnonzero(k_out[:cnt] != keys[perm])
    assert bad.size == 0, "keys_out differs at %d of %d positions, first %d" % (bad.size, cnt, bad[0])
    want = perm.astype(np.uint32) if vals is None else vals[perm]
    bad = np.flatnonzero(v_out[:cnt] != want)
    assert bad.size == 0, "vals_out differs at %d of %d positions, first %d (a stable order keeps ties in input order)" % (bad.size, cnt, bad[0])


def small_sizes(items):
    wv, b = 64 * items, 256 * items
    return [1, 63, 64, 65, wv - 1, wv, wv + 1, b - 1, b, b + 1, 3 * b + wv + 5]


def _seed(*parts):
    """a seed that depends on the case alone (hash() of a str changes from process to process)"""
    return sum((i + 1) * ord(c) for i, c in enumerate("/".join(str(p) for p in parts)))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("entry", ENTRIES, ids=_entry_id)
@pytest.mark.parametrize("items", [8, 16, 32])
def test_sort_small_sizes(items, entry, pattern):
    """n around the wave run (64 * items), the block (256 * items) and a few blocks with a ragged tail; with values and without."""
    name, end_bit = entry
    rng = np.random.default_rng(_seed(items, name, end_bit, pattern))
    for n in small_sizes(items):
        keys = make_keys(pattern, name, end_bit, n, rng)
        perm = ref_perm(keys, name, end_bit)
        for vals in (make_vals(n, rng), None):
            try:
                check_sort(name, items, keys, vals, end_bit, perm)
            except AssertionError as e:
                raise AssertionError("n=%d vals_in=%s: %s" % (n, "null" if vals is None else "random", e)) from None


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("entry", LARGE_ENTRIES, ids=_entry_id)
@pytest.mark.parametrize("items", [8, 16, 32])
def test_sort_258_blocks(items, entry, pattern):
    """n = 257 blocks + 17: scan_rows_kernel makes a second trip over its row of block counts and carries the first trip's sum."""
    name, end_bit = entry
    n = 257 * 256 * items + 17
    rng = np.random.default_rng(_seed(items, name, end_bit, pattern, "large"))
    keys = make_keys(pattern, name, end_bit, n, rng)
    perm = ref_perm(keys, name, end_bit)
    for vals in (make_vals(n, rng), None):
        try:
            check_sort(name, items, keys, vals, end_bit, perm)
        except AssertionError as e:
            raise AssertionError("n=%d vals_in=%s: %s" % (n, "null" if vals is None else "random", e)) from None


@pytest.mark.parametrize("cap_kind", ["B+1", "3B+5"])
@pytest.mark.parametrize("entry", [("u32", 17), ("u16", 13)], ids=_entry_id)
@pytest.mark.parametrize("items", [8, 16, 32])
def test_sort_device_side_count(items, entry, cap_kind):
    """n is a capacity and the count m is read on the device: the first min(m, cap) outputs are the sort of the first min(m, cap) inputs,
    whatever lies behind them in the input."""
    name, end_bit = entry
    wv, b = 64 * items, 256 * items
    cap = b + 1 if cap_kind == "B+1" else 3 * b + 5
    rng = np.random.default_rng(_seed(items, name, cap_kind))
    keys = make_keys("uniform", name, end_bit, cap, rng)      # random all the way: the items past m are the poison
    vals = make_vals(cap, rng)
    for m in (0, 1, wv, b, cap - 1, cap, cap + 1000):
        cnt = min(m, cap)
        perm = ref_perm(keys[:cnt], name, end_bit)
        for v in (vals, None):
            try:
                check_sort(name, items, keys, v, end_bit, perm, m=m)
            except AssertionError as e:
                raise AssertionError("cap=%d m=%d vals_in=%s: %s" % (cap, m, "null" if v is None else "random", e)) from None


@pytest.mark.parametrize("entry", ["u32", "u16", "u32_27"])
def test_sort_host_side_answers(entry):
    """Answers given before anything is launched: n = 0, a temp buffer one byte short, a bad end_bit, a bad override."""
    end_bit = {"u32": 17, "u16": 13, "u32_27": 27}[entry]
    rng = np.random.default_rng(5)
    keys = make_keys("uniform", entry, end_bit, 1000, rng)
    vals = make_vals(1000, rng)

    def untouched(res):
        _, k_out, v_out, temp = res
        return bool((k_out.view(np.uint8) == OUT_BYTE).all() and (v_out.view(np.uint8) == OUT_BYTE).all() and (temp.host() == TEMP_BYTE).all())

    res = call_sort(entry, 8, keys, vals, end_bit, n=0)
    assert res[0] == 0 and untouched(res)
    res = call_sort(entry, 8, keys, vals, end_bit, temp_short=1)
    assert res[0] == HIP_ERROR_INVALID_VALUE and untouched(res)
    res = call_sort(entry, 12, keys, vals, end_bit)              # not an instantiation
    assert res[0] == HIP_ERROR_INVALID_VALUE and untouched(res)
    if entry == "u16":
        res = call_sort(entry, 8, keys, vals, 17)
        assert res[0] == HIP_ERROR_INVALID_VALUE and untouched(res)


def test_sort_size_rule_picks_16_items():
    """override 0 just above 3 M items: the size rule, the temp sizing and the 16-item kernels agree."""
    n = (3 << 20) + 1
    rng = np.random.default_rng(11)
    keys = make_keys("uniform", "u32", 17, n, rng)
    check_sort("u32", 0, keys, make_vals(n, rng), 17, ref_perm(keys, "u32", 17))


def test_temp_bytes_bound_every_instantiation():
    """The layouts the entry points carve out of temp (radegs_sort.hip), recomputed here for every allowed override, fit *_temp_bytes(n)."""
    L = _lib()
    up = lambda x: (x + 255) & ~255
    for n in [1, 2047, 2048, 2049, 8193, (2 << 20), (2 << 20) + 1, (3 << 20) + 1, (32 << 20) + 1, 50_000_000, 400_000_000]:
        for items in (8, 16, 32):
            nblocks = -(-n // (256 * items))
            need = 2 * up(4 * n) + up(512 * nblocks * 4) + up(512 * 4)
            assert need <= L.sortcheck_sort_temp_bytes(n), (n, items)
        for items in (4, 16):
            nb64 = (-(-n // (256 * items)) + 64) & ~63
            assert nb64 * 12 + 4 * n <= L.sortcheck_scan_temp_bytes(n), (n, items)


# ------------------------------------------------------- the order of two-word pairs -------------------------------------------------------

PAIR_SIZES = [1, 63, 2047, 2048, 2049, 3 * 2048 + 517]      # the size rule picks the 8-item instantiation: a block is 2048
PAIR_BITS = [(1, 1), (17, 21), (32, 32)]                    # (minor_end_bit, major_end_bit)
PAIR_PATTERNS = ["uniform", "equal_major", "equal_minor", "major_only", "ties8"]


def _words(n, rng):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def make_pairs(pattern, n, rng):
    minor, major = _words(n, rng), _words(n, rng)
    if pattern == "equal_major":                              # the minor word alone decides
        major[:] = major[0]
    elif pattern == "equal_minor":
        minor[:] = minor[0]
    elif pattern == "major_only":                             # neighbours in the input that differ in bit 0 of the major word and nowhere else:
        minor, major = minor[np.arange(n) // 2], major[np.arange(n) // 2] & np.uint32(0xFFFFFFFE)   # the minor sort leaves them adjacent
        major = major | ((np.arange(n) & 1) ^ rng.integers(0, 2, n)[np.arange(n) // 2]).astype(np.uint32)
    elif pattern == "ties8":                                  # eight distinct pairs: stability is what orders the rest
        pick = rng.integers(0, 8, n)
        minor, major = _words(8, rng)[pick], (_words(8, rng) & np.uint32(0xFFFFFFF8) | np.arange(8, dtype=np.uint32))[pick]
    else:
        assert pattern == "uniform", pattern
    return np.ascontiguousarray(minor), np.ascontiguousarray(major)


def ref_pair_perm(minor, major, bits):
    mask = [np.uint32(0xFFFFFFFF >> (32 - b)) for b in bits]
    return np.lexsort((minor & mask[0], major & mask[1]))   # stable: ties keep input order


def call_sort_2x(minor, major, bits, n=None, m=None, temp_short=0, join=True):
    """One call.  minor / major: host arrays of the capacity `n` (default: their length); m: the device-side count or None; join=False
    passes a null `joined`, join=None calls the entry point that has no such argument.  Returns (rc, major_sorted, perm, untouched, joined) after asserting guards and untouched inputs; untouched: no
    byte of the outputs, the three scratch arrays or temp was written; joined: the 8-byte-per-item output as raw bytes."""
    L = _lib()
    n = len(minor) if n is None else n
    d_minor, d_major = _upload(minor), _upload(major)
    d_m = None if m is None else torch.tensor([m], dtype=torch.int64).to(torch.int32).to(DEV)
    temp_bytes = L.sortcheck_sort_temp_bytes(n) - temp_short
    temp = Guarded(temp_bytes, TEMP_BYTE)
    outs = [Guarded(len(minor) * 4, OUT_BYTE) for _ in range(5)]      # major_sorted, perm, s0, s1, s2
    joined = Guarded(len(minor) * 8, OUT_BYTE)
    args = (temp.ptr, temp_bytes, _ptr(d_minor), _ptr(d_major), *[o.ptr for o in outs], n, bits[0], bits[1], _stream(), _ptr(d_m))
    rc = L.sortcheck_sort_2xu32(*args) if join is None else L.sortcheck_sort_2xu32_joined(*args, joined.ptr if join else None)
    if DEV != "cpu":
        torch.cuda.synchronize()
    assert temp.guards_intact(), "temp guards overwritten"
    for name, o in zip(("major_sorted", "perm", "s0", "s1", "s2"), outs):
        assert o.guards_intact(), name + " guards overwritten"
    assert joined.guards_intact(), "joined guards overwritten"
    assert _unchanged(d_minor, minor), "minor modified"
    assert _unchanged(d_major, major), "major modified"
    assert d_m is None or int(d_m.cpu()[0]) == np.int32(np.uint32(m)), "n_dev modified"
    untouched = bool((temp.host() == TEMP_BYTE).all()) and all(bool((o.host() == OUT_BYTE).all()) for o in outs)
    return rc, outs[0].host(np.uint32), outs[1].host(np.uint32), untouched, joined.host()


def check_sort_2x(minor, major, bits, perm, m=None):
    rc, major_sorted, perm_out, _, joined = call_sort_2x(minor, major, bits, m=m)
    assert rc == 0, "hip error %d" % rc
    cnt = len(perm)
    want = major[perm].astype(np.uint64) << np.uint64(32) | minor[perm].astype(np.uint64)      # the raw words, the bits above the end bits too
    bad = np.flatnonzero(joined[:8 * cnt].view(np.uint64) != want)
    assert bad.size == 0, "joined differs at %d of %d positions, first %d" % (bad.size, cnt, bad[0])
    assert (joined[8 * cnt:] == OUT_BYTE).all(), "joined written past the first %d positions" % cnt
    bad = np.flatnonzero(perm_out[:cnt] != perm.astype(np.uint32))
    assert bad.size == 0, "perm differs at %d of %d positions, first %d (a stable order keeps ties in input order)" % (bad.size, cnt, bad[0])
    bad = np.flatnonzero(major_sorted[:cnt] != major[perm])
    assert bad.size == 0, "major_sorted differs at %d of %d positions, first %d" % (bad.size, cnt, bad[0])


@pytest.mark.parametrize("pattern", PAIR_PATTERNS)
@pytest.mark.parametrize("bits", PAIR_BITS, ids=lambda b: "bits%d_%d" % b)
def test_sort_2xu32(bits, pattern):
    """n = 1, a ragged wave, around one block, and three blocks with a ragged tail (the carry across blocks)."""
    rng = np.random.default_rng(_seed("2xu32", bits, pattern))
    for n in PAIR_SIZES:
        minor, major = make_pairs(pattern, n, rng)
        try:
            check_sort_2x(minor, major, bits, ref_pair_perm(minor, major, bits))
        except AssertionError as e:
            raise AssertionError("n=%d: %s" % (n, e)) from None


@pytest.mark.parametrize("bits", PAIR_BITS, ids=lambda b: "bits%d_%d" % b)
def test_sort_2xu32_device_side_count(bits):
    """n is a capacity and the count m is read on the device: the first min(m, cap) outputs are the order of the first min(m, cap) pairs,
    whatever lies behind them in the input."""
    cap = 2049
    rng = np.random.default_rng(_seed("2xu32", bits, "n_dev"))
    minor, major = make_pairs("uniform", cap, rng)           # random all the way: the pairs past m are the poison
    for m in (0, 1, 2048, 2049, 3049):
        cnt = min(m, cap)
        try:
            check_sort_2x(minor, major, bits, ref_pair_perm(minor[:cnt], major[:cnt], bits), m=m)
        except AssertionError as e:
            raise AssertionError("cap=%d m=%d: %s" % (cap, m, e)) from None


def test_sort_2xu32_host_side_answers():
    """Answers given before anything is launched: n = 0, a temp buffer one byte short, an end bit outside 1 .. 32."""
    minor, major = make_pairs("uniform", 1000, np.random.default_rng(5))
    rc, _, _, untouched, joined = call_sort_2x(minor, major, (17, 21), n=0)
    assert rc == 0 and untouched and (joined == OUT_BYTE).all()
    rc, _, _, untouched, joined = call_sort_2x(minor, major, (17, 21), temp_short=1)
    assert rc == HIP_ERROR_INVALID_VALUE and untouched and (joined == OUT_BYTE).all()
    for bits in ((0, 21), (33, 21), (17, 0), (17, 33)):
        rc, _, _, untouched, joined = call_sort_2x(minor, major, bits)
        assert rc == HIP_ERROR_INVALID_VALUE and untouched and (joined == OUT_BYTE).all(), bits


def test_sort_2xu32_without_join():
    """A null `joined`, and the entry point without the argument: nothing is written there, and perm and major_sorted are what the call
    with it gives."""
    minor, major = make_pairs("uniform", 2049, np.random.default_rng(6))
    with_join = call_sort_2x(minor, major, (17, 21))
    assert with_join[0] == 0
    for join in (False, None):
        rc, major_sorted, perm, _, joined = call_sort_2x(minor, major, (17, 21), join=join)
        assert rc == 0
        assert (joined == OUT_BYTE).all()
        assert np.array_equal(perm, with_join[2]) and np.array_equal(perm, ref_pair_perm(minor, major, (17, 21)).astype(np.uint32))
        assert np.array_equal(major_sorted, with_join[1]) and np.array_equal(major_sorted, major[perm])


# ---------------------------------------------------------------- scan ----------------------------------------------------------------

def make_scan_vals(n, packed, rng):
    if not packed:
        c = rng.integers(0, 41, n, dtype=np.uint64)
        c[rng.random(n) < 0.5] = 0                       # culled Gaussians touch no tile
        return c.astype(np.uint32)
    x0, y0 = rng.integers(0, 256, n, dtype=np.uint64), rng.integers(0, 256, n, dtype=np.uint64)      # must be ignored
    w, h = rng.integers(0, 16, n, dtype=np.uint64), rng.integers(0, 16, n, dtype=np.uint64)
    big = rng.choice(n, size=8 if n >= 8 else 1, replace=False)   # 8 x (255 * 255)^2 > 2^32 while the plain sum stays below it
    w[big] = 255
    h[big] = 255
    return (x0 | (y0 << 8) | (w << 16) | (h << 24)).astype(np.uint32)


def check_scan(items, n, use_idx, packed, want_sq, rng):
    L = _lib()
    vals = make_scan_vals(n, packed, rng)
    idx = rng.permutation(n).astype(np.uint32) if use_idx else None
    g = vals if idx is None else vals[idx]
    c = (((g >> 16) & 255) * (g >> 24) if packed else g).astype(np.uint64)
    d_vals, d_idx = _upload(vals), _upload(idx)
    temp_bytes = L.sortcheck_scan_temp_bytes(n)
    temp, out, sq = Guarded(temp_bytes, TEMP_BYTE), Guarded(4 * n, OUT_BYTE), Guarded(8, OUT_BYTE)
    p_out = Guarded(4 * n, OUT_BYTE) if packed else None
    rc = L.sortcheck_scan(temp.ptr, temp_bytes, _ptr(d_vals), _ptr(d_idx), out.ptr, n, _stream(), p_out.ptr if packed else None,
                          sq.ptr if want_sq else None, items)
    if DEV != "cpu":
        torch.cuda.synchronize()
    assert rc == 0, "hip error %d" % rc
    for name, b in (("temp", temp), ("out", out), ("sq_sum", sq), ("packed_out", p_out)):
        assert b is None or b.guards_intact(), name + " guards overwritten"
    assert _unchanged(d_vals, vals), "vals modified"
    assert _unchanged(d_idx, idx), "idx modified"
    bad = np.flatnonzero(out.host(np.uint32) != np.cumsum(c).astype(np.uint32))
    assert bad.size == 0, "out differs at %d of %d positions, first %d" % (bad.size, n, bad[0])
    if packed:
        assert np.array_equal(p_out.host(np.uint32), g), "packed_out != vals[idx]"
    if want_sq:
        assert int(sq.host(np.uint64)[0]) == int((c * c).sum()), "sq_sum %d != %d" % (int(sq.host(np.uint64)[0]), int((c * c).sum()))
    else:
        assert (sq.host() == OUT_BYTE).all(), "sq_sum written although no pointer was passed"


def scan_sizes(items):
    bs = 256 * items
    return [1, 63, 64, 65, bs - 1, bs, bs + 1, 2 * bs + items + 1, 257 * bs + 3]


SCAN_CASES = [(j, n) for j in (4, 16) for n in scan_sizes(j)]


@pytest.mark.parametrize("want_sq", [False, True], ids=["nosq", "sq"])
@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("use_idx", [False, True], ids=["identity", "perm"])
@pytest.mark.parametrize("case", SCAN_CASES, ids=lambda c: "items%d-n%d" % c)
def test_scan(case, use_idx, packed, want_sq):
    """n around the block (256 * items), a ragged third block, and 258 blocks: the loop over the earlier blocks' sums runs a second trip."""
    items, n = case
    check_scan(items, n, use_idx, packed, want_sq, np.random.default_rng(_seed(items, n, use_idx, packed, want_sq)))


@pytest.mark.parametrize("n", [2 << 20, (2 << 20) + 1])
def test_scan_size_rule_switch(n):
    """override 0 on both sides of the 4 -> 16 items switch: rule, temp sizing and kernels agree."""
    check_scan(0, n, True, True, True, np.random.default_rng(n))


def test_scan_host_side_answers():
    L = _lib()
    n = 1000
    d_vals = _upload(make_scan_vals(n, False, np.random.default_rng(3)))
    for n_arg, short, items, want in ((0, 0, 4, 0), (n, 1, 4, HIP_ERROR_INVALID_VALUE), (n, 0, 8, HIP_ERROR_INVALID_VALUE)):
        temp_bytes = L.sortcheck_scan_temp_bytes(n) - short
        temp, out, sq = Guarded(temp_bytes, TEMP_BYTE), Guarded(4 * n, OUT_BYTE), Guarded(8, OUT_BYTE)
        rc = L.sortcheck_scan(temp.ptr, temp_bytes, _ptr(d_vals), None, out.ptr, n_arg, _stream(), None, sq.ptr, items)
        if DEV != "cpu":
            torch.cuda.synchronize()
        assert rc == want, (n_arg, short, items, rc)
        assert (temp.host() == TEMP_BYTE).all() and (out.host() == OUT_BYTE).all() and (sq.host() == OUT_BYTE).all()
        assert temp.guards_intact() and out.guards_intact() and sq.guards_intact()
