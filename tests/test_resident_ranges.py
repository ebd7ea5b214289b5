"""Where a DP request of the stage driver finds its bases in a resident chromosome (host/stage_driver.cc: resident_range, exported
as sdfh_resident_range): the rule of INTEGRATION.md section 2 against a brute-force model and against real bytes."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from sedef_amd import host as h
    from sedef_amd.build import build_library
    build_library()
    h.build_host()
    lib = h.load_host()
    lib.sdfh_resident_range.argtypes = [C.c_longlong] * 5 + [C.c_int, C.POINTER(C.c_longlong)]
    lib.sdfh_resident_range.restype = C.c_int
    return lib


def call(lib, base, start, seq_len, s, length, rc):
    off = C.c_longlong(-12345)
    r = lib.sdfh_resident_range(base, start, seq_len, s, length, int(rc), C.byref(off))
    return r, int(off.value)


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(b):
    return b.translate(_COMP)[::-1]


def model(base, start, seq_len, s, length, rc):
    """Positions, one by one: byte x of the host's copy is chromosome base start + x forward, start + seq_len - 1 - x reversed;
    the range is the set of pool bytes the request's bytes come from, which must be contiguous, named by its lowest."""
    if s < 0 or length < 0 or s + length > seq_len:
        return None
    at = [base + (start + seq_len - 1 - x if rc else start + x) for x in range(s, s + length)]
    if not at:  # (an empty request: where its first byte would be -- forward -- or just behind its last -- reversed)
        return base + (start + seq_len - s if rc else start + s)
    assert sorted(at) == list(range(min(at), min(at) + length))
    return min(at)


def test_resident_range_against_brute_force(lib):
    for base, start in ((0, 0), (1000, 7), ((1 << 31) + 5, 123456)):
        for seq_len in range(0, 13):
            for s in range(-1, seq_len + 2):
                for length in range(-1, seq_len + 2):
                    for rc in (False, True):
                        want = model(base, start, seq_len, s, length, rc)
                        r, off = call(lib, base, start, seq_len, s, length, rc)
                        if want is None:
                            assert r == -1, (base, start, seq_len, s, length, rc)
                        else:
                            assert (r, off) == (0, want), (base, start, seq_len, s, length, rc)


def test_resident_range_names_the_bytes_of_the_host_copy(lib):
    """The named pool range, reverse-complemented when rc, IS the substring of the host's copy."""
    rng = np.random.default_rng(5)
    pool = bytes(np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, 50000)])
    for _ in range(400):
        base = int(rng.integers(0, 20000))
        start = int(rng.integers(0, 10000))
        seq_len = int(rng.integers(1, 20000))
        s = int(rng.integers(0, seq_len))
        length = int(rng.integers(0, seq_len - s + 1))
        for rc in (False, True):
            fetched = pool[base + start:base + start + seq_len]
            copy = revcomp(fetched) if rc else fetched
            r, off = call(lib, base, start, seq_len, s, length, rc)
            assert r == 0
            named = pool[off:off + length]
            assert (revcomp(named) if rc else named) == copy[s:s + length]
