"""CPU side of sdf_pool_fetch_ranges: the settings it adds are listed with their defaults, the exports exist, and
sdf_pool_fetch_plan -- the pure helper that turns ranges into the device form's records -- agrees with a Python model."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEG = 16384
SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID = -3, -4


def _lib():
    from sedef_amd.build import build_library
    from sedef_amd.extz2 import load_library
    build_library()
    return load_library()


def plan(lib, rows, pool_bytes, dst_bytes, want_recs=True):
    from sedef_amd.extz2 import POOL_FETCH_DTYPE, POOL_FETCH_REC_DTYPE
    r = np.zeros(len(rows), POOL_FETCH_DTYPE)
    for i, row in enumerate(rows):
        r[i] = row
    recs = np.zeros(len(rows), POOL_FETCH_REC_DTYPE)
    any_rc, n_seg, nbytes, bad = C.c_int(-1), C.c_longlong(-1), C.c_size_t(77), C.c_size_t(77)
    rc = lib.sdf_pool_fetch_plan(r.ctypes.data if len(r) else None, len(r), pool_bytes, dst_bytes,
                                 recs.ctypes.data if want_recs and len(r) else None, C.byref(any_rc), C.byref(n_seg),
                                 C.byref(nbytes), C.byref(bad))
    return rc, recs, any_rc.value, n_seg.value, nbytes.value, bad.value


def model(rows):
    """(records, any_rc, n_seg, bytes) as include/sedef_hip.h describes them."""
    recs, seg, any_rc, total = [], 0, 0, 0
    for off, ln, flags, dst_off in rows:
        recs.append((off, dst_off, ln, 1 if flags & 1 else 0, seg))
        seg += -(-ln // SEG)
        any_rc |= flags & 1
        total += ln
    return recs, any_rc, seg, total


def test_settings_are_listed_with_their_defaults():
    from sedef_amd import host
    from sedef_amd.extz2 import Config, describe_config
    _lib()
    line = [ln for ln in describe_config().splitlines() if ln.startswith("SDF_FETCH_STAGE_BYTES")]
    assert len(line) == 1 and "fetch_stage_bytes" in line[0] and "default 67108864" in line[0]
    assert Config(from_env=False).as_dict()["SDF_FETCH_STAGE_BYTES"] == 64 << 20
    assert Config(from_env=False, SDF_FETCH_STAGE_BYTES=65536).as_dict()["SDF_FETCH_STAGE_BYTES"] == 65536
    # the stage driver's switch: in the CLI's list next to SDF_STAGE_RESIDENT, default 0, read and checked like its neighbours
    host.build_host()
    env = {k: v for k, v in os.environ.items() if not k.startswith("SDF_")}
    r = subprocess.run([host.CLI, "help"], capture_output=True, text=True, env=env)
    assert r.returncode == 0
    assert "SDF_STAGE_RESIDENT=1" in r.stderr and "SDF_STAGE_FETCH_DEVICE=1 (default 0" in r.stderr
    r = subprocess.run([host.CLI, "help"], capture_output=True, text=True, env=dict(env, SDF_STAGE_FETCH_DEVICE="2"))
    assert r.returncode != 0 and "SDF_STAGE_FETCH_DEVICE=2: out of range" in r.stderr
    r = subprocess.run([host.CLI, "help"], capture_output=True, text=True, env=dict(env, SDF_STAGE_FETCH_DEVICE="1"))
    assert r.returncode == 0


def test_exports():
    lib = _lib()
    for name in ("sdf_pool_fetch_ranges", "sdf_pool_fetch_ranges_device", "sdf_pool_fetch_plan"):
        assert hasattr(lib, name), name
    assert len(lib.sdf_pool_fetch_ranges.argtypes) == 5 and len(lib.sdf_pool_fetch_ranges_device.argtypes) == 7


def test_plan_against_the_model():
    lib = _lib()
    rng = np.random.default_rng(3)
    long_len = (1 << 20) + 3
    n = long_len + 90
    rows, d = [(5, long_len, 0, 7)], 7 + long_len
    for k in range(1000):
        ln = 1 + int(rng.integers(0, 40))
        rows.append((int(rng.integers(0, n - ln)), ln, int(rng.integers(0, 2)), d))
        d += ln
    rows.append((11, long_len, 1, d))
    d += long_len
    for ln in (SEG, SEG - 1, SEG + 1, 0, 2 * SEG, 2 * SEG + 1):
        rows.append((3, ln, ln & 1, d))
        d += ln
    rc, recs, any_rc, n_seg, nbytes, bad = plan(lib, rows, n, d)
    exp, exp_rc, exp_seg, exp_bytes = model(rows)
    assert rc == 0 and (any_rc, n_seg, nbytes) == (exp_rc, exp_seg, exp_bytes) and exp_rc == 1
    assert [tuple(int(x) for x in r) for r in recs.tolist()] == exp
    assert n_seg == 2 * 65 + 1000 + 1 + 1 + 2 + 0 + 2 + 3
    # counts alone, without records
    assert plan(lib, rows, n, d, want_recs=False)[2:5] == (exp_rc, exp_seg, exp_bytes)
    # forward only: any_rc == 0
    fwd = [(o, ln, 0, dd) for o, ln, _, dd in rows]
    assert plan(lib, fwd, n, d)[2] == 0
    # a table of empty ranges: no segment, every seg0 zero
    empty = [(0, 0, 0, 0), (n, 0, 1, d), (17, 0, 0, 5)]
    rc, recs, any_rc, n_seg, nbytes, bad = plan(lib, empty, n, d)
    assert rc == 0 and n_seg == 0 and nbytes == 0 and any_rc == 1 and (recs["seg0"] == 0).all() and (recs["len"] == 0).all()
    assert plan(lib, [], n, d)[:5:4] == (0, 0)


def test_plan_refusals_name_the_first_offending_range():
    lib = _lib()
    ok = (10, 100, 0, 0)
    for bad_row, code in (((-1, 4, 0, 0), SDF_ERR_INVALID), ((0, -1, 0, 0), SDF_ERR_INVALID), ((4000, 97, 0, 0), SDF_ERR_INVALID),
                          ((4097, 0, 0, 0), SDF_ERR_INVALID), ((0, 4, 0, -1), SDF_ERR_INVALID), ((0, 4, 1, 509), SDF_ERR_INVALID),
                          ((0, 0, 0, 513), SDF_ERR_INVALID), ((0, 4, 2, 0), SDF_ERR_UNSUPPORTED), ((0, 4, 0x101, 0), SDF_ERR_UNSUPPORTED)):
        for rows, at in (([bad_row], 0), ([ok, ok, bad_row, bad_row], 2), ([bad_row, ok], 0)):
            rc, _, any_rc, n_seg, nbytes, bad = plan(lib, rows, 4096, 512)
            assert rc == code and bad == at and (any_rc, n_seg, nbytes) == (0, 0, 0), (bad_row, rows)
    # ranges that end exactly at the bounds are fine
    assert plan(lib, [(4000, 96, 1, 416), (4096, 0, 0, 512)], 4096, 512)[0] == 0
