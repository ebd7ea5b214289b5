"""The acceptance step of the search driver on the device: sdf_search_accept / sdf_search_accept_device
(sedef_amd/csrc/search_accept.hip).

Expected values: the host form (sdf_search_accept_host) and the model of tests/driver_model.py, which
tests/test_search_driver_cpu.py checks against each other.  Every comparison is exact, the status record included."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import found_model as FM  # noqa: E402
from test_search_driver_cpu import big_rounds, check_accept, hand_made_rounds  # noqa: E402

pytestmark = pytest.mark.gpu

SDF_ERR_OVERFLOW = -5

CANARY = 4


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


def ex():
    from sedef_amd import extz2
    return extz2


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def ptr(t):
    return t.data_ptr() if t.numel() else None


def same_as_host(eng, case):
    """The case through sdf_search_accept: the model's answer, and the host form's bytes."""
    extz2 = ex()
    dev = check_accept(eng.search_accept_raw, case, extz2)
    host = check_accept(extz2.search_accept_host, case, extz2)
    for a, b in zip(dev, host):
        assert a.tobytes() == b.tobytes(), case[0]


def test_accept_is_the_host_form_on_hand_made_rounds(eng):
    for case in hand_made_rounds():
        same_as_host(eng, case)


@pytest.mark.parametrize("case", big_rounds(), ids=lambda c: c[0])
def test_accept_is_the_host_form_at_its_size_boundaries(eng, case):
    """65 candidates (more than lanes), the cap and one more, a round of one window, of 300, of 2,100 (the frontier's
    workgroup takes 1,024 windows a pass)."""
    same_as_host(eng, case)


def device_accept(eng, A, found, out, found_cap, out_cap, base=0, stream=None):
    """sdf_search_accept_device on arrays uploaded here.  Returns the status record and the bytes of the two lists with their
    canary records."""
    extz2 = ex()
    d = {k: up(A[k]) for k in ("q", "act", "windows", "first", "rolls", "overlap", "filt", "hits", "hit_filter")}
    found_buf = np.frombuffer(bytearray(b"\xEE" * (16 * (found_cap + CANARY))), extz2.SEARCH_FOUND_DTYPE)
    out_buf = np.frombuffer(bytearray(b"\xEE" * (24 * (out_cap + CANARY))), extz2.SEARCH_PAIR_HIT_DTYPE)
    found_buf[:len(found)], out_buf[:len(out)] = found, out
    d_found, d_out = up(found_buf), up(out_buf)
    d_status = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    R = extz2.accept_round(ptr(d["q"]), len(A["q"]), ptr(d["act"]), len(A["act"]), ptr(d["windows"]), ptr(d["first"]), len(A["rolls"]),
                           ptr(d["rolls"]), ptr(d["overlap"]), ptr(d["filt"]), ptr(d["hits"]), ptr(d["hit_filter"]), A["init_len"],
                           A["min_read_size"], base)
    before = eng.last_launches()
    eng.search_accept_device(R, d_found.data_ptr(), len(found), found_cap, d_out.data_ptr(), len(out), out_cap, d_status.data_ptr(),
                             stream=stream.cuda_stream if stream is not None else None)
    launches = eng.last_launches() - before
    if stream is not None:
        stream.synchronize()
    status = np.frombuffer(d_status.cpu().numpy().tobytes(), extz2.ACCEPT_STATUS_DTYPE)[0]
    return status, d_found.cpu().numpy().tobytes(), d_out.cpu().numpy().tobytes(), launches


@pytest.mark.parametrize("own_stream", (False, True))
def test_the_device_form_on_device_arrays(eng, own_stream):
    """Every array in HBM, on the context's stream and on the caller's: the host form's bytes, canaries untouched, and three
    launches whatever the round holds (one for an empty round)."""
    extz2 = ex()
    cases = [c for c in big_rounds() if c[0].startswith(("a round of 300", "65"))] + hand_made_rounds()[:3]
    assert len(cases) == 6
    for name, Rd, found, outs, found_cap, out_cap, base, shows in cases:
        A = Rd.arrays(extz2)
        n = len(A["rolls"])
        found_cap = len(found) + n if found_cap is None else found_cap
        out_cap = len(outs) + n if out_cap is None else out_cap
        found_in = FM.found_records(found)
        out_in = np.zeros(len(outs), extz2.SEARCH_PAIR_HIT_DTYPE)
        for k, row in enumerate(outs):
            out_in[k] = row
        rc, want, want_found, want_out = extz2.search_accept_host(A["q"], A["act"], A["windows"], A["first"], A["rolls"], A["overlap"],
                                                                  A["filt"], A["hits"], A["hit_filter"], A["init_len"], A["min_read_size"],
                                                                  found_in, out_in, found_cap=found_cap, out_cap=out_cap, window_base=base)
        assert rc == 0
        status, got_found, got_out, launches = device_accept(eng, A, found_in, out_in, found_cap, out_cap, base,
                                                             torch.cuda.Stream() if own_stream else None)
        assert status.tobytes() == want.tobytes(), name
        assert got_found == want_found.tobytes() and got_out == want_out.tobytes(), name
        assert launches == (3 if len(A["act"]) else 1), name


def test_the_device_form_refuses_before_it_launches(eng):
    extz2 = ex()
    d_zero = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    z = d_zero.data_ptr()

    def code(found=z + 1024, found_cap=4, out=z + 1536, out_cap=4, status=z + 2048, nf=0, **change):
        args = dict(q=z, nq=2, act=z, na=1, windows=z, first=z, n_max=0, rolls=None, overlap=None, filt=None, hits=None, hit_filter=None,
                    init_len=100, min_read_size=100)
        args.update(change)
        R = extz2.accept_round(**args)
        before = eng.last_launches()
        rc = eng.lib.sdf_search_accept_device(eng.ctx, C.byref(R), found, nf, found_cap, out, 0, out_cap, status, None)
        assert rc == 0 or eng.last_launches() == before
        return rc
    assert code() == 0
    assert code(init_len=0) == -4 and code(min_read_size=-1) == -4 and code(status=None) == -4 and code(found=None) == -4
    assert code(nf=5) == -4 and code(act=None) == -4 and code(first=None) == -4 and code(n_max=1) == -4
    assert code(init_len=(1 << 30) + 1) == -3 and code(na=1 << 31) == -3 and code(found_cap=1 << 31) == -3 and code(reserved=1) == -3


# ---- the driver: sdf_search_pair against sdf_search_pair_host on the drawn inputs ----

from test_search_driver_cpu import INPUTS, host_pair  # noqa: E402
import driver_model as DM  # noqa: E402

_hosted, _driven = {}, {}


def hosted(which):
    """The inputs and sdf_search_pair_host's answer for them (which tests/test_search_driver_cpu.py pins on the model)."""
    if which not in _hosted:
        I = DM.inputs(*which)
        rc, hits, used, stats = host_pair(I)
        assert rc == 0 and used == len(hits) >= 5
        _hosted[which] = (I, hits, stats)
    return _hosted[which]


def drive(eng, which, cap=None, **kw):
    """sdf_search_pair on the input's characters, uploaded as the pool."""
    extz2 = ex()
    I = hosted(which)[0]
    eng.pool_upload(I["pool"])
    eng.pool_sync()
    return eng.search_pair(I["q_range"], I["r_range"], k=I["k"], w=I["w"], min_read_size=I["init_len"], same_genome=I["same_genome"],
                           limit=I["limit"], extend=extz2.extend_params(same_genome=bool(I["same_genome"]), max_sd_size=int(2.5 * I["init_len"])),
                           cap=cap, **kw)


def same_answer(got, want):
    rc, hits, used, stats = got
    _, want_hits, want_stats = want
    assert rc == 0 and used == len(want_hits)
    assert hits.tobytes() == want_hits.tobytes()
    for f in ("attempted", "jaccard_failed", "interval_failed", "windows_scheduled"):
        assert int(stats[f]) == int(want_stats[f]), f


@pytest.mark.parametrize("round_windows", (1, 2, 7, 64, 0))
@pytest.mark.parametrize("which", INPUTS)
def test_the_driver_is_the_host_form_for_every_round_size(eng, which, round_windows):
    """round_windows = 1 is the sequential order run through the device."""
    got = drive(eng, which, round_windows=round_windows)
    same_answer(got, hosted(which))
    stats = got[3]
    print(which, round_windows, {f: int(stats[f]) for f in stats.dtype.names})
    assert int(stats["rounds"]) >= 1 and int(stats["windows_run"]) >= int(stats["windows_scheduled"])
    if round_windows == 1:
        assert int(stats["rounds"]) + int(stats["windows_host"]) >= int(stats["windows_scheduled"])
    # ... and exactly the rounds of the model, which needs no more than the starting capacities here
    R = DM.rounds(ex(), hosted(which)[0], round_windows)
    assert all(p[2] <= DM.PAIR_INTERVALS_START and p[3] <= DM.PAIR_ENTRIES_START for p in R["per_round"])
    assert {f: int(stats[f]) for f in ("rounds", "windows_run", "windows_host")} == {f: R[f] for f in ("rounds", "windows_run", "windows_host")}
    _driven[(which, round_windows)] = {f: int(stats[f]) for f in stats.dtype.names}


def test_some_round_had_a_frontier_short_of_its_end(eng):
    """The seam is crossed: with rounds of 64 windows some window ran twice, because a record of its own round reached it."""
    for which in INPUTS:
        if (which, 64) not in _driven:
            got = drive(eng, which, round_windows=64)
            _driven[(which, 64)] = {f: int(got[3][f]) for f in got[3].dtype.names}
    repeats = [d["windows_run"] - d["windows_scheduled"] for (w, r), d in _driven.items() if r == 64]
    more_rounds = [d["rounds"] - (d["windows_scheduled"] + 63) // 64 for (w, r), d in _driven.items() if r == 64]
    print(repeats, more_rounds)
    assert max(repeats) >= 1 and max(more_rounds) >= 1


@pytest.mark.parametrize("which", INPUTS)
def test_windows_completed_on_the_host_leave_the_answer_as_it_is(eng, which):
    got = drive(eng, which, debug_host_every=3)
    same_answer(got, hosted(which))
    scheduled = int(got[3]["windows_scheduled"])
    assert int(got[3]["windows_host"]) >= scheduled // 3 >= 1


def test_out_one_short_through_the_driver(eng):
    which = INPUTS[0]
    want = hosted(which)[1]
    rc, hits, used, _ = drive(eng, which, cap=len(want) - 1)
    assert rc == SDF_ERR_OVERFLOW and used == len(want) and len(hits) == 0
    # ... and nothing is written: the call itself, on a buffer of its own
    extz2 = ex()
    I = hosted(which)[0]
    limit = np.ascontiguousarray(I["limit"], np.int32)
    P = extz2._PairParams(I["k"], I["w"], 1, 1, I["init_len"], 0, extz2.filter_params(),
                          extz2.extend_params(max_sd_size=int(2.5 * I["init_len"])), limit.ctypes.data, len(limit), 0, 0)
    ranges = [extz2._MinimRange(*I["q_range"]), extz2._MinimRange(*I["r_range"])]
    out = np.full((len(want) - 1) * 6, -1, np.int32)
    need, stats = C.c_size_t(0), np.zeros(1, extz2.PAIR_STATS_DTYPE)
    rc = eng.lib.sdf_search_pair(eng.ctx, C.byref(ranges[0]), C.byref(ranges[1]), C.byref(P), out.ctypes.data, len(want) - 1, C.byref(need),
                                 stats.ctypes.data)
    assert rc == SDF_ERR_OVERFLOW and need.value == len(want) and (out == -1).all()


def test_the_driver_refuses_before_it_launches(eng):
    which = INPUTS[0]
    I = hosted(which)[0]
    eng.pool_upload(I["pool"])
    eng.pool_sync()
    before = eng.last_launches()

    def code(q_range=I["q_range"], r_range=I["r_range"], **kw):
        args = dict(k=I["k"], w=I["w"], min_read_size=I["init_len"], same_genome=0, limit=I["limit"])
        args.update(kw)
        return eng.search_pair(q_range, r_range, **args)[0]
    assert code(k=16) == -3 and code(w=0) == -3 and code(limit=[0, 1, 0]) == -3 and code(r_range=I["r_range"][:2] + (2,)) == -3
    assert code(min_read_size=0) == -4 and code(q_range=(0, len(I["pool"]) + 1, 0)) == -4 and code(q_range=(-1, 5, 0)) == -4
    assert code(same_genome=1) == -4 and code(same_genome=1, r_range=I["q_range"][:2] + (1,)) == -4
    assert eng.last_launches() == before
