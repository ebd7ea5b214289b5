"""Search seeding, the WIDE and FOUND_WIDE windows finished on the device: sdf_search_windows_wide_device
(sedef_amd/csrc/search_seeds_wide.hip).

Expected values: wide_model.wide_expected of sdf_search_windows_found_host's answer -- tests/test_search_wide_cpu.py shows what
every input holds.  Every comparison is byte for byte: first[], windows[], out[]."""
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
import search_model as S  # noqa: E402
import wide_model as WM  # noqa: E402
from test_gpu_search_found import device_windows, ptr, up  # noqa: E402
from test_search_windows_cpu import same_records  # noqa: E402

pytestmark = pytest.mark.gpu

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID, SDF_ERR_OVERFLOW = -3, -4, -5
CANARY = 8  # records behind every capacity, filled with 0xEE
NOT_WRITTEN = -7


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


def ex():
    from sedef_amd import extz2
    return extz2


def wide_device(eng, name, cap, n_wide_max, stream=None, with_index=True):
    """sdf_search_windows_wide_device on an input's arrays, uploaded here.  Returns (code, used, first, windows, the bytes of
    out and of the canary records behind out[cap], the eligible windows the call counted)."""
    extz2 = ex()
    q, r, found, visible, kw = WM.the_input(name)
    limit = np.ascontiguousarray(kw["limit"], np.int32)
    d_q, d_r, d_limit, d_found, d_vis = up(q), up(r), up(limit), up(found), up(visible)
    d_first = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
    d_win = torch.full((len(q) * 20,), 0xEE, dtype=torch.uint8, device="cuda")
    d_out = torch.full(((cap + CANARY) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    d_total = torch.full((1,), NOT_WRITTEN, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    used = C.c_size_t(0)
    code = eng.lib.sdf_search_windows_wide_device(
        eng.ctx, d_q.data_ptr(), len(q), int(kw["len_q"]), ptr(d_r), len(r), int(kw["r_threshold"]), int(kw["init_len"]),
        int(kw["same_genome"]), int(kw["uppercase_seeds"]), ptr(d_limit), len(limit), ptr(d_found), len(found),
        extz2.found_entries(found), None, d_vis.data_ptr() if with_index else None, d_first.data_ptr(), d_win.data_ptr(), d_out.data_ptr(),
        cap, C.byref(used), n_wide_max, d_total.data_ptr(), stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    windows = np.frombuffer(d_win.cpu().numpy().tobytes(), extz2.SEARCH_WINDOW_DTYPE)
    return code, int(used.value), d_first.cpu().numpy(), windows, d_out.cpu().numpy().tobytes(), int(d_total.cpu()[0])


def check(eng, name, n_wide_max, stream=None, with_index=True):
    """The call's answer is wide_expected of the host form, with nothing written behind the intervals.  Returns it."""
    wf, ww, wo, total = WM.wide_expected(WM.hosted(name), n_wide_max)
    code, used, gf, gw, raw, got_total = wide_device(eng, name, len(wo), n_wide_max, stream=stream, with_index=with_index)
    assert code == 0 and (stream is not None or used == len(wo))
    same_records((gf, gw, np.frombuffer(raw[:8 * len(wo)], ex().SEARCH_INTERVAL_DTYPE)), (wf, ww, wo))
    assert raw[8 * len(wo):] == b"\xEE" * (8 * CANARY)
    assert got_total == (total if n_wide_max else NOT_WRITTEN)
    return wf, ww, wo, total


# ---- 1. the gather seams ----

@pytest.mark.parametrize("name", ["seams", "seams_same_genome"])
def test_gathered_counts_at_every_seam_of_both_kernels(eng, name):
    q, r, found, visible, kw, counts, at = WM.seams_input(int(name == "seams_same_genome"))
    wf, ww, wo, total = check(eng, name, 64)
    flags = dict(zip(counts, (int(ww["flags"][a]) for a in at)))
    assert total == 6 and flags[4096] == 0 and flags[32769] == S.WIDE and flags[32768] == flags[4097] == WM.WIDE_DONE
    assert all(wf[a + 1] > wf[a] for a, g in zip(at, counts) if 4096 <= g != 32769)  # (the small blocks lie below the same_genome floor)
    check(eng, name, 64, with_index=False)  # (no record and no prefixes: the plain instantiations, without an index)


def test_duplicates_and_a_merge_where_every_position_passes_and_where_none_does(eng):
    wf, ww, wo, total = check(eng, "merge", 64)
    done = np.flatnonzero(ww["flags"] == WM.WIDE_DONE)
    assert total == 3 and (wf[done + 1] - wf[done]).tolist() == [109, 0, 1]
    assert ww["n_candidates"][done].tolist() == [4000, 5000, 6000] and ww["n_gathered"][done[0]] == 8000


# ---- 2. the members seam ----

def test_a_window_of_1025_members_is_left_as_it_is(eng):
    wf, ww, wo, total = check(eng, "members", 64)
    assert total == 0 and ww["n_members"][0] == 1025 and ww["flags"][0] == S.WIDE and not (ww["flags"] & WM.WIDE_DONE).any()
    q, r, found, visible, kw = WM.the_input("members")
    dev = device_windows(eng, q, r, found, visible, len(wo), **kw)
    assert dev[3].tobytes() == ww.tobytes() and np.array_equal(dev[2], wf)


# ---- 3. the found records ----

@pytest.mark.parametrize("name", ["found_256", "found_257", "found_600_half_hidden", "found_600_gather_5000"])
def test_found_records_beyond_the_staged_256(eng, name):
    wf, ww, wo, total = check(eng, name, 64)
    assert total == WM.INPUTS[name][1]
    assert ww["flags"][0] == (0 if name == "found_256" else WM.WIDE_DONE) and wf[1] > 0
    if name == "found_600_gather_5000":
        assert ww["n_gathered"][0] == 5000 and (ww["flags"][:9] == WM.WIDE_DONE).all()


# ---- 4. a list shorter than the need ----

def test_five_eligible_windows_and_room_for_two(eng):
    wf, ww, wo, total = check(eng, "five", 2)
    flagged = np.flatnonzero(ww["flags"])
    assert total == 5 and ww["flags"][flagged].tolist() == [WM.WIDE_DONE] * 2 + [S.WIDE] * 3
    again = [wide_device(eng, "five", len(wo), 2) for _ in range(2)]
    assert all(a[5] == 5 for a in again)
    assert again[0][2].tobytes() == again[1][2].tobytes() and again[0][3].tobytes() == again[1][3].tobytes() and again[0][4] == again[1][4]


# ---- 5. n_wide_max == 0 ----

@pytest.mark.parametrize("name", ["five", "found_600_half_hidden"])
def test_without_a_list_the_call_is_the_existing_device_form(eng, name):
    wf, ww, wo, total = check(eng, name, 0)
    q, r, found, visible, kw = WM.the_input(name)
    launches = eng.last_launches()
    code, used, gf, gw, raw, need = device_windows(eng, q, r, found, visible, len(wo), **kw)
    per_call = eng.last_launches() - launches
    got = wide_device(eng, name, len(wo), 0)
    assert eng.last_launches() - launches == 2 * per_call
    assert code == 0 and got[0] == 0 and got[1] == used and np.array_equal(got[2], gf) and got[3].tobytes() == gw.tobytes() and got[4] == raw


# ---- 6. capacity ----

def test_capacity_at_the_need_below_it_and_zero(eng):
    wf, ww, wo, total = WM.wide_expected(WM.hosted("five"), 8)
    need = len(wo)
    done = np.flatnonzero(ww["flags"] == WM.WIDE_DONE)
    assert need > 100 and len(done) == 5
    for cap in (need, need - 1, 0):
        code, used, gf, gw, raw, got_total = wide_device(eng, "five", cap, 8)
        assert code == (0 if cap >= need else SDF_ERR_OVERFLOW) and used == need and gf[-1] == need
        assert np.array_equal(gf, wf) and gw.tobytes() == ww.tobytes() and got_total == 5
        assert raw[8 * cap:] == b"\xEE" * (8 * CANARY)  # nothing at or behind out[cap]
        whole = max([int(wf[i + 1]) for i in range(len(ww)) if wf[i + 1] <= cap] + [0])
        assert raw[:8 * whole] == wo[:whole].tobytes()
    # a capacity that ends inside a wide window's intervals: the ones below it are there
    wf, ww, wo, total = WM.wide_expected(WM.hosted("merge"), 8)
    first_done = int(np.flatnonzero(ww["flags"] == WM.WIDE_DONE)[0])
    inside = int(wf[first_done]) + 50
    assert inside < wf[first_done + 1] - 1
    code, used, gf, gw, raw, got_total = wide_device(eng, "merge", inside, 8)
    assert code == SDF_ERR_OVERFLOW and used == len(wo) and raw[8 * inside:] == b"\xEE" * (8 * CANARY)
    assert raw[:8 * (inside - 1)] == wo[:inside - 1].tobytes()
    assert np.frombuffer(raw[8 * (inside - 1):8 * inside], ex().SEARCH_INTERVAL_DTYPE)["start"][0] == wo["start"][inside - 1]


# ---- 7. the caller's stream ----

@pytest.mark.parametrize("name", ["five", "found_600_gather_5000"])
def test_on_a_callers_stream_as_on_the_contexts(eng, name):
    check(eng, name, 64, stream=torch.cuda.Stream())


# ---- 8. refusals ----

def test_refusals_launch_nothing(eng):
    d_zero = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    z = d_zero.data_ptr()
    launches = eng.last_launches()
    used = C.c_size_t(0)
    good = [eng.ctx, z, 2, 10 ** 9, z, 1, 1 << 31, 100, 0, 1, z, 64, z, 1, 1, None, z, z + 1024, z + 2048, None, 0, C.byref(used), 4, None,
            None]
    for at, value, want in ((1, None, SDF_ERR_INVALID), (12, None, SDF_ERR_INVALID), (16, None, SDF_ERR_INVALID), (17, None, SDF_ERR_INVALID),
                            (7, 0, SDF_ERR_INVALID), (7, (1 << 30) + 1, SDF_ERR_UNSUPPORTED), (13, 1 << 31, SDF_ERR_UNSUPPORTED),
                            (14, 1 << 31, SDF_ERR_UNSUPPORTED), (22, (1 << 20) + 1, SDF_ERR_UNSUPPORTED)):
        bad = list(good)
        bad[at] = value
        assert eng.lib.sdf_search_windows_wide_device(*bad) == want, at
    assert b"n_wide_max" in eng.lib.sdf_last_error(eng.ctx)
    none = list(good)
    none[2] = 0  # nq == 0: SDF_OK without a launch
    assert eng.lib.sdf_search_windows_wide_device(*none) == 0
    assert eng.last_launches() == launches
    # ... and a good call launches: three for the index, five of the count pass, the list and the wide count, the two emits
    assert eng.lib.sdf_search_windows_wide_device(*good) == SDF_ERR_OVERFLOW and used.value > 0  # (cap 0: counted, nothing emitted)
    assert eng.last_launches() == launches + 12


def test_the_convenience_form_brings_the_answer_back(eng):
    q, r, found, visible, kw = WM.the_input("found_600_gather_5000")
    wf, ww, wo, total = WM.wide_expected(WM.hosted("found_600_gather_5000"), 3)
    first, windows, out, got_total = eng.search_windows_wide(q, r, found=found, visible=visible, n_wide_max=3, **kw)
    same_records((first, windows, out), (wf, ww, wo))
    assert got_total == total == 9
