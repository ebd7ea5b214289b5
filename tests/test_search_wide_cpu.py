"""CPU: the statement of sdf_search_windows_wide_device (tests/wide_model.py) on the inputs of tests/test_gpu_search_wide.py and
tests/test_gpu_search_wide_driver.py -- each input holds the windows its name promises, and no test can pass on empty answers."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import driver_model as DM  # noqa: E402
import found_model as FM  # noqa: E402
import search_model as S  # noqa: E402
import wide_model as WM  # noqa: E402


def ex():
    from sedef_amd import extz2
    return extz2


def test_the_headers_defines_are_the_bindings():
    src = open(os.path.join(ROOT, "include", "sedef_hip.h")).read()
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(SDF_SEARCH_\w+)\s+(0x[0-9a-fA-F]+|\d+)", src)}
    extz2 = ex()
    assert defines["SDF_SEARCH_WIDE_DONE"] == extz2.SEARCH_WIDE_DONE == WM.WIDE_DONE == 0x10
    assert defines["SDF_SEARCH_WIDE_MAX_GATHER"] == extz2.SEARCH_WIDE_MAX_GATHER == WM.WIDE_MAX_GATHER == 32768
    flags = [defines[n] for n in ("SDF_SEARCH_SHORT", "SDF_SEARCH_NOLIMIT", "SDF_SEARCH_WIDE", "SDF_SEARCH_FOUND_WIDE", "SDF_SEARCH_WIDE_DONE")]
    assert flags == [1, 2, 4, 8, 16]
    assert defines["SDF_SEARCH_MAX_GATHER"] < defines["SDF_SEARCH_WIDE_MAX_GATHER"]
    lib = extz2.load_library()
    for name in ("sdf_search_windows_wide_device", "sdf_search_pair_wide", "sdf_search_pair_indexed_wide"):
        assert hasattr(lib, name)


@pytest.mark.parametrize("name", sorted(WM.INPUTS))
def test_every_input_holds_the_windows_its_name_says(name):
    q, r, found, visible, kw = WM.the_input(name)
    host = WM.hosted(name)
    first, windows, out = host
    listed = [i for i in range(len(q)) if WM.eligible(windows[i])]
    assert len(listed) == WM.INPUTS[name][1]
    per = np.diff(first)
    if listed:
        assert any(per[i] > 0 for i in listed)  # (no test passes on empty answers)
    # the whole list taken: the host form with the two flags swapped for WIDE_DONE, everything else as it is
    wf, ww, wo, total = WM.wide_expected(host, len(q))
    assert total == len(listed)
    for i in range(len(q)):
        if i in listed:
            assert ww["flags"][i] == WM.WIDE_DONE and ww["n_candidates"][i] == windows["n_candidates"][i]
            assert wo[wf[i]:wf[i + 1]].tobytes() == out[first[i]:first[i + 1]].tobytes()
    # nothing taken: the device form as found_model states it
    dev = FM.search_windows_found(q, r, found=found, visible=visible, device=True, **kw) if len(q) < 600 else None
    zf, zw, zo, _ = WM.wide_expected(host, 0)
    if dev is not None:
        assert np.array_equal(zf, dev[0]) and zw.tobytes() == dev[1].tobytes() and zo.tobytes() == dev[2].tobytes()
    assert not (zw["flags"] & WM.WIDE_DONE).any()


def test_the_seams_are_where_the_names_say():
    q, r, found, visible, kw, counts, at = WM.seams_input(0)
    first, windows, out = WM.hosted("seams")
    assert windows["n_gathered"][at].tolist() == counts
    wf, ww, wo, total = WM.wide_expected((first, windows, out), 64)
    by_count = dict(zip(counts, (int(ww["flags"][a]) for a in at)))
    assert by_count[4096] == 0 and by_count[77] == 0 and by_count[32769] == S.WIDE
    assert all(by_count[g] == WM.WIDE_DONE for g in (4097, 8191, 8192, 8193, 32767, 32768))
    a = at[counts.index(32769)]
    assert ww["n_candidates"][a] == 0 and wf[a] == wf[a + 1] and first[a] < first[a + 1]
    # the same_genome floor removes positions: fewer candidates, still intervals
    same = WM.hosted("seams_same_genome")
    assert all(same[1]["n_candidates"][a] < windows["n_candidates"][a] and same[0][a] < same[0][a + 1] for a in at if counts[at.index(a)] > 4096)


def test_the_merge_input_has_every_kind_of_window():
    q, r, found, visible, kw = WM.the_input("merge")
    first, windows, out = WM.hosted("merge")
    starts = [i for i in range(len(q)) if i == 0 or q["loc"][i] - q["loc"][i - 1] > 10 ** 6]
    assert len(starts) == 4
    dup, none, every, plain = starts
    assert (windows["n_gathered"][dup], windows["n_candidates"][dup]) == (8000, 4000) and first[dup + 1] - first[dup] == 109
    assert windows["n_candidates"][none] == 5000 and first[none + 1] == first[none]
    assert windows["n_candidates"][every] == 6000 and first[every + 1] - first[every] == 1
    assert windows["flags"][plain] == 0 and first[plain + 1] > first[plain]


def test_the_found_inputs_cover_and_hide():
    for name, flags0 in (("found_256", 0), ("found_257", FM.FOUND_WIDE), ("found_600_half_hidden", FM.FOUND_WIDE),
                         ("found_600_gather_5000", FM.FOUND_WIDE | S.WIDE)):
        assert WM.hosted(name)[1]["flags"][0] == flags0, name
    # the visible covering records drop positions, the hidden one does not
    q, r, found, visible, kw = WM.the_input("found_600_gather_5000")
    code, first, windows, out, used = ex().search_windows_found_host(q, r, found=found[:0], visible=np.zeros(len(q), np.uint32), **kw)
    with_records = WM.hosted(name)[1]
    assert windows["n_candidates"][0] - with_records["n_candidates"][0] >= 200
    all_seen = ex().search_windows_found_host(q, r, found=found, visible=np.full(len(q), len(found), np.uint32), **kw)[2]
    assert all_seen["n_candidates"][0] < with_records["n_candidates"][0]
    assert visible[0] == 300 and len(found) == 600


def test_a_short_list_takes_the_lowest_windows():
    host = WM.hosted("five")
    listed = [i for i in range(len(host[1])) if WM.eligible(host[1][i])]
    wf, ww, wo, total = WM.wide_expected(host, 2)
    assert total == 5 and [int(ww["flags"][i]) for i in listed] == [WM.WIDE_DONE] * 2 + [S.WIDE] * 3
    assert all(wf[i] == wf[i + 1] for i in listed[2:]) and all(wf[i] < wf[i + 1] for i in listed[:2])


def test_the_drivers_pair_is_wide_for_the_seeding_alone():
    """On the CPU first: a scheduled window is WIDE within the wide kernel's reach, the index threshold drops none of the
    unit's groups, and the pair reports hits."""
    extz2 = ex()
    I = WM.wide_pair()
    P = DM.Pair(extz2, I)
    assert len(P.q) + len(P.r) < 6000
    code, first, windows, out, used = extz2.search_windows_host(P.q, P.r_sorted, **P.wkw)
    assert code == 0
    sched = DM.greedy_schedule(P.q, I["init_len"], 1)
    wide = [i for i in sched if windows["flags"][i] & S.WIDE]
    assert len(wide) >= 3 and all(WM.eligible(windows[i]) for i in wide)
    assert all(4096 < windows["n_gathered"][i] <= WM.WIDE_MAX_GATHER for i in wide)
    # no group of the unit is at or over the threshold: the largest group of the reference is below it
    keys = S.keys_of(P.r_sorted)
    assert np.unique(keys, return_counts=True)[1].max() < P.threshold
    rc, hits, n, stats = extz2.search_pair_host(I["pool"], I["q_range"], I["r_range"], **DM.pair_kwargs(extz2, I))
    assert rc == 0 and n >= 1
