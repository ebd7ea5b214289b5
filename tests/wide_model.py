"""What sdf_search_windows_wide_device must write, stated in Python on top of the host form's answer, and the inputs of
tests/test_gpu_search_wide.py and tests/test_gpu_search_wide_driver.py (tests/test_search_wide_cpu.py shows on the CPU that
each input holds what its name says).

wide_expected takes what search_windows_found_host returns -- every window complete, WIDE and FOUND_WIDE kept -- and applies
  eligibility     WIDE and/or FOUND_WIDE, no NOLIMIT, n_members <= MAX_MEMBERS, n_gathered <= WIDE_MAX_GATHER;
  lowest first    the lowest n_wide_max eligible indices are taken;
  flag rewrite    a taken window keeps its counts and intervals, WIDE and FOUND_WIDE are cleared, WIDE_DONE is set;
  the device rule (found_model.search_windows_found(device=True)) for every other WIDE / FOUND_WIDE window: n_candidates 0, no
                  interval."""
import numpy as np

import driver_model as DM
import found_model as FM
import search_model as S
from test_search_found_cpu import kwargs, wide_case
from test_search_windows_cpu import wide_arrays

WIDE_DONE, WIDE_MAX_GATHER = 0x10, 32768


def eligible(W):
    return bool(W["flags"] & (S.WIDE | FM.FOUND_WIDE)) and not W["flags"] & S.NOLIMIT and W["n_members"] <= S.MAX_MEMBERS and \
        W["n_gathered"] <= WIDE_MAX_GATHER


def wide_expected(host_records, n_wide_max):
    """(first, windows, intervals, the number of eligible windows) as sdf_search_windows_wide_device writes them."""
    first, windows, intervals = host_records
    windows = windows.copy()
    listed = [i for i in range(len(windows)) if eligible(windows[i])]
    taken = set(listed[:n_wide_max])
    out, new_first = [], [0]
    for i in range(len(windows)):
        mine = intervals[int(first[i]):int(first[i + 1])]
        if i in taken:
            windows["flags"][i] = (int(windows["flags"][i]) & ~(S.WIDE | FM.FOUND_WIDE)) | WIDE_DONE
        elif windows["flags"][i] & (S.WIDE | FM.FOUND_WIDE):
            windows["n_candidates"][i] = 0
            mine = mine[:0]
        out.append(mine)
        new_first.append(new_first[-1] + len(mine))
    T = np.concatenate(out) if out else intervals[:0]
    return np.array(new_first, np.int64), windows, T.astype(S.INTERVAL), len(listed)


# ---- the inputs: name -> (q, r_sorted, found, visible, arguments, the eligible windows) ----

def block(q_rows, r_rows, b, apart=20_000_000):
    """Rows (hash, loc, status) of one block of minimizers, moved to block b's hashes and place."""
    return ([(h + 1000 * b, loc + apart * b, st) for h, loc, st in q_rows], [(h + 1000 * b, loc + apart * b, st) for h, loc, st in r_rows])


def seams_input(same_genome):
    """Windows of every gathered count at which the two kernels change hands, between ordinary ones (blocks_of of
    tests/test_gpu_search_windows.py: one block per count, the block's first window gathers it)."""
    from test_gpu_search_windows import blocks_of
    counts = [77, 4096, 300, 4097, 8191, 77, 8192, 8193, 300, 32767, 32768, 32769]
    q, r, at = blocks_of(counts)
    return q, r, None, None, kwargs(init_len=1000, limit=[1] + [3] * 60, same_genome=same_genome), counts, at


def merge_input():
    """Block 0: two members with one key, so that every gathered position comes twice (8,000 gathered, 4,000 distinct), in runs
    of 37 positions with gaps wider than init_len: a head per run, in every wavefront and round of the merge.  Block 1: 5,000
    positions 2,000 apart: none passes the merge.  Block 2: 6,000 positions three apart: every one passes, one interval.
    Block 3: an ordinary window."""
    runs = [3108 * (t // 37) + 3 * (t % 37) + 5000 for t in range(4000)]
    blocks = [([(100, 0, 0), (100, 5, 0)], [(100, p, 0) for p in runs]),
              ([(100, 0, 0)], [(100, 2000 * t + 5000, 0) for t in range(5000)]),
              ([(100, 0, 0)], [(100, 3 * t + 5000, 0) for t in range(6000)]),
              ([(100 + j, 5 * j, 0) for j in range(40)], [(100 + j, 7 * j + 5000 + 100 * (j % 3), 0) for j in range(40)] + [(100, 9000, 0)] * 37)]
    q_rows, r_rows = [], []
    for b, (qr, rr) in enumerate(blocks):
        a, c = block(qr, rr, b)
        q_rows += a
        r_rows += c
    return S.records(q_rows), S.index_order(S.records(r_rows)), None, None, kwargs(init_len=1000, limit=[1] + [2] * 60)


def members_input():
    """1,025 members in a window (tests/test_gpu_search_windows.py's member seam): WIDE by the count the wide kernel does not raise."""
    q = S.records([(7 + (j % 3), j, j % 2) for j in range(1200)])
    r = S.index_order(S.records([(7, 50, 0), (8, 60, 0), (7, 90, 0), (9, 2000, 1), (9, 2001, 0)]))
    return q, r, None, None, kwargs(len_q=5000, init_len=1024, uppercase_seeds=0, limit=[1, 1, 1, 1, 1, 1, 2])


def found_input(n, hide_half):
    """wide_case(n) of tests/test_search_found_cpu.py: n records meet window 0, the first of them covers a gathered position;
    hide_half: every window sees the first half of the list alone."""
    q, r, found, visible, kw = wide_case(n)
    if hide_half:
        visible = np.full(len(q), len(found) // 2, np.uint32)
    return q, r, found, visible, kw


def found_gather_input():
    """FOUND_WIDE and WIDE at once: 5,000 gathered positions (wide_arrays) and 600 records that meet window 0, the later half
    hidden.  Records 0 and 270 (the second chunk of 256) cover positions of the member at loc 0 and of the one at loc 5;
    record 400 would cover more, and is hidden."""
    q, r = wide_arrays(5000)
    rows = [(t % 900, t % 900 + 1, 10 ** 6, 10 ** 6 + 5) for t in range(600)]
    rows[0] = (0, 1, 300, 900)        # the big group's positions 300, 303 .. 897, for the member at loc 0 alone
    rows[270] = (5, 6, 0, 100)        # the member at loc 5 has one position, 8
    rows[400] = (0, 1, 3000, 9000)
    found = FM.found_records(rows)
    visible = np.full(len(q), 300, np.uint32)
    return q, r, found, visible, kwargs(init_len=1000, limit=[1] + [3] * 60)


def five_input():
    from test_gpu_search_windows import blocks_of
    q, r, at = blocks_of([5000, 77, 6000, 4100, 300, 7000, 4500])
    return q, r, None, None, kwargs(init_len=1000, limit=[1] + [3] * 60)


INPUTS = {  # name -> (builder, eligible windows)
    "seams": (lambda: seams_input(0)[:5], 6),
    "seams_same_genome": (lambda: seams_input(1)[:5], 6),
    "merge": (merge_input, 3),
    "members": (members_input, 0),
    "found_256": (lambda: found_input(256, False), 0),
    "found_257": (lambda: found_input(257, False), 1),
    "found_600_half_hidden": (lambda: found_input(600, True), 1),
    "found_600_gather_5000": (found_gather_input, 9),  # (window 0, and the eight behind it that 256 < 300 - loc records still meet)
    "five": (five_input, 5),
}
_built, _hosted = {}, {}


def the_input(name):
    """(q, r_sorted, found, visible, arguments): found and visible an empty list and zeros where the input has none."""
    if name not in _built:
        q, r, found, visible, kw = INPUTS[name][0]()
        if found is None:
            found, visible = FM.found_records([]), np.zeros(len(q), np.uint32)
        _built[name] = (q, r, found, visible, kw)
    return _built[name]


def hosted(name):
    """sdf_search_windows_found_host's answer for an input, computed once: (first, windows, intervals)."""
    if name not in _hosted:
        from sedef_amd import extz2
        q, r, found, visible, kw = the_input(name)
        code, first, windows, out, used = extz2.search_windows_found_host(q, r, found=found, visible=visible, **kw)
        assert code == 0 and used == int(first[-1]) == len(out)
        _hosted[name] = (first.astype(np.int64), windows, out)
    return _hosted[name]


# ---- the driver's pair ----

def wide_pair(r_copies=100, q_copies=12, seed=11):
    """A unit of 100 bases about 100 times in the reference, a dozen copies between unique flanks in the query, a few point
    changes a copy: at k = 8, w = 4 a window of 400 bases inside the array has some 65 members whose groups hold up to a hundred
    positions each -- 5,000 gathered and more."""
    return DM.arrays_input(seed, 100, q_copies, r_copies, 0.01, 400, flank=400)
