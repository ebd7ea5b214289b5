"""The search filter on the device: uppercase and q-gram verdicts per pair of ranges of the resident pool (sdf_search_filter,
sdf_search_filter_device, sdf_search_filter_tasks_device; sedef_amd/csrc/search_filter.hip).

Expected values: the reference's own answers (tests/golden/search_filter_kat.json.gz), sdf_search_filter_host and
tests/filter_model.py, which tests/test_search_filter_cpu.py checks against that fixture.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch  # (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import filter_model as F  # noqa: E402
import search_model as S  # noqa: E402
from test_search_filter_cpu import case_tasks, host, load_fixture, params_of, roll_arrays, same_as_fixture  # noqa: E402
from test_search_windows_cpu import case_args  # noqa: E402

pytestmark = pytest.mark.gpu

SDF_ERR_UNSUPPORTED, SDF_ERR_INVALID = -3, -4
GUARD = 4  # records of 0xEE behind d_out[n]
WAVE_MAX = 4096  # SDF_FILTER_WAVE_MAX_LEN
BIG = 1 << 20


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def kat():
    return load_fixture()


def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if len(a) else np.zeros(8, np.uint8)).cuda()


def device_form(eng, tasks, P, any_rc=True, stream=None):
    """sdf_search_filter_device on tasks uploaded here: (the records, the bytes behind them)."""
    n = len(tasks)
    d_tasks = up(tasks)
    d_out = torch.full(((n + GUARD) * 20,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the tensors were filled on torch's stream)
    eng.pool_sync()
    eng.search_filter_device(d_tasks.data_ptr(), n, any_rc, d_out.data_ptr(), params_of(P), stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    raw = d_out.cpu().numpy().tobytes()
    return np.frombuffer(raw[:20 * n], F.REC), raw[20 * n:]


def check_both(eng, pool, tasks, P, want=None, stream=None):
    """Both forms against `want` (default: the host form, which must be the model's)."""
    if want is None:
        code, want = host(pool, tasks, P)
        assert code == 0
        assert want.tobytes() == F.filter_pairs(pool, tasks, **P).tobytes()
    code, got = eng.search_filter_raw(tasks, params_of(P))
    assert code == 0, eng.lib.sdf_last_error(eng.ctx).decode()
    assert got.tobytes() == want.tobytes(), [(int(t), tasks[t], got[t], want[t]) for t in np.flatnonzero(got != want)[:5]]
    dev, behind = device_form(eng, tasks, P, stream=stream)
    assert dev.tobytes() == want.tobytes(), [(int(t), tasks[t], dev[t], want[t]) for t in np.flatnonzero(dev != want)[:5]]
    assert behind == b"\xEE" * (20 * GUARD)
    return want


def test_fixture_record_for_record(eng, kat):
    stream = torch.cuda.Stream()
    n = 0
    for c in kat["cases"]:
        pool = c["pool"].encode()
        eng.pool_upload(pool)
        want = check_both(eng, pool, case_tasks(c), c["params"], stream=stream)
        same_as_fixture(want, c, "host form")
        n += len(want)
    assert n >= 1500


@pytest.fixture(scope="module")
def edge_pool():
    """2^20 'A', then 2^17 + 13 mixed characters -- both cases, n, N, other letters, bytes of 128 and more -- with a
    homopolymer and a dinucleotide stretch; the size is no multiple of 8."""
    rng = np.random.default_rng(31)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtacgtNnRx" + bytes([0xC1, 0xE7, 0x8A, 0xFF]), np.uint8)
    tail = alphabet[rng.integers(0, len(alphabet), (1 << 17) + 13)].copy()
    tail[5000:5600] = ord("t")
    tail[9000:9800] = np.frombuffer(b"CA" * 400, np.uint8)
    pool = b"A" * BIG + tail.tobytes()
    assert len(pool) % 8 == 5
    return pool


def test_sizes_where_the_kernel_can_go_wrong(eng, edge_pool):
    pool, base, end = edge_pool, BIG, len(edge_pool)
    eng.pool_upload(pool)
    rows = []
    lengths = [0, 1, 4, 5, 6, 63, 64, 65, 127, 128, 129, 704, 705, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, 4 * 64 * 17, 4 * 64 * 17 + 1]
    for k, n in enumerate(lengths):  # equal sides at every alignment, every strand
        rows.append((base + 16 + k % 8, base + 40000 + (3 * k) % 8, n, n, k % 4))
    for k in range(8):  # unequal sides, one of them empty, off % 8 = 0 .. 7 on both
        rows.append((base + 4096 + k, base + 60000 + 7 - k, 700 + k, 0 if k % 3 == 0 else 650 - 9 * k, (k + 1) % 4))
        rows.append((base + 4990 + k, base + 8990 + k, 640, 830, k % 4))  # the homopolymer and the dinucleotide stretch
    for n in (1, 7, 8, 9, 700, WAVE_MAX + 3):  # ranges that end on the pool's last byte
        rows.append((end - n, end - n - 3, n, n, 3))
        rows.append((end, end - n, 0, n, 0))
    for n in (65535, 65536):  # (where 16-bit counts would end: these run in the long class)
        rows.append((base - 100, base + 11, n, n + 1, 0))
        rows.append((base + 3, base + 40001, n, n, 3))
    rows.append((0, 0, 0, 0, F.SKIP))
    rows.append((0, 1, BIG, BIG - 1, 0))  # one letter: a bin reaches 2^20 - 4
    rows.append((0, base + 5000, BIG, 600, F.Q_RC))  # ... 'T' on the other strand, against the run of 't'
    rows.append((9, 9, 5, 5, F.SKIP | F.Q_RC))
    tasks = np.array([r + (0,) for r in rows], F.TASK)
    strict = check_both(eng, pool, tasks, dict(F.DEFAULTS, min_uppercase=0, max_error=0.1, max_edit_error=0.02))
    assert (strict["flags"] & F.QGRAM_FAIL).any() and not (strict["flags"] & F.UPPER_FAIL).any()
    P = dict(F.DEFAULTS)
    want = check_both(eng, pool, tasks, P)
    big = want[len(rows) - 3]
    assert (int(big["q_up"]), int(big["dist"])) == (BIG, BIG - 5) and int(want[len(rows) - 2]["dist"]) == 596
    assert {0, 1} <= set((want["flags"] & 3).tolist()) and (want["flags"] & F.SHORT).any() and ((want["flags"] & F.SKIPPED) != 0).sum() == 2
    # any_rc == 0: every side is read forward
    dev, _ = device_form(eng, tasks, P, any_rc=False)
    fwd = tasks.copy()
    fwd["flags"] &= F.SKIP
    assert dev.tobytes() == F.filter_pairs(pool, fwd, **P).tobytes()


def test_batches_of_one_homopolymer(eng, edge_pool):
    pool = edge_pool
    eng.pool_upload(pool)
    for n in (1, 65):
        tasks = np.zeros(n, F.TASK)
        tasks["q_off"], tasks["r_off"] = np.arange(n), BIG + 5000 + np.arange(n) % 5
        tasks["q_len"], tasks["r_len"], tasks["flags"] = 700, 590, F.R_RC
        want = check_both(eng, pool, tasks, dict(F.DEFAULTS, min_uppercase=0))
        assert want["dist"].tolist() == [586] * n and (want["flags"] == 0).all()


def test_more_tasks_than_one_launch_takes(eng, edge_pool):
    """2^22 tasks a launch: a batch of 2^22 + 5, all SKIP but those next to the seam and one of the long class behind it."""
    pool = edge_pool
    eng.pool_upload(pool)
    n = (1 << 22) + 5
    tasks = np.zeros(n, F.TASK)
    tasks["flags"] = F.SKIP
    live = [0, (1 << 22) - 1, 1 << 22, n - 2, n - 1]
    tasks[live] = [(BIG + 10 * k, BIG + 3000 + k, 700, 650 + k, k % 4, 0) for k in range(5)]
    tasks[n - 2]["r_len"] = WAVE_MAX + 9
    code, want = host(pool, tasks[live], F.DEFAULTS)
    launches = eng.last_launches()
    code2, got = eng.search_filter_raw(tasks, params_of(F.DEFAULTS))
    assert code == 0 and code2 == 0 and eng.last_launches() == launches + 4
    assert got[live].tobytes() == want.tobytes() == F.filter_pairs(pool, tasks[live], **F.DEFAULTS).tobytes()
    rest = np.ones(n, bool)
    rest[live] = False
    assert (got["flags"][rest] == F.SKIPPED).all() and not got["dist"][rest].any()
    dev, behind = device_form(eng, tasks, F.DEFAULTS)
    assert dev.tobytes() == got.tobytes() and behind == b"\xEE" * (20 * GUARD)


def test_device_form_skips_what_it_may_not_read(eng, edge_pool):
    pool, end = edge_pool, len(edge_pool)
    eng.pool_upload(pool)
    tasks = np.array([(BIG, BIG + 900, 700, 700, 0, 0), (end - 699, 0, 700, 700, 0, 0), (0, end + 1, 10, 0, 0, 0), (-1, 0, 5, 5, 0, 0),
                      (0, 0, -1, 5, 0, 0), (0, 0, 5, 5, 8, 0), (0, 0, 5, 5, 0, 1), (5, (1 << 63) - 1, 5, 5, 0, 0), (0, 0, 5, 2147483647, 0, 0),
                      (end - 700, BIG, 700, WAVE_MAX + 1, 3, 0)], F.TASK)
    good = np.array([True] + [False] * 8 + [True])
    fine = tasks.copy()
    fine[~good] = (0, 0, 0, 0, F.SKIP, 0)
    want = F.filter_pairs(pool, fine, **F.DEFAULTS)
    dev, behind = device_form(eng, tasks, F.DEFAULTS)
    assert dev.tobytes() == want.tobytes() and behind == b"\xEE" * (20 * GUARD)
    assert ((dev["flags"] & F.SKIPPED) != 0).tolist() == (~good).tolist()


def test_chain_on_one_stream_against_the_host_chain(eng, kat):
    """windows -> roll -> tasks -> filter on the caller's stream, no host read in between."""
    from sedef_amd import extz2
    for name in ("roll k12 reversed reference allow_extend 1", "roll k12 0 allow_extend 0"):
        c = next(c for c in kat["cases"] if c["name"] == name)
        rc, (q, windows, first, intervals, r, len_r, init_len, limit), rolls = roll_arrays(c)
        kw = case_args(rc)
        pool = c["pool"].encode()
        eng.pool_upload(pool)
        eng.pool_sync()
        cap = len(intervals) + 50
        d_q, d_rs, d_r, d_limit = up(q), up(S.index_order(r)), up(r), up(limit)
        d_first = torch.zeros(len(q) + 1, dtype=torch.int64, device="cuda")
        d_win = torch.zeros(len(q) * 20, dtype=torch.uint8, device="cuda")
        d_iv = torch.zeros(cap * 8, dtype=torch.uint8, device="cuda")
        d_rolls = torch.zeros(cap * 24, dtype=torch.uint8, device="cuda")
        d_tasks = torch.full(((cap + GUARD) * 32,), 0xEE, dtype=torch.uint8, device="cuda")
        d_out = torch.full(((cap + GUARD) * 20,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        st = stream.cuda_stream
        eng.search_windows_device(d_q.data_ptr(), len(q), kw["len_q"], d_rs.data_ptr(), len(r), kw["r_threshold"], init_len, kw["same_genome"],
                                  kw["uppercase_seeds"], d_limit.data_ptr(), len(limit), d_first.data_ptr(), d_win.data_ptr(), d_iv.data_ptr(),
                                  cap, stream=st)
        eng.search_roll_device(d_q.data_ptr(), len(q), d_win.data_ptr(), d_first.data_ptr(), d_iv.data_ptr(), cap, d_r.data_ptr(), len(r), len_r,
                               init_len, d_limit.data_ptr(), len(limit), d_rolls.data_ptr(), stream=st)
        eng.search_filter_tasks_device(d_q.data_ptr(), len(q), d_win.data_ptr(), d_first.data_ptr(), d_iv.data_ptr(), d_rolls.data_ptr(), cap,
                                       len(rc["q"]), len_r, init_len, c["q_off"], 0, c["r_off"], rc["r_rc"], c["allow_extend"],
                                       d_tasks.data_ptr(), stream=st)
        eng.search_filter_device(d_tasks.data_ptr(), cap, True, d_out.data_ptr(), params_of(c["params"]), stream=st)
        stream.synchronize()
        n = len(intervals)
        assert n > 100 and int(d_first.cpu()[-1]) == n
        # the host chain: sdf_search_filter_tasks_host on the fixture's rolls, then sdf_search_filter_host
        code, tasks = extz2.search_filter_tasks_host(q, windows, first, intervals, rolls, len(rc["q"]), len_r, init_len, c["q_off"], 0, c["r_off"],
                                                     rc["r_rc"], c["allow_extend"])
        assert code == 0 and tasks.tobytes() == case_tasks(c).tobytes()
        skip = np.zeros(cap - n, F.TASK)
        skip["flags"] = F.SKIP
        raw = d_tasks.cpu().numpy().tobytes()
        assert raw[:32 * cap] == tasks.tobytes() + skip.tobytes() and raw[32 * cap:] == b"\xEE" * (32 * GUARD)
        code, want = host(pool, np.concatenate([tasks, skip]), c["params"])
        raw = d_out.cpu().numpy().tobytes()
        assert code == 0 and raw[:20 * cap] == want.tobytes() and raw[20 * cap:] == b"\xEE" * (20 * GUARD)
        same_as_fixture(want[:n], c, "chain")
        # the convenience form, which reads back between the steps
        got = eng.search_filter((c["q_off"], len(rc["q"])), (c["r_off"], len(rc["r"]), bool(rc["r_rc"])), rc["k"], rc["w"], rc["sl"], init_len,
                                rc["same_genome"], rc["uppercase_seeds"], rc["limit"], r_threshold=rc["threshold"],
                                params=params_of(c["params"]), allow_extend=c["allow_extend"])
        assert got[3].tobytes() == rolls.tobytes() and got[4].tobytes() == want[:n].tobytes()


def test_on_a_view_of_another_context(eng, kat):
    import sedef_amd
    c = kat["cases"][0]
    pool = c["pool"].encode()
    eng.pool_upload(pool)
    view = sedef_amd.Extz2Engine(0)
    try:
        assert view.pool_share(eng) == len(pool)
        want = check_both(view, pool, case_tasks(c), c["params"])
        same_as_fixture(want, c, "view")
    finally:
        view.close()


def test_refusals_launch_nothing(eng, edge_pool):
    from sedef_amd import extz2
    pool, end = edge_pool, len(edge_pool)
    eng.pool_upload(pool)
    good = np.array([(BIG, BIG + 800, 700, 700, 0, 0), (BIG + 3, BIG + 9, 0, 5000, 3, 0)], F.TASK)
    launches = eng.last_launches()

    def refused(tasks, P=F.DEFAULTS):
        out = np.full(len(tasks) * 20, 0x55, np.uint8).view(F.REC)
        code, _ = eng.search_filter_raw(tasks, params_of(P), out=out)
        assert out.tobytes() == b"\x55" * (20 * len(tasks)) and eng.last_launches() == launches
        return code

    def with_(**kw):
        t = good.copy()
        for k, v in kw.items():
            t[k][1] = v
        return t
    assert refused(with_(r_off=end - 4999)) == SDF_ERR_INVALID and b"outside the resident pool" in eng.lib.sdf_last_error(eng.ctx)
    assert refused(with_(q_off=end + 1)) == SDF_ERR_INVALID
    assert refused(with_(q_off=-1)) == SDF_ERR_INVALID
    assert refused(with_(r_len=-1)) == SDF_ERR_INVALID
    assert refused(with_(flags=8)) == SDF_ERR_UNSUPPORTED
    assert refused(with_(reserved=7)) == SDF_ERR_UNSUPPORTED
    assert refused(good, dict(F.DEFAULTS, max_error=float("nan"))) == SDF_ERR_INVALID
    assert refused(good, dict(F.DEFAULTS, gap_frequency=float("inf"))) == SDF_ERR_INVALID
    assert refused(good, dict(F.DEFAULTS, reserved=2)) == SDF_ERR_UNSUPPORTED
    lib, P = eng.lib, extz2.filter_params()
    assert lib.sdf_search_filter(eng.ctx, None, good.ctypes.data, 2, good.ctypes.data) == SDF_ERR_INVALID
    assert lib.sdf_search_filter(eng.ctx, P, None, 2, good.ctypes.data) == SDF_ERR_INVALID
    assert lib.sdf_search_filter(eng.ctx, P, good.ctypes.data, 2, None) == SDF_ERR_INVALID
    assert lib.sdf_search_filter(eng.ctx, None, None, 0, None) == 0  # n == 0
    assert lib.sdf_search_filter_device(eng.ctx, P, None, 0, 1, None, None) == 0
    assert lib.sdf_search_filter_device(eng.ctx, P, None, 3, 1, 8, None) == SDF_ERR_INVALID
    assert lib.sdf_search_filter_device(eng.ctx, extz2.filter_params(max_edit_error=float("nan")), 8, 3, 1, 8, None) == SDF_ERR_INVALID
    tf = lib.sdf_search_filter_tasks_device
    assert tf(eng.ctx, None, 0, None, None, None, None, 7, 100, 100, 10, 0, 0, 0, 0, 1, None, None) == 0  # nq == 0
    assert tf(eng.ctx, 8, 5, 8, 8, 8, 8, 0, 100, 100, 10, 0, 0, 0, 0, 1, None, None) == 0  # n_max == 0
    assert tf(eng.ctx, 8, 5, 8, 8, 8, None, 7, 100, 100, 10, 0, 0, 0, 0, 1, 8, None) == SDF_ERR_INVALID
    assert tf(eng.ctx, 8, 5, 8, 8, 8, 8, 7, 100, 100, 0, 0, 0, 0, 0, 1, 8, None) == SDF_ERR_INVALID  # init_len
    assert tf(eng.ctx, 8, 5, 8, 8, 8, 8, 7, 100, -1, 10, 0, 0, 0, 0, 1, 8, None) == SDF_ERR_INVALID
    assert eng.last_launches() == launches
    # ... one launch for the wavefront class alone, two with a long task, two from the device form
    assert eng.search_filter_raw(good[:1])[0] == 0 and eng.last_launches() == launches + 1
    assert eng.search_filter_raw(good)[0] == 0 and eng.last_launches() == launches + 3
    device_form(eng, good, F.DEFAULTS)
    assert eng.last_launches() == launches + 5
