"""GPU: the two contracts that sit around the DP kernels in every batch call.

1. Tasks the reference returns from before doing any work (extern/ksw2_extz2_sse.cc:57: a side without a base; :81: a
   scoring with -min_sc > 2 (q + e)).  The planner drops them (sdf_batch.h: task_runs) and reset_results_kernel alone writes
   their records: a record left over from an earlier call, or from the caller's own buffer, must never come back.
2. SDF_ERR_CIGAR_OVERFLOW (include/sedef_hip.h): a CIGAR pool that is too small makes the call return the need in
   *cigar_used, writes nothing at or behind cigar_pool[cigar_cap], and leaves the context usable -- with a second part, early
   chunks, the claim counters and the give-up list in flight at that moment.

One seeded batch of ~520 tasks serves every test: lane-sized full-band tasks, same-geometry banded tasks (pairs, a mixed
pair), full-band tasks for the stripe / strip kernels, score-only tasks, ~2 % N, and a tenth of the indices EMPTY tasks --
at index 0, at index n - 1, five in a row, between the two members of a pair.  Every expectation is the oracle's, computed
once per module (oracle/extz2_oracle.c has the reference's early return; tests/test_oracle_vs_ref.py pins that to the
reference kernel).

What decides the route of a task depends on the SIZE of the batch (sdf_plan.hip: the lane kernel from 8,192 eligible tasks,
a pipeline of chunks from 2,048 tasks, the two-part start from two cut blocks of 4,096, the early start of the heavy chunks
where the cut is scanned on several threads).  So the batch also runs TILED: twenty copies of its task array over the same
pool, 10,440 tasks whose expected records are the copies of the 522 -- no more work for the oracle, a few milliseconds on
the device -- and the lane kernel is also asked for on the small batch through SDF_LANE_MIN."""
import numpy as np
import pytest
import torch  # (at collection, like the modules that import bench: before the library brings a HIP runtime of its own along)

from oracle.binding import NEG_INF, mutate, random_codes, sedef_mat

pytestmark = pytest.mark.gpu

WANT_CIGAR, WANT_SCORE, WANT_ALL = 1, 2, 7
WANT_FAST = WANT_CIGAR | WANT_SCORE  # (the register-resident kernels: lane, pair, wave, stripe, strip)
OVERFLOW = -5                        # SDF_ERR_CIGAR_OVERFLOW
SCORE_ONLY = 0x01                    # SDF_FLAG_SCORE_ONLY
FILL = 0xA5                          # every byte of the caller's records before a call
SENTINEL = 0xC1A0C1A0                # every word of the caller's CIGAR pool before a call
GUARD = 64                           # words behind cigar_cap that no call may touch
TILES = 20
DEGENERATE = dict(mat=sedef_mat(1, -20), gapo=4, gape=2)  # 20 > 2 (4 + 2): extern/ksw2_extz2_sse.cc:81

KSW_FIELDS = ("score", "max", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "zdropped")
COUNTERS = ("matches", "mismatches", "gaps", "gap_bases")
# what a call without SDF_WANT_EXT promises of a task that ran (include/sedef_hip.h: SDF_WANT_SCORE, SDF_WANT_CIGAR)
FAST_FIELDS = ("score", "mte", "mte_q", "zdropped", "n_cigar") + COUNTERS
ALL_FIELDS = KSW_FIELDS + ("n_cigar",) + COUNTERS

# Settings on top of the library's defaults (names as tests/test_gpu_extz2.py gives them: through sdf_config, never the
# environment).  (tiled): the setting changes something only for the tiled form of the batch.
SETTINGS = {
    "default": {},
    "lane": dict(SDF_LANE_MIN=64),                                    # the lane kernel on the small batch: counting sort ...
    "lane_sort": dict(SDF_LANE_MIN=64, SDF_LANE_PLAN=1),             # ... and the radix sort + scans
    "no_lane": dict(SDF_LANE_MIN=64, SDF_NO_LANE=1),
    "force_general": dict(SDF_FORCE_GENERAL=1),
    "strip_always": dict(SDF_STRIP_ALWAYS=1),                        # strips and chained strips whatever the count
    "split_min": dict(SDF_SPLIT_MIN=64),                             # two parts (tiled: 4,096 + 6,344 tasks)
    "early_heavy": dict(SDF_PLAN_POOL_FROM=0, SDF_SCAN_POOL_FROM=0),  # the cut in two passes: heavy chunks start early (tiled)
    "early_heavy_off": dict(SDF_PLAN_POOL_FROM=0, SDF_SCAN_POOL_FROM=0, SDF_EARLY_HEAVY=0),
    "pipeline_off": dict(SDF_PIPELINE=0),
    "cut_chunks": dict(SDF_CUT_NCH=5),
}


# ---- the batches ------------------------------------------------------------------------------------------------------------
class Batch:
    """tasks: byte offsets into `pool` (codes 0..4) -- and into `chars`, the same sequences as FASTA characters."""

    def __init__(self, tasks, pool):
        self.tasks, self.pool = tasks, pool
        self.chars = np.frombuffer(b"ACGTN", np.uint8)[pool].tobytes()
        self.n = len(tasks)
        self.empty = (tasks["qlen"] == 0) | (tasks["tlen"] == 0)
        self.exp = {}

    def seqs(self, k):
        t = self.tasks[k]
        return (self.pool[int(t["q_off"]):int(t["q_off"]) + int(t["qlen"])],
                self.pool[int(t["t_off"]):int(t["t_off"]) + int(t["tlen"])])

    def expect(self, oracle, **scoring):
        """(records, CIGAR words) of the whole batch as the oracle gives them, CIGARs back to back in task order."""
        from sedef_amd import RESULT_DTYPE
        key = tuple(sorted((k, np.asarray(v).tobytes()) for k, v in scoring.items()))
        if key not in self.exp:
            rec, cigs, off = np.zeros(self.n, RESULT_DTYPE), [], 0
            for k in range(self.n):
                q, t = self.seqs(k)
                tk = self.tasks[k]
                e = oracle.extz2(q, t, w=int(tk["w"]), zdrop=int(tk["zdrop"]), flag=int(tk["flag"]), **scoring)
                for f in KSW_FIELDS:
                    rec[f][k] = e[f]
                rec["n_cigar"][k], rec["cigar_off"][k] = len(e["cigar"]), off
                for f, v in oracle.counts(e["cigar"], q, t).items():
                    rec[f][k] = v
                cigs.append(e["cigar"])
                off += len(e["cigar"])
            rec.setflags(write=False)
            cig = np.concatenate(cigs).astype(np.uint32)
            cig.setflags(write=False)
            self.exp[key] = (rec, cig)
        return self.exp[key]

    def tiled(self, oracle, times=TILES):
        """`times` copies of the task array over the same pool, and what the oracle expects of them."""
        rec, cig = self.expect(oracle)
        b = Batch(np.tile(self.tasks, times), self.pool)
        trec = np.tile(rec, times)
        trec["cigar_off"] += np.repeat(np.arange(times, dtype=np.int64) * len(cig), self.n)
        b.exp[()] = (trec, np.tile(cig, times))
        return b


def _mixture(seed):
    """The shared batch (see the module's text).  Real tasks first, then the empty ones go to chosen and random places."""
    from sedef_amd import TASK_DTYPE
    rng = np.random.default_rng(seed)
    real = []  # (query, target, w, flag)

    def same_geometry(ql, tl, w, count):
        for _ in range(count):
            q = random_codes(rng, ql, 0.02)
            t = mutate(rng, q, 0.04, 0.0, 0.0)
            t = np.concatenate([t, random_codes(rng, max(tl - ql, 0))])[:tl]
            real.append((q, t, w, 0))

    for _ in range(450):  # lane-sized, full band
        q = random_codes(rng, int(rng.integers(1, 61)), 0.02)
        t = mutate(rng, q)[:60] if rng.random() < 0.8 else random_codes(rng, int(rng.integers(1, 61)), 0.02)
        real.append((q, t, -1, 0))
    pair_at = len(real)  # (the first two of these are the pair an empty task is put between)
    same_geometry(500, 500, 64, 4)
    same_geometry(480, 510, 64, 4)
    for tl in (300, 350, 401, 450, 512, 520):  # full band: window kernels below SDF_STRIPE_MIN, stripes / strips above
        q = random_codes(rng, tl - int(rng.integers(0, 30)), 0.02)
        real.append((q, np.resize(mutate(rng, q), tl).astype(np.uint8), -1, 0))
    same_geometry(1100, 1100, -1, 2)  # stripes / chained strips, and the heavy tasks of the tiled form
    for _ in range(4):
        q = random_codes(rng, int(rng.integers(20, 200)), 0.02)
        real.append((q, mutate(rng, q), -1, SCORE_ONLY))
    # a random order, except that the pair stays two neighbours
    order = [k for k in rng.permutation(len(real)).tolist() if k not in (pair_at, pair_at + 1)]
    while order.count(None) + 8 < (len(order) + 10) // 10:  # (None: an empty task) anywhere, a tenth of the batch in all
        order.insert(int(rng.integers(1, len(order))), None)
    at = int(rng.integers(100, len(order) - 50))
    order[at:at] = [pair_at, None, pair_at + 1]  # directly between the pair's members
    run_at = int(rng.integers(5, at - 10))
    order[run_at:run_at] = [None] * 5           # five empty neighbours
    order = [None] + order + [None]             # index 0 and index n - 1
    run_at += 1
    pair_slot = order.index(pair_at)
    assert order[pair_slot + 1] is None and order[pair_slot + 2] == pair_at + 1

    chunks, off, tasks = [], 0, np.zeros(len(order), TASK_DTYPE)
    for k, r in enumerate(order):
        if r is None:
            continue
        q, t, w, flag = real[r]
        tasks[k] = (off, off + len(q), len(q), len(t), w, -1, flag, 0)
        chunks += [q, t]
        off += len(q) + len(t)
    pool = np.concatenate(chunks)
    kinds = 0
    for k, r in enumerate(order):
        if r is not None:
            continue
        # no base on one side or on both; the other side a valid range; offsets anywhere in the pool, its end included;
        # any band, z-drop and KSW_EZ_* flags -- nothing of it is ever read
        kind = kinds % 3
        kinds += 1
        ql = 0 if kind != 1 else int(rng.integers(1, 700))
        tl = 0 if kind != 0 else int(rng.integers(1, 700))
        q_off = len(pool) if rng.random() < 0.3 and ql == 0 else int(rng.integers(0, len(pool) - ql + 1))
        t_off = len(pool) if rng.random() < 0.3 and tl == 0 else int(rng.integers(0, len(pool) - tl + 1))
        tasks[k] = (q_off, t_off, ql, tl, int(rng.choice([-1, 0, 1, 64, 5000])), int(rng.choice([-1, 0, 100])),
                    int(rng.choice([0, 0x01, 0x02, 0x04, 0x08, 0x18, 0x40, 0x80, 0xff])), 0)
    tasks.setflags(write=False)
    pool.setflags(write=False)
    b = Batch(tasks, pool)
    b.pair_slot = pair_slot
    assert b.empty[0] and b.empty[-1] and b.empty[run_at:run_at + 5].all() and 0.09 < b.empty.mean() < 0.13
    assert (tasks["q_off"][b.empty] == len(pool)).any() and (tasks["t_off"][b.empty] == len(pool)).any()
    return b


@pytest.fixture(scope="module")
def mix(oracle):
    b = _mixture(20251)
    b.expect(oracle)
    return b


@pytest.fixture(scope="module")
def other(oracle):
    """Another draw of the same mixture: what a context runs after a call that failed."""
    b = _mixture(20252)
    b.expect(oracle)
    return b


@pytest.fixture(scope="module")
def mix_tiled(mix, oracle):
    return mix.tiled(oracle)


@pytest.fixture(scope="module")
def other_tiled(other, oracle):
    return other.tiled(oracle)


@pytest.fixture(scope="module")
def engine():
    import sedef_amd
    eng = sedef_amd.Extz2Engine(0)
    yield eng
    eng.close()


def _engine(name):
    import sedef_amd
    return sedef_amd.Extz2Engine(0, config=SETTINGS[name])


# ---- the checks -------------------------------------------------------------------------------------------------------------
def _reset_record():
    from sedef_amd import RESULT_DTYPE
    r = np.zeros(1, RESULT_DTYPE)
    r["score"] = r["mqe"] = r["mte"] = NEG_INF
    r["max_q"] = r["max_t"] = r["mqe_t"] = r["mte_q"] = -1
    return r[0]


def _check_records(batch, exp, got, cig, used, want, what):
    """`got` (sdf_result or sdf_result_brief records) and the CIGAR words against the oracle's."""
    rec, ecig = exp
    assert used == len(ecig), what
    assert len(got) == batch.n
    brief = "score" not in got.dtype.names
    ran = rec["n_cigar"] > 0
    # the CIGARs of the tasks that have one: ascending, back to back in task order -- an empty task shifts nothing
    assert np.array_equal(got["n_cigar"], rec["n_cigar"]), what
    assert np.array_equal(got["cigar_off"][ran], rec["cigar_off"][ran]), what
    assert np.array_equal(np.asarray(cig[:used], np.uint32), ecig), what
    if brief:
        assert np.array_equal(got["matches"], rec["matches"]), what
        return
    for f in (ALL_FIELDS if want & 4 else FAST_FIELDS):
        bad = np.flatnonzero(got[f] != rec[f])
        assert len(bad) == 0, (what, f, bad[:8].tolist(), got[f][bad[:8]].tolist(), rec[f][bad[:8]].tolist())
    # a task that never ran: the reset record, every field of it, whatever was asked for
    reset = _reset_record()
    for f in ALL_FIELDS:
        assert (got[f][batch.empty] == reset[f]).all(), (what, f)


def _guard_intact(cig, cap):
    return len(cig) == cap + GUARD and (np.asarray(cig[cap:], np.uint32) == SENTINEL).all()


def _host_call(eng, form, batch, cap, want=WANT_FAST, **kw):
    """One host-form call on caller's buffers full of FILL / SENTINEL.  -> (rc, used, records, pool words + guard, error)"""
    return eng.batch_call(form, batch.tasks, batch.pool, want=want, cigar_cap=cap, guard=GUARD, sentinel=SENTINEL, fill=FILL, **kw)


class DeviceBatch:
    """The batch as sdf_extz2_batch_device takes it: sequences packed (sdf_pack_codes) in HBM, word offsets."""

    def __init__(self, batch):
        import sedef_amd
        words, off, tasks = [], 0, batch.tasks.copy()
        cache = {}
        for k in range(batch.n):
            for side, ln in (("q_off", "qlen"), ("t_off", "tlen")):
                key = (int(tasks[side][k]), int(tasks[ln][k]))
                if key[1] and key not in cache:  # (the tiled form names every range twenty times)
                    cache[key] = off
                    w = sedef_amd.pack_codes(batch.pool[key[0]:key[0] + key[1]])
                    words.append(w)
                    off += len(w)
                tasks[side][k] = cache.get(key, off)  # (no base: no word -- the offset may be the pool's end)
        self.tasks, self.n = tasks, batch.n
        self.dev = torch.device("cuda", 0)
        self.d_pool = torch.from_numpy(np.concatenate(words).view(np.int32)).to(self.dev)

    def call(self, eng, cap, want=WANT_FAST, null_cigar=False, **kw):
        """-> (rc, used, records, pool words + guard, error); d_out starts as FILL bytes, d_cig as SENTINEL words."""
        from sedef_amd import RESULT_DTYPE
        d_out = torch.full((self.n * 16,), int(np.array([FILL] * 4, np.uint8).view(np.int32)[0]), dtype=torch.int32, device=self.dev)
        d_cig = torch.full((cap + GUARD,), int(np.array([SENTINEL], np.uint32).view(np.int32)[0]), dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize()
        rc, used, err = eng.align_batch_device(self.tasks, self.d_pool.data_ptr(), d_out.data_ptr(),
                                               None if null_cigar else d_cig.data_ptr(), cap, want=want, check=False, **kw)
        torch.cuda.synchronize()
        return rc, used, d_out.cpu().numpy().view(RESULT_DTYPE), d_cig.cpu().numpy().view(np.uint32), err


def _roomy(batch):
    return int((batch.tasks["qlen"].astype(np.int64) + batch.tasks["tlen"] + 2).sum()) + 1


def _run_ok(eng, form, batch, exp, want=WANT_FAST, what=None, **kw):
    """A call with room to spare: SDF_OK, the oracle's records and words, the guard behind the pool untouched."""
    cap = _roomy(batch)
    rc, used, got, cig, err = _host_call(eng, form, batch, cap, want, **kw)
    assert rc == 0, (what or form, err)
    assert _guard_intact(cig, cap)
    _check_records(batch, exp, got, cig, used, want if form in ("batch", "pairs_full") else WANT_FAST, what or form)
    assert eng.last_reran() == 0 and eng.last_launches() >= 0
    return got, cig[:used]


# ---- 1. skipped tasks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,want", [("batch", WANT_ALL), ("batch", WANT_FAST), ("brief", WANT_FAST), ("pairs", WANT_FAST),
                                       ("pairs_full", WANT_ALL), ("pairs_full", WANT_FAST)])
def test_empty_tasks_host_forms(engine, oracle, mix, form, want):
    """Every host form on caller's records full of 0xA5: the oracle's fields and CIGARs, reset records for the empty tasks."""
    if form.startswith("pairs"):
        engine.pool_upload(mix.chars)
    _run_ok(engine, form, mix, mix.expect(oracle), want)


def test_empty_tasks_pairs_view(engine, oracle, mix):
    """sdf_extz2_batch_pairs_view: the records and words in the context's staging."""
    engine.pool_upload(mix.chars)
    got, cig = engine.align_batch_pairs(mix.tasks, view=True)
    _check_records(mix, mix.expect(oracle), got, cig, len(cig), WANT_FAST, "pairs_view")
    assert engine.last_reran() == 0


@pytest.mark.parametrize("want", [WANT_ALL, WANT_FAST])
def test_empty_tasks_device_form(engine, oracle, mix, want):
    """sdf_extz2_batch_device on a d_out of 0xA5 bytes and a d_cig of sentinel words: the empty tasks' records come back reset."""
    dev = DeviceBatch(mix)
    cap = _roomy(mix)
    rc, used, got, cig, err = dev.call(engine, cap, want)
    assert rc == 0, err
    _check_records(mix, mix.expect(oracle), got, cig, used, want, "device")
    assert _guard_intact(cig, cap) and (cig[used:] == SENTINEL).all()
    assert engine.last_reran() == 0


@pytest.fixture(scope="module")
def default_bytes(engine, oracle, mix, mix_tiled):
    """The default context's records and words for the batch and its tiled form, checked against the oracle."""
    out = {}
    for name, b in (("small", mix), ("tiled", mix_tiled)):
        got, cig = _run_ok(engine, "batch", b, b.expect(oracle), WANT_ALL, "default, every field, " + name)
        out[name, WANT_ALL] = (got.tobytes(), cig.tobytes())
        got, cig = _run_ok(engine, "batch", b, b.expect(oracle), WANT_FAST, "default " + name)
        out[name, WANT_FAST] = (got.tobytes(), cig.tobytes())
    assert engine.last_lane_tasks() > 8192  # (the tiled form's small tasks are the lane kernel's by default)
    return out


@pytest.mark.parametrize("name", [s for s in SETTINGS if s != "default"])
def test_empty_tasks_under_every_start_path(oracle, mix, mix_tiled, default_bytes, name):
    """sdf_extz2_batch under each setting, on the batch and on its tiled form: the oracle's results, and byte for byte the
    default context's (force_general: with every field asked for on both sides, see below)."""
    eng = _engine(name)
    for size, b in (("small", mix), ("tiled", mix_tiled)):
        got, cig = _run_ok(eng, "batch", b, b.expect(oracle), WANT_FAST, "%s %s" % (name, size))
        lanes = eng.last_lane_tasks()
        # (the general kernel computes max, max_q, max_t, mqe, mqe_t whether SDF_WANT_EXT asks for them or not, the
        # register-resident kernels leave them reset: bytes are compared where every field is asked for)
        want = WANT_ALL if name == "force_general" else WANT_FAST
        if want != WANT_FAST:
            got, cig = _run_ok(eng, "batch", b, b.expect(oracle), want, "%s %s, every field" % (name, size))
        assert (got.tobytes(), cig.tobytes()) == default_bytes[size, want], (name, size)
        if name in ("lane", "lane_sort"):
            assert lanes > 400
        elif name in ("no_lane", "force_general") or (name == "pipeline_off") or (size == "small"):
            assert lanes == 0  # (the lane kernel runs on a stream of its own: not without the pipeline)
    eng.close()


def _small_batches(mix):
    from sedef_amd import TASK_DTYPE
    rng = np.random.default_rng(7)
    n_pool = len(mix.pool)
    hollow = np.zeros(300, TASK_DTYPE)
    for k in range(300):
        ql = 0 if k % 3 != 1 else int(rng.integers(1, 300))
        tl = 0 if k % 3 != 0 else int(rng.integers(1, 300))
        hollow[k] = (int(rng.integers(0, n_pool - ql + 1)), int(rng.integers(0, n_pool - tl + 1)), ql, tl, int(rng.choice([-1, 7])),
                     int(rng.choice([-1, 50])), int(rng.choice([0, 1, 0x40])), 0)
    hollow["q_off"][::7][hollow["qlen"][::7] == 0] = n_pool
    real = mix.tasks[np.flatnonzero(~mix.empty)[:1]]
    return {"all empty": Batch(hollow, mix.pool), "one empty": Batch(hollow[:1].copy(), mix.pool), "one real": Batch(real.copy(), mix.pool)}


@pytest.mark.parametrize("form", ["batch", "pairs"])
def test_all_empty_and_one_task_batches(engine, oracle, mix, form):
    """300 empty tasks, one empty task, one real task: SDF_OK, reset records, no CIGAR word -- with no CIGAR pool at all for
    the batch that has nothing to write."""
    if form == "pairs":
        engine.pool_upload(mix.chars)
    for name, b in _small_batches(mix).items():
        exp = b.expect(oracle)
        _run_ok(engine, form, b, exp, WANT_ALL, name)
        if name != "one real":
            assert len(exp[1]) == 0
            rc, used, got, cig, err = _host_call(engine, form, b, 0, WANT_ALL, null_cigar=True)
            assert (rc, used) == (0, 0), (name, err)
            _check_records(b, exp, got, cig, used, WANT_ALL, name + ", no pool")
            assert engine.last_launches() >= 0


def test_degenerate_scoring_leaves_nothing_behind(engine, oracle, mix, mix_tiled):
    """-min_sc > 2 (q + e): every task of the batch, real or empty, comes back reset and no CIGAR word is counted; then the
    same context runs the batch under SEDEF's scoring and equals the oracle."""
    reset = _reset_record()
    exp = mix.expect(oracle, **DEGENERATE)
    assert len(exp[1]) == 0 and all((exp[0][f] == reset[f]).all() for f in ALL_FIELDS)  # (the oracle's early return)
    engine.pool_upload(mix.chars)
    dev = DeviceBatch(mix)
    for form, want in (("batch", WANT_ALL), ("batch", WANT_FAST), ("brief", WANT_FAST), ("pairs", WANT_FAST), ("pairs_full", WANT_ALL)):
        rc, used, got, cig, err = _host_call(engine, form, mix, _roomy(mix), want, **DEGENERATE)
        assert (rc, used) == (0, 0), (form, err)
        assert (cig == SENTINEL).all()
        if form in ("batch", "pairs_full"):
            for f in ALL_FIELDS:
                assert (got[f] == reset[f]).all(), (form, f)
        else:
            assert not got["n_cigar"].any() and not got["matches"].any()
        _run_ok(engine, form, mix, mix.expect(oracle), want, form + " after a degenerate call")
    rc, used, got, cig, err = dev.call(engine, _roomy(mix), WANT_FAST, **DEGENERATE)
    assert (rc, used) == (0, 0) and (cig == SENTINEL).all(), err
    for f in ALL_FIELDS:
        assert (got[f] == reset[f]).all(), ("device", f)
    # the tiled form: lane kernel, chunks and heavy tasks -- none of them has anything to do
    tiled_deg = (np.tile(exp[0], TILES), exp[1])
    rc, used, got, cig, err = _host_call(engine, "batch", mix_tiled, 0, WANT_FAST, **DEGENERATE)
    assert (rc, used) == (0, 0), err
    _check_records(mix_tiled, tiled_deg, got, cig, used, WANT_FAST, "tiled, degenerate")
    assert all((got[f] == reset[f]).all() for f in ALL_FIELDS) and engine.last_lane_tasks() == 0
    _run_ok(engine, "batch", mix_tiled, mix_tiled.expect(oracle), WANT_FAST, "tiled after a degenerate call")


# ---- 2. a CIGAR pool that is too small --------------------------------------------------------------------------------------
def _caps(need):
    return [0, 1, need // 2, need - 1]


@pytest.mark.parametrize("form", ["batch", "brief", "pairs", "pairs_full"])
def test_cigar_overflow_host_forms(engine, oracle, mix, other, form):
    """Too small by everything, by half, by one word: -5, the need, a message, the guard behind the pool untouched -- and the
    context runs another batch right afterwards.  Exactly the need: the bytes of a roomy call."""
    exp = mix.expect(oracle)
    need = len(exp[1])
    if form.startswith("pairs"):
        engine.pool_upload(mix.chars)
    roomy = _run_ok(engine, form, mix, exp)
    for cap in _caps(need):
        if form.startswith("pairs"):
            engine.pool_upload(mix.chars)
        rc, used, got, cig, err = _host_call(engine, form, mix, cap)
        assert (rc, used) == (OVERFLOW, need) and err, (form, cap, rc, used, err)
        assert _guard_intact(cig, cap), (form, cap)
        assert engine.last_reran() == 0
        if form.startswith("pairs"):
            engine.pool_upload(other.chars)
        _run_ok(engine, form, other, other.expect(oracle), what="%s after an overflow at cap %d" % (form, cap))
    if form.startswith("pairs"):
        engine.pool_upload(mix.chars)
    rc, used, got, cig, err = _host_call(engine, form, mix, need)
    assert (rc, used) == (0, need), err
    assert _guard_intact(cig, need)
    assert got.tobytes() == roomy[0].tobytes() and cig[:need].tobytes() == roomy[1].tobytes()
    assert engine.last_reran() == 0


def test_cigar_overflow_device_form(engine, oracle, mix, other):
    """The same on HBM buffers, where the compaction kernel writes into the caller's own pool: no word at or behind
    d_cig[cigar_cap].  No pool at all although CIGARs are wanted: an overflow with the need."""
    exp = mix.expect(oracle)
    need = len(exp[1])
    dev, dev_other = DeviceBatch(mix), DeviceBatch(other)
    rc, used, roomy_rec, roomy_cig, err = dev.call(engine, _roomy(mix))
    assert (rc, used) == (0, need), err
    for cap in _caps(need) + [None]:
        rc, used, got, cig, err = dev.call(engine, cap if cap is not None else need + 100, null_cigar=cap is None)
        assert (rc, used) == (OVERFLOW, need) and err, (cap, rc, used, err)
        if cap is not None:
            assert _guard_intact(cig, cap), cap
        assert engine.last_reran() == 0
        rc, used, got, cig, err = dev_other.call(engine, _roomy(other))
        assert rc == 0, err
        _check_records(other, other.expect(oracle), got, cig, used, WANT_FAST, "device after an overflow at cap %r" % (cap,))
    rc, used, got, cig, err = dev.call(engine, need)
    assert (rc, used) == (0, need), err
    assert _guard_intact(cig, need)
    assert got.tobytes() == roomy_rec.tobytes() and cig[:need].tobytes() == roomy_cig[:need].tobytes()
    assert engine.last_reran() == 0


def test_scores_alone_need_no_cigar_pool(engine, oracle, mix):
    """want = SDF_WANT_SCORE, cigar_cap = 0 and no pool: SDF_OK and the oracle's scores, from every form that takes `want`."""
    rec, _ = mix.expect(oracle)
    engine.pool_upload(mix.chars)
    runs = [("batch", _host_call(engine, "batch", mix, 0, WANT_SCORE, null_cigar=True)),
            ("pairs_full", _host_call(engine, "pairs_full", mix, 0, WANT_SCORE, null_cigar=True)),
            ("device", DeviceBatch(mix).call(engine, 0, WANT_SCORE, null_cigar=True))]
    reset = _reset_record()
    for form, (rc, used, got, cig, err) in runs:
        assert (rc, used) == (0, 0), (form, err)
        for f in ("score", "mte", "mte_q", "zdropped"):
            assert np.array_equal(got[f], rec[f]), (form, f)
        assert not got["n_cigar"].any()
        for f in ALL_FIELDS:
            assert (got[f][mix.empty] == reset[f]).all(), (form, f)


@pytest.mark.parametrize("name", ["default", "lane", "split_min", "early_heavy"])
def test_cigar_overflow_with_work_in_flight(oracle, mix, other, mix_tiled, other_tiled, name):
    """The bail-out with a second part on another context (split_min), with heavy chunks started early (early_heavy), with
    the lane kernel's stream and the chunks of a pipeline (default, tiled): -5 and the need, then the same context runs a
    different batch and equals the oracle, then the first one again with exactly the need."""
    eng = _engine(name)
    for size, b, o in (("small", mix, other), ("tiled", mix_tiled, other_tiled)):
        exp = b.expect(oracle)
        need = len(exp[1])
        roomy = _run_ok(eng, "batch", b, exp, what="%s %s" % (name, size))
        for cap in (need // 2, need - 1):
            rc, used, got, cig, err = _host_call(eng, "batch", b, cap)
            assert (rc, used) == (OVERFLOW, need) and err, (name, size, cap, rc, used, err)
            assert _guard_intact(cig, cap)
            assert eng.last_reran() == 0
            _run_ok(eng, "batch", o, o.expect(oracle), what="%s %s after an overflow at cap %d" % (name, size, cap))
        rc, used, got, cig, err = _host_call(eng, "batch", b, need)
        assert (rc, used) == (0, need), err
        assert _guard_intact(cig, need)
        assert got.tobytes() == roomy[0].tobytes() and cig[:need].tobytes() == roomy[1].tobytes()
        assert eng.last_reran() == 0
    eng.close()
