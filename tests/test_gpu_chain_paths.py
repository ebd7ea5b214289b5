"""GPU: every path behind sdf_chain_batch, at its size boundaries.

The entry point routes a pair by its number of anchors m (sdf_seed_api.hip): to one of six LDS classes of chain_wave_kernel
(one wavefront per pair, everything in LDS; the caps of classes 0..4 are 2..32 KiB, class 5 ends where the device's grant
of dynamic LDS ends), or to chain_kernel (one thread per pair, scratch in HBM) -- pairs beyond class 5, the whole of class
5 once a call holds more than 512 such pairs, and every pair under SDF_CHAIN_THREADS=1.  No test guesses the route:
sdf_last_chain_classes says what ran, tests/chaingen.py restates the rule, and every test asserts that the two agree.

Expected values: oracle.chain_anchors (its tree pinned on the reference's SegmentTree class, tests/test_chain_oracle.py),
for EQUALITY of path and boundaries; the inputs (tests/chaingen.py) must hold chains, links and ties by the oracle's
result alone before the device is asked anything.  The CPU half -- the host's chain_anchors on the same inputs -- is
tests/test_chain_oracle.py: test_host_chains_equal_oracle_at_every_size, test_host_chains_order_keys_as_int."""
import numpy as np
import pytest

import chaingen


@pytest.fixture(scope="module")
def host():
    from sedef_amd import host as h
    h.load_host()
    return h


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_threads():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0, config={"SDF_CHAIN_THREADS": 1})
    yield e
    e.close()


@pytest.fixture(scope="module")
def cap5(eng):
    cap = eng.last_chain_classes()[7]
    assert cap in (64 * 1024, 160 * 1024), cap  # (what sdf_create asks for, or what every kernel has)
    return cap


@pytest.fixture(scope="module")
def real(host):
    return chaingen.RealAnchors(host, np.random.default_rng(61))


@pytest.fixture(scope="module")
def edge(oracle, real, cap5):
    """The class-edge list and the oracle's answers under both settings (computed once, never written to)."""
    cases = chaingen.edge_cases(np.random.default_rng(62), real, cap5, accept=chaingen.has_chain_of_three(oracle))
    exp = {s: [oracle.chain_anchors(a, *s) for a in cases] for s in chaingen.SETTINGS}
    for s in chaingen.SETTINGS:
        chaingen.check_inputs(cases, exp[s], cap5)
    return cases, exp


@pytest.fixture(scope="module")
def edge_default(eng, edge):
    """What a default engine returns for the class-edge list, and the classes it reports."""
    cases, _ = edge
    got = {s: eng.chain_batch(cases, *s) for s in chaingen.SETTINGS}
    return got, eng.last_chain_classes()


def _sizes(cases):
    return [len(a) for a in cases]


def _mismatches(cases, got, exp):
    return [(k, len(a)) for k, (a, g, r) in enumerate(zip(cases, got, exp)) if not chaingen.same(g, r)]


def _run(engine, oracle, cases, counts, gap=210, score=4, exp=None):
    """One call: the reported classes equal `counts`, the results equal the oracle's."""
    got = engine.chain_batch(cases, gap, score)
    cls = engine.last_chain_classes()
    print("classes", cls)
    assert cls[:7] == counts, (cls, counts)
    if exp is None:
        exp = [oracle.chain_anchors(a, gap, score) for a in cases]
    assert not _mismatches(cases, got, exp), (gap, score)
    return got


@pytest.mark.gpu
def test_class_edges_on_the_wave_kernel(host, edge, edge_default, cap5):
    """Both sides of every class boundary (from the device's cap, not from a table), 2^k - 1, 2^k, 2^k + 1 up to 2,049 and
    0, 1, 2, in one call: each LDS class of the wavefront kernel runs, what lies above the last one goes to the threads."""
    cases, exp = edge
    got, cls = edge_default
    print("classes", cls, "tops", chaingen.class_tops(cap5))
    tops = chaingen.class_tops(cap5)
    sizes = _sizes(cases)
    for t in tops:
        assert t in sizes and t + 1 in sizes
    assert tops[:5] == [14, 32, 64, 128, 256] and tops[5] == {64 * 1024: 512, 160 * 1024: 1526}[cap5]
    assert cls[:7] == chaingen.class_counts(sizes, cap5)
    assert all(cls[c] > 0 for c in range(6))
    assert cls[6] == sum(m > tops[5] for m in sizes) > 0
    assert sizes != sorted(sizes, reverse=True) and sizes.count(0) >= 3 and sizes.count(1) >= 3 and sizes.count(2) >= 3
    for s in chaingen.SETTINGS:
        assert not _mismatches(cases, got[s], exp[s]), s
        assert not [len(a) for a, r in zip(cases, exp[s]) if not chaingen.same(host.chain_raw(a, *s), r)], s


@pytest.mark.gpu
def test_large_lds_class_alone(oracle, eng, real, cap5):
    """Twelve pairs that need more than 64 KiB of dynamic LDS each (513 anchors .. the top of class 5), nothing else in
    the call: the launch the kernel's raised LDS limit exists for."""
    if cap5 == 64 * 1024:
        pytest.skip("this device grants chain_wave_kernel 64 KiB of dynamic LDS: no pair of more than 512 anchors runs in LDS")
    rng = np.random.default_rng(63)
    top = chaingen.class_tops(cap5)[5]
    sizes = [513, top] + [int(m) for m in rng.integers(514, top, 10)]
    assert all(chaingen.wave_lds_bytes(m) > 64 * 1024 for m in sizes)
    cases = chaingen.cases_of(rng, real, sizes)[::2]  # (twelve of the twenty-four, lattices and real ones as they fall)
    assert len(cases) == 12
    exp = [oracle.chain_anchors(a, 210, 4) for a in cases]
    chaingen.check_inputs(cases, exp, cap5)
    _run(eng, oracle, cases, [0, 0, 0, 0, 0, 12, 0], exp=exp)
    _run(eng, oracle, cases, [0, 0, 0, 0, 0, 12, 0], 50, 3)


@pytest.mark.gpu
def test_thread_per_pair_kernel_forced(oracle, eng_threads, real, edge, edge_default):
    """SDF_CHAIN_THREADS=1: the class-edge list and two pairs of 3,000 and 6,000 real anchors, every pair on chain_kernel
    (its heap sorts, its scratch layout at ws_off, its `which` order); equal to the oracle and to the wavefront kernel."""
    cases, exp = edge
    rng = np.random.default_rng(64)
    long_cases = [real.take(rng, 3000), real.take(rng, 6000)]
    every = cases + long_cases
    for s in chaingen.SETTINGS:
        long_exp = [oracle.chain_anchors(a, *s) for a in long_cases]
        got = eng_threads.chain_batch(every, *s)
        cls = eng_threads.last_chain_classes()
        print("classes", cls)
        assert cls[:6] == [0] * 6 and cls[6] == len(every)
        assert not _mismatches(every, got, exp[s] + long_exp), s
        for (gp, gb), (dp_, db) in zip(got, edge_default[0][s]):
            assert gp.tobytes() == dp_.tobytes() and gb.tobytes() == db.tobytes()


@pytest.mark.gpu
def test_pairs_beyond_lds_in_a_default_engine(oracle, eng, real, cap5):
    """Two pairs too large for LDS between small ones: scratch offsets for some pairs only, both kernels writing one path /
    bounds buffer."""
    rng = np.random.default_rng(65)
    top = chaingen.class_tops(cap5)[5]
    sizes = [9, 40, top + 1, 0, 130, 17, 4000, 3, 300, 1]
    cases = [chaingen.lattice(rng, m) if k % 2 else real.take(rng, m) for k, m in enumerate(sizes)]
    counts = chaingen.class_counts(sizes, cap5)
    assert counts[6] == 2
    for s in chaingen.SETTINGS:
        _run(eng, oracle, cases, counts, *s)


@pytest.mark.gpu
def test_many_large_pairs_spill_to_the_threads(oracle, eng, cap5):
    """More than 512 pairs of class 5 in one call all go to the thread-per-pair kernel (their scratch offsets are given
    in a second pass, behind those of the pairs beyond LDS); 512 of them stay where they are."""
    rng = np.random.default_rng(66)
    large = [chaingen.lattice(rng, int(m)) for m in rng.integers(257, 301, 513)]
    small_sizes = [0, 1, 2, 5, 14, 15, 30, 33, 60, 64, 65, 100, 128, 129, 200, 256, 7, 31, 127, 255]
    small = [chaingen.lattice(rng, m) for m in small_sizes]
    small_counts = chaingen.class_counts(small_sizes, cap5)
    assert small_counts[5] == small_counts[6] == 0 and all(small_counts[:5])
    exp_large = [oracle.chain_anchors(a, 210, 4) for a in large]
    exp_small = [oracle.chain_anchors(a, 210, 4) for a in small]
    chaingen.check_inputs(large, exp_large, cap5)
    for n_large, c5, c6 in ((513, 0, 513), (512, 512, 0)):
        both = list(zip(large[:n_large], exp_large))
        for k, pair in enumerate(zip(small, exp_small)):  # the small ones spread among the large ones
            both.insert(k * 25, pair)
        cases, exp = [a for a, _ in both], [r for _, r in both]
        counts = small_counts[:5] + [c5, c6]
        assert counts == chaingen.class_counts(_sizes(cases), cap5)
        _run(eng, oracle, cases, counts, exp=exp)


@pytest.mark.gpu
def test_one_context_calls_of_changing_size(oracle, real, cap5):
    """Large, tiny, empty, all-empty pairs, large again on ONE context: the call's device buffers are reused at every size,
    every call is exact, and the classes are those of the last call alone."""
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    rng = np.random.default_rng(67)
    top = chaingen.class_tops(cap5)[5]
    assert e.last_chain_classes() == [0] * 7 + [cap5]
    _run(e, oracle, [real.take(rng, 4000)], [0, 0, 0, 0, 0, 0, 1])
    _run(e, oracle, [chaingen.lattice(rng, 6), real.take(rng, 20), chaingen.lattice(rng, 1)], [2, 1, 0, 0, 0, 0, 0])
    assert e.chain_batch([]) == []
    assert e.last_chain_classes() == [0] * 7 + [cap5]
    _run(e, oracle, [np.zeros((0, 4), np.int32)] * 5, [5, 0, 0, 0, 0, 0, 0])
    _run(e, oracle, [chaingen.lattice(rng, top + 1), real.take(rng, 70), real.take(rng, 3000)], [0, 0, 0, 1, 0, 0, 2], 50, 3)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["a", "b", "b1", "c"])
def test_keys_are_ordered_as_int(oracle, eng, eng_threads, edge, cap5, variant):
    """Negative coordinates next to non-negative ones (a), negative chain scores (b), coordinates near 10^9 (c): the
    wavefront kernel sorts packed 64-bit keys, the thread-per-pair kernel compares ints; both return what the reference's
    pair<int, int> order gives."""
    cases, gap, score = chaingen.signed_variants(edge[0])[variant]
    if variant == "a":
        assert chaingen.mixed_signs(cases) >= 10
    exp = [oracle.chain_anchors(a, gap, score) for a in cases]
    if variant == "b":
        assert all(int(r["dp"].max()) < 0 for a, r in zip(cases, exp) if len(a))
    if variant == "b1":
        assert sum(int(r["dp"].min()) < 0 <= int(r["dp"].max()) for a, r in zip(cases, exp) if len(a)) >= 10
    sizes = _sizes(cases)
    bad_threads = _mismatches(cases, eng_threads.chain_batch(cases, gap, score), exp)
    assert eng_threads.last_chain_classes()[:7] == chaingen.class_counts(sizes, cap5, threads_only=True)
    bad_wave = _mismatches(cases, eng.chain_batch(cases, gap, score), exp)
    assert eng.last_chain_classes()[:7] == chaingen.class_counts(sizes, cap5)
    print("mismatches: wavefront engine", bad_wave, "thread engine", bad_threads)
    assert not bad_wave and not bad_threads
