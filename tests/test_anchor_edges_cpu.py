"""Seed anchors at the 1000-occurrence rule (src/chain.cc:61) on the CPU: the cases of tests/anchor_edge_cases.py hold what they
claim, the model (tests/bruteforce.py) answers them as the reasoning written next to each builder expects, its answers at 999
and at 1000 occurrences differ, and the host form (sedef_amd/csrc/host/chain.cc) equals the model, order and has_u included."""
import collections

import pytest

import anchor_edge_cases as aec

FAMILIES = ("A1", "A2", "A3", "A4", "B", "C", "D")
# The model's own count over the file is 98,871 anchors (k = 8: 32,955; 11: 32,961; 15: 32,955): nearly all of them the
# k-long or unit-long matches with the N-separated copies of the cases below the cap.  A file whose copies no longer matched
# anything would lose those first, so the floor is 30,000 a k: nine tenths of what the model counts.
FLOOR_PER_K = 30000


@pytest.fixture(scope="module")
def host():
    from sedef_amd import host as h
    h.build_host()
    return h


@pytest.mark.parametrize("k", aec.K_VALUES)
def test_cases_are_small_and_every_family_is_built(k):
    cases = aec.cases(k)  # (every builder asserts its premise with count_by_code / count_by_string)
    assert collections.Counter(c.family for c in cases) == dict(A1=4, A2=4, A3=4, A4=4, B=9, C=9, D=8)
    assert len({c.label for c in cases}) == len(cases)
    for c in cases:
        q, r, same, delta = c.pair
        assert len(q) <= 400 and len(r) <= 40000 and c.k == k
        assert set(q + r) <= set("ACGTNacgtnRMrm"), c.label
    for fam in "A1", "A2", "A3", "A4":
        assert [c.occ for c in cases if c.family == fam] == list(aec.COUNTS)


def test_the_counters_count_what_they_say():
    r = "ACGTANACGTRNacgtaNAAGTANACGTNC"
    assert aec.count_by_string(r, "ACGTA") == 2 and aec.count_by_string(r, "ACGTA", fold=False) == 1
    assert aec.count_by_code(r, "ACGTA") == 3  # ACGTA, ACGTR, acgta; ACGTN holds an N
    assert aec.count_by_code(r, "ACGTA", skip_n=False) == 4  # ... and with the N hashed as the A it codes as
    assert aec.count_by_code("AAAAA", "AAAA") == 2 and aec.count_by_string("AAAAA", "AAAA") == 2
    assert aec.count_by_code("TTTTNTTTT", "TTTT") == 2 and aec.count_by_code("ACG", "ACGT") == 0


@pytest.mark.parametrize("k", aec.K_VALUES)
def test_model_agrees_with_the_reasoning_on_the_focus_diagonal(k):
    for c, exp in zip(aec.cases(k), aec.expected(k)):
        assert aec.on_diagonal(exp, c.diag) == c.focus, c.label
        assert list(exp) == sorted(exp, key=lambda a: (a[0], a[1])), c.label


@pytest.mark.parametrize("k", aec.K_VALUES)
def test_model_differs_between_999_and_1000_in_every_family(k):
    cases, exp = aec.cases(k), aec.expected(k)
    groups = collections.defaultdict(dict)
    for c, e in zip(cases, exp):
        groups[c.group].setdefault(c.occ, (c, e))
    seen = set()
    for name, by_occ in groups.items():
        if aec.CAP - 1 not in by_occ or aec.CAP not in by_occ:
            continue
        (below, e_below), (at, e_at) = by_occ[aec.CAP - 1], by_occ[aec.CAP]
        assert e_below != e_at, name
        copies_at = len(below.pair[0]) + aec.PAD + 1  # the copies lie behind the in-place stretch and its "N"
        far_below, far_at = [a for a in e_below if a[1] >= copies_at], [a for a in e_at if a[1] >= copies_at]
        excluded = below.family == "D" and not below.focus  # (the focus diagonal is within k of the main one at any count)
        if below.family == "A2" or excluded:
            assert aec.on_diagonal(e_below, below.diag) == aec.on_diagonal(e_at, at.diag), name
        else:  # the start on the focus diagonal moves, or the anchor goes
            assert aec.on_diagonal(e_below, below.diag) != aec.on_diagonal(e_at, at.diag), name
        # the diagonals of the copies: every copy below the cap, none at it
        assert len(far_below) >= aec.CAP - 4 and not far_at, (name, len(far_below), len(far_at))
        seen.add(below.family)
    assert seen == set(FAMILIES)
    # 998 behaves as 999 does and 1001 as 1000 on the focus diagonal
    for fam in "A1", "A2", "A3", "A4":
        f = {c.occ: c.focus for c in cases if c.family == fam}
        assert f[998] == f[999] and f[1000] == f[1001], fam


@pytest.mark.parametrize("k", aec.K_VALUES)
def test_the_file_expects_anchors_and_both_values_of_has_u(k):
    cases, exp = aec.cases(k), aec.expected(k)
    assert sum(len(e) for e in exp) >= FLOOR_PER_K
    both = [e for c, e in zip(cases, exp) if c.group.startswith("B3") and c.occ < aec.CAP]
    assert len(both) == 1 and {a[3] for a in both[0]} == {0, 1}
    at_cap = [e for c, e in zip(cases, exp) if c.group.startswith("B3") and c.occ >= aec.CAP]
    assert len(at_cap) == 1 and len(at_cap[0]) >= 1


@pytest.mark.parametrize("k", aec.K_VALUES)
def test_host_anchors_equal_the_model(host, k):
    for c, exp in zip(aec.cases(k), aec.expected(k)):
        q, r, same, delta = c.pair
        got = host.anchors(q, r, k, bool(same), 0, delta)
        assert got == list(exp), (c.label, len(got), len(exp))
