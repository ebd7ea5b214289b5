"""The 60 kb chunking of a DP request (host/dp_provider.cc: for_each_chunk, exported as sdfh_dp_chunks) against the loop of
align_helper as the reference writes it (src/align.cc:46-57), with a step of 8 bases: the form the coded pool takes (both
sequences forward) and the form the resident pool takes (a reversed target, read from the end of its range)."""
import pytest

STEP = 8
T_OFF = 1000


@pytest.fixture(scope="module")
def host():
    from sedef_amd import host as h
    from sedef_amd.build import build_library
    build_library()
    h.build_host()
    return h


def model(qlen, tlen, step):
    """src/align.cc:46-57: (SP, query length, target length) of every ksw_extz2_sse call"""
    out = []
    sp = 0
    while sp < min(tlen, qlen):
        out.append((sp, min(step, qlen - sp), min(step, tlen - sp)))
        sp += step
    return out


def shapes():
    for m in (0, 1, 7, 8, 9, 16, 17):
        for more in (3, STEP, 2 * STEP + 3):
            yield m, m + more  # qlen < tlen
            yield m + more, m  # qlen > tlen
        yield m, m


@pytest.mark.parametrize("qlen,tlen", sorted(set(shapes())))
def test_chunks_forward_and_reversed(host, qlen, tlen):
    want = model(qlen, tlen, STEP)
    fwd = host.dp_chunks(qlen, tlen, STEP, False, T_OFF)
    rev = host.dp_chunks(qlen, tlen, STEP, True, T_OFF)
    assert len(fwd) == len(rev) == len(want) == (min(qlen, tlen) + STEP - 1) // STEP
    assert (len(want) == 0) == (min(qlen, tlen) == 0)
    assert [(q, ql, tl) for q, _, ql, tl in fwd] == want == [(q, ql, tl) for q, _, ql, tl in rev]
    assert all(ql >= 1 and tl >= 1 for _, _, ql, tl in fwd + rev)
    # forward: the chunks tile [0, .) of both sequences, in order
    q_at, t_at = 0, T_OFF
    for q, t, ql, tl in fwd:
        assert (q, t) == (q_at, t_at)
        q_at, t_at = q + ql, t + tl
    assert t_at - T_OFF == sum(tl for _, _, tl in want) <= tlen and q_at <= qlen
    # reversed: chunk after chunk lies in front of the one before, the first ends where the target's range ends
    t_end = T_OFF + tlen
    for (sp, _, tl), (q, t, _, _) in zip(want, rev):
        assert q == sp and t + tl == t_end and t == T_OFF + tlen - sp - tl
        t_end = t
    assert t_end >= T_OFF
