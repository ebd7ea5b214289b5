"""CPU: the winnowed minimizers and their index, pinned on the reference (tests/golden/minimizers_kat.json.gz, written by
tests/golden/make_golden_minimizers.py from the reference's own get_minimizers / Index::Index):
  * tests/minim_model.py -- the deque loop and Index::Index transcribed -- gives the fixture's lists;
  * the closed form the device kernels implement (sedef_amd/csrc/minimizers.hip) gives the model's, on seeded random input;
  * the library exports the entry points and its records have the documented sizes."""
import ctypes
import gzip
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import minim_model as M  # noqa: E402


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "minimizers_kat.json.gz"), "rb") as f:
        return json.loads(f.read().decode())


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def sequence(case):
    s = case["seq"].encode()
    return M.rev_comp(s) if case["rc"] else s


def digest(rows):
    return hashlib.sha256(np.asarray(rows, dtype="<i4").reshape(-1, 3).tobytes()).hexdigest()


def test_fixture_holds_the_cases_it_promises(fixture):
    cases = fixture["cases"]
    assert 200 <= len(cases) and all(len(c["seq"]) <= 400 for c in cases)
    for k, w in ((12, 16), (1, 1), (15, 3)):
        got = {len(c["seq"]) - k + 1 for c in cases if (c["k"], c["w"]) == (k, w) and c["name"].startswith("nk=")}
        assert {0, 1, w - 1, w, w + 1, w + 2} <= got
    assert any(len(c["seq"]) < c["k"] for c in cases) and any(c["w"] == 1 for c in cases)
    assert {1, 2, 12, 15} <= {c["k"] for c in cases} and {0, 1} == {c["sl"] for c in cases} == {c["rc"] for c in cases}
    assert {0, 1, 2} == {m[2] for c in cases for m in c["minimizers"]}
    for c in cases:
        if c["name"].startswith("poly-"):  # every start >= w is a minimizer
            assert [m[1] for m in c["minimizers"]] == list(range(c["w"], len(c["seq"]) - c["k"] + 1))
    # R is no N forward and an N after the reverse complement
    assert any("R" in c["seq"] and c["rc"] for c in cases) and any("R" in c["seq"] and not c["rc"] for c in cases)
    long_cases = fixture["long_cases"]
    assert sum(c["threshold"] != M.THRESHOLD_NONE for c in long_cases) >= 2
    assert any(c["threshold"] == M.THRESHOLD_NONE for c in long_cases)
    assert all(c["n_minimizers"] >= 100000 for c in long_cases)  # (ignore >= 1: the walk takes at least one step)


def test_model_gives_the_fixture(fixture):
    for c in fixture["cases"]:
        mins = M.get_minimizers(sequence(c), c["k"], c["w"], bool(c["sl"]))
        assert [list(m) for m in mins] == c["minimizers"], c["name"]
        n_groups, threshold, groups = M.index(mins)
        assert (n_groups, threshold) == (c["n_groups"], c["threshold"]), c["name"]
        assert [[st, h, locs] for (st, h), locs in groups] == c["groups"], c["name"]


def test_model_gives_the_long_cases(fixture):
    for c in fixture["long_cases"]:
        mins = M.get_minimizers(sequence(c), c["k"], c["w"], bool(c["sl"]))
        assert len(mins) == c["n_minimizers"] and digest(mins) == c["minimizers_sha256"], c["name"]
        n_groups, threshold, groups = M.index(mins)
        assert (n_groups, threshold) == (c["n_groups"], c["threshold"]), c["name"]
        assert digest([(h, loc, st) for (st, h), locs in groups for loc in locs]) == c["groups_sha256"], c["name"]
        assert np.array_equal(M.closed_form_np(sequence(c), c["k"], c["w"], bool(c["sl"])), np.asarray(mins, np.int64)), c["name"]


def test_closed_form_is_the_deque_loop_on_keys():
    """(status, hash) keys with heavy ties, lengths 0..80, w 1..20: the loop as written against the closed form."""
    rng = np.random.default_rng(11)
    for it in range(4000):
        n, w, top = int(rng.integers(0, 81)), int(rng.integers(1, 21)), int(rng.integers(1, 5))
        key = [(int(s), int(h)) for s, h in zip(rng.choice([0, 0, 0, 1, 2], n), rng.integers(0, top + 1, n))]
        assert M.closed_form_keys(key, w) == M.deque_keys(key, w), (it, key, w)


def test_closed_form_is_the_model_on_sequences():
    rng = np.random.default_rng(12)
    alphabet = np.frombuffer(b"ACGTacgtNnRr-AAAAaaaa", np.uint8)
    for it in range(1500):
        n, k, w = int(rng.integers(0, 160)), int(rng.choice([1, 2, 3, 5, 12, 15])), int(rng.integers(1, 24))
        sl = bool(rng.integers(0, 2))
        s = alphabet[rng.integers(0, len(alphabet), n)].tobytes()
        want = M.get_minimizers(s, k, w, sl)
        assert M.closed_form(s, k, w, sl) == want, (it, s, k, w, sl)
        assert [tuple(r) for r in M.closed_form_np(s, k, w, sl).tolist()] == want, (it, s, k, w, sl)


def test_library_exports_the_entry_points_and_record_sizes():
    from sedef_amd.build import build_library
    lib = ctypes.CDLL(build_library())
    for name in ("sdf_pool_minimizers", "sdf_pool_minimizers_device", "sdf_pool_minimizer_index", "sdf_minimizer_block"):
        assert hasattr(lib, name), name
    lib.sdf_minimizer_block.restype = ctypes.c_int
    block = lib.sdf_minimizer_block()
    assert block % 64 == 0 and block > 1000  # (the block at start 0 holds every start <= w, w up to SDF_MINIM_MAX_W)
    from sedef_amd import extz2
    assert extz2.MINIM_RANGE_DTYPE.itemsize == 16 and extz2.MINIMIZER_DTYPE.itemsize == 16
    assert extz2.MINIMIZER_DTYPE.names == ("hash", "loc", "status", "range")
    assert [extz2.MINIM_RANGE_DTYPE.fields[f][1] for f in ("off", "len", "flags")] == [0, 8, 12]
    header = open(os.path.join(ROOT, "include", "sedef_hip.h")).read()
    assert "#define SDF_MINIM_BLOCK %d" % block in header and "#define SDF_MINIM_MAX_W %d" % extz2.MINIM_MAX_W in header
    for name in ("pool_minimizers", "pool_minimizers_device", "pool_minimizer_index"):
        assert callable(getattr(extz2.Extz2Engine, name))
