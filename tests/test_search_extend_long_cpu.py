"""CPU: the search extension on LONG growths -- a winnow range grown by more than SDF_EXTEND_MAX_GROW = 1,792 records at an end --
pinned on the reference (tests/golden/search_extend_long_kat.json.gz, written by tests/golden/make_golden_search_extend_long.py
from the reference's own SlidingMap and Index through the driver of make_golden_search_extend.py): tests/extend_model.py and
sdf_search_extend_host both give the fixture's records.  The host form is the truth of tests/test_gpu_search_extend_long.py."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import extend_model as E  # noqa: E402
from test_search_extend_cpu import case_extend_inputs, host, model, same_hits  # noqa: E402


def load_fixture():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "search_extend_long_kat.json.gz"), "rb") as f:
        return json.loads(f.read().decode())


def case_expected(c):
    """The reference's answers.  It does not know SDF_EXTEND_WIDE: compare with without_wide() of a form's records."""
    rows = [tuple(t[8:17]) + (t[7],) for w in c["windows"] for t in w[2]]
    return np.array(rows, E.HIT) if rows else np.zeros(0, E.HIT)


def grown(args, hits):
    """Per interval, the largest growth of the four ends of its winnow ranges (0 where there is no hit)."""
    q, windows, first, intervals, rolls = args[:5]
    i = np.searchsorted(first, np.arange(len(hits)), "right") - 1
    g = np.maximum.reduce([i - hits["q_winnow_start"], hits["q_winnow_end"] - (i + windows["n_members"][i]),
                           rolls["winnow_start"] - hits["r_winnow_start"], hits["r_winnow_end"] - rolls["winnow_end"]])
    return np.where(hits["query_end"] != 0, g, 0)


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


@pytest.fixture(scope="module")
def inputs(fixture):
    return [case_extend_inputs(c) for c in fixture["cases"]]


def without_wide(hits):
    out = hits.copy()
    out["flags"] &= ~np.uint32(E.WIDE)
    return out


def test_every_case_grows_beyond_the_short_cap(fixture, inputs):
    assert len(fixture["cases"]) >= 4 and any(c["same_genome"] for c in fixture["cases"]) and any(not c["same"] for c in fixture["cases"])
    for c, (args, params) in zip(fixture["cases"], inputs):
        want = case_expected(c)
        assert (want["flags"] == 0).any() and grown(args, want).max() > E.MAX_GROW, c["name"]


def test_model_gives_the_fixture(fixture, inputs):
    seen = {}
    for c, (args, params) in zip(fixture["cases"], inputs):
        got = model(args, params, seen=seen)
        want = case_expected(c)
        same_hits(without_wide(got), want, c["name"])
        # WIDE exactly where a growth passed the cap (a kept step: these walks take nothing back beyond it)
        assert (((got["flags"] & E.WIDE) != 0) >= (grown(args, want) > E.MAX_GROW)).all(), c["name"]
        assert ((got["flags"] & E.WIDE) != 0).sum() >= 1
    assert seen.get("guards", 0) == 0  # (no committed case reaches what the reference leaves undefined)


def test_host_form_gives_the_fixture_and_the_model(fixture, inputs):
    for c, (args, params) in zip(fixture["cases"], inputs):
        code, got = host(args, params)
        assert code == 0, c["name"]
        same_hits(without_wide(got), case_expected(c), c["name"])
        same_hits(got, model(args, params), c["name"])
