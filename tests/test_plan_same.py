"""Every plan of a corpus of batches, pinned: tests/golden/plan_digests.json holds the digests of everything the launcher reads
of a plan -- the cut's figures, every PlanTask field, the launch order, the chunks, their launches, the lane figures and
records (the library's sdf_debug_plan_dump hook) -- for each batch of tests/golden/make_golden_plans.py under its settings,
planned on 0 and on 3 threads.  A change of the planner that means to leave its plans alone passes without the file being
written again; one that means to change a plan says which, by the digests it rewrites.  No GPU: the planner is host code."""
import importlib.util
import json
import os

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_plans", os.path.join(_HERE, "golden", "make_golden_plans.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

_CASES = gen.corpus()
_cache = {}


@pytest.fixture(scope="module")
def golden():
    with open(gen.OUT) as f:
        return json.load(f)


def test_the_file_holds_the_corpus_and_nothing_else(golden):
    assert sorted(golden) == sorted("%s|t%d" % (c[0], th) for c in _CASES for th in gen.THREADS)


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_plan_is_the_pinned_one(golden, case):
    name, build, args, settings = case
    lib = gen.load()
    t = gen.built(_cache, build, args)
    got = {th: gen.plan_digest(lib, t, th, **settings) for th in gen.THREADS}
    for th in gen.THREADS:
        assert got[th] == golden["%s|t%d" % (name, th)], (name, th)
    if not settings.get("two_pass"):  # (the cut in two passes needs scan threads: without them it is the one-pass cut)
        assert got[0] == got[3]
