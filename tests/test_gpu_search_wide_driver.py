"""The search driver with the seeding's WIDE and FOUND_WIDE windows finished on the device: sdf_search_pair_wide,
sdf_search_pair_indexed_wide and `sedef search` under SDF_SEARCH_WIDE_DEVICE.

Expected values: sdf_search_pair_host's bytes, and fewer windows handed to the host than sdf_search_pair hands over.
tests/test_search_wide_cpu.py shows on the CPU that the pair of wide_model.wide_pair has scheduled WIDE windows within the wide
kernel's reach."""
import os
import subprocess
import sys

import pytest
import torch  # noqa: F401  (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import driver_model as DM  # noqa: E402
import wide_model as WM  # noqa: E402
from test_search_driver_paths_cpu import hosted, the_input  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("attempted", "jaccard_failed", "interval_failed", "windows_scheduled")
_host = {}


@pytest.fixture(scope="module")
def eng():
    import sedef_amd
    e = sedef_amd.Extz2Engine(0)
    yield e
    e.close()


def ex():
    from sedef_amd import extz2
    return extz2


def host_answer(I):
    """sdf_search_pair_host's (hits, stats) for the seed-WIDE pair, computed once."""
    if "pair" not in _host:
        rc, hits, used, stats = ex().search_pair_host(I["pool"], I["q_range"], I["r_range"], **DM.pair_kwargs(ex(), I))
        assert rc == 0 and used == len(hits) >= 1
        _host["pair"] = (hits, stats)
    return _host["pair"]


def same_answer(got, want):
    rc, hits, used, stats = got
    want_hits, want_stats = want
    assert rc == 0 and used == len(want_hits)
    assert hits.tobytes() == want_hits.tobytes()
    for f in COUNTERS:
        assert int(stats[f]) == int(want_stats[f]), f


def upload(eng, I):
    eng.pool_upload(I["pool"])
    eng.pool_sync()
    return DM.pair_kwargs(ex(), I)


@pytest.mark.parametrize("round_windows", [1, 64])
def test_a_seed_wide_pair_stays_on_the_device(eng, round_windows):
    I = WM.wide_pair()
    kw = upload(eng, I)
    want = host_answer(I)
    plain = eng.search_pair(I["q_range"], I["r_range"], round_windows=round_windows, **kw)
    wide = eng.search_pair_wide(I["q_range"], I["r_range"], n_wide_max=64, round_windows=round_windows, **kw)
    same_answer(plain, want)
    same_answer(wide, want)
    print(round_windows, {f: (int(plain[3][f]), int(wide[3][f])) for f in ("rounds", "windows_run", "windows_host")})
    assert int(plain[3]["windows_host"]) >= 3
    assert int(wide[3]["windows_host"]) < int(plain[3]["windows_host"])
    # n_wide_max == 0 is sdf_search_pair, its stats included
    zero = eng.search_pair_wide(I["q_range"], I["r_range"], n_wide_max=0, round_windows=round_windows, **kw)
    assert zero[1].tobytes() == plain[1].tobytes() and zero[3].tobytes() == plain[3].tobytes()


@pytest.mark.parametrize("round_windows", [1, 64])
def test_a_window_that_meets_more_records_than_the_plain_kernel_stages(eng, round_windows):
    """Input e of tests/test_gpu_search_driver_paths.py: FOUND_WIDE windows, handed to the host by sdf_search_pair."""
    I = the_input("e")
    kw = upload(eng, I)
    plain = eng.search_pair(I["q_range"], I["r_range"], round_windows=round_windows, **kw)
    wide = eng.search_pair_wide(I["q_range"], I["r_range"], n_wide_max=64, round_windows=round_windows, **kw)
    same_answer(plain, hosted("e"))
    same_answer(wide, hosted("e"))
    print(round_windows, {f: (int(plain[3][f]), int(wide[3][f])) for f in ("rounds", "windows_run", "windows_host")})
    assert int(plain[3]["windows_host"]) >= 1
    assert int(wide[3]["windows_host"]) < int(plain[3]["windows_host"])


def test_two_handles_as_two_ranges(eng):
    I = WM.wide_pair()
    kw = upload(eng, I)
    wide = eng.search_pair_wide(I["q_range"], I["r_range"], n_wide_max=64, **kw)
    handles = []
    try:
        for rng in (I["q_range"], I["r_range"]):
            rc, h = eng.search_index_build(rng, I["k"], I["w"], 1)
            assert rc == 0
            handles.append(h)
        indexed = eng.search_pair_indexed_wide(handles[0], handles[1], n_wide_max=64, **kw)
        assert indexed[0] == 0 and indexed[1].tobytes() == wide[1].tobytes() and indexed[3].tobytes() == wide[3].tobytes()
        launches = eng.last_launches()
        refused = eng.search_pair_indexed_wide(handles[0], handles[1], n_wide_max=(1 << 20) + 1, **kw)
        assert refused[0] == -3 and eng.last_launches() == launches
        assert eng.search_pair_wide(I["q_range"], I["r_range"], n_wide_max=(1 << 20) + 1, **kw)[0] == -3 and eng.last_launches() == launches
    finally:
        for h in handles:
            eng.search_index_free(h)
    same_answer(wide, host_answer(I))


def test_the_command_prints_the_same_bed_with_the_setting(tmp_path):
    """`sedef search` on the fixture of tests/test_gpu_search_cmd.py, each run a fresh child process."""
    import test_gpu_search_cmd as T
    from sedef_amd import host
    host.build_host()
    path = str(tmp_path / "genome.fa")
    T.G.write_fasta(path, T.NAMES, T.RECS, T.WIDTHS)

    def run(env):
        p = subprocess.run([host.CLI, "search", path, "c1", "c1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                           env=dict(os.environ, **env))
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return p.stdout
    without, with_setting = run({}), run({"SDF_SEARCH_WIDE_DEVICE": "64"})
    assert without.count(b"\n") >= 1 and with_setting == without
    bad = subprocess.run([host.CLI, "search", path, "c1", "c1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                         env=dict(os.environ, SDF_SEARCH_WIDE_DEVICE="many"))
    assert bad.returncode != 0 and b"SDF_SEARCH_WIDE_DEVICE" in bad.stderr
