"""CPU: what the lanes of the search driver (include/sedef_hip.h: sdf_search_lanes_open, sdf_search_pairs_indexed) promise without
a device -- the refusals of a null context, the job queue on its own under a thread sanitizer, and SDF_SEARCH_LANES as the
command reads it."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_a_null_context_is_refused_without_a_device():
    import sedef_amd
    lib = sedef_amd.load_library()
    lanes, used, first = C.c_void_p(0), C.c_size_t(7), (C.c_uint64 * 1)(7)
    assert lib.sdf_search_lanes_open(None, 4, C.byref(lanes)) == -4 and not lanes.value
    assert lib.sdf_search_lanes_close(None, None) == -4
    assert lib.sdf_search_pairs_indexed(None, None, None, 0, None, 0, None, 0, C.byref(used), first, None) == -4
    assert used.value == 7 and first[0] == 7  # (nothing written)


def test_the_job_record_and_the_lane_limit_are_the_headers():
    from sedef_amd import extz2
    src = open(os.path.join(ROOT, "include", "sedef_hip.h")).read()
    assert "#define SDF_SEARCH_LANES_MAX %d\n" % extz2.SEARCH_LANES_MAX in src
    assert "typedef struct { const sdf_search_index *q, *r; int32_t same_genome, reserved; } sdf_search_pair_job;" in src
    assert extz2.PAIR_JOB_DTYPE.names == ("q", "r", "same_genome", "reserved") and extz2.PAIR_JOB_DTYPE.itemsize == 24


def test_the_job_queue_alone_under_the_thread_sanitizer(tmp_path):
    """tests/job_queue_main.cc: a program of its own around sedef_amd/csrc/sdf_job_queue.h with a stub job -- every job once, a
    lane's state touched by its thread alone, nothing started behind a failure -- built with -fsanitize=thread and run here."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "job_queue")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-I", os.path.join(ROOT, "sedef_amd", "csrc"),
                           os.path.join(ROOT, "tests", "job_queue_main.cc"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stdout == b"job queue ok\n" and b"ThreadSanitizer" not in p.stderr, p.stderr.decode()[-2000:]


@pytest.mark.parametrize("value, why", [("0", "out of range"), ("17", "out of range"), ("four", "not a number")])
def test_the_command_refuses_a_lane_count_it_cannot_take(value, why):
    from sedef_amd import host
    host.build_host()
    env = {k: v for k, v in os.environ.items() if not k.startswith("SDF_")}
    p = subprocess.run([host.CLI, "search", "-t", "no_such_genome.fa", "0", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                       env=dict(env, SDF_SEARCH_LANES=value))
    assert p.returncode == 1 and p.stdout == b"" and ("SDF_SEARCH_LANES=%s: %s" % (value, why)).encode() in p.stderr
    # ... and says so in its help
    p = subprocess.run([host.CLI, "help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, env=env)
    assert p.returncode == 0 and b"SDF_SEARCH_LANES=N (1..16, default 1)" in p.stderr
