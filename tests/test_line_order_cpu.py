"""CPU: the order of `sedef report`.  The model (tests/report_model.py) against GNU sort and uniq themselves where they are at
hand; sdf_line_records and sdf_line_order_host through sedef_amd/report.py against the model on every case table
(tests/report_cases.py); the host form alone under the address and undefined sanitizers; what the command says without a
device."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import report_cases as R  # noqa: E402
import report_model as M  # noqa: E402

TABLES = R.tables()
KEYS = "-k1,1V -k9,9r -k10,10r -k4,4V -k2,2n -k3,3n -k5,5n -k6,6n"


def gnu_sort():
    try:
        return b"GNU coreutils" in subprocess.run(["sort", "--version"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=30).stdout
    except OSError:
        return False


def tool(args, lines):
    p = subprocess.run("sort %s | uniq" % args, shell=True, input=b"".join(x + b"\n" for x in lines), stdout=subprocess.PIPE, timeout=60,
                       env=dict(os.environ, LC_ALL="C"))
    assert p.returncode == 0
    return p.stdout.split(b"\n")[:-1]


def test_the_model_orders_the_chromosome_names_as_written_out():
    assert sorted(R.NAMES, key=__import__("functools").cmp_to_key(M.filevercmp)) == R.NAMES_SORTED
    assert M.filevercmp(b"chr1", b"chr1") == 0 and M.filevercmp(b"a01", b"a1") < 0 and M.filevercmp(b"#chr1", b"chrX") > 0
    assert M.filevercmp(b"\tchr2", b"\tchr10") < 0  # (a field keeps its leading blank)


def test_the_model_equals_gnu_sort_on_the_chromosome_names():
    if not gnu_sort():
        pytest.skip("sort is not GNU coreutils")
    assert tool("-k1,1V", list(reversed(R.NAMES))) == R.NAMES_SORTED


@pytest.mark.parametrize("name", sorted(TABLES))
def test_the_model_equals_gnu_sort_and_uniq(name):
    if not gnu_sort():
        pytest.skip("sort is not GNU coreutils")
    assert tool(KEYS, TABLES[name]) == M.sort_uniq(TABLES[name])


def test_the_mirror_carries_the_headers_constants():
    from sedef_amd import report
    assert (report.DUP, report.WIDE, report.RUN) == (M.DUP, M.WIDE, M.RUN) and report.LINE_REC_DTYPE.itemsize == 48


@pytest.mark.parametrize("name", sorted(TABLES))
def test_host_form_equals_the_model(name):
    from sedef_amd import report
    lines = TABLES[name]
    pool, recs, plain = report.line_records(lines)
    assert plain == M.plain(lines) and len(recs) == len(lines)
    assert all(int(r["off"]) % 16 == 0 and bytes(pool[int(r["off"]):int(r["off"]) + int(r["len"])]) == x for r, x in zip(recs, lines))
    rc, order, flags, kept = report.line_order_host(pool, recs)
    assert rc == 0 and (order.tolist(), flags.tolist(), kept) == R.expected(name)
    assert R.wide_only_on_long_runs(lines, order.tolist(), flags.tolist())


def test_the_keys_alone_order_the_lines_as_the_models_comparisons_do():
    """(the records' eight keys against key_cmp, pair by pair: ranks, reversed ranks and values)"""
    from sedef_amd import report
    for name in ("empty_name_mixed", "decimal_point", "only_k1_differs", "n_field_without_digits", "size_255", "header_line"):
        lines = TABLES[name]
        _, recs, _ = report.line_records(lines)
        keys = [tuple(int(k) for k in r["key"]) for r in recs]
        for i in range(len(lines)):
            for j in range(len(lines)):
                assert M.sign((keys[i] > keys[j]) - (keys[i] < keys[j])) == M.key_cmp(lines[i], lines[j]), (name, lines[i], lines[j])


def test_host_form_refuses_what_the_header_says():
    from sedef_amd import report
    pool, recs, _ = report.line_records(TABLES["three_identical_spread"])
    for f, v in (("off", int(recs["off"][-1]) + 8), ("reserved", 1), ("len", len(pool) - int(recs["off"][-1]) + 1), ("off", len(pool) + 16)):
        bad = recs.copy()
        bad[f][-1] = v
        assert report.line_order_host(pool, bad)[0] == M.ERR_INVALID, (f, v)
    L = report._lib()
    o, f, k = np.zeros(8, np.uint32), np.zeros(8, np.uint32), np.zeros(1, np.uint64)
    args = (pool.ctypes.data, len(pool), recs.ctypes.data, len(recs), o.ctypes.data, f.ctypes.data, k.ctypes.data)
    assert L.sdf_line_order_host(*args) == 0 and int(k[0]) == 5
    for hole in (0, 2, 4, 5, 6):
        assert L.sdf_line_order_host(*(args[:hole] + (None,) + args[hole + 1:])) == M.ERR_INVALID
    assert L.sdf_line_order_host(*(args[:3] + ((1 << 30) + 1,) + args[4:])) == M.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        report.line_records([b"a\nb"])


def test_the_host_form_alone_under_the_address_and_undefined_sanitizers(tmp_path):
    """tests/line_order_main.cc: a program of its own around sdf_line_records and sdf_line_order_host, against the order written
    out in C++ on pools of exact size, its host side built with -fsanitize=address,undefined and run here, on the CPU."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src, exe = os.path.join(ROOT, "sedef_amd", "csrc"), str(tmp_path / "line_order")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-I", src,
                           os.path.join(src, "line_order.hip"), os.path.join(src, "sdf_report_api.hip"), "-x", "hip",
                           os.path.join(ROOT, "tests", "line_order_main.cc"), "-o", exe], stderr=subprocess.DEVNULL)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stdout == b"line order ok\n" and b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, \
        p.stderr.decode()[-2000:]


# ---- the command, as far as it goes without a device ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cli():
    from sedef_amd import host
    host.build_host()
    return host.CLI


def run(cli, args):
    p = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=dict(os.environ, SDF_REPORT_HOST="1"))
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def test_help_describes_report(cli):
    rc, out, err = run(cli, ["help"])
    assert rc == 0 and "sedef report [genome.fa]" in err and "SDF_REPORT_HOST=1" in err and "-k1,1V -k9,9r" in err


def test_argument_errors_of_the_command(cli, tmp_path):
    rc, _, err = run(cli, ["report", "genome.fa", str(tmp_path)])
    assert rc == 1 and "Not enough arguments to report" in err
    rc, _, err = run(cli, ["report", "genome.fa", str(tmp_path / "none"), str(tmp_path / "out")])
    assert rc == 1 and "none does not exist" in err
    os.makedirs(str(tmp_path / "empty"))
    (tmp_path / "empty" / "bucket_0000.log").write_text("x\n")
    rc, _, err = run(cli, ["report", "genome.fa", str(tmp_path / "empty"), str(tmp_path / "out")])
    assert rc == 1 and "No *.aligned.bed files in" in err and not os.path.exists(str(tmp_path / "out"))
