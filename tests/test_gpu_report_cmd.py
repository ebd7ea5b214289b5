"""GPU: `sedef report` as a child process (report_cmd.cc over sdf_line_order and stats_generate) on a small genome and three
overlapping *.aligned.bed files (tests/report_cmd_gen.py): aligned.bed and final.bed equal, byte for byte, the files of the
SDF_REPORT_HOST=1 run, what the model (tests/report_model.py) makes of the buckets and of `stats generate`'s own output, and --
where `sort` is GNU's -- the literal pipeline of sedef.sh:220-229 on the same files."""
import os
import subprocess
import sys

import pytest
import torch  # noqa: F401  (at collection: before the library brings a HIP runtime of its own along)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import report_cmd_gen as G  # noqa: E402
import report_model as M  # noqa: E402

pytestmark = pytest.mark.gpu


def run(cli, args, env=None):
    e = {k: v for k, v in os.environ.items() if k != "SDF_REPORT_HOST"}
    e.update(env or {})
    p = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e)
    return p.returncode, p.stdout, p.stderr.decode()


def gnu_sort():
    try:
        return b"GNU coreutils" in subprocess.run(["sort", "--version"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=30).stdout
    except OSError:
        return False


def pipeline(text):
    """`sort -k1,1V ... | uniq` under LC_ALL=C, the tool itself"""
    p = subprocess.run("sort %s | uniq" % G.KEYS, shell=True, input=text, stdout=subprocess.PIPE, timeout=60, env=dict(os.environ, LC_ALL="C"))
    assert p.returncode == 0
    return p.stdout


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from sedef_amd import host
    host.build_host()
    folder = str(tmp_path_factory.mktemp("report"))
    fasta, align = G.write_inputs(folder)
    out = {}
    for mode, env in (("device", {}), ("host", {"SDF_REPORT_HOST": "1"})):
        out_dir = os.path.join(folder, "out_" + mode)
        rc, _, err = run(host.CLI, ["report", fasta, align, out_dir], env)
        assert rc == 0, err[-2000:]
        out[mode] = (open(os.path.join(out_dir, "aligned.bed"), "rb").read(), open(os.path.join(out_dir, "final.bed"), "rb").read(), err)
    # the same from the files named one by one, in another order
    files = sorted(os.path.join(align, f) for f in G.bucket_files())[::-1]
    out_dir = os.path.join(folder, "out_files")
    rc, _, err = run(host.CLI, ["report", fasta] + files + [out_dir])
    assert rc == 0, err[-2000:]
    out["files"] = (open(os.path.join(out_dir, "aligned.bed"), "rb").read(), open(os.path.join(out_dir, "final.bed"), "rb").read(), err)
    rc, table, err = run(host.CLI, ["stats", "generate", fasta, os.path.join(folder, "out_device", "aligned.bed")])
    assert rc == 0, err[-2000:]
    return out, "".join(G.bucket_files().values()).encode(), table


def test_device_run_equals_the_host_run(runs):
    out, _, _ = runs
    assert out["device"][:2] == out["host"][:2] == out["files"][:2]
    aligned, final, err = out["device"]
    assert aligned.count(b"\n") == 7 and final.count(b"\n") >= 7 and final.endswith(b"\n")
    assert "Report: 7 lines in" in err and "%d lines in" % final.count(b"\n") in err
    assert "ordered on the host" not in err


def test_both_files_equal_the_model(runs):
    out, cat, table = runs
    aligned, final, _ = out["device"]
    assert aligned == M.sort_uniq_text(cat)
    assert table.startswith(b"#chr1\t") and table.count(b"\n") >= 8
    assert final == M.sort_uniq_text(table)
    assert final.splitlines()[-1].startswith(b"#chr1\t")  # (version order puts '#' behind the letters: the header ends the file)


def test_both_files_equal_the_literal_pipeline(runs):
    if not gnu_sort():
        pytest.skip("sort is not GNU coreutils")
    out, cat, table = runs
    aligned, final, _ = out["device"]
    assert aligned == pipeline(cat) and final == pipeline(table)


def test_a_decimal_point_in_a_number_column_takes_the_host_path_and_says_so(tmp_path):
    """No SDF_REPORT_HOST: the command itself sends the buckets' lines to the host form, in one line on stderr; the stats table,
    whose number columns are plain, stays on the device.  Both files as the model and the tool order them."""
    from sedef_amd import host
    host.build_host()
    folder = str(tmp_path)
    fasta, _ = G.write_inputs(folder)
    bucket, out_dir = os.path.join(folder, "decimal.aligned.bed"), os.path.join(folder, "out")
    with open(bucket, "w") as f:
        f.write(G.decimal_bucket())
    cat = G.decimal_bucket().encode()
    assert not M.plain(cat.split(b"\n")[:-1])
    rc, _, err = run(host.CLI, ["report", fasta, bucket, out_dir])
    assert rc == 0, err[-2000:]
    said = [x for x in err.splitlines() if "ordered on the host" in x]
    assert len(said) == 1 and "the aligned buckets" in said[0] and "decimal point" in said[0]
    aligned, final = (open(os.path.join(out_dir, n), "rb").read() for n in ("aligned.bed", "final.bed"))
    assert aligned == M.sort_uniq_text(cat) and aligned.count(b"\n") == 3
    assert aligned.splitlines()[0].split(b"\t")[1] == b"200"  # (200 sorts in front of 200.5: the order reads the fraction)
    rc, table, err = run(host.CLI, ["stats", "generate", fasta, os.path.join(out_dir, "aligned.bed")])
    assert rc == 0, err[-2000:]
    assert final == M.sort_uniq_text(table) and final.count(b"\n") >= 3
    if gnu_sort():
        assert aligned == pipeline(cat) and final == pipeline(table)
    # the same files from the host run, which has nothing to say
    rc, _, err = run(host.CLI, ["report", fasta, bucket, os.path.join(folder, "out_host")], {"SDF_REPORT_HOST": "1"})
    assert rc == 0 and "ordered on the host" not in err
    assert (aligned, final) == tuple(open(os.path.join(folder, "out_host", n), "rb").read() for n in ("aligned.bed", "final.bed"))
