"""Line order: sdf_line_order_device, sdf_line_order, sdf_line_order_host and `LC_ALL=C sort ... | uniq` once each, in one
process, on synthetic lines of `align generate`'s shape -- 200 to 4,000 bytes, the CIGAR column taking the length --, 30% of them
copies of another line in runs of 2 to 8, shuffled.  Per form: a warm-up call, then the seconds of one call (a host clock around
a call that has returned; the `_device` form is followed by a wait on the context's stream and times neither the uploads nor
the copy back; the parse, sdf_line_records, is timed on its own and is part of none).  The share of lines in WIDE runs is
reported with them.  A record, not a gate: nobody fixed a ratio in advance.  To be run by hand under a time limit.

    python profiles/report_order.py [--out FILE] [--lines 400000]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = "-k1,1V -k9,9r -k10,10r -k4,4V -k2,2n -k3,3n -k5,5n -k6,6n"


def make_lines(rng, n):
    chroms = [b"chr%d" % c for c in range(1, 23)] + [b"chrX", b"chrY"]
    lines, filler = [], bytes(rng.integers(48, 58, 4096, dtype=np.uint8))
    while len(lines) < n:
        c1, c2 = chroms[int(rng.integers(0, 24))], chroms[int(rng.integers(0, 24))]
        s1, s2, ln = int(rng.integers(0, 150 * 10 ** 6)), int(rng.integers(0, 150 * 10 ** 6)), int(rng.integers(1000, 30000))
        head = b"%s\t%d\t%d\t%s\t%d\t%d\t\t%.1f\t+\t%s\t%d\t%d\t" % (c1, s1, s1 + ln, c2, s2, s2 + ln, ln * 0.9, b"+-"[int(rng.integers(0, 2)):][:1], ln, ln)
        size = int(rng.integers(200, 4001))
        at = int(rng.integers(0, 64))
        line = head + (filler[at:] + filler)[:max(1, size - len(head) - 1)].replace(b"0", b"M") + b"M"
        copies = int(rng.integers(2, 9)) if rng.random() < 0.3 / 3.5 else 1  # (runs of 2 to 8, 4 extra copies on average: 30% of the lines)
        lines += [line] * copies
    lines = lines[:n]
    return [lines[i] for i in rng.permutation(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_order.txt"))
    ap.add_argument("--lines", type=int, default=400000)
    a = ap.parse_args()
    import torch
    import sedef_amd
    from sedef_amd import report
    out = []

    def say(text):
        out.append(text)
        print(text, flush=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")

    lines = make_lines(np.random.default_rng(2026), a.lines)
    t0 = time.perf_counter()
    pool, recs, plain = report.line_records(lines)
    t_parse = time.perf_counter() - t0
    assert plain
    say("line order (profiles/report_order.py): %d lines of 200 to 4,000 bytes, %d bytes in the pool; GPU_MAX_HW_QUEUES=%s"
        % (len(lines), len(pool), os.environ.get("GPU_MAX_HW_QUEUES", "unset")))
    say("%-24s %.4f s (the parse in front of every form; part of none of the figures below)" % ("sdf_line_records", t_parse))
    eng = sedef_amd.Extz2Engine(0)
    d_pool, d_recs = torch.from_numpy(pool).cuda(), torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).cuda()
    d_order, d_flags = torch.zeros(len(recs), dtype=torch.int32, device="cuda"), torch.zeros(len(recs), dtype=torch.int32, device="cuda")
    d_counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def device_call():
        report.line_order_device(eng, d_pool.data_ptr(), len(pool), d_recs.data_ptr(), len(recs), d_order.data_ptr(), d_flags.data_ptr(),
                                 d_counts.data_ptr())
        eng.pool_sync()

    forms = {"sdf_line_order_device": device_call, "sdf_line_order": lambda: report.line_order(eng, pool, recs),
             "sdf_line_order_host": lambda: report.line_order_host(pool, recs)}
    rc, order, flags, kept = forms["sdf_line_order_host"]()  # (warm-up of the host form, and the answer)
    assert rc == 0
    got = forms["sdf_line_order"]()
    assert got[0].tobytes() == order.tobytes() and got[1].tobytes() == flags.tobytes() and got[2] == kept
    device_call()
    wide = (flags & report.WIDE) != 0
    dev_order, dev_flags = d_order.cpu().numpy().view(np.uint32), d_flags.cpu().numpy().view(np.uint32)
    assert dev_order[~wide].tobytes() == order[~wide].tobytes() and dev_flags[~wide].tobytes() == flags[~wide].tobytes()
    say("lines kept: %d of %d; lines in WIDE runs (more than %d lines of equal keys): %d = %.3f%%"
        % (kept, len(lines), report.RUN, int(wide.sum()), 100.0 * wide.sum() / max(1, len(lines))))
    secs = {}
    for name, f in forms.items():
        t0 = time.perf_counter()
        f()
        secs[name] = time.perf_counter() - t0
        say("%-24s %.4f s" % (name, secs[name]))
    text = b"".join(x + b"\n" for x in lines)
    env = dict(os.environ, LC_ALL="C")
    for _ in range(2):  # (a warm-up, then the one that counts)
        t0 = time.perf_counter()
        p = subprocess.run("sort %s | uniq" % KEYS, shell=True, input=text, stdout=subprocess.PIPE, env=env)
        secs["sort | uniq"] = time.perf_counter() - t0
    assert p.returncode == 0 and p.stdout == b"".join(lines[i] + b"\n" for i, f in zip(order.tolist(), flags.tolist()) if not f & report.DUP)
    say("%-24s %.4f s (LC_ALL=C, the text through a pipe, the tool's own threads)" % ("sort | uniq", secs["sort | uniq"]))
    say("sort | uniq / sdf_line_order_device: %.1f; / sdf_line_order (uploads and copy back included): %.1f; / sdf_line_order_host: %.1f"
        % tuple(secs["sort | uniq"] / secs[k] for k in ("sdf_line_order_device", "sdf_line_order", "sdf_line_order_host")))


if __name__ == "__main__":
    main()
