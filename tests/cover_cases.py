"""Inputs of the coverage tests (test_pool_cover_cpu.py, test_gpu_pool_cover.py): one pool of sixteen regions with short
filler records between them, and the interval lists of every case.  PIECE is pool_cover.hip's kCoverPieceBytes."""
import numpy as np

PIECE = 8192
REGION_LENS = (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, PIECE - 1, PIECE, PIECE + 1, 70000, 100, 1000)
P0, P1 = 8, 9  # the two regions whose first 400 bytes hold exact uppercase counts (partner_cases)


def _region(rng, n):
    """Uppercase ACGT with lowercase stretches, an N run, an n run, R / Y letters and a few bytes of 128 and above."""
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    if n >= 31:
        for _ in range(max(1, n // 400)):
            at, m = int(rng.integers(0, n)), int(rng.integers(1, max(2, n // 8)))
            s[at:at + m] |= 0x20
        at = int(rng.integers(0, n - 8))
        s[at:at + 7] = ord("N")
        at = int(rng.integers(0, n - 8))
        s[at:at + 5] = ord("n")
        for c in b"RYry":
            s[rng.integers(0, n, max(1, n // 50))] = c
        s[rng.integers(0, n, max(1, n // 100))] = rng.integers(128, 256, max(1, n // 100))
    return s


def _partner_block(s):
    """bytes 0..99 uppercase, 100..199 lowercase, 200..298 uppercase, 299..399 lowercase."""
    s[0:100], s[100:200], s[200:299], s[299:400] = ord("A"), ord("c"), ord("G"), ord("t")


def build_pool(seed=77):
    """Returns (records, regions): the records to append in order -- regions and fillers -- as uint8 arrays, and the (off, len)
    of every region; region k lies at an offset of residue k mod 16."""
    rng = np.random.default_rng(seed)
    records, regions, at = [], [], 0
    for k, n in enumerate(REGION_LENS):
        pad = (k - at) % 16
        if k and pad == 0:
            pad = 16  # (a filler between any two regions)
        if pad:
            records.append(np.frombuffer(b"acgtNnRY", np.uint8)[rng.integers(0, 8, pad)].copy())
            at += pad
        s = _region(rng, n)
        if k in (P0, P1):
            _partner_block(s)
        records.append(s)
        regions.append((at, n))
        at += n
    assert sorted(off % 16 for off, _ in regions) == list(range(16))
    return records, regions


def upload(eng, records):
    """Every record as a FASTA record of one line behind the ones resident; returns the offsets."""
    offs = []
    for i, rec in enumerate(records):
        offs.append(eng.pool_append_fasta(rec.tobytes() + b"\n", len(rec), len(rec), len(rec) + 1, reset=i == 0))
    eng.pool_sync()
    return offs


def edge_case(regions):
    """Per region every interval shape that fits it; partner -1 (painted)."""
    iv = []
    for r, (_, n) in enumerate(regions):
        a, b = r & 1, 1 - (r & 1)
        shapes = [(n - 1, 1, a), (0, 0, a), (n, 0, b),               # the last base alone; len == 0 at both ends
                  (32, 32, a), (31, 34, b), (33, 30, a), (96, 64, b),  # on word boundaries, one bit off either side
                  (64 + 3, 5, a), (64 + 10, 7, a), (64 + 6, 9, b),      # two in one word that do not overlap; both sets in it
                  (200, 200, b), (250, 50, b), (200, 200, b), (400, 100, b), (500, 10, a), (510, 10, a),  # nested, identical, touching
                  (0, PIECE, a), (100, PIECE, b), (PIECE - 16, 32, a), (5, 2 * PIECE, b), (PIECE, 1, b), (3, 3 * PIECE + 1, a)]  # piece seams
        iv += [(r, s, m, which, -1) for s, m, which in shapes if s + m <= n]
    return iv


def whole_case(regions):
    """Every region whole in one set, its last base in the other."""
    iv = []
    for r, (_, n) in enumerate(regions):
        iv += [(r, 0, n, r & 1, -1), (r, n - 1, 1, 1 - (r & 1), -1)]
    return iv


def partner_case():
    """Pairs with 99 / 100, 100 / 99, 100 / 100 and 99 / 99 uppercase bytes, a partner in another region, and an interval
    without a partner and without an uppercase byte.  Returns (intervals, expected upper, expected painted)."""
    x100, x99 = (0, 150), (200, 150)
    iv, up, pa = [], [], []
    for (a, ua), (b, ub), rb in ((x99, 99), (x100, 100), P0), ((x100, 100), (x99, 99), P0), ((x100, 100), (x100, 100), P1), ((x99, 99), (x99, 99), P0):
        at = len(iv)
        iv += [(P0, a[0], a[1], 0, at + 1), (rb, b[0], b[1], 0, at)]
        up += [ua, ub]
        pa += [int(ua >= 100 and ub >= 100)] * 2
    iv.append((P1, 100, 50, 1, -1))
    up.append(0)
    pa.append(1)
    iv.append((P1, 0, 100, 1, 0))  # a one-way partner: 100 here, 99 there
    up.append(100)
    pa.append(0)
    return iv, up, pa


def random_case(regions, seed, per_region=6):
    rng = np.random.default_rng(seed)
    iv = []
    for r, (_, n) in enumerate(regions):
        for _ in range(per_region):
            s = int(rng.integers(0, n))
            iv.append((r, s, int(rng.integers(0, n - s + 1)), int(rng.integers(0, 2)), -1))
    for i in range(len(iv)):  # a third with a partner anywhere
        if rng.random() < 0.33:
            iv[i] = iv[i][:4] + (int(rng.integers(0, len(iv))),)
    return iv
