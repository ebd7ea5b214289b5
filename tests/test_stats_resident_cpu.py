"""CPU: what the stats calls on the resident pool promise without a GPU -- the two entry points are exported, the Python
constants are the header's, and the piece-to-range mapping of `stats generate` on resident chromosomes (host/stats.cc:
stats_piece_range; reference: src/align_main.cc:317-321) against a numpy model."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "sedef_hip.h")).read()


def test_library_exports_the_resident_stats_calls():
    from sedef_amd.build import build_library
    lib = ctypes.CDLL(build_library())
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("sdf_stats_columns_pairs", "sdf_stats_columns_pairs_device"):
        assert re.search(r"\b%s\s*\(" % name, src), name  # declared ...
        assert hasattr(lib, name), name                   # ... and exported
    import sedef_amd
    L = sedef_amd.load_library()  # bound by the mirror
    assert L.sdf_stats_columns_pairs.argtypes is not None and len(L.sdf_stats_columns_pairs.argtypes) == 6
    assert len(L.sdf_stats_columns_pairs_device.argtypes) == 7


def test_python_constants_equal_the_header():
    from sedef_amd.extz2 import STATS_A_RC, STATS_B_RC, STATS_TASK_DTYPE
    d = dict((m.group(1), int(m.group(2), 0)) for m in re.finditer(r"#define\s+(SDF_STATS_[AB]_RC)\s+(0x[0-9a-fA-F]+|\d+)", _header()))
    assert d == {"SDF_STATS_A_RC": STATS_A_RC, "SDF_STATS_B_RC": STATS_B_RC} and STATS_A_RC != STATS_B_RC
    # the bits travel in the word that was reserved: name, size and position as they were
    assert STATS_TASK_DTYPE.fields["reserved"] == (np.dtype("<u4"), 36) and STATS_TASK_DTYPE.itemsize == 40


def test_piece_range_against_a_numpy_model():
    """A piece covers columns [s, e) of a side that was fetched from [start, end) of its chromosome and, on the reverse
    strand, reverse-complemented: the model cuts the piece's bases out of the fetched string and finds them again in the
    chromosome -- forward as they are, reversed through the reverse complement of the range."""
    from sedef_amd import host
    host.build_host()
    rng = np.random.default_rng(41)
    chrom = rng.integers(0, 1 << 30, 5000)  # (distinct "bases": a range is found in one place only)
    comp = lambda x: -x - 1  # noqa: E731  an involution without fixed points stands for the complement
    cases = []
    for k in range(1000):
        start = int(rng.integers(0, 4000))
        end = int(rng.integers(start + 1, min(5000, start + 900) + 1))
        n = end - start
        s = int(rng.integers(0, n + 1))
        e = int(rng.integers(s, n + 1))
        if k % 50 == 0:
            e = s  # an empty piece
        if k % 50 == 1:
            s, e = 0, n  # the whole side
        cases.append((start, end, s, e, bool(k % 2)))
    assert any(c[2] == c[3] for c in cases) and any(c[2] == 0 and c[3] == c[1] - c[0] and c[4] for c in cases)
    for start, end, s, e, rc in cases:
        fetched = chrom[start:end]
        side = comp(fetched[::-1]) if rc else fetched
        piece = side[s:e]
        first, length = host.stats_piece_range(start, end, s, e, rc)
        assert length == e - s and 0 <= first and first + length <= len(chrom)
        back = chrom[first:first + length]
        assert np.array_equal(comp(back[::-1]) if rc else back, piece), (start, end, s, e, rc)
        assert first == (end - e if rc else start + s)
