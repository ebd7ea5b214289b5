"""Drawn genomes for the tests of the resident search index and of `sedef search`: records of random bases with planted,
diverged copies (one may be inverted), lowercase stretches and an N run; their FASTA text with a .fai; and the Python
statements the command's tests compare with -- the BED line of a search hit, generate_translation, the pair loop."""
import numpy as np

COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rev_comp(s):
    return s.translate(COMP)[::-1]


def mutate(rng, s, rate):
    """Substitutions at `rate`, and an insertion or a deletion of one base at a tenth of it."""
    out = bytearray()
    for c in s:
        x = rng.random()
        if x < rate:
            out.append(b"ACGT"[(b"ACGT".index(c) + int(rng.integers(1, 4))) % 4])
        elif x < rate * 1.05:
            continue
        elif x < rate * 1.10:
            out.append(c)
            out.append(b"ACGT"[int(rng.integers(0, 4))])
        else:
            out.append(c)
    return bytes(out)


def records(seed, lens, copies, lower=(), n_runs=()):
    """lens: the records' lengths.  copies: (source record, source start, length, target record, target start, divergence,
    inverted) -- written over the target's bases in this order.  lower: (record, start, length) stretches made lowercase;
    n_runs: the same made N."""
    rng = np.random.default_rng(seed)
    recs = [bytearray(bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, n))) for n in lens]
    for src, s0, n, dst, d0, rate, inverted in copies:
        piece = mutate(rng, bytes(recs[src][s0:s0 + n]), rate)
        if inverted:
            piece = rev_comp(piece)
        piece = piece[:len(recs[dst]) - d0]
        recs[dst][d0:d0 + len(piece)] = piece
    for r, s0, n in lower:
        recs[r][s0:s0 + n] = bytes(recs[r][s0:s0 + n]).lower()
    for r, s0, n in n_runs:
        recs[r][s0:s0 + n] = b"N" * n
    return [bytes(r) for r in recs]


def write_fasta(path, names, recs, widths, last_newline=False):
    """The records as FASTA with line widths widths[i]; the file's last line ends without a newline unless asked; the .fai
    beside it."""
    text, fai = b"", []
    for i, (name, rec, width) in enumerate(zip(names, recs, widths)):
        text += b">" + name.encode() + b"\n"
        off = len(text)
        lines = [rec[j:j + width] for j in range(0, len(rec), width)]
        text += b"\n".join(lines)
        if i + 1 < len(recs) or last_newline:
            text += b"\n"
        fai.append("%s\t%d\t%d\t%d\t%d" % (name, len(rec), off, width, width + 1))
    with open(path, "wb") as f:
        f.write(text)
    with open(path + ".fai", "w") as f:
        f.write("\n".join(fai) + "\n")


def hit_bed(qname, rname, qs, qe, rs, re_, ref_rc=False, ref_len=0):
    """Hit::to_bed() of a search hit (src/hit.cc:134-196): no name, no alignment, comment OK; under ref_rc the reference's
    coordinates are flipped by its length, with the reference's + 1."""
    maxlen = max(qe - qs, re_ - rs)  # (of the ends as the search reports them)
    if ref_rc:
        as_int = lambda v: (v + 2 ** 31) % 2 ** 32 - 2 ** 31  # noqa: E731  (size_t arithmetic brought to an int)
        rs, re_ = as_int(ref_len - re_ + 1), as_int(ref_len - rs + 1)
    return "%s\t%d\t%d\t%s\t%d\t%d\t\t\t+\t%s\t%d\t0\t\t;OK" % (qname, qs, qe, rname, rs, re_, "-" if ref_rc else "+", maxlen)


def translation_model(recs, max_size):
    """generate_translation (src/search_main.cc:93-120) over (length, name) pairs: descending by (length, name); a new group
    when the running size -- a 32-bit int -- plus the record would exceed max_size."""
    groups, cur = [], 0
    for length, name in sorted(recs, reverse=True):
        if not groups or (cur % 2 ** 64 + length) % 2 ** 64 > max_size:
            groups.append([name])
            cur = length
        else:
            groups[-1].append(name)
            cur += length
        cur = (cur + 2 ** 31) % 2 ** 32 - 2 ** 31
    return groups


def expected_search(extz2, names, recs, qr, rr, reverse, limit, k=12, w=16, min_uppercase=12, max_error=0.30, max_edit_error=0.15,
                    gap_frequency=0.005):
    """What `sedef search` prints for the chromosomes qr against rr: sdf_search_pair_host per pair, r outer and q inner, on
    a pool of the two records, and the BED model above.  Returns the text."""
    by_name = dict(zip(names, recs))
    min_read_size = int(1000 * (1 - max_error))
    out = []
    for r in rr:
        for q in qr:
            same = q == r and not reverse
            pool = by_name[q] if same else by_name[q] + by_name[r]
            q_range = (0, len(by_name[q]), 0)
            r_range = q_range if same else (len(by_name[q]), len(by_name[r]), 1 if reverse else 0)
            rc, hits, used, stats = extz2.search_pair_host(
                pool, q_range, r_range, k=k, w=w, min_read_size=min_read_size, same_genome=same, limit=limit,
                filter=extz2.filter_params(min_uppercase, max_error, max_edit_error, gap_frequency),
                extend=extz2.extend_params(max_error, max_edit_error, same_genome=same))
            assert rc == 0, rc
            for h in hits:
                out.append(hit_bed(q, r, int(h["query_start"]), int(h["query_end"]), int(h["ref_start"]), int(h["ref_end"]), reverse,
                                   len(by_name[r])))
    return "".join(line + "\n" for line in out)
