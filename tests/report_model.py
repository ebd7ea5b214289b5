"""The order of `sedef report`, as plain Python: what

    LC_ALL=C sort -k1,1V -k9,9r -k10,10r -k4,4V -k2,2n -k3,3n -k5,5n -k6,6n | uniq

(reference sedef.sh:218-229) does with lines, taken literally from the coreutils manual: no -t, so a field ends where a
non-blank is followed by a blank and keeps its leading blanks; V is version order, the bare r fields are byte strings reversed,
n is the number in front; equal keys fall back to the whole lines' bytes, the shorter first; uniq drops a line equal to the one
before it.  Lines are bytes without their newline.

`filevercmp` is this file's own restatement of the manual's "version sort" section: runs of
non-digits compare character by character in the order '~' < end of string < letters < every other byte; runs of digits by
value; a file suffix (\\.[A-Za-z~][A-Za-z0-9~]*)*$ is set aside unless the strings are equal without it; "" , "." and ".." and
names with a leading '.' come first; strings that still compare equal fall back to byte order.  Names with two dots in a row
or a dot at their end were not compared against the tool and are no part of the case tables."""
import functools
import re
from fractions import Fraction

DUP, WIDE, RUN = 1, 2, 64
ERR_UNSUPPORTED, ERR_INVALID = -3, -4
KEY_FIELDS = (1, 9, 10, 4, 2, 3, 5, 6)
BLANK = b" \t"
SUFFIX = re.compile(rb"(\.[A-Za-z~][A-Za-z0-9~]*)*\Z")


def sign(x):
    return (x > 0) - (x < 0)


GROUP = re.compile(rb"[ \t]*[^ \t]*")


@functools.lru_cache(maxsize=1 << 16)
def _fields(line):
    out, at = [], 0
    for _ in range(10):
        m = GROUP.match(line, at)
        out.append(m.group())
        at = m.end()
    return tuple(out)


def field(line, k):
    """Field k (1 .. 10): behind k - 1 groups of blanks-then-non-blanks, the k-th group, its leading blanks included; b"" when
    there is none."""
    return _fields(line)[k - 1]


def _char_order(c):
    if c is None or 48 <= c <= 57:
        return 0
    if 65 <= c <= 90 or 97 <= c <= 122:
        return c
    return -1 if c == 126 else c + 256


def _ver_body(a, b):
    i = j = 0
    while i < len(a) or j < len(b):
        while (i < len(a) and not 48 <= a[i] <= 57) or (j < len(b) and not 48 <= b[j] <= 57):
            x, y = _char_order(a[i] if i < len(a) else None), _char_order(b[j] if j < len(b) else None)
            if x != y:
                return sign(x - y)
            i, j = i + 1, j + 1
        da, db = i, j
        while i < len(a) and 48 <= a[i] <= 57:
            i += 1
        while j < len(b) and 48 <= b[j] <= 57:
            j += 1
        x, y = int(a[da:i] or b"0"), int(b[db:j] or b"0")
        if x != y:
            return sign(x - y)
    return 0


def filevercmp(a, b):
    if a == b:
        return 0
    simple = -1 if a < b else 1
    for first in (b"", b".", b".."):
        if a == first:
            return -1
        if b == first:
            return 1
    if a.startswith(b".") != b.startswith(b"."):
        return -1 if a.startswith(b".") else 1
    if a.startswith(b"."):
        a, b = a[1:], b[1:]
    ca, cb = a[:SUFFIX.search(a).start()], b[:SUFFIX.search(b).start()]
    r = _ver_body(a, b) if ca == cb else _ver_body(ca, cb)
    return r or simple


NUMBER = re.compile(rb"[ \t]*(-?)([0-9]*)(?:(\.)([0-9]*))?")


def number(f):
    """The value `sort -n` reads in front of a field: blanks, an optional '-', digits, an optional point and digits."""
    m = NUMBER.match(f)
    whole, frac = m.group(2), m.group(4) or b""
    v = Fraction(int(whole or b"0")) + (Fraction(int(frac), 10 ** len(frac)) if frac else 0)
    return -v if m.group(1) else v


def number_is_plain(f):
    """What the records take as a value: no sign and no point in front, at most ten digits, below 2^32."""
    m = NUMBER.match(f)
    rest = f[m.start(2):]
    return not m.group(1) and not m.group(3) and not rest.startswith(b".") and len(m.group(2)) <= 10 and int(m.group(2) or b"0") < 2 ** 32


def plain(lines):
    return all(number_is_plain(field(x, k)) for x in lines for k in (2, 3, 5, 6))


def bytes_cmp(a, b):
    return (a > b) - (a < b)  # (bytes compare unsigned, a prefix first: memcmp and then the lengths)


@functools.lru_cache(maxsize=1 << 16)
def _key_parts(line):
    return tuple(number(field(line, k)) if k in (2, 3, 5, 6) else field(line, k) for k in KEY_FIELDS)


def key_cmp(a, b):
    """The eight keys of two lines, in order; 0 when all are equal."""
    for k, fa, fb in zip(KEY_FIELDS, _key_parts(a), _key_parts(b)):
        if k in (1, 4):
            c = filevercmp(fa, fb)
        elif k in (9, 10):
            c = -bytes_cmp(fa, fb)
        else:
            c = sign(fa - fb)
        if c:
            return c
    return 0


def line_cmp(a, b):
    return key_cmp(a, b) or bytes_cmp(a, b)


def line_order(lines):
    """-> (order, flags, n_kept) as include/sedef_hip.h: sdf_line_order defines them."""
    order = sorted(range(len(lines)), key=functools.cmp_to_key(lambda i, j: line_cmp(lines[i], lines[j]) or i - j))
    flags = [DUP if p and lines[order[p]] == lines[order[p - 1]] else 0 for p in range(len(order))]
    p = 0
    while p < len(order):
        hi = p + 1
        while hi < len(order) and key_cmp(lines[order[p]], lines[order[hi]]) == 0:
            hi += 1
        if hi - p > RUN:
            for q in range(p, hi):
                flags[q] |= WIDE
        p = hi
    return order, flags, sum(1 for f in flags if not f & DUP)


def sort_uniq(lines):
    """The lines `sort ... | uniq` prints."""
    order, flags, _ = line_order(lines)
    return [lines[i] for i, f in zip(order, flags) if not f & DUP]


def sort_uniq_text(text):
    """The same on a file's bytes (a last line without a newline gets one, as sort gives it)."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return b"".join(x + b"\n" for x in sort_uniq(lines))
