"""Recorded answers of the reference's own code for the tests that compare this repository's code with it on seeded inputs.

Those tests used to call the reference live (oracle/_ref, compiled from a reference checkout) and skipped where it was not
built.  `ref_calls(name, make_live)` gives them an object with the same methods whose answers come from
tests/golden/ref_calls/<name>.json.gz, in call order; every call is checked against a digest of its arguments (a path
to an existing file counts by the file's contents), so a test whose inputs drift fails instead of comparing against
the wrong answers.  Where the reference is built (`make_live()` returns an object) every call also goes to it and both
answers must agree: a stale recording fails too.

SDF_RECORD_REF_CALLS=1 (with the reference built) writes the recordings instead:
    SDF_RECORD_REF_CALLS=1 python -m pytest tests -m "not gpu" -k "live or oracle_vs_ref"
"""
import gzip
import hashlib
import json
import os

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_calls")


def encode(x):
    """A JSON form of an answer or an argument that keeps the types apart (tuple / list, array dtype and shape)."""
    if isinstance(x, np.ndarray):
        return {"a": [x.dtype.str, list(x.shape), x.reshape(-1).tolist()]}
    if isinstance(x, np.generic):
        return encode(x.item())
    if isinstance(x, tuple):
        return {"t": [encode(v) for v in x]}
    if isinstance(x, list):
        return [encode(v) for v in x]
    if isinstance(x, dict):
        return {"d": [[encode(k), encode(v)] for k, v in x.items()]}
    if isinstance(x, bytes):
        return {"b": x.hex()}
    if isinstance(x, float):
        return {"f": repr(x)}  # (exact, NaN and infinities included)
    if x is None or isinstance(x, (bool, int, str)):
        return x
    raise TypeError("ref_calls: cannot record a %s" % type(x).__name__)


def decode(x):
    if isinstance(x, list):
        return [decode(v) for v in x]
    if not isinstance(x, dict):
        return x
    (tag, v), = x.items()
    if tag == "a":
        return np.array(v[2], dtype=np.dtype(v[0])).reshape(v[1])
    if tag == "t":
        return tuple(decode(e) for e in v)
    if tag == "d":
        return {decode(k): decode(e) for k, e in v}
    if tag == "b":
        return bytes.fromhex(v)
    return float(v)


def _digest(name, args, kwargs):
    def arg(a):
        if isinstance(a, str) and len(a) < 4096 and os.path.isfile(a):
            with open(a, "rb") as f:
                return {"file": hashlib.sha256(f.read()).hexdigest()}
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            return {"a": [a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()]}
        if isinstance(a, (tuple, list)):
            return [arg(v) for v in a]
        return encode(a)
    text = json.dumps([name, [arg(a) for a in args], sorted((k, arg(v)) for k, v in kwargs.items())], sort_keys=True)
    return hashlib.sha256(text.encode()).hexdigest()[:16]


class _Calls:
    def __init__(self, name, live, record):
        self._name, self._live, self._record, self._pos = name, live, record, 0
        self._path = os.path.join(DIR, name + ".json.gz")
        if record:
            self._calls = []
        else:
            with gzip.open(self._path, "rb") as f:
                self._calls = json.loads(f.read().decode())

    def __getattr__(self, method):
        if method.startswith("_"):
            raise AttributeError(method)

        def call(*args, **kwargs):
            key = _digest(method, args, kwargs)
            if self._record:
                got = getattr(self._live, method)(*args, **kwargs)
                self._calls.append([method, key, encode(got)])
                return got
            assert self._pos < len(self._calls), "%s: more calls than recorded" % self._name
            m, k, enc = self._calls[self._pos]
            self._pos += 1
            assert (m, k) == (method, key), "%s: call %d is %s with other arguments than recorded" % (
                self._name, self._pos - 1, method)
            if self._live is not None:
                assert encode(getattr(self._live, method)(*args, **kwargs)) == enc, \
                    "%s: the live reference disagrees with the recording at call %d" % (self._name, self._pos - 1)
            return decode(enc)
        return call

    def _finish(self):
        if self._record:
            os.makedirs(DIR, exist_ok=True)
            with gzip.GzipFile(self._path, "wb", mtime=0) as f:
                f.write(json.dumps(self._calls, separators=(",", ":")).encode())
        else:
            assert self._pos == len(self._calls), "%s: %d of %d recorded calls made" % (self._name, self._pos,
                                                                                       len(self._calls))


def ref_calls(name, make_live):
    """The recorded reference for one test (see the module's text).  Use as a context manager: on a clean exit it checks
    that every recorded call was made (or writes the recording)."""
    try:
        live = make_live()
    except Exception:  # noqa: BLE001  (not built, and no checkout to build it from)
        live = None
    record = os.environ.get("SDF_RECORD_REF_CALLS") == "1"
    if record and live is None:
        raise RuntimeError("SDF_RECORD_REF_CALLS=1 needs the reference built (oracle/_ref)")
    return _Recording(_Calls(name, live, record))


class _Recording:
    def __init__(self, calls):
        self.calls = calls

    def __enter__(self):
        return self.calls

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.calls._finish()
        return False
