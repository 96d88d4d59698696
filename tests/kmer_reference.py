"""Plain-Python truth of the k-mer calls (include/caps_sa_hip.h "k-mers from SA and LCP"), from the definitions and nothing of the
library: collections.Counter over the text for the table and the spectrum, the per-rank rule for the census."""
from collections import Counter

import numpy as np


def _bytes(T) -> bytes:
    return T if isinstance(T, bytes) else np.ascontiguousarray(T, dtype=np.uint8).tobytes()


def signed_key(b: bytes) -> bytes:
    """Sort key of the library's byte order: bytes as signed char (0x80 .. 0xFF before 0x00 .. 0x7F)."""
    return bytes(x ^ 0x80 for x in b)


def table(T, k: int, min_count: int = 1, max_count: int = 0):
    """[(k-mer bytes, count)] in signed-char order, min_count <= count (<= max_count unless that is 0)."""
    t = _bytes(T)
    n = len(t)
    c = Counter(t[i:i + k] for i in range(n - k + 1)) if 1 <= k <= n else Counter()
    lo = max(min_count, 1)
    return [(m, c[m]) for m in sorted(c, key=signed_key) if c[m] >= lo and (max_count == 0 or c[m] <= max_count)]


def positions(T, kmer: bytes):
    t = _bytes(T)
    out, at = [], t.find(kmer)
    while at >= 0:
        out.append(at)
        at = t.find(kmer, at + 1)
    return out


def spectrum(T, k: int, bins: int) -> np.ndarray:
    hist = np.zeros(bins + 1, dtype=np.uint64)
    for _, c in table(T, k):
        hist[min(c, bins)] += 1
    return hist


def census_by_counter(T, max_k: int):
    distinct = np.zeros(max_k + 1, dtype=np.uint64)
    unique = np.zeros(max_k + 1, dtype=np.uint64)
    for k in range(1, max_k + 1):
        tab = table(T, k)
        distinct[k] = len(tab)
        unique[k] = sum(1 for _, c in tab if c == 1)
    return distinct, unique


def census_by_rank(SA, LCP, max_k: int):
    """The per-rank rule: rank i adds 1 to distinct[k] for a < k <= b and to unique[k] for a' < k <= b."""
    sa = np.asarray(SA).astype(np.int64)
    lcp = np.asarray(LCP).astype(np.int64)
    n = sa.size
    dd = np.zeros(max_k + 2, dtype=np.int64)
    du = np.zeros(max_k + 2, dtype=np.int64)
    if n:
        a = lcp.copy()
        a[0] = 0
        nxt = np.zeros(n, dtype=np.int64)
        nxt[:-1] = lcp[1:]
        a2 = np.maximum(a, nxt)
        b = np.where(sa < n, n - sa, 0)
        for lo, diff in ((a, dd), (a2, du)):
            ok = lo < b
            np.add.at(diff, np.minimum(lo[ok] + 1, max_k + 1), 1)
            np.add.at(diff, np.minimum(b[ok] + 1, max_k + 1), -1)
    distinct = np.cumsum(dd)[:max_k + 1]
    unique = np.cumsum(du)[:max_k + 1]
    distinct[0] = unique[0] = 0
    return distinct.astype(np.uint64), unique.astype(np.uint64)
