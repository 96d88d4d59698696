"""What the kernel-level entry points (include/caps_sa_hip.h: sort_suffixes, sort_segments, merge, upper_bound, lcp) must answer, in
plain numpy.  Shares nothing with csrc/ or oracle/: the order of the suffixes is the inverse of the suffix array that
sa_check.sa_lcp builds by prefix doubling (not quadratic on periodic texts, as the oracle is), and an LCP is the first index at which
two slices of the text differ.  Order: bytes as signed char, the shorter suffix first -- test_emul_kernel_entry.py ties that to the
oracle's lcp / merge_sort / merge / upper_bound on two small texts."""
import numpy as np

from sa_check import sa_lcp


def rank(T) -> np.ndarray:
    """rank[x] = the place of suffix x among all suffixes of T."""
    sa, _ = sa_lcp(T, 64)
    r = np.empty(sa.size, dtype=np.int64)
    r[sa.astype(np.int64)] = np.arange(sa.size, dtype=np.int64)
    return r


def lcp(T, x: int, y: int) -> int:
    """The definition: n - x for x == y, else the first index at which T[x : x + m] and T[y : y + m] differ, m = n - max(x, y); m if
    there is none."""
    T = np.asarray(T, dtype=np.uint8)
    n = int(T.size)
    if x == y:
        return n - x
    m = n - max(x, y)
    d = np.nonzero(T[x:x + m] != T[y:y + m])[0]
    return int(d[0]) if d.size else m


class Reference:
    """rank and LCPs of one text, computed once.  lcps(a, b) answers many pairs at once: the LCP of two suffixes is the minimum of
    the text's LCP array between their ranks (a sparse table of minima over it); `lcp` above is the definition it is checked
    against (check_against_definition, and every caller may sample it)."""

    def __init__(self, T):
        self.T = np.ascontiguousarray(np.asarray(T, dtype=np.uint8))
        self.n = int(self.T.size)
        sa, l = sa_lcp(self.T, 64)
        self.sa = sa.astype(np.int64)
        self.lcp_array = l.astype(np.int64)
        self.rank = np.empty(self.n, dtype=np.int64)
        self.rank[self.sa] = np.arange(self.n, dtype=np.int64)
        self._levels = [self.lcp_array]
        k = 1
        while 2 * k <= self.n:
            prev = self._levels[-1]
            self._levels.append(np.minimum(prev[:-k], prev[k:]))
            k *= 2

    def lcps(self, a, b) -> np.ndarray:
        a = np.asarray(a, dtype=np.int64)
        b = np.asarray(b, dtype=np.int64)
        out = np.empty(a.size, dtype=np.int64)
        same = a == b
        out[same] = self.n - a[same]
        ra, rb = self.rank[a[~same]], self.rank[b[~same]]
        lo, hi = np.minimum(ra, rb) + 1, np.maximum(ra, rb)          # minimum of lcp_array[lo .. hi]
        if lo.size:
            j = np.floor(np.log2(hi - lo + 1)).astype(np.int64)
            res = np.empty(lo.size, dtype=np.int64)
            for lev in np.unique(j).tolist():
                m = j == lev
                t = self._levels[lev]
                res[m] = np.minimum(t[lo[m]], t[hi[m] - (1 << lev) + 1])
            out[~same] = res
        return out

    def check_against_definition(self, a, b):
        for x, y, l in zip(np.asarray(a).tolist(), np.asarray(b).tolist(), self.lcps(a, b).tolist()):
            assert l == lcp(self.T, x, y), (x, y, l)

    def neighbour_lcps(self, s) -> np.ndarray:
        """0 at the head, the LCP of neighbours elsewhere."""
        s = np.asarray(s, dtype=np.int64)
        out = np.zeros(s.size, dtype=np.int64)
        if s.size > 1:
            out[1:] = self.lcps(s[:-1], s[1:])
        return out

    def sort_suffixes(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        s = idx[np.argsort(self.rank[idx], kind="stable")]
        return s, self.neighbour_lcps(s)

    def merge(self, X, Y):
        return self.sort_suffixes(np.concatenate([np.asarray(X, dtype=np.int64), np.asarray(Y, dtype=np.int64)]))

    def upper_bound(self, X, piv) -> np.ndarray:
        X = np.asarray(X, dtype=np.int64)
        piv = np.asarray(piv, dtype=np.int64)
        return np.searchsorted(self.rank[X], self.rank[piv], side="right").astype(np.int64)

    def sort_segments(self, idx, seg):
        """Every segment sorted on its own; a segment head's LCP is that with the last suffix of the nearest non-empty segment
        below, 0 at position 0."""
        idx = np.asarray(idx, dtype=np.int64)
        sa = np.empty_like(idx)
        lc = np.zeros(idx.size, dtype=np.int64)
        last = None
        for g in range(len(seg) - 1):
            a, b = int(seg[g]), int(seg[g + 1])
            if a == b:
                continue
            sa[a:b], lc[a:b] = self.sort_suffixes(idx[a:b])
            if last is not None:
                lc[a] = self.lcps([last], [sa[a]])[0]
            last = int(sa[b - 1])
        return sa, lc
