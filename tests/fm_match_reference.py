"""Matching statistics and maximal exact matches from their definitions (include/caps_sa_hip.h "FM-index: matching statistics"),
in plain Python and numpy.  It shares no code with the library and does not know how the kernel walks:

* L[e] = the largest l <= e such that P[e - l .. e) occurs in T comes from substring search on the bytes ("occurs" is monotone in
  l by definition -- a piece of an occurring piece occurs -- so the largest l is found by bisection);
* the SA interval of a piece comes from fm_reference's naive suffix array: the ranks whose suffix starts with the piece;
* a MEM is a piece P[s .. e) that occurs, cannot be extended to the left (s = 0 or P[s - 1 .. e) does not occur) and cannot be
  extended to the right (e = m or P[s .. e + 1) does not occur).  mems_brute tries every (s, e); mems uses only that the piece
  ending at e which cannot be extended to the left is the longest one, L[e].  Neither uses the L[e + 1] <= L[e] rule of the kernel.
"""
import bisect

import numpy as np

MEM_DTYPE = np.dtype([("pattern", "<u8"), ("start", "<u4"), ("length", "<u4"), ("first", "<u8"), ("count", "<u8")])


class Text:
    """A text with its naive suffix array (fm_reference.naive_sa's order), ready for the three questions."""

    def __init__(self, T, SA):
        self.tb = np.ascontiguousarray(T, dtype=np.uint8).tobytes()
        self.n = len(self.tb)
        key = bytes(b ^ 0x80 for b in self.tb)
        self.suffixes = [key[int(i):] for i in SA]             # in rank order, signed-char keys
        assert all(self.suffixes[k] < self.suffixes[k + 1] for k in range(self.n - 1)), "SA is not the suffix array"

    def occurs(self, piece):
        return len(piece) > 0 and piece in self.tb

    def lengths(self, P, max_len=0):
        """L[e] for e = 1 .. m as np.uint32[m] (slot e - 1)."""
        pb = bytes(P)
        out = np.zeros(len(pb), dtype=np.uint32)
        for e in range(1, len(pb) + 1):
            top = min(e, max_len) if max_len else e
            lo, hi = 0, top                                    # pieces of length <= lo occur (or lo = 0), those above hi do not
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if self.occurs(pb[e - mid:e]):
                    lo = mid
                else:
                    hi = mid - 1
            out[e - 1] = lo
        return out

    def interval(self, piece):
        """(first, count): the ranks whose suffix starts with piece; (0, 0) for the empty piece or none."""
        if not piece:
            return 0, 0
        pk = bytes(b ^ 0x80 for b in piece)
        lo = bisect.bisect_left(self.suffixes, pk)
        a, b = lo, self.n                                      # the suffixes that start with the piece stand together from lo on
        while a < b:
            mid = (a + b) // 2
            if self.suffixes[mid].startswith(pk):
                a = mid + 1
            else:
                b = mid
        return (lo, a - lo) if a > lo else (0, 0)

    def intervals(self, P, L):
        pb = bytes(P)
        first = np.zeros(len(pb), dtype=np.uint64)
        count = np.zeros(len(pb), dtype=np.uint64)
        for e in range(1, len(pb) + 1):
            first[e - 1], count[e - 1] = self.interval(pb[e - int(L[e - 1]):e])
        return first, count

    def mems_brute(self, P, min_len=1):
        """[(start, length, first, count)] by increasing end, every (s, e) tried."""
        pb = bytes(P)
        m = len(pb)
        out = []
        for e in range(1, m + 1):
            for s in range(e):
                piece = pb[s:e]
                if not self.occurs(piece) or len(piece) < max(min_len, 1):
                    continue
                if s > 0 and self.occurs(pb[s - 1:e]):
                    continue
                if e < m and self.occurs(pb[s:e + 1]):
                    continue
                out.append((s, e - s) + self.interval(piece))
        return out

    def mems(self, P, min_len=1, L=None):
        """The same for long patterns: the only piece ending at e that occurs and cannot be extended to the left is the longest."""
        pb = bytes(P)
        m = len(pb)
        L = self.lengths(pb) if L is None else L
        out = []
        for e in range(1, m + 1):
            l = int(L[e - 1])
            if l < max(min_len, 1):
                continue
            if e < m and self.occurs(pb[e - l:e + 1]):
                continue
            out.append((e - l, l) + self.interval(pb[e - l:e]))
        return out


def records(per_pattern):
    """The record bytes of a batch: per_pattern[j] = the list mems() gave for pattern j -> (MEM_DTYPE array, mem_off u64[q + 1])."""
    off = np.zeros(len(per_pattern) + 1, dtype=np.uint64)
    rows = []
    for j, ms in enumerate(per_pattern):
        off[j + 1] = off[j] + np.uint64(len(ms))
        rows += [(j, s, l, f, c) for s, l, f, c in ms]
    return np.array(rows, dtype=MEM_DTYPE), off


def mem_rule(L, min_len=1):
    """The kernel's rule on a checked L (one pattern): ends e with L[e] >= min_len and (e = m or L[e + 1] <= L[e]).  For the large
    GPU case only, where L itself is verified by count; every other test takes its MEMs from Text.mems / mems_brute."""
    L = np.asarray(L, dtype=np.int64)
    if L.size == 0:
        return np.zeros(0, dtype=np.int64)
    nxt = np.append(L[1:], 0)
    return np.flatnonzero((L >= max(min_len, 1)) & (nxt <= L)) + 1
