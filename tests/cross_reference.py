"""Plain-Python reference for the MUMs and MEMs between two texts (include/caps_sa_hip.h "MUMs and MEMs between two texts"), from
the TEXT definitions only: all pairs (a < split <= b), extensions by comparing bytes, left-maximality on the text, occurrence counts
by substring search, the longest common substring by brute force.  No rank rule appears in the first half of this file; the second
half (``rank_rule``) restates the header's rank rules in numpy for texts too long for the brute force, and the tests tie the two
together on the small texts."""
import functools

import numpy as np


def signed_key(T: bytes, i: int):
    """The suffix at i in the library's byte order (signed char)."""
    return [b - 256 if b >= 128 else b for b in T[i:]]


def naive_sa_lcp_bwt(T: bytes):
    """(SA, LCP, BWT) as Python lists: suffixes in signed-char order, a shorter suffix before its extensions; LCP[0] = 0;
    BWT[r] = T[SA[r] - 1] (T[n - 1] at the rank with SA[r] == 0, which nothing looks at)."""
    n = len(T)
    SA = sorted(range(n), key=lambda i: signed_key(T, i))
    LCP = [0] * n
    for r in range(1, n):
        LCP[r] = lce(T, SA[r - 1], SA[r])
    BWT = [T[SA[r] - 1] if SA[r] else T[n - 1] for r in range(n)]
    return SA, LCP, BWT


def lce(T: bytes, i: int, j: int) -> int:
    n, l = len(T), 0
    while i + l < n and j + l < n and T[i + l] == T[j + l]:
        l += 1
    return l


@functools.lru_cache(maxsize=1 << 16)
def occurrences(T: bytes, w: bytes) -> int:
    return sum(1 for i in range(len(T) - len(w) + 1) if T[i:i + len(w)] == w)


def all_mems(T: bytes, split: int):
    """Every maximal exact match between the sides: (a, b, len) with a < split <= b, len >= 1 the full extension to the right, and
    the bytes to the left different or one of them at the start of T."""
    out = []
    for a in range(split):
        for b in range(split, len(T)):
            l = lce(T, a, b)
            if l and (a == 0 or b == 0 or T[a - 1] != T[b - 1]):
                out.append((a, b, l))
    return out


def mums(T: bytes, split: int, min_len: int):
    """The maximal unique matches of at least min_len bytes: maximal exact matches whose string occurs exactly twice in T."""
    return sorted((a, b, l) for a, b, l in all_mems(T, split) if l >= min_len and occurrences(T, T[a:a + l]) == 2)


def mems(T: bytes, split: int, min_len: int, max_occ: int):
    """(records, skipped): the maximal exact matches of at least min_len bytes whose first min_len bytes occur at most max_occ times
    in T, and the number of distinct strings of min_len bytes that occur more often than that."""
    rec = sorted((a, b, l) for a, b, l in all_mems(T, split) if l >= min_len and occurrences(T, T[a:a + min_len]) <= max_occ)
    seeds = {T[i:i + min_len] for i in range(len(T) - min_len + 1)}
    return rec, sum(1 for w in seeds if occurrences(T, w) > max_occ)


def lcs(T: bytes, split: int):
    """(len, candidates): the length of the longest common substring of the sides and every (a, b) that attains it; (0, [])
    when the sides share no byte."""
    best, at = 0, []
    for a in range(split):
        for b in range(split, len(T)):
            l = lce(T, a, b)
            if l > best:
                best, at = l, []
            if l and l == best:
                at.append((a, b))
    return best, at


# ---- the header's rank rules, restated in numpy (any arrays, any size) ------------------------------------------------------------
def rank_rule(SA, LCP, BWT, split: int, min_len: int, max_occ: int | None):
    """(records as a list of (a, b, len) in the order of the header, summary as a list of 8 ints).  max_occ None: MUM mode."""
    SA = np.asarray(SA, dtype=np.uint64)
    L = np.asarray(LCP, dtype=np.uint64).copy()
    B = np.asarray(BWT, dtype=np.uint8)
    n = int(SA.size)
    summary = [0] * 8
    if n == 0:
        return [], summary
    L[0] = 0
    side = SA >= np.uint64(split)
    cross = np.zeros(n, dtype=bool)
    cross[1:] = side[1:] != side[:-1]
    cand = np.flatnonzero(cross & (L > 0))
    if cand.size:
        r = int(cand[np.argmax(L[cand])])              # argmax: the first of the maxima
        sp, sq = int(SA[r - 1]), int(SA[r])
        summary[2] = int(L[r])
        summary[3] = sp if sp < split else sq
        summary[4] = sq if sp < split else sp

    def pair(p, q, l):
        sp, sq = int(SA[p]), int(SA[q])
        return (sp, sq, l) if sp < split else (sq, sp, l)

    rec = []
    if max_occ is None:
        prev = np.zeros(n, dtype=np.uint64)
        prev[1:] = L[:-1]
        nxt = np.zeros(n, dtype=np.uint64)
        nxt[:-1] = L[1:]
        lm = np.zeros(n, dtype=bool)
        lm[1:] = (SA[1:] == 0) | (SA[:-1] == 0) | (B[1:] != B[:-1])
        ok = cross & (L >= np.uint64(min_len)) & (prev < L) & (nxt < L) & lm
        for r in np.flatnonzero(ok):
            rec.append(pair(int(r) - 1, int(r), int(L[r])))
    else:
        heads = np.flatnonzero(L < np.uint64(min_len))          # rank 0 is one: L[0] = 0 < min_len
        ends = np.append(heads[1:], n)
        for h, e in zip(heads.tolist(), ends.tolist()):
            if e - h < 2:
                continue
            if e - h > max_occ:
                summary[1] += 1
                continue
            for q in range(h + 1, e):
                l = int(L[q])
                for p in range(q - 1, h - 1, -1):
                    l = min(l, int(L[p + 1]))
                    if side[p] != side[q] and (SA[p] == 0 or SA[q] == 0 or B[p] != B[q]):
                        rec.append(pair(p, q, l))
    summary[0] = len(rec)
    return rec, summary
