"""Plain-Python truth for LPF, Prev and the LZ77 parse (include/caps_sa_hip.h "LPF and LZ77 from SA and LCP").

  lpf_brute(t)            LPF by the text definition: the longest prefix of t[i:] that also starts at some j < i
  lpf_naive(SA, LCP)      (LPF, Prev) by the per-rank rule, scanning rank by rank (quadratic on monotone permutations)
  lpf_stack(SA, LCP)      the same by the all-nearest-smaller-values stacks, linear for any arrays (stack_sides: per rank)
  lz_parse(LPF, Prev, n)  the clamped chain: [(pos, len, src)], src = LITERAL for a one-byte literal
  lz_decode(rec, t)       the text back from the records alone (the literal bytes are taken from t)
"""
import numpy as np

LITERAL = 0xFFFFFFFFFFFFFFFF


def none_of(dtype):
    return int(np.iinfo(dtype).max)


def lpf_brute(t: bytes):
    n = len(t)
    L = [0] * n
    for i in range(n):
        for j in range(i):
            ln = 0
            while i + ln < n and t[i + ln] == t[j + ln]:
                ln += 1
            if ln > L[i]:
                L[i] = ln
    return L


def _pick(left, right, none):
    """((length, SA value) or None) x 2 -> (LPF, Prev): on equal lengths the lower-rank side wins."""
    lv, rv = (left[0] if left else 0), (right[0] if right else 0)
    if rv > lv:
        return rv, right[1]
    if lv > 0:
        return lv, left[1]
    return 0, none


def lpf_naive(SA, LCP, none=None):
    """The rule, word for word.  SA: a permutation of 0 .. n - 1; LCP: any integers, LCP[0] counts as 0."""
    sa = [int(x) for x in SA]
    lcp = [int(x) for x in LCP]
    n = len(sa)
    if n:
        lcp[0] = 0
    none = none_of(np.asarray(SA).dtype) if none is None else none
    L, P = [0] * n, [none] * n
    for r in range(n):
        i = sa[r]
        left = right = None
        m = None
        for p in range(r - 1, -1, -1):
            m = lcp[p + 1] if m is None else min(m, lcp[p + 1])
            if sa[p] < i:
                left = (m, sa[p])
                break
        m = None
        for q in range(r + 1, n):
            m = lcp[q] if m is None else min(m, lcp[q])
            if sa[q] < i:
                right = (m, sa[q])
                break
        L[i], P[i] = _pick(left, right, none)
    return L, P


def lpf_stack(SA, LCP, none=None):
    sa = [int(x) for x in SA]
    left, right = stack_sides(SA, LCP)
    return _finish(sa, left, right, none_of(np.asarray(SA).dtype) if none is None else none)


def stack_sides(SA, LCP):
    """Per rank (left, right), each (length, SA value) or None where no smaller value lies on that side, in linear time.  A stack of ranks whose SA values ascend, from each side; an entry carries the minimum of LCP over
    the span between its rank and the rank of the entry under it, so that the spans of popped entries fold into the next one."""
    sa = [int(x) for x in SA]
    lcp = [int(x) for x in LCP]
    n = len(sa)
    if n:
        lcp[0] = 0
    left = [None] * n
    st = []                                               # [SA value, min LCP(rank of the entry under it, its rank]]
    for r in range(n):
        m = lcp[r]                                        # the top of the stack is rank r - 1
        while st and st[-1][0] >= sa[r]:
            m = min(m, st[-1][1])
            st.pop()
        if st:
            left[r] = (m, st[-1][0])
        st.append([sa[r], m])
    right = [None] * n
    st = []                                               # [SA value, min LCP(its rank, rank of the entry under it]]
    for r in range(n - 1, -1, -1):
        m = lcp[r + 1] if r + 1 < n else 0                # the top of the stack is rank r + 1
        while st and st[-1][0] >= sa[r]:
            m = min(m, st[-1][1])
            st.pop()
        if st:
            right[r] = (m, st[-1][0])
        st.append([sa[r], m])
    return left, right


def _finish(sa, left, right, none):
    n = len(sa)
    L, P = [0] * n, [none] * n
    for r in range(n):
        L[sa[r]], P[sa[r]] = _pick(left[r], right[r], none)
    return L, P


def lz_parse(LPF, Prev, n):
    out = []
    s = 0
    while s < n:
        lp = int(LPF[s])
        ln = min(max(1, lp), n - s)
        out.append((s, ln, int(Prev[s]) if lp > 0 else LITERAL))
        s += ln
    return out


def lz_decode(rec, t: bytes) -> bytes:
    out = bytearray()
    for pos, ln, src in rec:
        assert pos == len(out)
        if src == LITERAL:
            assert ln == 1
            out.append(t[pos])
        else:
            assert src < pos
            for k in range(ln):                           # byte by byte: source and target may overlap
                out.append(out[src + k])
    return bytes(out)
