"""Plain-Python truth of the collection k-mer calls (include/caps_sa_hip.h "k-mers across a collection").

First half, from the TEXT definitions and nothing of the library: per document the set of its k-mers by slicing, a Counter of the
occurrences that lie inside a document, the k-mers in signed-char order, docs / occ / freq / shared from those sets.  No rank rule
appears there.  `count` (the run's length in ranks: every occurrence in the text, inside a document or not) comes from slicing the whole
text.

Second half (`rank_rule`): an independent restatement of the header's rank rules in numpy, for texts too long for the first half and
for arrays that are no text's.  The tests tie the two together on the small texts."""
from collections import Counter

import numpy as np

from kmer_reference import signed_key

MAX_DOCS = 64


def _bytes(T) -> bytes:
    return T if isinstance(T, bytes) else np.ascontiguousarray(T, dtype=np.uint8).tobytes()


def popcount(x: int) -> int:
    return bin(int(x)).count("1")


def passes(docs: int, min_docs=1, max_docs=0, all_of=0, none_of=0) -> bool:
    c = popcount(docs)
    return c >= max(min_docs, 1) and (max_docs == 0 or c <= max_docs) and (docs & all_of) == all_of and (docs & none_of) == 0


def text_table(T, k: int, docs):
    """[(k-mer bytes, count, occ, docs mask)] of the collection k-mers in signed-char order, from the text alone."""
    t = _bytes(T)
    n = len(t)
    every = Counter(t[i:i + k] for i in range(n - k + 1)) if 1 <= k <= n else Counter()
    inside = Counter()
    mask = {}
    for d, (s, l) in enumerate(docs):
        body = t[s:s + l]
        for i in range(len(body) - k + 1):
            w = body[i:i + k]
            inside[w] += 1
            mask[w] = mask.get(w, 0) | (1 << d)
    return [(w, every[w], inside[w], mask[w]) for w in sorted(mask, key=signed_key)]


def summary_of(masks, m: int):
    """(freq[65], shared[m, m]) of an iterable of docs masks."""
    freq = np.zeros(MAX_DOCS + 1, dtype=np.uint64)
    shared = np.zeros((m, m), dtype=np.uint64)
    for x in masks:
        x = int(x)
        freq[popcount(x)] += 1
        bits = [d for d in range(m) if (x >> d) & 1]
        for a in bits:
            for b in bits:
                shared[a, b] += 1
    return freq, shared


def text_summary(T, k: int, docs):
    """(freq, shared) from per-document SETS of k-mers: |set a & set b| for every pair, the frequency of membership counts."""
    t = _bytes(T)
    sets = [{t[s + i:s + i + k] for i in range(l - k + 1)} for s, l in docs]
    m = len(docs)
    shared = np.array([[len(sets[a] & sets[b]) for b in range(m)] for a in range(m)], dtype=np.uint64).reshape(m, m)
    freq = np.zeros(MAX_DOCS + 1, dtype=np.uint64)
    for w in set().union(*sets):
        freq[sum(1 for s in sets if w in s)] += 1
    return freq, shared


def rank_rule(SA, LCP, k: int, docs, min_docs=1, max_docs=0, all_of=0, none_of=0):
    """The header's rules on any two arrays: (records as a list of (first, count, occ, docs), unfiltered masks as a list)."""
    sa = [int(x) for x in np.asarray(SA).tolist()]
    lcp = [int(x) for x in np.asarray(LCP).tolist()]
    n = len(sa)
    bit = np.zeros(n, dtype=np.uint64)
    sa_np = np.asarray(sa, dtype=np.uint64) if n else np.zeros(0, dtype=np.uint64)
    for d, (s, l) in enumerate(docs):
        if l >= k:
            inside = (sa_np >= np.uint64(s)) & (sa_np <= np.uint64(s + l - k))
            bit[inside] |= np.uint64(1 << d)
    bit = [int(x) for x in bit.tolist()]
    heads = [r for r in range(n) if r == 0 or lcp[r] < k]
    rec, masks = [], []
    for j, h in enumerate(heads):
        e = heads[j + 1] if j + 1 < len(heads) else n
        x = 0
        occ = 0
        for r in range(h, e):
            x |= bit[r]
            occ += 1 if bit[r] else 0
        if x:
            masks.append(x)
            if passes(x, min_docs, max_docs, all_of, none_of):
                rec.append((h, e - h, occ, x))
    return rec, masks


def rank_rule_np(SA, LCP, k: int, docs):
    """The same, vectorised for long arrays: (first, count, occ, docs) as four np.uint64 arrays over the collection k-mers, unfiltered."""
    sa = np.asarray(SA).astype(np.uint64)
    lcp = np.asarray(LCP).astype(np.uint64)
    n = sa.size
    if n == 0:
        z = np.zeros(0, dtype=np.uint64)
        return z, z, z, z
    bit = np.zeros(n, dtype=np.uint64)
    for d, (s, l) in enumerate(docs):
        if l >= k:
            bit[(sa >= np.uint64(s)) & (sa <= np.uint64(s + l - k))] |= np.uint64(1 << d)
    is_head = lcp < np.uint64(k)
    is_head[0] = True
    first = np.flatnonzero(is_head)
    count = np.diff(np.append(first, n))
    docs_of = np.bitwise_or.reduceat(bit, first)
    occ = np.add.reduceat((bit != 0).astype(np.int64), first)
    keep = docs_of != 0
    return first[keep].astype(np.uint64), count[keep].astype(np.uint64), occ[keep].astype(np.uint64), docs_of[keep]
