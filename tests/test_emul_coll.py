"""CPU: k-mers across a collection of sequences from SA and LCP (include/caps_sa_hip.h "k-mers across a collection",
caps_sa_hip_coll_kmers_*, caps_sa_hip_coll_sharing_*) through the host emulation of the kernels.

Every comparison is exact: the records word for word in rank order, all 65 words of freq and the whole matrix.  The truth of the short
texts is coll_reference's first half (the text definitions: per-document sets by slicing, a Counter of the occurrences inside a
document); longer cases and arrays that are no text's use its numpy restatement of the rank rules, which the short texts tie to the
text definitions.  The sweeps are functions of a "form" (the host or the device entry points of a library on some memory), so that
test_gpu_coll.py runs the same ones on the GPU.  The device form works on buffers preset to 0xA5: the records start 72 bytes in with 64
guard bytes behind them, the workspace has exactly caps_sa_hip_coll_workspace_bytes with a guard behind it; freq and shared lie between
guard words in both forms.  Every check of a case also recomputes freq and shared from the unfiltered records."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import coll_reference as R
from cross_reference import naive_sa_lcp_bwt
from emul_util import EMUL_DIR, ROOT, emul, emul_rev, emul_small
from sa_check import sa_lcp

EINVAL = -1
FILL = 0xA5
GUARD = 64
FRONT = 72
REC = 32
TILE = 16384                                                # ranks of a tile of ck_run_kernel (kernels.h KMER_TILE)
LANE = 64                                                   # ranks of a lane
SIZES = [1, 63, 64, 65, 16383, 16384, 16385, 32767, 32768, 32769, 49153]
LETTERS3 = bytes([0x41, 0x43, 0xC8])                        # (0xC8 sorts first: signed char)
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
SEP = 0xFF
WORD = 0xA5A5A5A5A5A5A5A5
NO_FILTER = dict(min_docs=1, max_docs=0, all_of=0, none_of=0)


def naive(t: bytes):
    """(SA, LCP) of a short text by sorting its suffixes (sa_check's prefix doubling needs n + 2 > the byte range)."""
    SA, LCP, _ = naive_sa_lcp_bwt(t)
    return np.array(SA, dtype=np.uint64), np.array(LCP, dtype=np.uint64)


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


class HostMem:
    """Memory of the *_device entry points of the emulation: host memory."""

    def filled(self, nbytes):
        return np.full(nbytes, FILL, dtype=np.uint8)

    def put(self, a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return a.copy() if a.size else np.zeros(8, dtype=np.uint8)

    def ptr(self, buf):
        return buf.ctypes.data

    def get(self, buf):
        return buf


class Arrays:
    """SA and LCP of one case in the index width, on the host and -- for the device form -- on `mem`."""

    def __init__(self, SA, LCP, bits, mem=None):
        self.bits, self.n = bits, int(len(SA))
        self.sa = np.ascontiguousarray(SA, dtype=_dt(bits))
        self.lcp = np.ascontiguousarray(LCP, dtype=_dt(bits))
        assert self.lcp.size == self.n
        self.mem = mem
        if mem is not None:
            self.d = [mem.put(self.sa), mem.put(self.lcp)]


def doc_arrays(docs):
    d = np.asarray(list(docs), dtype=np.uint64).reshape(-1, 2)
    return np.ascontiguousarray(d[:, 0]), np.ascontiguousarray(d[:, 1]), int(d.shape[0])


class Form:
    """One family of entry points: the counting call, then the writing call into a guarded buffer; and the summary call."""

    def __init__(self, lib, mem=None):
        self.lib, self.mem = lib, mem
        self.name = "device" if mem is not None else "host"

    def load(self, SA, LCP, bits):
        return Arrays(SA, LCP, bits, self.mem)

    def fn(self, what, bits):
        return self.lib._f(f"coll_{what}{'_device' if self.mem is not None else ''}_{'u32' if bits == 32 else 'u64'}")

    def _arrays(self, a):
        if self.mem is None:
            return [x.ctypes.data if a.n else None for x in (a.sa, a.lcp)]
        return [self.mem.ptr(x) if a.n else None for x in a.d]

    def _tail(self, ws):
        if self.mem is None:
            return (0,)
        w, wb = (self.mem.ptr(ws[0]), ws[1]) if ws else (None, 0)
        return (w, wb, None)

    def call_kmers(self, a, k, docs, filt, rec_ptr, capacity, found, ws=None):
        """The raw return code of one coll_kmers call; found: a ctypes.c_uint64."""
        st, ln, m = doc_arrays(docs)
        return self.fn("kmers", a.bits)(*self._arrays(a), a.n, k, st.ctypes.data, ln.ctypes.data, m, filt["min_docs"], filt["max_docs"],
                                        filt["all_of"], filt["none_of"], rec_ptr or None, capacity, ctypes.byref(found), *self._tail(ws))

    def _ws(self, a, own_ws):
        if self.mem is None or not own_ws:
            return None
        wb = self.lib.coll_workspace_bytes(a.n, a.bits)
        return (self.mem.filled(wb + GUARD), wb)

    def _after(self, a, ws):
        m = self.mem
        if m is None:
            return
        if ws:
            assert (m.get(ws[0])[ws[1]:] == FILL).all(), "the guard of the workspace was written"
        for dev, host in zip(a.d, (a.sa, a.lcp)):
            assert np.array_equal(m.get(dev)[:host.nbytes], host.view(np.uint8)), "an input array was written"

    def run(self, a, k, docs, own_ws=True, **filt):
        """The records as a list of (first, count, occ, docs)."""
        filt = {**NO_FILTER, **filt}
        m = self.mem
        ws = self._ws(a, own_ws)
        f1 = ctypes.c_uint64(0x5A5A)
        assert self.call_kmers(a, k, docs, filt, 0, 0, f1, ws) == 0, self.lib._f("last_error")()
        found = f1.value
        f2 = ctypes.c_uint64(0x5A5A)
        nbytes = FRONT + REC * found + GUARD
        if m is None:
            buf = np.full(nbytes, FILL, dtype=np.uint8)
            assert self.call_kmers(a, k, docs, filt, buf.ctypes.data + FRONT, found, f2) == 0
            out = buf
        else:
            buf = m.filled(nbytes)
            assert self.call_kmers(a, k, docs, filt, m.ptr(buf) + FRONT, found, f2, ws) == 0
            out = m.get(buf)
            self._after(a, ws)
        assert (out[:FRONT] == FILL).all() and (out[FRONT + REC * found:] == FILL).all(), "a guard of the records was written"
        assert f2.value == found, "the counting call and the writing call disagree"
        rec = out[FRONT:FRONT + REC * found].copy().view("<u8").reshape(-1, 4)
        return [tuple(r) for r in rec.tolist()]

    def sharing(self, a, k, docs, own_ws=True):
        """(freq as a list of 65, shared as an (m, m) array)."""
        st, ln, m = doc_arrays(docs)
        ws = self._ws(a, own_ws)
        fq = np.full(8 + 65 + 8, WORD, dtype=np.uint64)
        sh = np.full(8 + m * m + 8, WORD, dtype=np.uint64)
        rc = self.fn("sharing", a.bits)(*self._arrays(a), a.n, k, st.ctypes.data, ln.ctypes.data, m, fq.ctypes.data + 64, sh.ctypes.data + 64,
                                        *self._tail(ws))
        assert rc == 0, self.lib._f("last_error")()
        self._after(a, ws)
        assert (fq[:8] == WORD).all() and (fq[-8:] == WORD).all() and (sh[:8] == WORD).all() and (sh[-8:] == WORD).all(), "a guard word was written"
        return fq[8:73].tolist(), sh[8:8 + m * m].reshape(m, m).copy()


def forms_of(lib, mem):
    return (Form(lib), Form(lib, mem))


def check_case(form, a, k, docs, want_rec, tag, filters=()):
    """The unfiltered records against want_rec, freq / shared against the masks of want_rec, and every filter against the filtered list."""
    m = len(docs)
    got = form.run(a, k, docs)
    assert got == want_rec, (tag, form.name, a.bits, got[:4], want_rec[:4])
    freq, shared = form.sharing(a, k, docs)
    wf, ws = R.summary_of([r[3] for r in want_rec], m)
    assert freq == wf.tolist(), (tag, form.name, freq[:m + 2], wf[:m + 2])
    assert np.array_equal(shared, ws), (tag, form.name, shared, ws)
    assert freq[0] == 0 and sum(freq) == len(want_rec) and np.array_equal(shared, shared.T)
    for f in filters:
        want = [r for r in want_rec if R.passes(r[3], **f)]
        assert form.run(a, k, docs, **f) == want, (tag, form.name, f)


# ---- 1. every short text, against the text definitions --------------------------------------------------------------------------------

def cuts_of(n: int):
    """Every cut of [0, n) into 1 .. 3 documents that touch, and the same cuts with a one-byte gap behind every document."""
    out = []
    for m in (1, 2, 3):
        for inner in itertools.combinations_with_replacement(range(n + 1), m - 1):
            c = (0,) + inner + (n,)
            out.append([(c[i], c[i + 1] - c[i]) for i in range(m)])
            out.append([(c[i], max(c[i + 1] - c[i] - 1, 0)) for i in range(m)])
    return out


def n_short_cases(max_len: int, ks=(1, 2, 3, 4)) -> int:
    return sum(3 ** n * len(cuts_of(n)) * len(ks) for n in range(1, max_len + 1))


def short_case_truth(t: bytes, SA, k: int, docs, first_of: dict):
    """(records, freq, shared) of one text, cut and k from the text definitions."""
    if k not in first_of:
        # the record's `first` is the rank of the k-mer's first suffix: the suffixes that start with it are consecutive
        first_of[k] = {}
        for r in range(len(t) - 1, -1, -1):
            first_of[k][t[int(SA[r]):int(SA[r]) + k]] = r
    want = [(first_of[k][w], count, occ, mask) for w, count, occ, mask in R.text_table(t, k, docs)]
    return (want,) + R.text_summary(t, k, docs)


def short_text_sweep(forms, max_len=7, ks=(1, 2, 3, 4), tie_rank_rule=True, batch=1, min_len=1):
    """Every text of min_len .. max_len bytes over 3 letters x every cut x k against the text definitions -> the number of cases.
    The (form, width) pairs take turns.  batch = 1: a call per case, on the text's own arrays.  batch > 1: the arrays of up to `batch`
    texts behind one another in one pair of arrays -- SA values moved by the texts' offsets; every text's rank 0 is a head, so no run
    crosses from one text into the next -- with all their documents in one call (at most 64): the records of every text, moved to
    its ranks and bits, the matrix block by block (0 between texts), freq as the sum."""
    combos = [(f, b) for f in forms for b in (32, 64)]
    done = calls = 0
    pending = {k: [] for k in ks}

    def flush(k):
        nonlocal calls
        items, pending[k] = pending[k], []
        if not items:
            return
        SAs, LCPs, docs_all, want, base, dbase = [], [], [], [], 0, 0
        m_all = sum(len(d) for _, _, _, d, _ in items)
        wfreq = np.zeros(65, dtype=np.uint64)
        wshared = np.zeros((m_all, m_all), dtype=np.uint64)
        for t, SA, LCP, docs, (rec, freq, shared) in items:
            SAs.append(SA + np.uint64(base))
            LCPs.append(LCP)
            docs_all += [(s + base, l) for s, l in docs]
            want += [(f + base, c, o, x << dbase) for f, c, o, x in rec]
            wfreq += freq
            wshared[dbase:dbase + len(docs), dbase:dbase + len(docs)] = shared
            base += len(t)
            dbase += len(docs)
        form, bits = combos[calls % len(combos)]
        calls += 1
        a = form.load(np.concatenate(SAs), np.concatenate(LCPs), bits)
        got = form.run(a, k, docs_all)
        assert got == want, ([i[0] for i in items], docs_all, k, form.name, bits, got, want)
        freq, shared = form.sharing(a, k, docs_all)
        assert freq == wfreq.tolist() and np.array_equal(shared, wshared), ([i[0] for i in items], docs_all, k, form.name, bits, freq[:5], shared)

    for n in range(min_len, max_len + 1):
        cuts = cuts_of(n)
        for letters in itertools.product(LETTERS3, repeat=n):
            t = bytes(letters)
            SA, LCP = naive(t)
            first_of = {}
            for docs in cuts:
                for k in ks:
                    truth = short_case_truth(t, SA, k, docs, first_of)
                    if tie_rank_rule:
                        assert R.rank_rule(SA, LCP, k, docs)[0] == truth[0], (t, docs, k)
                    if len(pending[k]) == batch or sum(len(i[3]) for i in pending[k]) + len(docs) > 64:
                        flush(k)
                    pending[k].append((t, SA, LCP, docs, truth))
                    done += 1
    for k in ks:
        flush(k)
    return done


def test_short_texts_quick():
    forms = forms_of(emul(), HostMem())
    assert short_text_sweep(forms, max_len=3) == n_short_cases(3)
    assert short_text_sweep(forms, max_len=4, min_len=4, batch=21) == n_short_cases(4) - n_short_cases(3)


@pytest.mark.slow
def test_every_short_text_against_the_text_definitions():
    """Every text of up to 7 bytes x every cut x k = 1 .. 4: up to length 4 a call per case, from there on the arrays of 21 texts in one
    call (the number of cases grows to 1.1 million)."""
    forms = forms_of(emul(), HostMem())
    assert short_text_sweep(forms, max_len=4) == n_short_cases(4)
    assert short_text_sweep(forms, max_len=7, min_len=5, batch=21, tie_rank_rule=False) == n_short_cases(7) - n_short_cases(4)


# ---- 2. sizes around the lane and the tile, text shapes, 1 / 2 / 3 / 64 equal parts ------------------------------------------------------

def shaped_text(shape: int, n: int, rs) -> np.ndarray:
    if shape == 0:
        return np.full(n, 0x41, dtype=np.uint8)
    if shape == 1:
        return rs.choice(DNA[:2], size=n).astype(np.uint8)
    if shape == 2:
        return rs.choice(DNA, size=n).astype(np.uint8)
    base = rs.choice(DNA, size=max(n // 5, 1)).astype(np.uint8)              # a base sequence and mutated copies
    copies = []
    while sum(c.size for c in copies) < n:
        c = base.copy()
        if copies:
            at = rs.randint(0, c.size, size=max(c.size // 23, 1))
            c[at] = DNA[(np.searchsorted(DNA, c[at]) + 1) % 4]
        copies.append(c)
    return np.concatenate(copies)[:n]


def equal_parts(n: int, m: int, sep: bool):
    """m equal parts of [0, n) (the last takes the rest); with sep the last byte of every part is a separator outside its document."""
    step = n // m
    docs = []
    for d in range(m):
        s = d * step
        l = (n - s) if d == m - 1 else step
        docs.append((s, max(l - 1, 0) if sep else l))
    return docs


def size_sweep(forms, sizes=SIZES, shapes=(0, 1, 2, 3), parts=(1, 2, 3, 64), ks=(1, 2, 11)):
    """-> the number of (size, shape, parts, separators) cases; the (form, width) pairs take turns, every k runs on each."""
    combos = [(f, b) for f in forms for b in (32, 64)]
    rs = np.random.RandomState(7)
    done = 0
    for n in sizes:
        for shape in shapes:
            plain = shaped_text(shape, n, rs)
            plain_arrays = None
            for m in parts:
                for sep in (False, True):
                    docs = equal_parts(n, m, sep)
                    T = plain
                    if sep:
                        T = plain.copy()
                        for s, l in docs:
                            if s + l < n:
                                T[s + l] = SEP
                        SA, LCP = naive(T.tobytes()) if n < 300 else sa_lcp(T, 64)
                    else:
                        if plain_arrays is None:
                            plain_arrays = naive(plain.tobytes()) if n < 300 else sa_lcp(plain, 64)
                        SA, LCP = plain_arrays
                    form, bits = combos[done % len(combos)]
                    a = form.load(SA, LCP, bits)
                    for k in ks:
                        first, count, occ, mask = R.rank_rule_np(SA, LCP, k, docs)
                        want = list(zip(first.tolist(), count.tolist(), occ.tolist(), mask.tolist()))
                        if shape == 0 and not sep and n >= k:
                            # 'A' * n: one run over every tile; the boundary occurrences of k > 1 are OUT
                            full = 0
                            for d, (s, l) in enumerate(docs):
                                full |= (1 << d) if l >= k else 0
                            n_in = sum(max(l - k + 1, 0) for s, l in docs)
                            assert want == ([(k - 1, n - k + 1, n_in, full)] if full else []), (n, m, k, want[:3])
                        check_case(form, a, k, docs, want, (n, shape, m, sep, k))
                    done += 1
    return done


@pytest.mark.parametrize("sizes", [tuple(SIZES[:6]), tuple(SIZES[6:9]), tuple(SIZES[9:])])
def test_sizes_and_text_shapes(sizes):
    assert size_sweep(forms_of(emul(), HostMem()), sizes) == len(sizes) * 4 * 4 * 2


# ---- 3. one run across the lane and tile edges: arrays that are no text's ------------------------------------------------------------------

EDGE_N = 3 * TILE + 130
EDGE_POS = sorted({e + d for e in (LANE, 2 * LANE, 3 * LANE, TILE, 2 * TILE, 3 * TILE) for d in (-2, -1, 0, 1, 2)})
EDGE_DOCS = [(0, 1000), (1000, 1000), (2000, 1000), (3000, 1000), (5000, 1000)]
EDGE_K = 5


def edge_cases():
    """(head, end) of the one long run: every edge position as a head and as an end, with near and far partners."""
    out = set()
    for p in EDGE_POS:
        for e in (p + 1, p + 2, p + LANE + 6, 2 * TILE + 5, EDGE_N):
            if p < e <= EDGE_N:
                out.add((p, e))
        for h in (0, 5, p - 1, p - 2, p - LANE - 6, TILE - 3):
            if 0 <= h < p:
                out.add((h, p))
    out.add((TILE - 3, 3 * TILE + 2))                       # two whole tiles without a head
    out.add((0, EDGE_N))
    return sorted(out)


def edge_arrays(head: int, end: int):
    """Every rank outside [head, end) is a run of its own in document 0 (or OUT); the run's ranks lie in document 0 or OUT, except for
    three planted bits: document 1 only in its first rank, document 2 only in its last, document 3 only in the rank just behind the
    first lane or tile edge inside it, document 4 only in the rank just in front of that edge."""
    r = np.arange(EDGE_N, dtype=np.int64)
    LCP = np.zeros(EDGE_N, dtype=np.int64)
    LCP[head + 1:end] = EDGE_K + (r[head + 1:end] % 3)
    SA = r % 990                                             # document 0 (990 + 5 <= 1000)
    SA[r % 7 == 3] = 1 << 31                                 # OUT: beyond n
    SA[r % 11 == 5] = 998                                    # OUT: runs past the end of document 0
    SA[r % 13 == 6] = 4500                                   # OUT: in a gap
    SA[head] = 1000
    if end - 1 > head:
        SA[end - 1] = 2995
    inner = [e for e in range(LANE, EDGE_N, LANE) if head + 1 < e < end - 1]
    if inner:
        SA[inner[0]] = 3100
        if inner[0] - 1 > head:
            SA[inner[0] - 1] = 5995
    return SA, LCP


def edge_sweep(forms, cases=None, widths=(32, 64)):
    combos = [(f, b) for f in forms for b in widths]
    done = 0
    for head, end in (cases if cases is not None else edge_cases()):
        SA, LCP = edge_arrays(head, end)
        first, count, occ, mask = R.rank_rule_np(SA, LCP, EDGE_K, EDGE_DOCS)
        want = list(zip(first.tolist(), count.tolist(), occ.tolist(), mask.tolist()))
        mine = [w for w in want if w[0] == head]
        assert len(mine) == 1 and mine[0][1] == end - head and mine[0][3] & 2, (head, end, mine)
        form, bits = combos[done % len(combos)]
        a = form.load(SA, LCP, bits)
        got = form.run(a, EDGE_K, EDGE_DOCS)
        assert got == want, (head, end, form.name, bits, [g for g in got if g[0] == head], mine)
        freq, shared = form.sharing(a, EDGE_K, EDGE_DOCS)
        wf, ws = R.summary_of(mask, len(EDGE_DOCS))
        assert freq == wf.tolist() and np.array_equal(shared, ws), (head, end, form.name, bits)
        done += 1
    return done


def test_one_run_across_the_lane_and_tile_edges():
    assert edge_sweep(forms_of(emul(), HostMem())) == len(edge_cases()) > 150


# ---- 4. document edge cases and filters ------------------------------------------------------------------------------------------------

def small_text(n=400, seed=3):
    rs = np.random.RandomState(seed)
    base = rs.choice(DNA, size=n // 4).astype(np.uint8)
    parts = [base]
    for _ in range(3):
        c = base.copy()
        at = rs.randint(0, c.size, size=6)
        c[at] = DNA[(np.searchsorted(DNA, c[at]) + 1) % 4]
        parts.append(c)
    return np.concatenate(parts)


FILTERS4 = [dict(min_docs=a, max_docs=b) for a in (0, 1, 4, 5) for b in (0, 1, 4, 5) if not (b and a > b)] + [
    dict(all_of=1), dict(all_of=0b1010), dict(none_of=0b0100), dict(none_of=0b1110), dict(all_of=0b0011, none_of=0b1000),
    dict(all_of=0b0001, none_of=0b1110, max_docs=1), dict(all_of=0b1111, min_docs=4), dict(all_of=0b1111, none_of=0, min_docs=5)]


def document_sweep(forms, widths=(32, 64)):
    """m = 1, m = 64 (bit 63), lengths 0 / k - 1 / k, gaps in front of the first and behind the last document, the last document ending
    at n, SA values >= n, and the filters -> the number of cases."""
    T = small_text()
    n = T.size
    t = T.tobytes()
    SA, LCP = sa_lcp(T, 64)
    k = 4
    q = n // 4
    cases = {
        "one": [(0, n)],
        "one inside": [(7, n - 20)],
        "four": [(0, q), (q, q), (2 * q, q), (3 * q, q)],
        "gaps": [(3, q - 5), (q + 2, q - 9), (2 * q, q), (3 * q + 1, q - 1)],
        "lengths": [(0, 0), (0, k - 1), (k - 1, k), (2 * k - 1, 0), (2 * k - 1, 0), (2 * k + 3, k + 1), (n - k, k), (n, 0)],
        "sixty-four": [(d * 6, 6) for d in range(63)] + [(378, n - 378)],
        "sixty-four, the last empty": [(d * 6, 6) for d in range(63)] + [(n, 0)],
    }
    done = 0
    for name, docs in cases.items():
        for ki in ((k, 1) if name in ("lengths", "sixty-four") else (k,)):
            table = R.text_table(t, ki, docs)
            want_np = R.rank_rule_np(SA, LCP, ki, docs)
            want = list(zip(*[x.tolist() for x in want_np]))
            assert [(w[1], w[2], w[3]) for w in want] == [(c, o, x) for _, c, o, x in table], name
            assert [t[int(SA[w[0]]):int(SA[w[0]]) + ki] for w in want] == [w for w, _, _, _ in table], name
            if name == "sixty-four":
                assert any(w[3] >> 63 for w in want)
            for form in forms:
                for bits in widths:
                    check_case(form, form.load(SA, LCP, bits), ki, docs, want, name, FILTERS4 if name in ("four", "gaps") else ())
                    done += 1
    # SA values >= n, and 2^32 - 1: OUT, whatever the documents
    bad = np.array(SA, dtype=np.int64)
    bad[::5] = n
    bad[1::7] = (1 << 32) - 1
    docs = cases["gaps"]
    want = list(zip(*[x.tolist() for x in R.rank_rule_np(bad, LCP, k, docs)]))
    assert R.rank_rule(bad, LCP, k, docs)[0] == want
    for form in forms:
        for bits in widths:
            check_case(form, form.load(bad, LCP, bits), k, docs, want, "SA >= n", FILTERS4[:3])
            done += 1
    # k > n, k huge: nothing
    for form in forms:
        a = form.load(SA, LCP, 32)
        for kk in (n + 1, 1 << 40, (1 << 64) - 1):
            assert form.run(a, kk, cases["four"]) == []
            freq, shared = form.sharing(a, kk, cases["four"])
            assert sum(freq) == 0 and not shared.any()
        assert len(form.run(a, n, [(0, n)])) == 1
    return done


def test_documents_and_filters():
    assert document_sweep(forms_of(emul(), HostMem())) > 30


# ---- 5. the protocol ----------------------------------------------------------------------------------------------------------------------

def capacity_sweep(lib, mem):
    T = small_text()
    SA, LCP = sa_lcp(T, 64)
    q = T.size // 4
    docs = [(0, q), (q, q), (2 * q, q), (3 * q, q)]
    want = list(zip(*[x.tolist() for x in R.rank_rule_np(SA, LCP, 3, docs)]))
    for form in forms_of(lib, mem):
        for bits in (32, 64):
            a = form.load(SA, LCP, bits)
            assert form.run(a, 3, docs, own_ws=False) == want                   # a NULL workspace: the call's own
            freq, shared = form.sharing(a, 3, docs, own_ws=False)
            assert sum(freq) == len(want)
            found = ctypes.c_uint64(7)
            nbytes = REC * len(want)
            buf = mem.filled(nbytes) if form.mem is not None else np.full(nbytes, FILL, dtype=np.uint8)
            ptr = mem.ptr(buf) if form.mem is not None else buf.ctypes.data
            assert form.call_kmers(a, 3, docs, NO_FILTER, ptr, len(want) - 1, found) == EINVAL          # one short
            assert found.value == len(want)
            assert ((mem.get(buf) if form.mem is not None else buf) == FILL).all(), "records were written although the capacity is too small"
            assert form.call_kmers(a, 3, docs, NO_FILTER, ptr, len(want), found) == 0 and found.value == len(want)
            got = (mem.get(buf) if form.mem is not None else buf).copy().view("<u8").reshape(-1, 4)
            assert [tuple(r) for r in got.tolist()] == want
            # a filter that nothing passes: zero records, a non-null buffer is fine
            assert form.call_kmers(a, 3, docs, dict(NO_FILTER, min_docs=5), ptr, 0, found) == 0 and found.value == 0


def test_counting_call_writing_call_and_capacity():
    capacity_sweep(emul(), HostMem())


def refusal_sweep(lib, mem):
    """Every refusal is CAPS_SA_EINVAL with nothing written: not the count, not freq or shared, not the records, not the workspace."""
    T = small_text(120)
    n = T.size
    for bits in (32, 64):
        sfx = "u32" if bits == 32 else "u64"
        SAh, LCPh = sa_lcp(T, bits)
        dS, dL = mem.put(SAh), mem.put(LCPh)
        S, Lp = mem.ptr(dS), mem.ptr(dL)
        hs, hl = SAh.ctypes.data, LCPh.ctypes.data
        wsb = lib.coll_workspace_bytes(n, bits)
        ws = mem.filled(wsb)
        recs = mem.filled(REC * n + 8)
        hrec = np.full(REC * n + 8, FILL, dtype=np.uint8)
        W, Rp, Hp = mem.ptr(ws), mem.ptr(recs), hrec.ctypes.data
        found = ctypes.c_uint64(0x5A5A)
        F = ctypes.byref(found)
        freq = np.full(65, WORD, dtype=np.uint64)
        shared = np.full(64 * 64, WORD, dtype=np.uint64)
        Fq, Sh = freq.ctypes.data, shared.ctypes.data
        good = doc_arrays([(0, 40), (40, 40), (80, 40)])
        keep = [good[0], good[1]]

        def D(docs):
            st, ln, m = doc_arrays(docs)
            keep.extend((st, ln))
            return st.ctypes.data, ln.ctypes.data, m

        G = (good[0].ctypes.data, good[1].ctypes.data, 3)
        kd, kh = lib._f(f"coll_kmers_device_{sfx}"), lib._f(f"coll_kmers_{sfx}")
        sd, sh = lib._f(f"coll_sharing_device_{sfx}"), lib._f(f"coll_sharing_{sfx}")
        big = 1 << 63
        bad_docs = [D([(0, 50), (40, 40)]),                   # overlap
                    D([(50, 10), (0, 10)]),                   # descending
                    D([(0, 40), (100, 21)]),                  # passes n
                    D([(n + 1, 0)]),
                    D([(0, big), (big, big)]),                # start + length overflows
                    D([((1 << 64) - 1, 2)]),
                    (G[0], G[1], 0), (G[0], G[1], 65),        # m
                    (None, G[1], 3), (G[0], None, 3)]         # null document arrays
        calls = []
        for dd in bad_docs:
            calls += [kd(S, Lp, n, 3, *dd, 1, 0, 0, 0, Rp, n, F, W, wsb, None), kh(hs, hl, n, 3, *dd, 1, 0, 0, 0, Hp, n, F, 0),
                      sd(S, Lp, n, 3, *dd, Fq, Sh, W, wsb, None), sh(hs, hl, n, 3, *dd, Fq, Sh, 0)]
        for args in ((0, 1, 0, 0, 0),                         # k == 0
                     (3, 3, 2, 0, 0),                         # min_docs > max_docs > 0
                     (3, 1, 0, 0b011, 0b010),                 # all_of & none_of
                     (3, 1, 0, 0b1000, 0), (3, 1, 0, 0, 1 << 63)):        # a mask bit at or above m
            k, filt = args[0], args[1:]
            calls += [kd(S, Lp, n, k, *G, *filt, Rp, n, F, W, wsb, None), kh(hs, hl, n, k, *G, *filt, Hp, n, F, 0)]
        calls += [sd(S, Lp, n, 0, *G, Fq, Sh, W, wsb, None), sh(hs, hl, n, 0, *G, Fq, Sh, 0),
                  kd(None, Lp, n, 3, *G, 1, 0, 0, 0, Rp, n, F, W, wsb, None), kd(S, None, n, 3, *G, 1, 0, 0, 0, Rp, n, F, W, wsb, None),
                  kh(None, hl, n, 3, *G, 1, 0, 0, 0, Hp, n, F, 0), kh(hs, None, n, 3, *G, 1, 0, 0, 0, Hp, n, F, 0),
                  sd(None, Lp, n, 3, *G, Fq, Sh, W, wsb, None), sd(S, None, n, 3, *G, Fq, Sh, W, wsb, None),
                  sh(None, hl, n, 3, *G, Fq, Sh, 0), sh(hs, None, n, 3, *G, Fq, Sh, 0),
                  kd(S, Lp, n, 3, *G, 1, 0, 0, 0, Rp, n, None, W, wsb, None), kh(hs, hl, n, 3, *G, 1, 0, 0, 0, Hp, n, None, 0),   # null outputs
                  sd(S, Lp, n, 3, *G, None, Sh, W, wsb, None), sd(S, Lp, n, 3, *G, Fq, None, W, wsb, None),
                  sh(hs, hl, n, 3, *G, None, Sh, 0), sh(hs, hl, n, 3, *G, Fq, None, 0),
                  kd(S, Lp, n, 3, *G, 1, 0, 0, 0, Rp + 4, n, F, W, wsb, None), kh(hs, hl, n, 3, *G, 1, 0, 0, 0, Hp + 4, n, F, 0),  # alignment
                  kd(S, Lp, n, 3, *G, 1, 0, 0, 0, Rp, n, F, W, wsb - 512, None), sd(S, Lp, n, 3, *G, Fq, Sh, W, wsb - 512, None)]  # workspace
        if bits == 32:                                       # n > UINT32_MAX with _u32: refused before anything is read
            b = 1 << 32
            calls += [kd(S, Lp, b, 3, *G, 1, 0, 0, 0, None, 0, F, None, 0, None), kh(hs, hl, b, 3, *G, 1, 0, 0, 0, None, 0, F, 0),
                      sd(S, Lp, b, 3, *G, Fq, Sh, None, 0, None), sh(hs, hl, b, 3, *G, Fq, Sh, 0)]
        assert calls == [EINVAL] * len(calls), calls
        assert found.value == 0x5A5A and (freq == WORD).all() and (shared == WORD).all() and (hrec == FILL).all()
        assert (mem.get(recs) == FILL).all() and (mem.get(ws) == FILL).all()
        out = ctypes.c_uint64(0)
        assert lib._f("coll_workspace_bytes")(n, 5, ctypes.byref(out)) == EINVAL
        assert lib._f("coll_workspace_bytes")(n, bits // 8, None) == EINVAL
        assert lib._f("coll_workspace_bytes")(1 << 32, 4, ctypes.byref(out)) == EINVAL
        # O(n / tile) words and a fixed part of at most 64 MB: no array of n entries
        assert lib.coll_workspace_bytes(1 << 30, bits) < (64 << 20) + (1 << 30) // 64
        # min_docs > m is no error: no record
        assert kd(S, Lp, n, 3, *G, 4, 0, 0, 0, None, 0, F, W, wsb, None) == 0 and found.value == 0
        # n = 0 succeeds with zeros, null arrays allowed
        Z = D([(0, 0), (0, 0)])
        found.value = 9
        assert kd(None, None, 0, 3, *Z, 1, 0, 0, 0, None, 0, F, None, 0, None) == 0 and found.value == 0
        found.value = 9
        assert kh(None, None, 0, 3, *Z, 1, 0, 0, 0, None, 0, F, 0) == 0 and found.value == 0
        for f, tail in ((sd, (None, 0, None)), (sh, (0,))):
            freq[:] = 9
            shared[:] = 9
            assert f(None, None, 0, 3, *Z, Fq, Sh, *tail) == 0 and not freq.any() and not shared[:4].any() and (shared[4:] == 9).all()
        freq[:] = WORD
        shared[:] = WORD


def test_refusals_and_the_empty_text():
    import caps_sa_amd
    assert caps_sa_amd.COLL_MAX_DOCS == 64 and caps_sa_amd.COLL_DTYPE.itemsize == REC
    refusal_sweep(emul(), HostMem())


# ---- 6. arrays that are no text's: a child process, the emulation only -----------------------------------------------------------------

_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [%(tests)r, %(root)r]
import caps_sa_amd
import coll_reference as R
from test_emul_coll import Form, HostMem
E = caps_sa_amd.CapsLib(%(so)r, "caps_sa_emul_")
rs = np.random.RandomState(21)
form = Form(E, HostMem())
for n in (1, 5, 4097, 16384, 40001):
    docsets = [[(0, n)], [(0, n // 3), (n // 3, n // 3), (n - n // 4, n // 4)], [(d * (n // 64), n // 64) for d in range(64)]]
    for bits in (32, 64):
        for trial in range(3):
            SA = rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
            LCP = rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
            if trial == 1:
                LCP %%= 40
                SA %%= 2 * n
            if trial == 2:
                SA %%= n
                LCP %%= 3
            if bits == 64 and trial == 0:
                SA = SA * SA
                LCP = LCP * LCP + SA
            a = form.load(SA, LCP, bits)
            for docs in docsets:
                for k in (1, 2, 17, 1 << 31, (1 << 32) + 5, (1 << 64) - 1):
                    got = form.run(a, k, docs)                  # (ends with CAPS_SA_OK, or this raises; asserts the guards)
                    freq, shared = form.sharing(a, k, docs)
                    want = list(zip(*[x.tolist() for x in R.rank_rule_np(a.sa, a.lcp, k, docs)]))
                    assert got == want, (n, bits, trial, k, len(docs))
                    wf, ws = R.summary_of([w[3] for w in want], len(docs))
                    assert freq == wf.tolist() and np.array_equal(shared, ws), (n, bits, trial, k, len(docs))
print("done")
"""


def test_garbage_arrays_terminate_inside_their_buffers():
    """SA / LCP of random 32-bit (and 64-bit) garbage: every call ends with CAPS_SA_OK, every guard is intact and the result is still
    what the rank rules give on the arrays.  In a child process, so that an access outside a buffer ends the child and not the suite.
    Never on a GPU."""
    emul()
    code = _CHILD % {"tests": os.path.join(ROOT, "tests"), "root": ROOT, "so": os.path.join(EMUL_DIR, "libcaps_sa_emul.so")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("done"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- 7. the reference's own arrays ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, k", [("dna_cli_140k", 12), ("two_letters_skewed_150k", 20), ("latin1_signed_136k", 3)])
def test_the_references_own_arrays(name, k):
    z = np.load(os.path.join(ROOT, "tests", "golden", f"large_{name}.npz"))
    T, SA, LCP = np.ascontiguousarray(z["text"]), z["sa"], z["lcp"]
    n = T.size
    # five documents of different lengths with gaps between some of them, the last one ending at n
    cut = [0, n // 7, n // 7 + 1, n // 3, n // 3, n // 2 + 11, n // 2 + 500, n - n // 5, n - n // 5, n]
    docs = [(cut[2 * d], cut[2 * d + 1] - cut[2 * d]) for d in range(5)]
    want = list(zip(*[x.tolist() for x in R.rank_rule_np(SA, LCP, k, docs)]))
    # ... tied to the text: every record's k-mer lies where its mask says, on a sample
    t = T.tobytes()
    for first, count, occ, mask in want[::max(len(want) // 200, 1)]:
        w = t[int(SA[first]):int(SA[first]) + k]
        assert len(w) == k and [d for d, (s, l) in enumerate(docs) if w in t[s:s + l]] == [d for d in range(5) if (mask >> d) & 1]
    form = Form(emul(), HostMem())
    check_case(form, form.load(SA, LCP, 32), k, docs, want, name, [dict(min_docs=5), dict(max_docs=1), dict(all_of=0b00101, none_of=0b10000)])


# ---- 8. the Python surface -----------------------------------------------------------------------------------------------------------------

def test_module_level_functions_and_dtype():
    import caps_sa_amd
    assert caps_sa_amd.COLL_DTYPE.names == ("first", "count", "occ", "docs")
    t = b"ACGTTGCAAGGCTA" + b"\xff" + b"GGCTATTGCAACGT" + b"\xff" + b"TTTT"
    docs = [(0, 14), (15, 14), (30, 4)]
    SA, LCP = (x.astype(np.uint32) for x in naive(t))
    E = emul()
    table = R.text_table(t, 3, docs)
    rec = caps_sa_amd.collection_kmers(SA, LCP, 3, docs, _lib=E)
    assert rec.dtype == caps_sa_amd.COLL_DTYPE
    assert [(t[int(SA[r["first"]]):int(SA[r["first"]]) + 3], int(r["count"]), int(r["occ"]), int(r["docs"])) for r in rec] == table
    core = caps_sa_amd.collection_kmers(SA.astype(np.uint64), LCP, 3, docs[:2], min_docs=2, _lib=E)
    assert len(core) == sum(1 for _, _, _, x in R.text_table(t, 3, docs[:2]) if x == 3) > 3
    private = caps_sa_amd.collection_kmers(SA, LCP, 3, docs, max_docs=1, all_of=4, _lib=E)
    assert [int(x) for x in private["docs"]] == [4] * len(private) and len(private) == 1
    freq, shared = caps_sa_amd.kmer_sharing(SA, LCP, 3, docs, _lib=E)
    wf, ws = R.text_summary(t, 3, docs)
    assert freq.dtype == np.uint64 and shared.shape == (3, 3) and np.array_equal(freq, wf) and np.array_equal(shared, ws)
    J = caps_sa_amd.jaccard_from_shared(shared)
    assert J[0, 0] == 1.0 and J[0, 1] == ws[0, 1] / (ws[0, 0] + ws[1, 1] - ws[0, 1]) and J[0, 2] == 0.0
    assert np.array_equal(caps_sa_amd.jaccard_from_shared(np.zeros((2, 2))), np.zeros((2, 2)))
    with pytest.raises(caps_sa_amd.CapsSaError):
        caps_sa_amd.collection_kmers(SA, LCP, 3, [(0, 20), (15, 14)], _lib=E)


# ---- 9. the other emulation builds ---------------------------------------------------------------------------------------------------

def small_sweeps(E):
    forms = forms_of(E, HostMem())
    assert short_text_sweep(forms, max_len=3, tie_rank_rule=False) == n_short_cases(3)
    assert short_text_sweep(forms, max_len=4, min_len=4, batch=21, tie_rank_rule=False) == n_short_cases(4) - n_short_cases(3)
    assert size_sweep(forms, [TILE + 1], shapes=(0, 3), parts=(3, 64), ks=(1, 2)) == 2 * 2 * 2
    edge_sweep(forms, cases=[(62, 66), (TILE - 1, TILE + 1), (TILE - 3, 3 * TILE + 2), (5, 2 * TILE), (0, EDGE_N)], widths=(32,))
    edge_sweep(forms, cases=[(LANE, 2 * LANE), (2 * TILE - 2, EDGE_N)], widths=(64,))


@pytest.mark.slow
def test_other_builds_give_the_same_answers():
    """The small sweeps once more on the build with small sort tiles, with the threads of every phase in descending order, with LDS
    and registers starting as 0xA5, and under the barrier-race detector (no race may be found)."""
    import caps_sa_amd
    small_sweeps(emul_small())
    small_sweeps(emul_rev(False))
    for name in ("libcaps_sa_emul_poison.so", "libcaps_sa_emul_race.so"):
        subprocess.check_call(["make", "-s", "-C", EMUL_DIR, name])
        path = os.path.join(EMUL_DIR, name)
        small_sweeps(caps_sa_amd.CapsLib(path, "caps_sa_emul_"))
        if "race" in name:
            raw = ctypes.CDLL(path)
            raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
            assert int(raw.caps_sa_emul_races_found()) == 0
