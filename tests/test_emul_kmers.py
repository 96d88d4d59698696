"""CPU: k-mer tables, spectra and the census from SA and LCP (include/caps_sa_hip.h "k-mers from SA and LCP", caps_sa_hip_kmers_*,
caps_sa_hip_kmer_spectrum_*, caps_sa_hip_kmer_census_*) through the host emulation of the kernels.

Every comparison is exact.  The truth is kmer_reference (collections.Counter over the text, the per-rank rule of the census); SA and
LCP come from sa_check, from a naive sort, from a closed form ('A' * n) or from the reference's own arrays under tests/golden.  The
sweeps are functions of a "form" (the host or the device entry points of a library), so that test_gpu_kmers.py runs the same ones on
the GPU.  The device form always writes into buffers preset to 0xA5 whose records start 72 bytes in (8-byte aligned, at an odd
multiple of 8) with 64 guard bytes behind them."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import kmer_reference as R
from emul_util import EMUL_DIR, ROOT, emul, emul_rev
from sa_check import sa_lcp

EINVAL = -1
FILL = 0xA5
GUARD = 64
FRONT = 72
REC = 24
SIZES = [0, 1, 2, 255, 256, 257, 16383, 16384, 16385, 32767, 32768, 32769, 49153]
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


# ---- memory of the *_device entry points: the emulation's "device" is host memory ------------------------------------------------

class HostMem:
    def filled(self, nbytes):
        return np.full(nbytes, FILL, dtype=np.uint8)

    def put(self, a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return a.copy() if a.size else np.zeros(8, dtype=np.uint8)

    def ptr(self, buf):
        return buf.ctypes.data

    def get(self, buf):
        return buf


class HostForm:
    """The host entry points (CapsLib.kmers / kmer_spectrum / kmer_census)."""
    name = "host"

    def __init__(self, lib):
        self.lib = lib

    def load(self, SA, LCP, bits):
        return (np.ascontiguousarray(SA, dtype=_dt(bits)), np.ascontiguousarray(LCP, dtype=_dt(bits)), bits)

    def table(self, h, k, min_count=1, max_count=0):
        return self.lib.kmers(h[0], h[1], k, min_count, max_count, idx_bits=h[2])

    def spectrum(self, h, k, bins):
        return self.lib.kmer_spectrum(h[0], h[1], k, bins, idx_bits=h[2])

    def census(self, h, max_k):
        return self.lib.kmer_census(h[0], h[1], max_k, idx_bits=h[2])


class DeviceForm:
    """The *_device entry points on `mem`: the counting call, then the writing call into a guarded buffer; every other call with a
    workspace of exactly kmer_workspace_bytes, itself guarded."""
    name = "device"

    def __init__(self, lib, mem):
        self.lib, self.mem = lib, mem

    def load(self, SA, LCP, bits):
        sa, lcp = np.ascontiguousarray(SA, dtype=_dt(bits)), np.ascontiguousarray(LCP, dtype=_dt(bits))
        return (self.mem.put(sa), self.mem.put(lcp), bits, int(sa.size), sa, lcp)

    def _ws(self, n, bits):
        nbytes = self.lib.kmer_workspace_bytes(n, bits)
        return self.mem.filled(nbytes + GUARD), nbytes

    def _check_inputs(self, h):
        nb = h[3] * (h[2] // 8)
        assert np.array_equal(self.mem.get(h[0])[:nb], h[4].view(np.uint8)) and np.array_equal(self.mem.get(h[1])[:nb], h[5].view(np.uint8)), \
            "SA or LCP was written"

    def table(self, h, k, min_count=1, max_count=0, own_ws=True):
        m, n, bits = self.mem, h[3], h[2]
        ws, wsb = self._ws(n, bits) if own_ws else (None, 0)
        args = (m.ptr(h[0]) if n else 0, m.ptr(h[1]) if n else 0, n, k, min_count, max_count)
        kw = dict(dWS_ptr=m.ptr(ws) if own_ws else 0, ws_bytes=wsb, idx_bits=bits)
        found = self.lib.kmers_device(*args, **kw)
        buf = m.filled(FRONT + REC * found + GUARD)
        if found:
            assert self.lib.kmers_device(*args, dRecords_ptr=m.ptr(buf) + FRONT, capacity=found, **kw) == found
        out = m.get(buf)
        assert (out[:FRONT] == FILL).all() and (out[FRONT + REC * found:] == FILL).all(), "a guard of the records was written"
        if own_ws:
            assert (m.get(ws)[wsb:] == FILL).all(), "the guard of the workspace was written"
        self._check_inputs(h)
        return out[FRONT:FRONT + REC * found].copy().view(R_DTYPE())

    def spectrum(self, h, k, bins):
        m, n, bits = self.mem, h[3], h[2]
        ws, wsb = self._ws(n, bits)
        hist = self.lib.kmer_spectrum_device(m.ptr(h[0]) if n else 0, m.ptr(h[1]) if n else 0, n, k, bins, m.ptr(ws), wsb, idx_bits=bits)
        assert (m.get(ws)[wsb:] == FILL).all(), "the guard of the workspace was written"
        return hist

    def census(self, h, max_k):
        m, n, bits = self.mem, h[3], h[2]
        ws, wsb = self._ws(n, bits)
        out = self.lib.kmer_census_device(m.ptr(h[0]) if n else 0, m.ptr(h[1]) if n else 0, n, max_k, m.ptr(ws), wsb, idx_bits=bits)
        assert (m.get(ws)[wsb:] == FILL).all(), "the guard of the workspace was written"
        return out


def R_DTYPE():
    import caps_sa_amd
    return caps_sa_amd.KMER_DTYPE


def forms_of(lib, mem):
    return (HostForm(lib), DeviceForm(lib, mem))


# ---- the checks --------------------------------------------------------------------------------------------------------------------

def check_table(T, SA, rec, want, k, occurrences=False):
    """rec against want = [(k-mer bytes, count)]: bytes through pos, the count, first = the head's rank, rank order."""
    t = T.tobytes()
    assert rec.size == len(want), (rec.size, len(want), k)
    if not rec.size:
        return
    pos, cnt, first = rec["pos"].tolist(), rec["count"].tolist(), rec["first"].tolist()
    assert cnt == [c for _, c in want], k
    assert [t[p:p + k] for p in pos] == [m for m, _ in want], k
    assert SA[rec["first"].astype(np.int64)].tolist() == pos
    assert all(a + c <= b for a, c, b in zip(first, cnt, first[1:] + [len(t)])), "runs overlap or leave the array"
    last = (rec["first"] + rec["count"] - 1).astype(np.int64)
    assert [t[p:p + k] for p in SA[last].tolist()] == [m for m, _ in want], "the last rank of a run is another k-mer"
    if occurrences:
        for (m, c), f in zip(want, first):
            assert sorted(SA[f:f + c].tolist()) == R.positions(t, m)


def check_all(form, T, SA, LCP, bits, ks, tables, occurrences=False):
    """Table, spectrum (1024 bins) and the census's identities for every k of ks; tables: a cache {k: reference table}."""
    n = T.size
    h = form.load(SA, LCP, bits)
    max_k = min(max(max(ks), 1), 1024)
    distinct, unique = form.census(h, max_k)
    assert distinct[0] == 0 and unique[0] == 0
    for k in ks:
        if k < 1:
            continue
        if k not in tables:
            tables[k] = R.table(T, k)
        want = tables[k]
        check_table(T, SA, form.table(h, k), want, k, occurrences)
        hist = form.spectrum(h, k, 1024)
        ref = np.zeros(1025, dtype=np.uint64)
        for _, c in want:
            ref[min(c, 1024)] += 1
        assert np.array_equal(hist, ref), (k, n)
        if k <= max_k:
            assert int(distinct[k]) == len(want) == int(hist.sum()), (k, n)
            assert int(unique[k]) == int(hist[1]) == sum(1 for _, c in want if c == 1), (k, n)
    return distinct, unique


def naive_sa_lcp(t: bytes):
    n = len(t)
    sa = sorted(range(n), key=lambda i: R.signed_key(t[i:]))
    lcp = [0] * n
    for r in range(1, n):
        a, b, ln = sa[r - 1], sa[r], 0
        while a + ln < n and b + ln < n and t[a + ln] == t[b + ln]:
            ln += 1
        lcp[r] = ln
    return np.array(sa, dtype=np.uint64), np.array(lcp, dtype=np.uint64)


def texts_of(n, seed=1):
    """(name, T, SA, LCP) for the three families at size n."""
    rs = np.random.RandomState(seed + n)
    yield "a^n", np.full(n, ord("A"), dtype=np.uint8), np.arange(n, dtype=np.uint64)[::-1].copy(), np.arange(n, dtype=np.uint64)
    for name, letters in (("two", DNA[:2]), ("four", DNA)):
        T = rs.choice(letters, size=n).astype(np.uint8)
        SA, LCP = sa_lcp(T, 64)
        yield name, T, SA, LCP


def ks_of(n):
    return sorted({k for k in (1, 2, 3, 8, 31, 32, 33, n - 1, n, n + 1) if k >= 1})


def size_sweep(forms, sizes, widths=(32, 64)):
    """Every size x text family x k x width through every form."""
    done = 0
    for n in sizes:
        for name, T, SA, LCP in texts_of(n):
            tables = {}
            for form, bits in itertools.product(forms, widths):
                distinct, unique = check_all(form, T, SA, LCP, bits, ks_of(n), tables)
                if name == "a^n" and n:
                    h = form.load(SA, LCP, bits)
                    for k in ks_of(n):                  # the closed form: one run across all tiles
                        rec = form.table(h, k)
                        if k <= n:
                            assert rec.tolist() == [(k - 1, n - k + 1, n - k)], (n, k)
                        else:
                            assert rec.size == 0
                    assert distinct[1:min(n, 1024) + 1].tolist() == [1] * min(n, 1024)
                done += 1
    return done


def census_sweep(forms, n=3000, widths=(32, 64)):
    """max_k = 1 and 1024 against the per-rank rule and against Counter; bins = 1, 2, 1024 against Counter."""
    rs = np.random.RandomState(9)
    T = rs.choice(DNA[:2], size=n).astype(np.uint8)
    T[100:1400] = T[1500:2800]                          # a long repeat: counts of 2 up to k = 1300
    SA, LCP = sa_lcp(T, 64)
    by_rank = R.census_by_rank(SA, LCP, 1024)
    by_counter = R.census_by_counter(T, 40)
    assert np.array_equal(by_rank[0][:41], by_counter[0]) and np.array_equal(by_rank[1][:41], by_counter[1])
    for form, bits in itertools.product(forms, widths):
        h = form.load(SA, LCP, bits)
        for max_k in (1, 2, 40, 1023, 1024):
            d, u = form.census(h, max_k)
            assert np.array_equal(d, by_rank[0][:max_k + 1]) and np.array_equal(u, by_rank[1][:max_k + 1]), max_k
        for k in (1, 2, 11):
            for bins in (1, 2, 3, 1024):
                assert np.array_equal(form.spectrum(h, k, bins), R.spectrum(T, k, bins)), (k, bins)


def filter_sweep(forms, n=20000, widths=(32, 64)):
    """min_count / max_count = 0, 1, 2, the largest count and one above it, in every combination that is not refused."""
    rs = np.random.RandomState(4)
    T = rs.choice(DNA, size=n, p=[0.55, 0.25, 0.15, 0.05]).astype(np.uint8)
    SA, LCP = sa_lcp(T, 64)
    for k in (1, 3, 6):
        full = R.table(T, k)
        top = max(c for _, c in full)
        for form, bits in itertools.product(forms, widths):
            h = form.load(SA, LCP, bits)
            for lo, hi in itertools.product((0, 1, 2, top, top + 1), (0, 1, 2, top, top + 1)):
                if hi and lo > hi:
                    continue
                check_table(T, SA, form.table(h, k, lo, hi), R.table(T, k, lo, hi), k)


# ---- 1. every short text ------------------------------------------------------------------------------------------------------------

LETTERS3 = bytes([0x41, 0x43, 0xC8])                     # (0xC8 sorts first: signed char)


def short_text_sweep(forms, max_len=7, widths=(32, 64)):
    done = 0
    for n in range(1, max_len + 1):
        for tup in itertools.product(LETTERS3, repeat=n):
            t = bytes(tup)
            T = np.frombuffer(t, dtype=np.uint8)
            SA, LCP = naive_sa_lcp(t)
            want = R.census_by_counter(t, n + 2)
            tables = {}
            for form, bits in itertools.product(forms, widths):
                d, u = check_all(form, T, SA, LCP, bits, range(1, n + 3), tables, occurrences=True)
                assert np.array_equal(d, want[0]) and np.array_equal(u, want[1]), t
                done += 1
    return done


@pytest.mark.slow
def test_every_short_text_and_every_k():
    E = emul()
    assert short_text_sweep((HostForm(E),)) == 2 * sum(3 ** n for n in range(1, 8))
    assert short_text_sweep((DeviceForm(E, HostMem()),), max_len=5) == 2 * sum(3 ** n for n in range(1, 6))


# ---- 2. sizes around one, two and three tiles ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_sizes_texts_and_ks(n):
    E = emul()
    assert size_sweep(forms_of(E, HostMem()), [n]) == 3 * 4


def test_census_and_bins():
    census_sweep(forms_of(emul(), HostMem()))


def test_count_filters():
    filter_sweep(forms_of(emul(), HostMem()))


# ---- 3. the counting call, the writing call, the capacity ---------------------------------------------------------------------------

def capacity_sweep(lib, mem, widths=(32, 64)):
    rs = np.random.RandomState(12)
    n = 40000
    T = rs.choice(DNA, size=n).astype(np.uint8)
    SA, LCP = sa_lcp(T, 64)
    want = R.table(T, 5, 2)
    for bits in widths:
        form = DeviceForm(lib, mem)
        h = form.load(SA, LCP, bits)
        args = (mem.ptr(h[0]), mem.ptr(h[1]), n, 5, 2, 0)
        found = lib.kmers_device(*args, idx_bits=bits)
        assert found == len(want) > 1
        buf = mem.filled(FRONT + REC * found + GUARD)
        with pytest.raises(Exception) as e:                 # one too small: refused, the number is still there, nothing is written
            lib.kmers_device(*args, dRecords_ptr=mem.ptr(buf) + FRONT, capacity=found - 1, idx_bits=bits)
        assert e.value.code == EINVAL and e.value.n_records == found
        assert (mem.get(buf) == FILL).all()
        assert lib.kmers_device(*args, dRecords_ptr=mem.ptr(buf) + FRONT, capacity=found + 3, idx_bits=bits) == found     # more room than needed
        out = mem.get(buf)
        assert (out[:FRONT] == FILL).all() and (out[FRONT + REC * found:] == FILL).all()
        check_table(T, SA, out[FRONT:FRONT + REC * found].copy().view(R_DTYPE()), want, 5)
        check_table(T, SA, form.table(h, 5, 2, own_ws=False), want, 5)          # a NULL workspace: the call's own
        # the host form's protocol
        sa, lcp = SA.astype(_dt(bits)), LCP.astype(_dt(bits))
        sfx = "u32" if bits == 32 else "u64"
        nrec = ctypes.c_uint64(7)
        rec = np.full(REC * found + GUARD, FILL, dtype=np.uint8)
        f = lib._f(f"kmers_{sfx}")
        assert f(sa.ctypes.data, lcp.ctypes.data, n, 5, 2, 0, None, 0, ctypes.byref(nrec), 0) == 0 and nrec.value == found
        nrec.value = 7
        assert f(sa.ctypes.data, lcp.ctypes.data, n, 5, 2, 0, rec.ctypes.data, found - 1, ctypes.byref(nrec), 0) == EINVAL and nrec.value == found
        assert (rec == FILL).all()
        assert f(sa.ctypes.data, lcp.ctypes.data, n, 5, 2, 0, rec.ctypes.data, found, ctypes.byref(nrec), 0) == 0 and nrec.value == found
        assert (rec[REC * found:] == FILL).all()
        check_table(T, SA, rec[:REC * found].copy().view(R_DTYPE()), want, 5)


def test_counting_call_writing_call_and_capacity():
    capacity_sweep(emul(), HostMem())


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------

def refusal_sweep(lib, mem):
    """Every refusal: CAPS_SA_EINVAL, and no output is touched."""
    n = 1000
    T = np.random.RandomState(3).choice(DNA, size=n).astype(np.uint8)
    SA, LCP = sa_lcp(T, 64)
    for bits in (32, 64):
        sfx = "u32" if bits == 32 else "u64"
        sa, lcp = SA.astype(_dt(bits)), LCP.astype(_dt(bits))
        dsa, dlcp = mem.put(sa), mem.put(lcp)
        S, Lp = mem.ptr(dsa), mem.ptr(dlcp)
        wsb = lib.kmer_workspace_bytes(n, bits)
        ws = mem.filled(wsb)
        W = mem.ptr(ws)
        recs = mem.filled(REC * n)
        Rp = mem.ptr(recs)
        nrec = ctypes.c_uint64(0x5A5A)
        hist = np.full(1026, 0x5A5A, dtype=np.uint64)
        d, u = hist.copy(), hist.copy()
        nr, H, D, U = ctypes.byref(nrec), hist.ctypes.data, d.ctypes.data, u.ctypes.data
        kd, sd, cd = lib._f(f"kmers_device_{sfx}"), lib._f(f"kmer_spectrum_device_{sfx}"), lib._f(f"kmer_census_device_{sfx}")
        kh, sh, ch = lib._f(f"kmers_{sfx}"), lib._f(f"kmer_spectrum_{sfx}"), lib._f(f"kmer_census_{sfx}")
        hs, hl = sa.ctypes.data, lcp.ctypes.data
        calls = [
            kd(S, Lp, n, 0, 1, 0, Rp, n, nr, W, wsb, None),                    # k = 0
            kd(S, Lp, n, 3, 5, 4, Rp, n, nr, W, wsb, None),                    # min_count > max_count > 0
            kd(None, Lp, n, 3, 1, 0, Rp, n, nr, W, wsb, None),                 # null pointers with n > 0
            kd(S, None, n, 3, 1, 0, Rp, n, nr, W, wsb, None),
            kd(S, Lp, n, 3, 1, 0, Rp, n, None, W, wsb, None),
            kd(S, Lp, n, 3, 1, 0, Rp + 4, n, nr, W, wsb, None),                # records not 8-byte aligned
            kd(S, Lp, n, 3, 1, 0, Rp, n, nr, W, wsb - 512, None),              # a workspace that is too small
            sd(S, Lp, n, 0, 16, H, W, wsb, None),
            sd(S, Lp, n, 3, 0, H, W, wsb, None),                               # bins outside 1 .. 1024
            sd(S, Lp, n, 3, 1025, H, W, wsb, None),
            sd(None, Lp, n, 3, 16, H, W, wsb, None),
            sd(S, Lp, n, 3, 16, None, W, wsb, None),
            sd(S, Lp, n, 3, 16, H, W, wsb - 512, None),
            cd(S, Lp, n, 0, D, U, W, wsb, None),                               # max_k outside 1 .. 1024
            cd(S, Lp, n, 1025, D, U, W, wsb, None),
            cd(S, None, n, 8, D, U, W, wsb, None),
            cd(S, Lp, n, 8, None, U, W, wsb, None),
            cd(S, Lp, n, 8, D, None, W, wsb, None),
            cd(S, Lp, n, 8, D, U, W, wsb - 512, None),
            kh(hs, hl, n, 0, 1, 0, None, 0, nr, 0),
            kh(hs, hl, n, 3, 5, 4, None, 0, nr, 0),
            kh(None, hl, n, 3, 1, 0, None, 0, nr, 0),
            kh(hs, hl, n, 3, 1, 0, None, 0, None, 0),
            sh(hs, hl, n, 0, 16, H, 0),
            sh(hs, hl, n, 3, 0, H, 0),
            sh(hs, hl, n, 3, 1025, H, 0),
            sh(hs, None, n, 3, 16, H, 0),
            ch(hs, hl, n, 0, D, U, 0),
            ch(hs, hl, n, 1025, D, U, 0),
            ch(None, hl, n, 8, D, U, 0),
        ]
        if bits == 32:                                       # n > UINT32_MAX with _u32: refused before anything is read
            big = 1 << 32
            calls += [kd(S, Lp, big, 3, 1, 0, None, 0, nr, None, 0, None), sd(S, Lp, big, 3, 16, H, None, 0, None),
                      cd(S, Lp, big, 8, D, U, None, 0, None), kh(hs, hl, big, 3, 1, 0, None, 0, nr, 0), sh(hs, hl, big, 3, 16, H, 0),
                      ch(hs, hl, big, 8, D, U, 0)]
        assert calls == [EINVAL] * len(calls), calls
        assert nrec.value == 0x5A5A and (hist == 0x5A5A).all() and (d == 0x5A5A).all() and (u == 0x5A5A).all()
        assert (mem.get(recs) == FILL).all() and (mem.get(ws) == FILL).all()
        out = ctypes.c_uint64(0)
        assert lib._f("kmer_workspace_bytes")(n, 5, ctypes.byref(out)) == EINVAL
        assert lib._f("kmer_workspace_bytes")(n, bits // 8, None) == EINVAL
        assert lib._f("kmer_workspace_bytes")(1 << 32, 4, ctypes.byref(out)) == EINVAL
        # n = 0 succeeds with zeros, null arrays allowed
        assert kd(None, None, 0, 3, 1, 0, None, 0, nr, None, 0, None) == 0 and nrec.value == 0
        assert sd(None, None, 0, 3, 16, H, None, 0, None) == 0 and (hist[:17] == 0).all() and hist[17] == 0x5A5A
        assert cd(None, None, 0, 8, D, U, None, 0, None) == 0 and (d[:9] == 0).all() and (u[:9] == 0).all() and d[9] == 0x5A5A
        nrec.value = 9
        assert kh(None, None, 0, 3, 1, 0, None, 0, nr, 0) == 0 and nrec.value == 0
        hist[:] = 7
        assert sh(None, None, 0, 3, 4, H, 0) == 0 and hist[:6].tolist() == [0] * 5 + [7]
        d[:] = 7
        u[:] = 7
        assert ch(None, None, 0, 2, D, U, 0) == 0 and d[:4].tolist() == [0, 0, 0, 7] and u[:4].tolist() == [0, 0, 0, 7]


def test_refusals_and_the_empty_text():
    refusal_sweep(emul(), HostMem())


# ---- 5. arrays that are no SA / LCP: a child process, the emulation only --------------------------------------------------------------

_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [%(tests)r, %(root)r]
import caps_sa_amd
from test_emul_kmers import DeviceForm, HostMem
E = caps_sa_amd.CapsLib(%(so)r, "caps_sa_emul_")
rs = np.random.RandomState(21)
form = DeviceForm(E, HostMem())
for n in (1, 5, 4097, 16384, 40001):
    for bits in (32, 64):
        for trial in range(3):
            SA = rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
            LCP = rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
            if trial == 1:
                LCP %%= 40
            if trial == 2:
                SA %%= n
                LCP %%= 3
            if bits == 64 and trial == 0:
                SA = SA * SA
                LCP = LCP * LCP + SA
            h = form.load(SA, LCP, bits)
            for k in (1, 2, 17, n, n + 1, 1 << 31, (1 << 32) + 5):
                rec = form.table(h, k)                      # (ends with CAPS_SA_OK, or this raises; asserts the guards)
                assert rec.size <= n
                form.table(h, k, 2, 0)
                form.spectrum(h, k, 3)
                form.spectrum(h, k, 1024)
            form.census(h, 1)
            form.census(h, 1024)
print("done")
"""


def test_garbage_arrays_terminate_inside_their_buffers():
    """SA / LCP of random 32-bit (and 64-bit) garbage: every call ends with CAPS_SA_OK and every guard is intact.  In a child process,
    so that an access outside a buffer ends the child and not the suite.  Never on a GPU."""
    emul()
    code = _CHILD % {"tests": os.path.join(ROOT, "tests"), "root": ROOT, "so": os.path.join(EMUL_DIR, "libcaps_sa_emul.so")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("done"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- 6. the reference's own arrays ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["large_dna_cli_140k", "large_latin1_signed_136k"])
def test_the_references_own_arrays(name):
    """(text, sa, lcp) made by the reference's script: the table at k = 1, 4, 12 and 31 against Counter over the text.  The latin1
    file pins the signed-char order."""
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    T, SA, LCP = np.ascontiguousarray(z["text"], dtype=np.uint8), z["sa"], z["lcp"]
    assert SA.size == T.size == LCP.size
    if "latin1" in name:
        assert (T >= 0x80).any() and (T < 0x80).any()
    form = HostForm(emul())
    h = form.load(SA, LCP, 32)
    SA64 = SA.astype(np.int64)
    for k in (1, 4, 12, 31):
        check_table(T, SA64, form.table(h, k), R.table(T, k), k)
    want2 = R.table(T, 12, 2, 3)
    check_table(T, SA64, DeviceForm(emul(), HostMem()).table(DeviceForm(emul(), HostMem()).load(SA, LCP, 64), 12, 2, 3), want2, 12)


# ---- 7. the Python surface -------------------------------------------------------------------------------------------------------------

def test_module_level_functions_and_dtype():
    import caps_sa_amd
    assert caps_sa_amd.KMER_DTYPE.itemsize == 24 and caps_sa_amd.KMER_DTYPE.names == ("first", "count", "pos")
    t = b"GATTACAGATTACA"
    T = np.frombuffer(t, dtype=np.uint8)
    SA, LCP = naive_sa_lcp(t)
    E = emul()
    rec = caps_sa_amd.kmers(SA.astype(np.uint32), LCP.astype(np.uint32), 4, _lib=E)
    check_table(T, SA.astype(np.int64), rec, R.table(t, 4), 4, occurrences=True)
    assert np.array_equal(caps_sa_amd.kmer_spectrum(SA, LCP, 4, bins=8, _lib=E), R.spectrum(t, 4, 8))
    d, u = caps_sa_amd.kmer_census(SA, LCP, 14, _lib=E)
    want = R.census_by_counter(t, 14)
    assert np.array_equal(d, want[0]) and np.array_equal(u, want[1])
    assert caps_sa_amd.kmers(SA, LCP, 4, min_count=2, _lib=E)["count"].tolist() == [c for _, c in R.table(t, 4, 2)]


# ---- 8. the other emulation builds ---------------------------------------------------------------------------------------------------

def small_sweeps(E):
    forms = forms_of(E, HostMem())
    assert short_text_sweep(forms, max_len=4, widths=(32,)) == 2 * sum(3 ** n for n in range(1, 5))
    assert size_sweep(forms, [257, 16385, 32769]) == 3 * 3 * 4
    census_sweep(forms, widths=(64,))


@pytest.mark.slow
def test_other_builds_give_the_same_answers():
    """The small sweeps once more with the threads of every phase in descending order, with LDS and registers starting as 0xA5 and
    the threads in a scattered order, and under the barrier-race detector (no race may be found)."""
    import caps_sa_amd
    small_sweeps(emul_rev(False))
    for name in ("libcaps_sa_emul_small_poison.so", "libcaps_sa_emul_small_race.so"):
        subprocess.check_call(["make", "-s", "-C", EMUL_DIR, name])
        path = os.path.join(EMUL_DIR, name)
        small_sweeps(caps_sa_amd.CapsLib(path, "caps_sa_emul_"))
        if "race" in name:
            raw = ctypes.CDLL(path)
            raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
            assert int(raw.caps_sa_emul_races_found()) == 0
