"""CPU: MUMs and rare MEMs between two texts from SA, LCP and BWT (include/caps_sa_hip.h "MUMs and MEMs between two texts",
caps_sa_hip_cross_mums_*, caps_sa_hip_cross_mems_*) through the host emulation of the kernels.

Every comparison is exact: the records byte for byte, in the header's order, and all 8 summary words.  The truth of the small texts is
cross_reference's first half (the text definitions: all pairs, extensions by comparing bytes, occurrence counts by substring search);
the larger cases use its numpy restatement of the rank rules, which the small texts tie to the brute force.  The sweeps are functions
of a "form" (the host or the device entry points of a library on some memory), so that test_gpu_cross.py runs the same ones on the GPU.
The device form works on buffers preset to 0xA5: the records start 72 bytes in (8-byte aligned, at an odd multiple of 8) with 64 guard
bytes behind them, and the workspace has exactly caps_sa_hip_cross_workspace_bytes with a guard behind it.

Which test pins which sentence of the header:
  inputs, left-maximal, MUM rules 1 - 4, MEM runs / pairs / "each exactly once", the records and their order, summary [0] .. [7] with
  the LCS tie rule                      test_every_short_text_both_modes_against_the_text_definitions, test_short_texts_quick
  LCP[0] counts as 0; the byte at the rank with SA == 0 is never looked at; split = 0 / 1 / n - 1 / n; no separator: still the
  rules' result                         test_split_at_the_ends_sa_zero_in_a_pair_and_no_separator
  tiles and their edges, the halo       test_sizes_and_text_shapes, test_mum_ranks_on_the_tile_edges,
                                        test_mem_runs_across_the_tile_edges_and_skipped_runs_counted_once
  longer runs skipped and counted once, 'A' * n is one run
                                        test_mem_runs_across_the_tile_edges_and_skipped_runs_counted_once, test_sizes_and_text_shapes
  the counting call, the capacity, the summary still valid, a NULL workspace
                                        test_counting_call_writing_call_and_capacity
  every refusal with nothing written, n = 0, the workspace's size, CAPS_SA_CROSS_MAX_OCC
                                        test_refusals_and_the_empty_text
  arrays that are no text's: termination, reads and writes inside the buffers, bounded work
                                        test_garbage_arrays_terminate_inside_their_buffers
  the device pointers and the stream    tests/test_gpu_cross.py"""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import cross_reference as R
from emul_util import EMUL_DIR, ROOT, emul, emul_rev
from sa_check import sa_lcp

EINVAL = -1
FILL = 0xA5
GUARD = 64
FRONT = 72
REC = 24
TILE = 16384                                                # ranks of a tile of xm_kernel (kernels.h XM_TILE)
SIZES = [t * TILE + d for t in (1, 2, 3) for d in (-1, 0, 1)]
EDGES = (TILE, 2 * TILE, 3 * TILE)
MAX_OCC = 64
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
LETTERS3 = bytes([0x41, 0x43, 0xC8])                     # (0xC8 sorts first: signed char)
SEPS = (0x80, 0x7F)                                      # the lowest and the highest byte in signed-char order


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
    """SA, LCP (in the index width) and BWT of one case, on the host and -- for the device form -- on `mem`."""

    def __init__(self, SA, LCP, BWT, bits, mem=None):
        self.bits, self.n = bits, int(len(SA))
        self.sa = np.ascontiguousarray(SA, dtype=_dt(bits))
        self.lcp = np.ascontiguousarray(LCP, dtype=_dt(bits))
        self.bwt = np.ascontiguousarray(BWT, dtype=np.uint8)
        assert self.lcp.size == self.n == self.bwt.size
        self.mem = mem
        if mem is not None:
            self.d = [mem.put(self.sa), mem.put(self.lcp), mem.put(self.bwt)]


class Form:
    """One family of entry points: the counting call, then the writing call into a guarded buffer; both summaries must agree."""

    def __init__(self, lib, mem=None):
        self.lib, self.mem = lib, mem
        self.name = "device" if mem is not None else "host"

    def load(self, SA, LCP, BWT, bits):
        return Arrays(SA, LCP, BWT, bits, self.mem)

    def fn(self, mode, bits):
        return self.lib._f(f"cross_{mode}{'_device' if self.mem is not None else ''}_{'u32' if bits == 32 else 'u64'}")

    def call(self, a, mode, split, min_len, max_occ, rec_ptr, capacity, summary, ws=None):
        """The raw return code of one call."""
        occ = (max_occ,) if mode == "mems" else ()
        if self.mem is None:
            p = [x.ctypes.data if a.n else None for x in (a.sa, a.lcp, a.bwt)]
            return self.fn(mode, a.bits)(*p, a.n, split, min_len, *occ, rec_ptr or None, capacity, summary.ctypes.data, 0)
        p = [self.mem.ptr(x) if a.n else None for x in a.d]
        w, wb = (self.mem.ptr(ws[0]), ws[1]) if ws else (None, 0)
        return self.fn(mode, a.bits)(*p, a.n, split, min_len, *occ, rec_ptr or None, capacity, summary.ctypes.data, w, wb, None)

    def run(self, a, mode, split, min_len, max_occ=MAX_OCC, own_ws=True):
        """(records as a list of (a, b, len), summary as a list of 8 ints)."""
        m = self.mem
        ws = None
        if m is not None and own_ws:
            wb = self.lib.cross_workspace_bytes(a.n, a.bits)
            ws = (m.filled(wb + GUARD), wb)
        s1 = np.full(8, 0x5A5A, dtype=np.uint64)
        assert self.call(a, mode, split, min_len, max_occ, 0, 0, s1, ws) == 0, self.lib._f("last_error")()
        found = int(s1[0])
        s2 = np.full(8, 0x5A5A, dtype=np.uint64)
        nbytes = FRONT + REC * found + GUARD
        if m is None:
            buf = np.full(nbytes, FILL, dtype=np.uint8)
            assert self.call(a, mode, split, min_len, max_occ, buf.ctypes.data + FRONT, found, s2) == 0
            out = buf
        else:
            buf = m.filled(nbytes)
            assert self.call(a, mode, split, min_len, max_occ, m.ptr(buf) + FRONT, found, s2, ws) == 0
            out = m.get(buf)
            if ws:
                assert (m.get(ws[0])[ws[1]:] == FILL).all(), "the guard of the workspace was written"
            for dev, host in zip(a.d, (a.sa, a.lcp, a.bwt)):
                assert np.array_equal(m.get(dev)[:host.nbytes], host.view(np.uint8)), "an input array was written"
        assert (out[:FRONT] == FILL).all() and (out[FRONT + REC * found:] == FILL).all(), "a guard of the records was written"
        assert s1.tolist() == s2.tolist(), "the counting call and the writing call disagree"
        assert s2[5:].tolist() == [0, 0, 0]
        rec = out[FRONT:FRONT + REC * found].copy().view("<u8").reshape(-1, 3)
        return [tuple(r) for r in rec.tolist()], s2.tolist()


def forms_of(lib, mem):
    return (Form(lib), Form(lib, mem))


def bwt_of(T, SA):
    T = np.asarray(T, dtype=np.uint8)
    return T[(np.asarray(SA).astype(np.int64) - 1) % max(T.size, 1)] if T.size else T


CONFIGS = [("mums", L, None) for L in (1, 2, 3, 4)] + [("mems", L, c) for L in (1, 2, 3, 4) for c in (2, 3, 64)]


# ---- 1. every short text, against the text definitions --------------------------------------------------------------------------------

def text_truth(t: bytes, split: int):
    """Everything the configurations of one text need, from the text definitions: {config: (records in the header's order, summary)}."""
    SA, LCP, BWT = R.naive_sa_lcp_bwt(t)
    rank = {p: r for r, p in enumerate(SA)}
    every = R.all_mems(t, split)
    best, at = R.lcs(t, split)
    summary_lcs = [0, 0, 0]
    if best:
        a, b = min((p for p in at if abs(rank[p[0]] - rank[p[1]]) == 1), key=lambda p: max(rank[p[0]], rank[p[1]]))
        summary_lcs = [best, a, b]
    occ = {}

    def occurrences(w):
        if w not in occ:
            occ[w] = R.occurrences(t, w)
        return occ[w]

    truth = {}
    for mode, L, c in CONFIGS:
        if mode == "mums":
            rec = [(a, b, l) for a, b, l in every if l >= L and occurrences(t[a:a + l]) == 2]
            rec.sort(key=lambda x: max(rank[x[0]], rank[x[1]]))
            skipped = 0
        else:
            rec = [(a, b, l) for a, b, l in every if l >= L and occurrences(t[a:a + L]) <= c]
            rec.sort(key=lambda x: (max(rank[x[0]], rank[x[1]]), -min(rank[x[0]], rank[x[1]])))
            skipped = sum(1 for w in {t[i:i + L] for i in range(len(t) - L + 1)} if occurrences(w) > c)
        truth[(mode, L, c)] = (rec, [len(rec), skipped] + summary_lcs + [0, 0, 0])
    return (SA, LCP, BWT), truth


def short_text_sweep(forms, max_len=7, widths=(32, 64), seps=SEPS, tie_rank_rule=True):
    """Every A . sep . B with |A| + |B| <= max_len over 3 letters x every configuration x width x form -> the number of texts."""
    done = 0
    for sep in seps:
        for la, lb in ((la, lb) for la in range(max_len + 1) for lb in range(max_len + 1 - la)):
            for A in itertools.product(LETTERS3, repeat=la):
                for B in itertools.product(LETTERS3, repeat=lb):
                    t = bytes(A) + bytes([sep]) + bytes(B)
                    split = la + 1
                    (SA, LCP, BWT), truth = text_truth(t, split)
                    if tie_rank_rule:
                        for (mode, L, c), want in truth.items():
                            assert R.rank_rule(SA, LCP, BWT, split, L, c) == want, (t, mode, L, c)
                    for form, bits in itertools.product(forms, widths):
                        a = form.load(SA, LCP, BWT, bits)
                        for (mode, L, c), want in truth.items():
                            assert form.run(a, mode, split, L, c) == want, (t, mode, L, c, form.name, bits)
                    done += 1
    return done


def n_short_texts(max_len):
    return sum((L + 1) * 3 ** L for L in range(max_len + 1))


@pytest.mark.slow
@pytest.mark.parametrize("sep", SEPS)
def test_every_short_text_both_modes_against_the_text_definitions(sep):
    """Rules 1-4 of MUM mode, the runs, pairs and order of MEM mode, the record layout, the skipped-run count and the longest common
    substring with its tie rule: |A| + |B| <= 7 over 3 letters, min_len 1 .. 4, max_occ 2 / 3 / 64, both widths, host and device."""
    assert short_text_sweep(forms_of(emul(), HostMem()), seps=(sep,)) == n_short_texts(7)


def test_short_texts_quick():
    assert short_text_sweep(forms_of(emul(), HostMem()), max_len=4) == 2 * n_short_texts(4)


# ---- 2. sizes around one, two and three tiles ------------------------------------------------------------------------------------------

def texts_of(n, seed=1):
    """(name, SA, LCP, BWT, split) for the three shapes at size n: 'A' * n (no separator: the rank rules alone), random letters
    around a separator, and B = A with planted substitutions."""
    rs = np.random.RandomState(seed + n)
    T = np.full(n, ord("A"), dtype=np.uint8)
    SA = np.arange(n, dtype=np.uint64)[::-1].copy()
    yield "a^n", SA, np.arange(n, dtype=np.uint64), bwt_of(T, SA), n // 2
    for name, letters in (("two", DNA[:2]), ("four", DNA)):
        T = rs.choice(letters, size=n).astype(np.uint8)
        split = n // 3 + 1
        T[split - 1] = 0xFF
        SA, LCP = sa_lcp(T, 64)
        yield name, SA, LCP, bwt_of(T, SA), split
    half = (n - 1) // 2
    A = rs.choice(DNA, size=half).astype(np.uint8)
    B = A.copy()
    for at in range(13, half, 97):
        B[at] = DNA[(int(np.searchsorted(DNA, B[at])) + 1 + at % 3) % 4]
    T = np.concatenate([A, np.array([0xFF], dtype=np.uint8), B, rs.choice(DNA, size=n - 1 - 2 * half).astype(np.uint8)])
    SA, LCP = sa_lcp(T, 64)
    yield "planted", SA, LCP, bwt_of(T, SA), half + 1


def size_sweep(forms, sizes, widths=(32, 64), configs=(("mums", 1, None), ("mums", 12, None), ("mems", 1, 2), ("mems", 6, 3), ("mems", 11, 64))):
    done = 0
    for n in sizes:
        for name, SA, LCP, BWT, split in texts_of(n):
            want = {c: R.rank_rule(SA, LCP, BWT, split, c[1], c[2]) for c in configs}
            if name == "a^n":                                   # one run across all tiles: skipped, counted once
                assert want[("mems", 1, 2)] == ([], [0, 1, n - n // 2, n // 2 - 1, n // 2, 0, 0, 0])
            if name == "planted":
                assert want[("mums", 12, None)][1][0] > n // 300 and want[("mems", 11, 64)][1][0] >= want[("mums", 12, None)][1][0]
            for form, bits in itertools.product(forms, widths):
                a = form.load(SA, LCP, BWT, bits)
                for c in configs:
                    assert form.run(a, c[0], split, c[1], c[2]) == want[c], (n, name, c, form.name, bits)
                done += 1
    return done


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_text_shapes(n):
    assert size_sweep(forms_of(emul(), HostMem()), [n]) == 4 * 4


# ---- 3. tile edges: arrays of the test's own making (no text's) -------------------------------------------------------------------------

def blank(n, seed):
    """LCP all zero, SA and BWT random: no rank yields anything until a case plants it."""
    rs = np.random.RandomState(seed)
    return rs.randint(1, 1 << 20, size=n).astype(np.uint64), np.zeros(n, dtype=np.uint64), rs.choice(DNA[:2], size=n).astype(np.uint8)


def mum_edge_sweep(forms, widths=(32, 64)):
    """A MUM rank on each of the first three tile edges, one before and one after; its neighbours' LCP one below it, and once equal
    (rule 3 then fails on that side)."""
    n, split = 3 * TILE + 50, 20000
    done = 0
    for d in (-1, 0, 1):
        SA, LCP, BWT = blank(n, 5 + d)
        want_rec = []
        for k, e in enumerate(EDGES):
            r = e + d
            LCP[r - 1], LCP[r], LCP[r + 1] = 6, 7, (6 if k != 1 else 7)          # (the middle edge: equal behind -- no record)
            SA[r - 1], SA[r] = (split + 5 + k, 100 + k) if k != 2 else (200, split + 9)
            BWT[r - 1], BWT[r] = ord("A"), ord("C")
            if k != 1:
                want_rec.append((min(int(SA[r - 1]), int(SA[r])), max(int(SA[r - 1]), int(SA[r])), 7))
        want = R.rank_rule(SA, LCP, BWT, split, 7, None)
        assert want[0] == want_rec and want[1][2] == 7
        for form, bits in itertools.product(forms, widths):
            assert form.run(form.load(SA, LCP, BWT, bits), "mums", split, 7) == want, (d, form.name, bits)
            done += 1
    return done


def mem_edge_sweep(forms, occs=(2, 3, 64), widths=(32, 64)):
    """Runs of exactly max_occ ranks (processed) and of max_occ + 1 ranks (skipped, counted once each), placed so that a tile edge
    falls at every offset inside them."""
    n, split, L = 3 * TILE + 200, 20000, 9
    done = 0
    for c in occs:
        for off in range(c + 2):
            rs = np.random.RandomState(100 * c + off)
            SA, LCP, BWT = blank(n, 1000 * c + off)
            SA = rs.randint(1, split, size=n).astype(np.uint64)
            SA[rs.rand(n) < 0.5] += np.uint64(split)
            long_runs = 0
            for k, e in enumerate(EDGES):
                size = c + (1 if (k + off) % 2 else 0)
                h = e - off
                LCP[h + 1:h + size] = rs.randint(L, L + 4, size=size - 1)
                long_runs += size > c
            want = R.rank_rule(SA, LCP, BWT, split, L, c)
            assert want[1][1] == long_runs and (want[1][0] > 0 or c <= 3)
            for form, bits in itertools.product(forms, widths):
                assert form.run(form.load(SA, LCP, BWT, bits), "mems", split, L, c) == want, (c, off, form.name, bits)
                done += 1
    return done


def test_mum_ranks_on_the_tile_edges():
    assert mum_edge_sweep(forms_of(emul(), HostMem())) == 3 * 4


@pytest.mark.parametrize("c", (2, 3, 64))
def test_mem_runs_across_the_tile_edges_and_skipped_runs_counted_once(c):
    assert mem_edge_sweep(forms_of(emul(), HostMem()), occs=(c,)) == (c + 2) * 4


# ---- 4. split at the ends, SA == 0 in a pair, no separator --------------------------------------------------------------------------

def corner_sweep(forms, widths=(32, 64)):
    rs = np.random.RandomState(17)
    # split = 0, 1, n - 1, n on a text without a separator: the rank rules alone
    T = rs.choice(DNA[:2], size=700).astype(np.uint8)
    SA, LCP = sa_lcp(T, 64)
    BWT = bwt_of(T, SA)
    n = T.size
    cases = [(SA, LCP, BWT, s, m, L, c) for s in (0, 1, 350, n - 1, n) for m, L, c in (("mums", 1, None), ("mums", 3, None), ("mems", 5, 4), ("mems", 7, 64))]
    # the rank with SA == 0 as p and as q of a pair whose BWT bytes are equal: left-maximal all the same
    for zero_first in (True, False):
        s, l, b = blank(40, 3)
        l[20] = 5
        s[19], s[20] = (0, 1 << 19) if zero_first else (1 << 19, 0)
        b[19] = b[20] = ord("A")
        cases += [(s, l, b, 1, "mums", 5, None), (s, l, b, 1, "mems", 5, 2)]
        s2 = s.copy()
        s2[19 if zero_first else 20] = 7                       # ... and without the zero the pair is not
        cases += [(s2, l, b, 8, "mums", 5, None), (s2, l, b, 8, "mems", 5, 2)]
    # LCP[0] counts as 0 whatever it holds
    s, l, b = blank(30, 4)
    l[0], l[1] = 1 << 30, 4
    s[0], s[1] = 3, 1 << 19
    b[0], b[1] = ord("A"), ord("C")
    cases += [(s, l, b, 10, "mums", 2, None), (s, l, b, 10, "mems", 2, 2)]
    done = 0
    for SA, LCP, BWT, split, mode, L, c in cases:
        want = R.rank_rule(SA, LCP, BWT, split, L, c)
        if split in (0, len(SA)):
            assert want[0] == [] and want[1][2:5] == [0, 0, 0]
        for form, bits in itertools.product(forms, widths):
            assert form.run(form.load(SA, LCP, BWT, bits), mode, split, L, c) == want, (split, mode, L, c, form.name, bits)
            done += 1
    z = [c for c in cases if len(c[0]) == 40]
    assert [len(R.rank_rule(*c[:4], c[5], c[6])[0]) for c in z] == [1, 1, 0, 0] * 2       # the zero makes the pair, its absence breaks it
    assert R.rank_rule(*cases[-2][:4], 2, None)[0] == [(3, 1 << 19, 4)]
    return done


def test_split_at_the_ends_sa_zero_in_a_pair_and_no_separator():
    assert corner_sweep(forms_of(emul(), HostMem())) > 100


# ---- 5. the counting call, the writing call, the capacity ---------------------------------------------------------------------------

def capacity_sweep(lib, mem, widths=(32, 64)):
    _, SA, LCP, BWT, split = list(texts_of(5000))[3]
    for bits, (mode, L, c) in itertools.product(widths, (("mums", 10, None), ("mems", 8, 5))):
        want = R.rank_rule(SA, LCP, BWT, split, L, c)
        found = want[1][0]
        assert found > 1
        for form in forms_of(lib, mem):
            a = form.load(SA, LCP, BWT, bits)
            assert form.run(a, mode, split, L, c, own_ws=False) == want              # a NULL workspace: the call's own
            m = form.mem or HostMem()
            buf = m.filled(FRONT + REC * found + GUARD)
            s = np.full(8, 0x5A5A, dtype=np.uint64)
            # one too small: refused, the summary is still valid, nothing is written
            assert form.call(a, mode, split, L, c, m.ptr(buf) + FRONT, found - 1, s) == EINVAL
            assert s.tolist() == want[1] and (m.get(buf) == FILL).all()
            # more room than needed
            assert form.call(a, mode, split, L, c, m.ptr(buf) + FRONT, found + 3, s) == 0 and s.tolist() == want[1]
            out = m.get(buf)
            assert (out[:FRONT] == FILL).all() and (out[FRONT + REC * found:] == FILL).all()
            assert [tuple(r) for r in out[FRONT:FRONT + REC * found].copy().view("<u8").reshape(-1, 3).tolist()] == want[0]


def test_counting_call_writing_call_and_capacity():
    capacity_sweep(emul(), HostMem())


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------

def refusal_sweep(lib, mem):
    """Every refusal: CAPS_SA_EINVAL, and no output is touched."""
    _, SA, LCP, BWT, split = list(texts_of(1000))[2]
    n = 1000
    for bits in (32, 64):
        sfx = "u32" if bits == 32 else "u64"
        a = Arrays(SA, LCP, BWT, bits, mem)
        S, Lp, B = (mem.ptr(x) for x in a.d)
        hs, hl, hb = a.sa.ctypes.data, a.lcp.ctypes.data, a.bwt.ctypes.data
        wsb = lib.cross_workspace_bytes(n, bits)
        ws = mem.filled(wsb)
        W = mem.ptr(ws)
        recs = mem.filled(REC * n)
        Rp = mem.ptr(recs)
        hrec = np.full(REC * n, FILL, dtype=np.uint8)
        Hp = hrec.ctypes.data
        summary = np.full(8, 0x5A5A, dtype=np.uint64)
        Sm = summary.ctypes.data
        ud, ed = lib._f(f"cross_mums_device_{sfx}"), lib._f(f"cross_mems_device_{sfx}")
        uh, eh = lib._f(f"cross_mums_{sfx}"), lib._f(f"cross_mems_{sfx}")
        calls = [
            ud(S, Lp, B, n, split, 0, Rp, n, Sm, W, wsb, None),                 # min_len == 0
            ed(S, Lp, B, n, split, 0, 4, Rp, n, Sm, W, wsb, None),
            ud(S, Lp, B, n, n + 1, 3, Rp, n, Sm, W, wsb, None),                 # split > n
            ed(S, Lp, B, n, n + 1, 3, 4, Rp, n, Sm, W, wsb, None),
            ed(S, Lp, B, n, split, 3, 0, Rp, n, Sm, W, wsb, None),              # max_occ outside 2 .. 64
            ed(S, Lp, B, n, split, 3, 1, Rp, n, Sm, W, wsb, None),
            ed(S, Lp, B, n, split, 3, 65, Rp, n, Sm, W, wsb, None),
            ud(None, Lp, B, n, split, 3, Rp, n, Sm, W, wsb, None),              # a null array with n > 0
            ud(S, None, B, n, split, 3, Rp, n, Sm, W, wsb, None),
            ud(S, Lp, None, n, split, 3, Rp, n, Sm, W, wsb, None),
            ed(None, Lp, B, n, split, 3, 4, Rp, n, Sm, W, wsb, None),
            ed(S, None, B, n, split, 3, 4, Rp, n, Sm, W, wsb, None),
            ed(S, Lp, None, n, split, 3, 4, Rp, n, Sm, W, wsb, None),
            ud(S, Lp, B, n, split, 3, Rp, n, None, W, wsb, None),               # a null summary
            ed(S, Lp, B, n, split, 3, 4, Rp, n, None, W, wsb, None),
            ud(S, Lp, B, n, split, 3, Rp + 4, n, Sm, W, wsb, None),             # records not 8-byte aligned
            ud(S, Lp, B, n, split, 3, Rp, n, Sm, W, wsb - 512, None),           # a workspace that is too small
            ed(S, Lp, B, n, split, 3, 4, Rp, n, Sm, W, wsb - 512, None),
            uh(hs, hl, hb, n, split, 0, Hp, n, Sm, 0),
            eh(hs, hl, hb, n, split, 0, 4, Hp, n, Sm, 0),
            uh(hs, hl, hb, n, n + 1, 3, Hp, n, Sm, 0),
            eh(hs, hl, hb, n, n + 1, 3, 4, Hp, n, Sm, 0),
            eh(hs, hl, hb, n, split, 3, 1, Hp, n, Sm, 0),
            eh(hs, hl, hb, n, split, 3, 65, Hp, n, Sm, 0),
            uh(None, hl, hb, n, split, 3, Hp, n, Sm, 0),
            uh(hs, None, hb, n, split, 3, Hp, n, Sm, 0),
            eh(hs, hl, None, n, split, 3, 4, Hp, n, Sm, 0),
            uh(hs, hl, hb, n, split, 3, Hp, n, None, 0),
            eh(hs, hl, hb, n, split, 3, 4, Hp, n, None, 0),
        ]
        if bits == 32:                                       # n > UINT32_MAX with _u32: refused before anything is read
            big = 1 << 32
            calls += [ud(S, Lp, B, big, split, 3, None, 0, Sm, None, 0, None), ed(S, Lp, B, big, split, 3, 4, None, 0, Sm, None, 0, None),
                      uh(hs, hl, hb, big, split, 3, None, 0, Sm, 0), eh(hs, hl, hb, big, split, 3, 4, None, 0, Sm, 0)]
        assert calls == [EINVAL] * len(calls), calls
        assert (summary == 0x5A5A).all() and (hrec == FILL).all()
        assert (mem.get(recs) == FILL).all() and (mem.get(ws) == FILL).all()
        out = ctypes.c_uint64(0)
        assert lib._f("cross_workspace_bytes")(n, 5, ctypes.byref(out)) == EINVAL
        assert lib._f("cross_workspace_bytes")(n, bits // 8, None) == EINVAL
        assert lib._f("cross_workspace_bytes")(1 << 32, 4, ctypes.byref(out)) == EINVAL
        # the workspace is O(n / tile) words: no array of n entries
        assert lib.cross_workspace_bytes(1 << 30, bits) < (1 << 30) // 64
        # n = 0 succeeds with no records, null arrays allowed; max_occ = 2 and 64 are the ends of the range
        for f, occ in ((ud, ()), (ed, (2,)), (ed, (64,))):
            summary[:] = 9
            assert f(None, None, None, 0, 0, 3, *occ, None, 0, Sm, None, 0, None) == 0 and (summary == 0).all()
        for f, occ in ((uh, ()), (eh, (2,)), (eh, (64,))):
            summary[:] = 9
            assert f(None, None, None, 0, 0, 3, *occ, None, 0, Sm, 0) == 0 and (summary == 0).all()


def test_refusals_and_the_empty_text():
    import caps_sa_amd
    assert caps_sa_amd.CROSS_MAX_OCC == MAX_OCC
    with open(os.path.join(ROOT, "include", "caps_sa_hip.h")) as f:
        assert "#define CAPS_SA_CROSS_MAX_OCC 64" in f.read()
    refusal_sweep(emul(), HostMem())


# ---- 7. arrays that are no text's: a child process, the emulation only -----------------------------------------------------------------

_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [%(tests)r, %(root)r]
import caps_sa_amd
import cross_reference as R
from test_emul_cross import Form, HostMem
E = caps_sa_amd.CapsLib(%(so)r, "caps_sa_emul_")
rs = np.random.RandomState(21)
form = Form(E, HostMem())
for n in (1, 5, 4097, 16384, 40001):
    for bits in (32, 64):
        for trial in range(3):
            SA = rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
            LCP = rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
            BWT = rs.randint(0, 256, size=n).astype(np.uint8)
            if trial == 1:
                LCP %%= 40
                BWT %%= 2
            if trial == 2:
                SA %%= n
                LCP %%= 3
            if bits == 64 and trial == 0:
                SA = SA * SA
                LCP = LCP * LCP + SA
            a = form.load(SA, LCP, BWT, bits)
            for split in (0, n // 2, 1 << 31, n):
                if split > n:
                    continue
                for L in (1, 2, 17, 1 << 31, (1 << 32) + 5):
                    for mode, c in (("mums", None), ("mems", 2), ("mems", 64)):
                        got = form.run(a, mode, split, L, c)          # (ends with CAPS_SA_OK, or this raises; asserts the guards)
                        if n <= 4097 or (L == 2 and split == n // 2):
                            assert got == R.rank_rule(a.sa, a.lcp, BWT, split, L, c), (n, bits, trial, split, L, mode, c)
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


# ---- 8. the Python surface -------------------------------------------------------------------------------------------------------------

def test_module_level_functions_and_dtype():
    import caps_sa_amd
    assert caps_sa_amd.CROSS_DTYPE.itemsize == 24 and caps_sa_amd.CROSS_DTYPE.names == ("a", "b", "len")
    t = b"ACGTTGCAAGGCTA" + b"\xff" + b"GGCTATTGCAACGT"
    split = 15
    SA, LCP, BWT = R.naive_sa_lcp_bwt(t)
    E = emul()
    sa32, lcp32, bwt = np.array(SA, dtype=np.uint32), np.array(LCP, dtype=np.uint32), np.array(BWT, dtype=np.uint8)
    want = R.mums(t, split, 2)
    assert len(want) >= 2
    rec = caps_sa_amd.cross_mums(sa32, lcp32, bwt, split, 2, sort=True, _lib=E)
    assert rec.dtype == caps_sa_amd.CROSS_DTYPE and [tuple(r) for r in rec.tolist()] == want          # (the reference is sorted by a)
    unsorted, summary = caps_sa_amd.cross_mums(np.array(SA, dtype=np.uint64), LCP, bytes(BWT), split, 2, return_summary=True, _lib=E)
    assert [tuple(r) for r in unsorted.tolist()] == R.rank_rule(SA, LCP, BWT, split, 2, None)[0]
    best, at = R.lcs(t, split)
    assert summary["records"] == len(want) and summary["skipped_runs"] == 0 and summary["lcs_len"] == best
    assert (summary["lcs_a"], summary["lcs_b"]) in at
    wm, skipped = R.mems(t, split, 2, 3)
    rec, summary = caps_sa_amd.cross_mems(sa32, lcp32, bwt, split, 2, max_occ=3, sort=True, return_summary=True, _lib=E)
    assert sorted(tuple(r) for r in rec.tolist()) == wm and rec["a"].tolist() == sorted(rec["a"].tolist())
    assert summary["records"] == len(wm) and summary["skipped_runs"] == skipped > 0
    assert all(t[a:a + l] == t[b:b + l] and a < split <= b for a, b, l in rec.tolist())
    full = caps_sa_amd.cross_mems(sa32, lcp32, bwt, split, 2, _lib=E)                          # max_occ defaults to 64
    assert sorted(tuple(r) for r in full.tolist()) == R.mems(t, split, 2, 64)[0]


# ---- 9. the other emulation builds ---------------------------------------------------------------------------------------------------

def small_sweeps(E):
    forms = forms_of(E, HostMem())
    assert short_text_sweep(forms, max_len=2, widths=(32,), tie_rank_rule=False) == 2 * n_short_texts(2)
    assert size_sweep(forms, [TILE + 1], widths=(32,)) == 4 * 2
    assert mum_edge_sweep(forms, widths=(64,)) == 3 * 2
    assert mem_edge_sweep(forms, occs=(3,), widths=(32,)) == 5 * 2
    corner_sweep(forms, widths=(64,))


@pytest.mark.slow
def test_other_builds_give_the_same_answers():
    """The small sweeps once more with the threads of every phase in descending order, with LDS and registers starting as 0xA5 and
    the threads in a scattered order, and under the barrier-race detector (no race may be found)."""
    import caps_sa_amd
    small_sweeps(emul_rev(False))
    for name in ("libcaps_sa_emul_poison.so", "libcaps_sa_emul_race.so"):
        subprocess.check_call(["make", "-s", "-C", EMUL_DIR, name])
        path = os.path.join(EMUL_DIR, name)
        small_sweeps(caps_sa_amd.CapsLib(path, "caps_sa_emul_"))
        if "race" in name:
            raw = ctypes.CDLL(path)
            raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
            assert int(raw.caps_sa_emul_races_found()) == 0
