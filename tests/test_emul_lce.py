"""CPU: the inverse suffix array, range minima over LCP and longest common extensions (include/caps_sa_hip.h "ISA and longest common
extensions", caps_sa_hip_isa_*, caps_sa_hip_lce_*) through the host emulation of the kernels.

Every comparison is exact.  The truth is lce_reference: lce by brute force on the text, the array rules as naive slices, a numpy
sparse table for batches of range minima and an encoder of the blob written from the header's format table; every blob is compared
with the encoder byte for byte.  The sweeps are functions of a "form" (the host or the device entry points of a library), so that
test_gpu_lce.py runs the same ones on the GPU.  The device form always works on buffers preset to 0xA5 with guard bytes before and
behind them."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import lce_reference as R
from emul_util import EMUL_DIR, ROOT, emul, emul_rev, emul_small
from sa_check import sa_lcp
from test_emul_kmers import HostMem, naive_sa_lcp
from test_emul_lz import permutations_of

EINVAL = -1
FILL = 0xA5
GUARD = 64
FRONT = 80                                                 # the index must be 16-byte aligned; nothing more
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288, 12289, 16383, 16384, 16385, 20481, 32767,
         32768, 32769, 36865]
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
N_ARB = 36865                                              # ten superblocks, the last of one rank; 577 blocks


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _sfx(bits):
    return "u32" if bits == 32 else "u64"


class HostForm:
    """The host entry points (CapsLib.isa / lce_build / lce_range_min / lce)."""
    name = "host"

    def __init__(self, lib):
        self.lib = lib

    def isa(self, SA, bits):
        return self.lib.isa(SA, idx_bits=bits)

    def build(self, SA, LCP, bits):
        return self.lib.lce_build(SA, LCP, idx_bits=bits)

    def range_min(self, index, lo, hi):
        return self.lib.lce_range_min(index, lo, hi)

    def lce(self, index, i, j, k=0):
        return self.lib.lce(index, i, j, k)


class DeviceForm:
    """The *_device entry points on `mem`.  An index is (buffer, bytes): the blob lies FRONT bytes into the buffer."""
    name = "device"

    def __init__(self, lib, mem):
        self.lib, self.mem = lib, mem

    def isa(self, SA, bits):
        m, w = self.mem, bits // 8
        sa = np.ascontiguousarray(SA, dtype=_dt(bits))
        n = int(sa.size)
        dsa, out = m.put(sa), m.filled(FRONT + n * w + GUARD)
        try:
            self.lib.isa_device(m.ptr(dsa) if n else 0, n, m.ptr(out) + FRONT, idx_bits=bits)
        finally:
            g = m.get(out)
            assert (g[:FRONT] == FILL).all() and (g[FRONT + n * w:] == FILL).all(), "a guard of ISA was written"
            assert np.array_equal(m.get(dsa)[:n * w], sa.view(np.uint8))
        return g[FRONT:FRONT + n * w].copy().view(_dt(bits))

    def build(self, SA, LCP, bits):
        m, w = self.mem, bits // 8
        sa, lcp = np.ascontiguousarray(SA, dtype=_dt(bits)), np.ascontiguousarray(LCP, dtype=_dt(bits))
        n = int(sa.size)
        need = self.lib.lce_index_bytes(n, bits)
        dsa, dlcp, buf = m.put(sa), m.put(lcp), m.filled(FRONT + need + GUARD)
        try:
            self.lib.lce_build_device(m.ptr(dsa) if n else 0, m.ptr(dlcp) if n else 0, n, m.ptr(buf) + FRONT, need, idx_bits=bits)
        finally:
            g = m.get(buf)
            assert (g[:FRONT] == FILL).all() and (g[FRONT + need:] == FILL).all(), "a guard of the index was written"
            assert np.array_equal(m.get(dsa)[:n * w], sa.view(np.uint8)) and np.array_equal(m.get(dlcp)[:n * w], lcp.view(np.uint8))
        return g[FRONT:FRONT + need].copy()

    def _pairs(self, call, index, a, b, extra):
        m = self.mem
        a, b = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1), np.ascontiguousarray(b, dtype=np.uint64).reshape(-1)
        q = int(a.size)
        buf = m.filled(FRONT + index.size + GUARD)
        host = m.get(buf).copy()
        host[FRONT:FRONT + index.size] = index
        buf = m.put(host)
        da, db, out = m.put(a), m.put(b), m.filled(FRONT + 8 * q + GUARD)
        try:
            call(m.ptr(buf) + FRONT, index.size, m.ptr(da) if q else 0, m.ptr(db) if q else 0, q, *extra, m.ptr(out) + FRONT)
        finally:
            g = m.get(out)
            assert (g[:FRONT] == FILL).all() and (g[FRONT + 8 * q:] == FILL).all(), "a guard of the answers was written"
            assert np.array_equal(m.get(buf), host), "the index was written"
            self.last = g[FRONT:FRONT + 8 * q].copy().view(np.uint64)
        return self.last

    def range_min(self, index, lo, hi):
        return self._pairs(self.lib.lce_range_min_device, index, lo, hi, ())

    def lce(self, index, i, j, k=0):
        return self._pairs(self.lib.lce_device, index, i, j, (k,))


def forms_of(lib, mem):
    return (HostForm(lib), DeviceForm(lib, mem))


# ---- the checks --------------------------------------------------------------------------------------------------------------------

def check_blob(form, SA, LCP, bits, want=None):
    """The blob of (SA, LCP) through `form`: the encoder's, byte for byte, and below the advertised bound."""
    n, w = int(np.asarray(SA).size), bits // 8
    blob = form.build(SA, LCP, bits)
    if want is None:
        want = R.encode(SA, LCP, w)
    assert blob.size == want.size == R.index_bytes(n, w) and blob.size < 2 * n * w + n * w // 8 + 16384
    assert np.array_equal(blob, want), (form.name, bits, n, int(np.flatnonzero(blob != want)[0]))
    return blob


def pairs_of(n, rs, count):
    """Pairs of positions: random ones, equal ones, neighbours and the text's two ends."""
    i, j = rs.randint(0, n, size=count), rs.randint(0, n, size=count)
    edge = [(0, 0), (n - 1, n - 1), (0, n - 1), (n - 1, 0), (0, 1 % n), (n // 2, n // 2), (max(n - 2, 0), n - 1)]
    return np.concatenate([i, [a for a, _ in edge]]).astype(np.uint64), np.concatenate([j, [b for _, b in edge]]).astype(np.uint64)


def texts_of(n, seed=1):
    """(name, T, SA, LCP) for the four families at size n."""
    rs = np.random.RandomState(seed + n)
    yield "a^n", np.full(n, ord("A"), dtype=np.uint8), np.arange(n, dtype=np.uint64)[::-1].copy(), np.arange(n, dtype=np.uint64)
    for name, letters in (("two", DNA[:2]), ("four", DNA)):
        T = rs.choice(letters, size=n).astype(np.uint8)
        yield (name, T) + tuple(sa_lcp(T, 64))
    T = rs.choice(DNA, size=n).astype(np.uint8)             # planted repeats: a third of the text copied twice, one copy overlapping
    k = n // 3
    if k:
        T[k:2 * k] = T[:k]
        T[n - k:] = T[k // 2:k // 2 + k]
    yield ("planted", T) + tuple(sa_lcp(T, 64))


def size_sweep(forms, sizes, widths=(32, 64), pairs=48, ks=(0, 1, 3)):
    done = 0
    for n in sizes:
        for name, T, SA, LCP in texts_of(n):
            rs = np.random.RandomState(n)
            I, J = pairs_of(n, rs, pairs)
            lo = rs.randint(0, n, size=pairs)
            hi = np.minimum(lo + rs.randint(0, n, size=pairs) // rs.choice([1, 7, 300], size=pairs), n - 1)
            isa, L0 = R.isa_of(SA), R.lcp0(LCP)
            t = T.tobytes()
            want_lce = {k: [R.lce_arrays(isa, L0, n, int(a), int(b), k) for a, b in zip(I, J)] for k in ks}
            for k in ks:                                     # the array rule against the text itself
                if name == "a^n":
                    assert want_lce[k] == [n - max(int(a), int(b)) for a, b in zip(I, J)]
                elif n <= 4097:
                    assert want_lce[k] == R.lce_brute_np(T, I, J, k, cap=n + 1).tolist()
                else:
                    assert want_lce[k][:8] == [R.lce_brute(t, int(a), int(b), k) for a, b in zip(I[:8], J[:8])]
            want_min = [R.range_min(L0, int(a), int(b)) for a, b in zip(lo, hi)]
            blobs = {}
            for form, bits in itertools.product(forms, widths):
                blob = blobs[bits] = check_blob(form, SA, LCP, bits, blobs.get(bits))
                assert form.isa(SA, bits).tolist() == isa, (form.name, bits, n)
                assert form.range_min(blob, lo, hi).tolist() == want_min, (form.name, bits, n, name)
                for k in ks:
                    assert form.lce(blob, I, J, k).tolist() == want_lce[k], (form.name, bits, n, name, k)
                done += 1
    return done


# ---- 1. every short text ------------------------------------------------------------------------------------------------------------

LETTERS3 = bytes([0x41, 0x43, 0xC8])                     # (0xC8 sorts first: signed char)


def test_the_reference_rule_against_brute_force_on_every_short_text():
    """lce_reference's kangaroo rule on the arrays equals the brute-force comparison of the text: every text of up to 7 bytes over 3
    letters, every pair, k = 0, 1, 2."""
    cases = 0
    for n in range(1, 8):
        for tup in itertools.product(LETTERS3, repeat=n):
            t = bytes(tup)
            SA, LCP = naive_sa_lcp(t)
            isa, L0 = R.isa_of(SA), R.lcp0(LCP)
            for i, j, k in itertools.product(range(n), range(n), range(3)):
                assert R.lce_arrays(isa, L0, n, i, j, k) == R.lce_brute(t, i, j, k), (t, i, j, k)
                cases += 1
    assert cases == 423180


def short_text_sweep(forms, max_len=7, widths=(32, 64)):
    """Every pair and k = 0 .. 2 of every short text through the forms, against brute force on the text."""
    done = 0
    for n in range(1, max_len + 1):
        ii, jj = (x.reshape(-1).astype(np.uint64) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
        for tup in itertools.product(LETTERS3, repeat=n):
            t = bytes(tup)
            SA, LCP = naive_sa_lcp(t)
            want = {k: [R.lce_brute(t, int(a), int(b), k) for a, b in zip(ii, jj)] for k in range(3)}
            for f, form in enumerate(forms):
                bits = widths[(done + f) % len(widths)]
                blob = form.build(SA, LCP, bits)
                for k in range(3):
                    assert form.lce(blob, ii, jj, k).tolist() == want[k], (t, k, form.name)
            done += 1
    return done


def test_every_short_text():
    E = emul()
    assert short_text_sweep((HostForm(E),)) == sum(3 ** n for n in range(1, 8))
    assert short_text_sweep((DeviceForm(E, HostMem()),), max_len=6) == sum(3 ** n for n in range(1, 7))


# ---- 2. sizes around blocks and superblocks: every top-level count ---------------------------------------------------------------------

def test_the_sizes_cover_every_top_level_count():
    assert {(n + 4095) // 4096 for n in SIZES} == {1, 2, 3, 4, 5, 6, 8, 9, 10}
    assert {R.layout(n, 4)["tl"] for n in SIZES} == {1, 2, 3, 4}


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_texts(n):
    assert size_sweep(forms_of(emul(), HostMem()), [n]) == 4 * 4


# ---- 3. range_min on arrays that are no text's ------------------------------------------------------------------------------------------

def arbitrary_arrays(n=N_ARB, seed=5, floor=1000):
    rs = np.random.RandomState(seed)
    return rs.permutation(n).astype(np.uint64), rs.randint(floor, 1 << 32, size=n).astype(np.uint64)


def block_pair_spans(superblocks=3, offs=(0, 1, 62, 63)):
    """Every block pair (bl <= bh) within the first superblocks at the offsets of each end."""
    nb = superblocks * 64
    bl, bh = np.triu_indices(nb)
    lo, hi = [], []
    for a, b in itertools.product(offs, offs):
        l, h = bl * 64 + a, bh * 64 + b
        keep = l <= h
        lo.append(l[keep])
        hi.append(h[keep])
    return np.concatenate(lo), np.concatenate(hi)


def tier_spans(n=N_ARB):
    """(lo, hi) whose whole blocks are a head run of h blocks up to a superblock edge, sc whole superblocks and a tail run of t blocks,
    with whole and partial blocks at either end; and spans that run to the last rank."""
    nb = (n + 63) // 64
    out = []
    for s0, sc, h, t in itertools.product((1, 2), (1, 2, 3, 4, 5, 7), (0, 1, 63), (0, 1, 63)):
        fb, le = 64 * s0 - h, 64 * (s0 + sc) + t
        if le > nb - 2:
            continue
        for dl, dh in itertools.product((0, 1, 63), (0, 1, 63)):
            out.append((fb * 64 - dl, le * 64 - 1 + dh))
    for h, t in itertools.product((0, 1, 63), (0, 1, 63)):   # no whole superblock between the two runs
        out.append(((128 - h) * 64 - 3, (128 + t) * 64 + 5))
    for lo in (0, 1, 63, 64, 65, 4095, 4096, 4097, 8191, n - 4097, n - 4096, n - 130, n - 66, n - 65, n - 64, n - 2, n - 1):
        out.append((lo, n - 1))
        if lo <= n - 2:
            out.append((lo, n - 2))
    return np.array([a for a, _ in out]), np.array([b for _, b in out])


def tiers_of(lo, hi, n):
    """The rank ranges [first, last] a span is answered from (the header's decomposition): partial blocks, block runs, superblocks."""
    bl, bh = lo // 64, hi // 64
    head_whole, tail_whole = lo % 64 == 0, hi % 64 == 63 or hi == n - 1
    if bl == bh and not (head_whole and tail_whole):
        return [(lo, hi)]
    out = []
    if not head_whole:
        out.append((lo, 64 * (bl + 1) - 1))
    if not tail_whole:
        out.append((64 * bh, hi))
    fb, le = (bl if head_whole else bl + 1), (bh + 1 if tail_whole else bh)
    if fb >= le:
        return out
    end = lambda b: min(64 * b, n) - 1
    if le - fb <= 64:
        return out + [(64 * fb, end(le))]
    e1, e2 = (fb + 63) // 64 * 64, le // 64 * 64
    for a, b in ((fb, e1), (e1, e2), (e2, le)):
        if b > a:
            out.append((64 * a, end(b)))
    return out


def arbitrary_sweep(forms, n=N_ARB):
    """Random 32-bit values as LCP: every span against the numpy sparse table."""
    SA, LCP = arbitrary_arrays(n)
    table = R.SparseTable(R.lcp0(LCP))
    lo1, hi1 = block_pair_spans()
    lo2, hi2 = tier_spans(n)
    lo, hi = np.concatenate([lo1, lo2]), np.concatenate([hi1, hi2])
    assert (lo <= hi).all() and (hi < n).all() and lo1.size == 16 * (192 * 193 // 2) - 6 * 192
    want = table.query(lo, hi)
    for form, bits in zip(forms, (32, 64)):
        blob = check_blob(form, SA, LCP, bits)
        assert np.array_equal(form.range_min(blob, lo, hi), want), form.name
    return int(lo.size)


def planted_sweep(forms, n=N_ARB):
    """The unique minimum put one rank outside a span (must not be seen) and at both ends of every tier the span uses (must be)."""
    SA, base = arbitrary_arrays(n)
    spans = [(130, 140), (130, 191), (128, 191), (100, 64 * 9 + 7), (64 * 63 - 5, 64 * 64 + 70), (64 * 2 + 9, 64 * 200 - 3),
             (64 * 64, 64 * 128 - 1), (64 * 61, 64 * 322 + 63), (4097, n - 1), (64 * 500 + 1, n - 1), (64 * 130, 64 * 131 - 2)]
    done = 0
    for s, (lo, hi) in enumerate(spans):
        tiers = tiers_of(lo, hi, n)
        assert sum(b - a + 1 for a, b in tiers) == hi - lo + 1
        inside = sorted({p for a, b in tiers for p in (a, b)} | {lo, hi})
        outside = [p for p in (lo - 1, hi + 1) if 1 <= p < n]
        plain = int(base[lo:hi + 1].min())
        form = forms[s % len(forms)]
        for p in inside + outside:
            LCP = base.copy()
            LCP[p] = 5
            blob = form.build(SA, LCP, 32 if done % 2 else 64)
            got = form.range_min(blob, [lo, max(lo - 1, 1), lo], [hi, hi, min(hi + 1, n - 1)]).tolist()
            assert got[0] == (5 if p in inside else plain), (lo, hi, p)
            assert got[1] == 5 or p == hi + 1 and got[2] == 5
            done += 1
    return done


def test_range_min_of_every_block_pair_and_tier():
    assert arbitrary_sweep(forms_of(emul(), HostMem())) > 290000


def test_a_planted_minimum_is_seen_inside_and_not_outside():
    assert planted_sweep(forms_of(emul(), HostMem())) > 60


# ---- 4. ISA, garbage LCP, refusals ------------------------------------------------------------------------------------------------------

def isa_sweep(forms, n=4097 + 64):
    for name, SA in permutations_of(n, 4096):
        want = np.argsort(SA.astype(np.int64), kind="stable")
        for form, bits in zip(forms, (64, 32)):
            got = form.isa(SA, bits)
            assert got.dtype == _dt(bits) and np.array_equal(got.astype(np.int64), want), (name, form.name)
    for form in forms:
        assert form.isa(np.zeros(0, dtype=np.uint64), 32).size == 0
    return True


def garbage_lcp_sweep(forms, n=20481):
    """A permutation with random 32-bit values as LCP: lce with up to 8 mismatches is the array rule's (the clamp makes it defined) and
    never beyond the text's end."""
    SA, LCP = arbitrary_arrays(n, seed=9, floor=0)
    LCP[::3] %= 50
    isa, L0 = R.isa_of(SA), R.lcp0(LCP)
    I, J = pairs_of(n, np.random.RandomState(4), 150)
    for form, bits in zip(forms, (32, 64)):
        blob = form.build(SA, LCP, bits)
        for k in (0, 2, 8):
            got = form.lce(blob, I, J, k)
            assert (got <= n - np.maximum(I, J)).all()
            assert got.tolist() == [R.lce_arrays(isa, L0, n, int(a), int(b), k) for a, b in zip(I, J)], (form.name, k)


def test_isa_of_six_permutations():
    assert isa_sweep(forms_of(emul(), HostMem()))


def test_garbage_lcp_terminates_in_range():
    garbage_lcp_sweep(forms_of(emul(), HostMem()))


def refusal_sweep(lib, mem):
    """Every refusal is CAPS_SA_EINVAL; what is refused before the work writes nothing."""
    n = 1000
    T = np.random.RandomState(3).choice(DNA, size=n).astype(np.uint8)
    SA, LCP = sa_lcp(T, 64)
    last = lambda: lib._f("last_error")()
    for bits in (32, 64):
        sfx, w = _sfx(bits), bits // 8
        sa, lcp = SA.astype(_dt(bits)), LCP.astype(_dt(bits))
        need = lib.lce_index_bytes(n, bits)
        assert need == R.index_bytes(n, w)
        blob = lib.lce_build(sa, lcp, idx_bits=bits)
        dsa, dlcp, dblob = mem.put(sa), mem.put(lcp), mem.put(blob)
        S, Lp, X = mem.ptr(dsa), mem.ptr(dlcp), mem.ptr(dblob)
        assert X % 16 == 0
        out, idx = mem.filled(8 * n), mem.filled(need)
        O, D = mem.ptr(out), mem.ptr(idx)
        qa = mem.put(np.arange(n, dtype=np.uint64))
        A = mem.ptr(qa)
        isa_d, isa_h, bld, blh = (lib._f(f"isa_device_{sfx}"), lib._f(f"isa_{sfx}"), lib._f(f"lce_build_device_{sfx}"), lib._f(f"lce_build_{sfx}"))
        rmd, rmh, lcd, lch = lib._f("lce_range_min_device"), lib._f("lce_range_min"), lib._f("lce_device"), lib._f("lce")
        hs, hl, hb = sa.ctypes.data, lcp.ctypes.data, blob.ctypes.data
        h1, hidx = np.full(n, 0x5A, dtype=np.uint64), np.full(need, 0x5A, dtype=np.uint8)
        ha = np.arange(n, dtype=np.uint64)
        calls = [
            isa_d(None, n, O, None), isa_d(S, n, None, None), isa_h(None, n, h1.ctypes.data, 0), isa_h(hs, n, None, 0),
            bld(None, Lp, n, D, need, None), bld(S, None, n, D, need, None), bld(S, Lp, n, None, need, None),
            bld(S, Lp, n, D, need - 1, None), bld(S, Lp, n, D + 8, need, None),
            blh(None, hl, n, hidx.ctypes.data, need, 0), blh(hs, None, n, hidx.ctypes.data, need, 0), blh(hs, hl, n, None, need, 0),
            blh(hs, hl, n, hidx.ctypes.data, need - 1, 0),
            rmd(None, need, A, A, n, O, None), rmd(X, need, None, A, n, O, None), rmd(X, need, A, None, n, O, None),
            rmd(X, need, A, A, n, None, None), rmd(X, need - 1, A, A, n, O, None), rmd(X, 255, A, A, n, O, None), rmd(X + 8, need, A, A, n, O, None),
            lcd(None, need, A, A, n, 0, O, None), lcd(X, need, None, A, n, 0, O, None), lcd(X, need, A, A, n, 0, None, None),
            lcd(X, need, A, A, n, 1025, O, None), lcd(X, need, A, A, n, 1 << 40, O, None), lcd(X, need - 1, A, A, n, 0, O, None),
            rmh(None, need, ha.ctypes.data, ha.ctypes.data, n, h1.ctypes.data, 0), rmh(hb, need, None, ha.ctypes.data, n, h1.ctypes.data, 0),
            rmh(hb, need, ha.ctypes.data, ha.ctypes.data, n, None, 0), rmh(hb, need - 1, ha.ctypes.data, ha.ctypes.data, n, h1.ctypes.data, 0),
            lch(None, need, ha.ctypes.data, ha.ctypes.data, n, 0, h1.ctypes.data, 0), lch(hb, need, ha.ctypes.data, None, n, 0, h1.ctypes.data, 0),
            lch(hb, need, ha.ctypes.data, ha.ctypes.data, n, 1025, h1.ctypes.data, 0),
        ]
        if bits == 32:                                       # n > UINT32_MAX with _u32: refused before anything is read
            big = 1 << 32
            calls += [isa_d(S, big, O, None), isa_h(hs, big, h1.ctypes.data, 0), bld(S, Lp, big, D, 1 << 40, None),
                      blh(hs, hl, big, hidx.ctypes.data, 1 << 40, 0)]
        assert calls == [EINVAL] * len(calls), calls
        assert (h1 == 0x5A).all() and (hidx == 0x5A).all() and (mem.get(out) == FILL).all() and (mem.get(idx) == FILL).all()
        res = ctypes.c_uint64(0)
        f = lib._f("lce_index_bytes")
        assert f(n, 5, ctypes.byref(res)) == EINVAL and f(n, w, None) == EINVAL and f(1 << 32, 4, ctypes.byref(res)) == EINVAL
        # the size: the header's formula and the advertised bound
        for m in (0, 1, 64, 65, 4096, 4097, n, 3 * 10 ** 9 + 1):
            if m <= 0xFFFFFFFF or bits == 64:
                assert lib.lce_index_bytes(m, bits) == R.index_bytes(m, w) < 2 * m * w + m * w // 8 + 16384, m
        # n = 0 and q = 0 succeed, null arrays allowed
        assert isa_d(None, 0, None, None) == 0 and isa_h(None, 0, None, 0) == 0
        empty = lib.lce_build(np.zeros(0, dtype=_dt(bits)), np.zeros(0, dtype=_dt(bits)), idx_bits=bits)
        assert empty.size == 256 and np.array_equal(empty, R.encode([], [], w))
        assert lib.lce(empty, [], []).size == 0 and lib.lce_range_min(blob, [], []).size == 0
        assert rmd(X, need, None, None, 0, None, None) == 0 and lcd(X, need, None, None, 0, 5, None, None) == 0
        with pytest.raises(Exception) as e:                  # no position is below n = 0
            lib.lce(empty, [0], [0])
        assert e.value.code == EINVAL
        # not a suffix array: a value >= n, a value twice
        for bad_at, bad_val in ((n // 2, n), (n // 2, np.iinfo(_dt(bits)).max), (7, int(sa[8]))):
            bad = sa.copy()
            bad[bad_at] = bad_val
            dbad = mem.put(bad)
            for rc in (isa_h(bad.ctypes.data, n, h1.ctypes.data, 0), blh(bad.ctypes.data, hl, n, hidx.ctypes.data, need, 0),
                       isa_d(mem.ptr(dbad), n, D, None), bld(mem.ptr(dbad), Lp, n, D, need, None)):
                assert rc == EINVAL and b"not a suffix array" in last()
            assert (h1 == 0x5A).all() and (hidx == 0x5A).all()
        # refused queries: 0 in their slots, the others answered, the call fails
        lo = np.array([5, 9, 0, n - 1, 3], dtype=np.uint64)
        hi = np.array([9, 5, n, n - 1, 1 << 40], dtype=np.uint64)
        L0 = R.lcp0(LCP)
        for form in forms_of(lib, mem):
            with pytest.raises(Exception) as e:
                form.range_min(blob, lo, hi)
            assert e.value.code == EINVAL
            if form.name == "device":
                assert form.last.tolist() == [R.range_min(L0, 5, 9), 0, 0, int(L0[n - 1]), 0]
            with pytest.raises(Exception) as e:
                form.lce(blob, [1, n, 2, 1 << 63], [2, 1, n, 3], 1)
            assert e.value.code == EINVAL
            if form.name == "device":
                assert form.last.tolist() == [R.lce_brute(T.tobytes(), 1, 2, 1), 0, 0, 0]
        hout = np.full(5, 77, dtype=np.uint64)
        assert rmh(hb, need, lo.ctypes.data, hi.ctypes.data, 5, hout.ctypes.data, 0) == EINVAL
        assert hout.tolist() == [R.range_min(L0, 5, 9), 0, 0, int(L0[n - 1]), 0]
        assert lib.lce(blob, [3], [9], 1024).tolist() == [R.lce_brute(T.tobytes(), 3, 9, 1024)]


def header_sweep(lib, mem):
    """Every damaged header word is refused by the host and the device query calls, before the body is read."""
    n = 5000
    SA, LCP = arbitrary_arrays(n)
    for bits in (32, 64):
        blob = lib.lce_build(SA, LCP, idx_bits=bits)
        assert np.array_equal(blob[:256].view(np.uint64), R.header(n, bits // 8))
        q = np.array([1, 2], dtype=np.uint64)
        dev = DeviceForm(lib, mem)
        for word, flip in itertools.product(range(32), (1 << 40, 1 << 63, 3)):
            bad = blob.copy()
            bad[:256].view(np.uint64)[word] ^= np.uint64(flip)
            if word == 2 and flip == 3:                      # n = 5003 has this very layout: a valid header of another n
                continue
            for call in (lambda: lib.lce(bad, q, q), lambda: lib.lce_range_min(bad, q, q), lambda: dev.lce(bad, q, q), lambda: dev.range_min(bad, q, q)):
                with pytest.raises(Exception) as e:
                    call()
                assert e.value.code == EINVAL, (word, flip)
        with pytest.raises(Exception):
            lib.lce(blob[:blob.size - 256].copy(), q, q)     # a truncated blob


def test_refusals_the_empty_text_and_values_that_are_no_positions():
    refusal_sweep(emul(), HostMem())


def test_every_damaged_header_word_is_refused():
    header_sweep(emul(), HostMem())


# ---- 5. a damaged body: a child process, the emulation only -----------------------------------------------------------------------------

_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [%(tests)r, %(root)r]
import caps_sa_amd
from test_emul_kmers import HostMem
from test_emul_lce import DeviceForm, arbitrary_arrays
E = caps_sa_amd.CapsLib(%(so)r, "caps_sa_emul_")
rs = np.random.RandomState(31)
n = 9000
SA, LCP = arbitrary_arrays(n, floor=0)
dev = DeviceForm(E, HostMem())
for bits in (32, 64):
    blob = E.lce_build(SA, LCP %% 60, idx_bits=bits)
    for trial in range(500):
        at = rs.randint(256, blob.size)
        blob[at] ^= np.uint8(1 << rs.randint(0, 8)) if trial %% 2 else np.uint8(0xFF)
        I, J = rs.randint(0, n, size=48).astype(np.uint64), rs.randint(0, n, size=48).astype(np.uint64)
        form = dev if trial %% 4 == 0 else None
        got = form.lce(blob, I, J, 8) if form else E.lce(blob.copy(), I, J, 8)        # (CAPS_SA_OK: the body is not checked; the guards are)
        assert (got <= n - np.maximum(I, J)).all()
        lo, hi = np.minimum(I, J), np.maximum(I, J)
        form.range_min(blob, lo, hi) if form else E.lce_range_min(blob.copy(), lo, hi)
print("done")
"""


def test_flipped_body_bytes_end_inside_the_buffers():
    """1,000 flipped body bytes, one after the other, queries after every one: every call ends with CAPS_SA_OK (or CAPS_SA_EINVAL),
    every extension stays inside the text and every guard is intact.  In a child process, so that an access outside a buffer ends the
    child and not the suite.  Never on a GPU."""
    emul()
    code = _CHILD % {"tests": os.path.join(ROOT, "tests"), "root": ROOT, "so": os.path.join(EMUL_DIR, "libcaps_sa_emul.so")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("done"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- 6. the reference's own arrays ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["large_dna_cli_140k", "large_latin1_signed_136k"])
def test_the_references_own_arrays(name):
    """(text, sa, lcp) made by the reference's script: the blob is the encoder's, extensions are the text's."""
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    T, SA, LCP = np.ascontiguousarray(z["text"], dtype=np.uint8), z["sa"], z["lcp"]
    n = int(T.size)
    E = emul()
    blob = check_blob(HostForm(E), SA, LCP, 32)
    I, J = pairs_of(n, np.random.RandomState(2), 3000)
    far = I != J
    for k in (0, 3):
        got = E.lce(blob, I, J, k)
        assert np.array_equal(got[far], R.lce_brute_np(T, I[far], J[far], k, cap=512))
        assert np.array_equal(got[~far], np.uint64(n) - I[~far])
    dev = DeviceForm(E, HostMem())
    assert np.array_equal(dev.lce(check_blob(dev, SA, LCP, 64), I[:500], J[:500], 3), E.lce(blob, I[:500], J[:500], 3))


# ---- 7. the Python surface -------------------------------------------------------------------------------------------------------------

def test_python_class_and_module_function(tmp_path):
    import caps_sa_amd
    t = b"GATTACAGATTACA"
    SA, LCP = naive_sa_lcp(t)
    E = emul()
    assert caps_sa_amd.isa(SA.astype(np.uint32), _lib=E).tolist() == R.isa_of(SA)
    x = caps_sa_amd.LCEIndex.from_arrays(SA.astype(np.uint32), LCP.astype(np.uint32), _lib=E)
    assert x.n == len(t) and x.nbytes == x.blob.size == R.index_bytes(len(t), 4) and x.isa().tolist() == R.isa_of(SA)
    assert x.lce([0, 0, 1], [7, 8, 8]).tolist() == [7, 0, 6] and x.lce([0], [8], mismatches=1).tolist() == [1]
    assert x.range_min([1], [len(t) - 1]).tolist() == [0]
    x.save(str(tmp_path / "x.lce"))
    y = caps_sa_amd.LCEIndex.load(str(tmp_path / "x.lce"), _lib=E)
    assert np.array_equal(y.blob, x.blob) and y.lce([0], [7]).tolist() == [7]
    for junk in (np.zeros(300, dtype=np.uint8), x.blob[:100]):
        with pytest.raises(ValueError):
            caps_sa_amd.LCEIndex(junk)
    with pytest.raises(ValueError):
        x.lce([0], [1], mismatches=-1)


# ---- 8. the other emulation builds ---------------------------------------------------------------------------------------------------

def small_sweeps(E):
    """The blob's constants are the same in every build: the same sweeps, the same blobs."""
    forms = forms_of(E, HostMem())
    assert short_text_sweep(forms, max_len=4) == sum(3 ** n for n in range(1, 5))
    assert size_sweep(forms, [65, 4097, 12289], widths=(32, 64), pairs=24, ks=(0, 2)) == 3 * 4 * 4
    tl, th = tier_spans()
    SA, LCP = arbitrary_arrays()
    blob = check_blob(forms[1], SA, LCP, 32)
    assert np.array_equal(forms[0].range_min(blob, tl, th), R.SparseTable(R.lcp0(LCP)).query(tl, th))
    isa_sweep(forms)


def test_reversed_order_and_small_tile_builds_give_the_same_answers():
    small_sweeps(emul_small())
    small_sweeps(emul_rev(True))
    small_sweeps(emul_rev(False))


@pytest.mark.slow
def test_poisoned_and_race_checked_builds_give_the_same_answers():
    """The small sweeps once more with LDS and registers starting as 0xA5 and the threads in a scattered order, and under the
    barrier-race detector (no race may be found)."""
    import caps_sa_amd
    for name in ("libcaps_sa_emul_small_poison.so", "libcaps_sa_emul_small_race.so"):
        subprocess.check_call(["make", "-s", "-C", EMUL_DIR, name])
        path = os.path.join(EMUL_DIR, name)
        small_sweeps(caps_sa_amd.CapsLib(path, "caps_sa_emul_"))
        if "race" in name:
            raw = ctypes.CDLL(path)
            raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
            assert int(raw.caps_sa_emul_races_found()) == 0
