"""CPU: LPF, Prev and the LZ77 factorization from SA and LCP (include/caps_sa_hip.h "LPF and LZ77 from SA and LCP", caps_sa_hip_lpf_*,
caps_sa_hip_lz77_*) through the host emulation of the kernels.

Every comparison is exact.  The truth is lz_reference: LPF by brute force over the text, (LPF, Prev) by the per-rank array rule (a naive
scan and a stack version that agree on every short text) and the clamped chain.  The sweeps are functions of a "form" (the host or the
device entry points of a library), so that test_gpu_lz.py runs the same ones on the GPU.  The device form always writes into buffers
preset to 0xA5 with guard bytes before and behind them and a workspace of exactly the advertised size, itself guarded."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import lz_reference as R
from emul_util import EMUL_DIR, ROOT, emul, emul_rev, emul_small
from sa_check import sa_lcp
from test_emul_kmers import HostMem, naive_sa_lcp

EINVAL = -1
FILL = 0xA5
GUARD = 64
FRONT = 72
REC = 24
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385, 32767, 32768, 32769, 49153]
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
LPF_TILE, LZ_TILE = 4096, 16384                           # kernels.h (the small-tile builds: 256 and 4096)
LZ_GROUP = 64 * LZ_TILE                                   # positions of a group of tiles (the small-tile builds: 16 * 4096)


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _none(bits):
    return int(np.iinfo(_dt(bits)).max)


def lz_dtype():
    import caps_sa_amd
    return caps_sa_amd.LZ_DTYPE


class HostForm:
    """The host entry points (CapsLib.lpf / lz77)."""
    name = "host"

    def __init__(self, lib):
        self.lib = lib

    def lpf(self, SA, LCP, bits):
        return self.lib.lpf(SA, LCP, idx_bits=bits)

    def lz77(self, SA, LCP, bits):
        return self.lib.lz77(SA, LCP, idx_bits=bits)


class DeviceForm:
    """The *_device entry points on `mem`."""
    name = "device"

    def __init__(self, lib, mem):
        self.lib, self.mem = lib, mem

    def _lpf_raw(self, SA, LCP, bits, own_ws=True):
        m, w = self.mem, bits // 8
        sa, lcp = np.ascontiguousarray(SA, dtype=_dt(bits)), np.ascontiguousarray(LCP, dtype=_dt(bits))
        n = int(sa.size)
        dsa, dlcp = m.put(sa), m.put(lcp)
        out_l, out_p = m.filled(FRONT + n * w + GUARD), m.filled(FRONT + n * w + GUARD)
        wsb = self.lib.lpf_workspace_bytes(n, bits)
        ws = m.filled(wsb + GUARD)
        self.lib.lpf_device(m.ptr(dsa) if n else 0, m.ptr(dlcp) if n else 0, n, m.ptr(out_l) + FRONT, m.ptr(out_p) + FRONT,
                            m.ptr(ws) if own_ws else 0, wsb if own_ws else 0, idx_bits=bits)
        for buf in (out_l, out_p):
            g = m.get(buf)
            assert (g[:FRONT] == FILL).all() and (g[FRONT + n * w:] == FILL).all(), "a guard of LPF or Prev was written"
        assert (m.get(ws)[wsb:] == FILL).all(), "the guard of the workspace was written"
        assert np.array_equal(m.get(dsa)[:n * w], sa.view(np.uint8)) and np.array_equal(m.get(dlcp)[:n * w], lcp.view(np.uint8))
        return out_l, out_p, n

    def lpf(self, SA, LCP, bits, own_ws=True):
        out_l, out_p, n = self._lpf_raw(SA, LCP, bits, own_ws)
        w = bits // 8
        return (self.mem.get(out_l)[FRONT:FRONT + n * w].copy().view(_dt(bits)), self.mem.get(out_p)[FRONT:FRONT + n * w].copy().view(_dt(bits)))

    def parse(self, LPF, Prev, bits, own_ws=True):
        """lz77_device on any two arrays: the counting call, then the writing call into a guarded buffer."""
        m = self.mem
        lpf, prev = np.ascontiguousarray(LPF, dtype=_dt(bits)), np.ascontiguousarray(Prev, dtype=_dt(bits))
        n = int(lpf.size)
        dl, dp = m.put(lpf), m.put(prev)
        wsb = self.lib.lz77_workspace_bytes(n, bits)
        ws = m.filled(wsb + GUARD)
        kw = dict(dWS_ptr=m.ptr(ws) if own_ws else 0, ws_bytes=wsb if own_ws else 0, idx_bits=bits)
        args = (m.ptr(dl) if n else 0, m.ptr(dp) if n else 0, n)
        z = self.lib.lz77_device(*args, **kw)
        buf = m.filled(FRONT + REC * z + GUARD)
        if z:
            assert self.lib.lz77_device(*args, dRecords_ptr=m.ptr(buf) + FRONT, capacity=z, **kw) == z
        out = m.get(buf)
        assert (out[:FRONT] == FILL).all() and (out[FRONT + REC * z:] == FILL).all(), "a guard of the records was written"
        assert (m.get(ws)[wsb:] == FILL).all(), "the guard of the workspace was written"
        return out[FRONT:FRONT + REC * z].copy().view(lz_dtype())

    def lz77(self, SA, LCP, bits):
        lpf, prev = self.lpf(SA, LCP, bits)
        return self.parse(lpf, prev, bits)


def forms_of(lib, mem):
    return (HostForm(lib), DeviceForm(lib, mem))


# ---- the checks --------------------------------------------------------------------------------------------------------------------

def check_arrays(form, SA, LCP, bits, want=None, T=None):
    """lpf and lz77 of (SA, LCP) through `form` against the array rule (want: its cached answer with none = -1)."""
    n = int(np.asarray(SA).size)
    if want is None:
        want = R.lpf_stack(SA, LCP, none=-1)
    L, P = want
    none = _none(bits)
    Pw = [none if x < 0 else x for x in P]
    l, p = form.lpf(SA, LCP, bits)
    assert l.dtype == _dt(bits) and l.size == n and p.size == n
    assert l.tolist() == L, (form.name, bits, n)
    assert p.tolist() == Pw, (form.name, bits, n)
    rec = form.lz77(SA, LCP, bits)
    parse = R.lz_parse(L, Pw, n)
    assert rec.tolist() == parse, (form.name, bits, n)
    if T is not None:
        assert R.lz_decode(parse, T.tobytes()) == T.tobytes()
    return want


def check_matches(T, L, P):
    """The text's side of the definition: Prev < i, the bytes agree for LPF bytes, and LPF[i] <= n - i."""
    t = T.tobytes()
    n = len(t)
    for i in range(n):
        if L[i]:
            assert 0 <= P[i] < i and L[i] <= n - i and t[P[i]:P[i] + L[i]] == t[i:i + L[i]], i
        else:
            assert P[i] < 0


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


def size_sweep(forms, sizes, widths=(32, 64)):
    done = 0
    for n in sizes:
        for name, T, SA, LCP in texts_of(n):
            want = None
            for form, bits in itertools.product(forms, widths):
                want = check_arrays(form, SA, LCP, bits, want, T)
                done += 1
            L, P = want
            if n <= 4096 or name == "a^n":
                check_matches(T, L, P)
            if name == "a^n" and n:
                assert L == [0] + list(range(n - 1, 0, -1)) and P[1:] == list(range(n - 1))
                assert len(R.lz_parse(L, P, n)) == min(n, 2)
    return done


def permutations_of(n, tile, seed=2):
    rs = np.random.RandomState(seed + n)
    ar = np.arange(n, dtype=np.uint64)
    yield "identity", ar.copy()
    yield "reversed", ar[::-1].copy()
    yield "random", rs.permutation(n).astype(np.uint64)
    for name, period in (("sawtooth 64", 64), ("sawtooth of a tile", tile)):
        # rank r holds (r mod period) * ceil(n / period) + r div period, squeezed to 0 .. n - 1: ascending teeth
        key = (ar % period) * ((n + period - 1) // period) + ar // period
        yield name, np.argsort(np.argsort(key, kind="stable"), kind="stable").astype(np.uint64)
    half = (n + 1) // 2
    yield "organ pipe", np.concatenate([ar[:half] * 2, (ar[half:][::-1] - half) * 2 + 1])[:n].astype(np.uint64) if n > 1 else ar.copy()


def lcps_of(n, tile, seed=3):
    rs = np.random.RandomState(seed + n)
    yield "random", rs.randint(0, 1 << 20, size=n).astype(np.uint64)
    yield "all equal", np.full(n, 7, dtype=np.uint64)
    for name, at in (("a 0 in a skipped block", n // 2 + 70), ("a 0 in a skipped tile", n // 2 - tile // 2)):
        a = rs.randint(5, 1 << 20, size=n).astype(np.uint64)
        a[min(max(at, 0), n - 1)] = 0
        yield name, a


def arbitrary_sweep(forms, n, tile, widths=(32, 64)):
    """Arrays that are no text's: every permutation x every LCP against the array rule (searches that leave their tile on either
    side, that find nothing, minima inside skipped summaries, ties between the sides)."""
    done = 0
    for (pn, SA), (ln, LCP) in itertools.product(permutations_of(n, tile), lcps_of(n, tile)):
        assert sorted(SA.tolist()) == list(range(n)), pn
        want = None
        for k, form in enumerate(forms):
            want = check_arrays(form, SA, LCP, widths[(done + k) % len(widths)], want)
        done += 1
    return done


def parse_sweep(form, lz_tile, widths=(32, 64)):
    """lz77_device on LPF / Prev arrays of its own making: phrases that start and end on every block and tile edge, literals only,
    one phrase, and garbage above n - s (the parse is the clamped chain)."""
    rs = np.random.RandomState(6)
    n = 2 * lz_tile + 77
    cases = [np.zeros(n), np.full(n, n), np.full(n, 1 << 31)]
    cases += [np.full(n, v) for v in (1, 2, 63, 64, 65, lz_tile - 1, lz_tile, lz_tile + 1, lz_tile + 64)]
    cases += [rs.randint(0, 4, size=n), rs.randint(0, 130, size=n), rs.randint(0, 3 * lz_tile, size=n), rs.randint(0, 1 << 32, size=n)]
    cases.append(64 - np.arange(n) % 64)                    # every phrase ends on the next multiple of 64
    for k, lpf in enumerate(cases):
        bits = widths[k % len(widths)]
        lpf = lpf.astype(np.uint64) & np.uint64(_none(bits))
        prev = rs.randint(0, 1 << 32, size=n).astype(np.uint64)
        rec = form.parse(lpf, prev, bits, own_ws=bool(k % 3))
        assert rec.tolist() == R.lz_parse(lpf, prev, n), k
    for n in (1, 2, 63, 64, 65, lz_tile, lz_tile + 1):
        assert form.parse(np.zeros(n), np.zeros(n), 32).tolist() == [(s, 1, R.LITERAL) for s in range(n)]
        assert form.parse(np.full(n, n), np.full(n, 5), 64).tolist() == [(0, n, 5)]
    assert form.parse(np.zeros(0), np.zeros(0), 32).size == 0


# ---- 1. every short text ------------------------------------------------------------------------------------------------------------

LETTERS3 = bytes([0x41, 0x43, 0xC8])                     # (0xC8 sorts first: signed char)


def short_text_sweep(forms, max_len=7, widths=(32, 64)):
    done = 0
    for n in range(1, max_len + 1):
        for tup in itertools.product(LETTERS3, repeat=n):
            t = bytes(tup)
            T = np.frombuffer(t, dtype=np.uint8)
            SA, LCP = naive_sa_lcp(t)
            L, P = R.lpf_naive(SA, LCP, none=-1)
            assert L == R.lpf_brute(t) and (L, P) == R.lpf_stack(SA, LCP, none=-1), t
            check_matches(T, L, P)
            for k, form in enumerate(forms):
                check_arrays(form, SA, LCP, widths[(done + k) % len(widths)], (L, P), T)
            done += 1
    return done


def test_every_short_text():
    E = emul()
    assert short_text_sweep((HostForm(E),)) == sum(3 ** n for n in range(1, 8))
    assert short_text_sweep((DeviceForm(E, HostMem()),)) == sum(3 ** n for n in range(1, 8))


# ---- 2. sizes around blocks and tiles -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_texts(n):
    assert size_sweep(forms_of(emul(), HostMem()), [n]) == 4 * 4


# ---- 3. arrays that are no text's -------------------------------------------------------------------------------------------------------

def test_arbitrary_arrays_of_twelve_tiles():
    assert arbitrary_sweep(forms_of(emul(), HostMem()), 49153, LPF_TILE) == 24


@pytest.mark.parametrize("n", [767, 768, 769])
def test_arbitrary_arrays_of_three_small_tiles(n):
    assert arbitrary_sweep(forms_of(emul_small(), HostMem()), n, 256) == 24


def monotone_sweep(form, n):
    """Reversed with no 0 in LCP: every left search runs to the front of the array and finds nothing.  Identity with an ascending
    LCP: the right side's minimum stays above the left result, so every right search runs to the end.  Closed forms."""
    ar = np.arange(n, dtype=np.uint64)
    l, p = form.lpf(ar[::-1].copy(), np.full(n, 9, dtype=np.uint64), 64)
    assert l.tolist() == [0] + [9] * (n - 1) and p.tolist() == [_none(64)] + list(range(n - 1))
    l, p = form.lpf(ar, ar + 1, 32)
    assert l.tolist() == [0] + list(range(2, n + 1)) and p.tolist() == [_none(32)] + list(range(n - 1))


def test_monotone_permutations_finish_because_the_search_skips():
    """65,537 ranks of the small-tile build (257 tiles, four levels above them): a search that walked rank by rank would make
    2^31 steps here."""
    monotone_sweep(HostForm(emul_small()), 65537)
    monotone_sweep(DeviceForm(emul(), HostMem()), 65537)


# ---- 4. the parse: counting call, writing call, capacity, edges -------------------------------------------------------------------------

def test_parse_edges_literals_and_garbage():
    parse_sweep(DeviceForm(emul(), HostMem()), LZ_TILE)
    parse_sweep(DeviceForm(emul_small(), HostMem()), 4096)


def group_sweep(form, gpos, lz_tile, widths=(32, 64)):
    """The hop's second level: three groups of tiles and a bit.  Phrases that land on a group's first positions (the composed exits),
    at 64 positions into it and beyond (the hop falls back to the group's tiles), exactly on group edges, and that jump over whole
    groups; short phrases between them so that every tile of a group is entered."""
    rs = np.random.RandomState(17)
    n = 3 * gpos + 2 * lz_tile + 5
    pos = np.arange(n, dtype=np.int64)
    to_edge = gpos - pos % gpos                             # from every position to the next group edge
    cases = [
        rs.randint(lz_tile // 8, lz_tile // 2, size=n),      # every tile entered, entries anywhere
        np.full(n, lz_tile + 3), np.full(n, gpos), np.full(n, gpos + 63), np.full(n, gpos + 64), np.full(n, gpos + 100),
        np.full(n, 2 * gpos + 7), np.full(n, n),
        to_edge, to_edge + 63, to_edge + 64, to_edge + lz_tile + 1,
        np.where(pos % gpos < lz_tile, to_edge + rs.randint(0, 200, size=n), rs.randint(lz_tile // 4, lz_tile, size=n)),
    ]
    for k, lpf in enumerate(cases):
        bits = widths[k % len(widths)]
        prev = rs.randint(0, 1 << 32, size=n).astype(np.uint64)
        rec = form.parse(lpf.astype(np.uint64), prev, bits, own_ws=bool(k % 2))
        assert rec.tolist() == R.lz_parse(lpf, prev, n), k


def test_parse_over_groups_of_tiles():
    group_sweep(DeviceForm(emul_small(), HostMem()), 16 * 4096, 4096)
    group_sweep(DeviceForm(emul(), HostMem()), LZ_GROUP, LZ_TILE, widths=(32,))


def capacity_sweep(lib, mem, widths=(32, 64)):
    rs = np.random.RandomState(12)
    n = 40000
    T = rs.choice(DNA, size=n).astype(np.uint8)
    SA, LCP = sa_lcp(T, 64)
    L, P = R.lpf_stack(SA, LCP, none=-1)
    for bits in widths:
        none = _none(bits)
        want = R.lz_parse(L, [none if x < 0 else x for x in P], n)
        z = len(want)
        form = DeviceForm(lib, mem)
        lpf, prev = form.lpf(SA, LCP, bits, own_ws=False)                 # a NULL workspace: the call's own
        dl, dp = mem.put(lpf), mem.put(prev)
        args = (mem.ptr(dl), mem.ptr(dp), n)
        assert lib.lz77_device(*args, idx_bits=bits) == z > 1
        buf = mem.filled(FRONT + REC * z + GUARD)
        with pytest.raises(Exception) as e:                 # one too small: refused, the number is still there, nothing is written
            lib.lz77_device(*args, dRecords_ptr=mem.ptr(buf) + FRONT, capacity=z - 1, idx_bits=bits)
        assert e.value.code == EINVAL and e.value.n_phrases == z
        assert (mem.get(buf) == FILL).all()
        assert lib.lz77_device(*args, dRecords_ptr=mem.ptr(buf) + FRONT, capacity=z + 3, idx_bits=bits) == z
        out = mem.get(buf)
        assert (out[:FRONT] == FILL).all() and (out[FRONT + REC * z:] == FILL).all()
        assert out[FRONT:FRONT + REC * z].copy().view(lz_dtype()).tolist() == want
        # the host form's protocol; only one of the two outputs of lpf
        sa, lcp = SA.astype(_dt(bits)), LCP.astype(_dt(bits))
        sfx = "u32" if bits == 32 else "u64"
        nz = ctypes.c_uint64(7)
        rec = np.full(REC * z + GUARD, FILL, dtype=np.uint8)
        f = lib._f(f"lz77_{sfx}")
        assert f(sa.ctypes.data, lcp.ctypes.data, n, None, 0, ctypes.byref(nz), 0) == 0 and nz.value == z
        nz.value = 7
        assert f(sa.ctypes.data, lcp.ctypes.data, n, rec.ctypes.data, z - 1, ctypes.byref(nz), 0) == EINVAL and nz.value == z
        assert (rec == FILL).all()
        assert f(sa.ctypes.data, lcp.ctypes.data, n, rec.ctypes.data, z, ctypes.byref(nz), 0) == 0 and nz.value == z
        assert (rec[REC * z:] == FILL).all() and rec[:REC * z].copy().view(lz_dtype()).tolist() == want
        g = lib._f(f"lpf_{sfx}")
        only = np.full(n, 3, dtype=_dt(bits))
        assert g(sa.ctypes.data, lcp.ctypes.data, n, only.ctypes.data, None, 0) == 0 and only.tolist() == L
        assert g(sa.ctypes.data, lcp.ctypes.data, n, None, only.ctypes.data, 0) == 0 and only.tolist() == [none if x < 0 else x for x in P]


def test_counting_call_writing_call_and_capacity():
    capacity_sweep(emul(), HostMem())


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------

def refusal_sweep(lib, mem):
    """Every refusal: CAPS_SA_EINVAL, and no output is touched."""
    n = 1000
    T = np.random.RandomState(3).choice(DNA, size=n).astype(np.uint8)
    SA, LCP = sa_lcp(T, 64)
    for bits in (32, 64):
        sfx = "u32" if bits == 32 else "u64"
        w = bits // 8
        sa, lcp = SA.astype(_dt(bits)), LCP.astype(_dt(bits))
        dsa, dlcp = mem.put(sa), mem.put(lcp)
        S, Lp = mem.ptr(dsa), mem.ptr(dlcp)
        wl, wz = lib.lpf_workspace_bytes(n, bits), lib.lz77_workspace_bytes(n, bits)
        ws = mem.filled(max(wl, wz))
        W = mem.ptr(ws)
        o1, o2, recs = mem.filled(n * w), mem.filled(n * w), mem.filled(REC * n)
        O1, O2, Rp = mem.ptr(o1), mem.ptr(o2), mem.ptr(recs)
        nz = ctypes.c_uint64(0x5A5A)
        nr = ctypes.byref(nz)
        ld, zd, lh, zh = (lib._f(f"lpf_device_{sfx}"), lib._f(f"lz77_device_{sfx}"), lib._f(f"lpf_{sfx}"), lib._f(f"lz77_{sfx}"))
        hs, hl = sa.ctypes.data, lcp.ctypes.data
        h1, h2 = np.full(n, 0x5A, dtype=_dt(bits)), np.full(n, 0x5A, dtype=_dt(bits))
        calls = [
            ld(None, Lp, n, O1, O2, W, wl, None),                              # a null SA or LCP with n > 0
            ld(S, None, n, O1, O2, W, wl, None),
            ld(S, Lp, n, None, None, W, wl, None),                             # both outputs null
            ld(S, Lp, n, O1, O2, W, wl - 512, None),                           # a workspace that is too small
            zd(None, O2, n, Rp, n, nr, W, wz, None),
            zd(O1, None, n, Rp, n, nr, W, wz, None),
            zd(O1, O2, n, Rp, n, None, W, wz, None),
            zd(O1, O2, n, Rp + 4, n, nr, W, wz, None),                         # records not 8-byte aligned
            zd(O1, O2, n, Rp, n, nr, W, wz - 512, None),
            lh(None, hl, n, h1.ctypes.data, h2.ctypes.data, 0),
            lh(hs, None, n, h1.ctypes.data, h2.ctypes.data, 0),
            lh(hs, hl, n, None, None, 0),
            zh(None, hl, n, None, 0, nr, 0),
            zh(hs, None, n, None, 0, nr, 0),
            zh(hs, hl, n, None, 0, None, 0),
        ]
        if bits == 32:                                       # n > UINT32_MAX with _u32: refused before anything is read
            big = 1 << 32
            calls += [ld(S, Lp, big, O1, O2, None, 0, None), zd(O1, O2, big, None, 0, nr, None, 0, None),
                      lh(hs, hl, big, h1.ctypes.data, h2.ctypes.data, 0), zh(hs, hl, big, None, 0, nr, 0)]
        assert calls == [EINVAL] * len(calls), calls
        assert nz.value == 0x5A5A and (h1 == 0x5A).all() and (h2 == 0x5A).all()
        for buf in (o1, o2, recs, ws):
            assert (mem.get(buf) == FILL).all()
        out = ctypes.c_uint64(0)
        for name in ("lpf_workspace_bytes", "lz77_workspace_bytes"):
            assert lib._f(name)(n, 5, ctypes.byref(out)) == EINVAL
            assert lib._f(name)(n, w, None) == EINVAL
            assert lib._f(name)(1 << 32, 4, ctypes.byref(out)) == EINVAL
        # the header's formulas, exactly, and the advertised bounds: no array of n entries for lpf, one for lz77
        up = lambda b: (b + 255) // 256 * 256
        for m in (1, 64, 65, n, 4097, 3 * 10 ** 9 + 1):
            nodes, c = 0, m
            while True:
                c = (c + 63) // 64
                nodes += c
                if c == 1:
                    break
            assert lib.lpf_workspace_bytes(m, bits) == 2 * up(nodes * w) + 1024, m
            nt, ng = (m + 16383) // 16384, (m + (1 << 20) - 1) >> 20
            assert lib.lz77_workspace_bytes(m, bits) == up(m * w) + up(ng * 64 * w) + up(ng * 8) + up(nt * 8) + up((nt + 1) * 8) + 512, m
        big = 3 * 10 ** 9 + 1
        assert lib.lpf_workspace_bytes(big, bits) <= big * w // 16
        assert lib.lz77_workspace_bytes(big, bits) <= big * w + 16 * (big // 16384 + 2) + (64 * w + 8) * (big // (1 << 20) + 1) + 2048
        # n = 0 succeeds with z = 0, null arrays allowed
        assert ld(None, None, 0, None, None, None, 0, None) == 0 and lh(None, None, 0, None, None, 0) == 0
        assert zd(None, None, 0, None, 0, nr, None, 0, None) == 0 and nz.value == 0
        nz.value = 9
        assert zh(None, None, 0, None, 0, nr, 0) == 0 and nz.value == 0
        # an SA value >= n: "not a suffix array", on the host: the value is never used as an index
        bad = sa.copy()
        bad[n // 2] = n
        assert lh(bad.ctypes.data, hl, n, h1.ctypes.data, h2.ctypes.data, 0) == EINVAL
        assert b"not a suffix array" in lib._f("last_error")()
        bad[n // 2] = _none(bits)
        assert zh(bad.ctypes.data, hl, n, None, 0, nr, 0) == EINVAL
        dbad = mem.put(bad)
        assert ld(mem.ptr(dbad), Lp, n, O1, None, None, 0, None) == EINVAL
        assert (mem.get(o2) == FILL).all()


def test_refusals_the_empty_text_and_values_that_are_no_positions():
    refusal_sweep(emul(), HostMem())


# ---- 6. arrays that are no SA / LCP: a child process, the emulation only --------------------------------------------------------------

_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [%(tests)r, %(root)r]
import caps_sa_amd
from test_emul_kmers import HostMem
from test_emul_lz import DeviceForm
E = caps_sa_amd.CapsLib(%(so)r, "caps_sa_emul_")
rs = np.random.RandomState(21)
form = DeviceForm(E, HostMem())
for n in (1, 5, 4097, 16384, 40001):
    for bits in (32, 64):
        for trial in range(4):
            SA = rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
            LCP = rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
            if trial == 1:
                SA %%= n                                     # values in range, duplicates and gaps
                LCP %%= 40
            if trial == 2:
                SA %%= n + 3                                 # a few values that are no positions
            if trial == 3:
                SA = np.full(n, n - 1, dtype=np.uint64)     # one value everywhere: nothing is ever below it
            if bits == 64 and trial == 0:
                SA = SA * SA
                LCP = LCP * LCP + SA
            try:
                form.lpf(SA, LCP, bits)                     # (CAPS_SA_OK or "not a suffix array"; asserts the guards)
            except caps_sa_amd.CapsSaError as e:
                assert e.code == -1 and (SA >= n).any()
            else:
                assert (SA < n).all()
            rec = form.parse(SA, LCP, bits)                 # any two arrays as LPF and Prev
            assert 1 <= rec.size <= n and int(rec["len"].sum()) == n
print("done")
"""


def test_garbage_arrays_terminate_inside_their_buffers():
    """Random 32-bit (and 64-bit) garbage as SA / LCP and as LPF / Prev: every call ends with CAPS_SA_OK or the documented refusal
    and every guard is intact.  In a child process, so that an access outside a buffer ends the child and not the suite.  Never on a
    GPU."""
    emul()
    code = _CHILD % {"tests": os.path.join(ROOT, "tests"), "root": ROOT, "so": os.path.join(EMUL_DIR, "libcaps_sa_emul.so")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("done"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- 7. the reference's own arrays ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["large_dna_cli_140k", "large_latin1_signed_136k"])
def test_the_references_own_arrays(name):
    """(text, sa, lcp) made by the reference's script: LPF and Prev against the stack rule, the bytes behind every Prev, and the
    parse decodes to the text.  The latin1 file pins that the order of the letters does not matter."""
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    T, SA, LCP = np.ascontiguousarray(z["text"], dtype=np.uint8), z["sa"], z["lcp"]
    assert SA.size == T.size == LCP.size
    want = check_arrays(HostForm(emul()), SA, LCP, 32, None, T)
    check_arrays(DeviceForm(emul(), HostMem()), SA, LCP, 64, want)
    L, P = np.array(want[0]), np.array(want[1])
    t = T.tobytes()
    for i in np.random.RandomState(1).randint(0, T.size, size=3000).tolist():       # maximal: the next byte differs or the text ends
        if L[i]:
            assert t[P[i]:P[i] + L[i]] == t[i:i + L[i]] and (i + L[i] == T.size or t[P[i] + L[i]] != t[i + L[i]])


# ---- 8. the Python surface -------------------------------------------------------------------------------------------------------------

def test_module_level_functions_and_dtype():
    import caps_sa_amd
    assert caps_sa_amd.LZ_DTYPE.itemsize == 24 and caps_sa_amd.LZ_DTYPE.names == ("pos", "len", "src")
    assert caps_sa_amd.LZ_LITERAL == R.LITERAL
    t = b"GATTACAGATTACA"
    SA, LCP = naive_sa_lcp(t)
    E = emul()
    L, P = caps_sa_amd.lpf(SA.astype(np.uint32), LCP.astype(np.uint32), _lib=E)
    assert L.dtype == np.uint32 and L.tolist() == R.lpf_brute(t)
    rec = caps_sa_amd.lz77(SA, LCP, _lib=E)
    assert rec.dtype == caps_sa_amd.LZ_DTYPE and R.lz_decode(rec.tolist(), t) == t
    assert rec.tolist() == R.lz_parse(L, P, len(t)) and rec.tolist()[-1] == (7, 7, 0)


def small_buffer_sweep(lib):
    """CapsLib.lz77 tries one call with room for n / 8 + 1024 records; a parse with more phrases (here nearly n: no LCP above 1)
    takes the second call with the exact number."""
    rs = np.random.RandomState(23)
    n = 20000
    SA, LCP = rs.permutation(n).astype(np.uint64), np.ones(n, dtype=np.uint64)
    L, P = R.lpf_stack(SA, LCP)
    want = R.lz_parse(L, P, n)
    assert len(want) > n // 8 + 1024
    assert lib.lz77(SA, LCP).tolist() == want
    assert lib.lz77(SA[:9].argsort().astype(np.uint32), LCP[:9]).tolist() == R.lz_parse(*R.lpf_stack(SA[:9].argsort(), LCP[:9]), 9)


def test_python_lz77_when_the_first_buffer_is_too_small():
    small_buffer_sweep(emul())


# ---- 9. the other emulation builds ---------------------------------------------------------------------------------------------------

def small_sweeps(E, small):
    forms = forms_of(E, HostMem())
    assert short_text_sweep(forms, max_len=4, widths=(32, 64)) == sum(3 ** n for n in range(1, 5))
    assert size_sweep(forms, [257, 769, 4097], widths=(32,)) == 3 * 4 * 2
    assert arbitrary_sweep(forms, 769 if small else 8193, 256 if small else LPF_TILE) == 24
    parse_sweep(forms[1], 4096 if small else LZ_TILE)


def test_reversed_order_and_small_tile_builds_give_the_same_answers():
    small_sweeps(emul_small(), True)
    small_sweeps(emul_rev(True), True)
    small_sweeps(emul_rev(False), False)


@pytest.mark.slow
def test_poisoned_and_race_checked_builds_give_the_same_answers():
    """The small sweeps once more with LDS and registers starting as 0xA5 and the threads in a scattered order, and under the
    barrier-race detector (no race may be found)."""
    import caps_sa_amd
    for name in ("libcaps_sa_emul_small_poison.so", "libcaps_sa_emul_small_race.so"):
        subprocess.check_call(["make", "-s", "-C", EMUL_DIR, name])
        path = os.path.join(EMUL_DIR, name)
        small_sweeps(caps_sa_amd.CapsLib(path, "caps_sa_emul_"), True)
        if "race" in name:
            raw = ctypes.CDLL(path)
            raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
            assert int(raw.caps_sa_emul_races_found()) == 0
