"""CPU: matching statistics and maximal exact matches of the FM-index (include/caps_sa_hip.h "FM-index: matching statistics",
caps_sa_hip_fm_match_*, caps_sa_hip_fm_mems_*) through the host emulation of the kernels.

Every comparison is exact.  The truth is fm_match_reference (substring search, the naive suffix array, the brute-force definition
of a MEM).  The sweeps are functions of a library object and of a memory object, so that test_gpu_fm_match.py runs the same ones
through the host and the device entry points on the GPU."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fm_match_reference as M
import fm_reference as R
from emul_util import EMUL_DIR, ROOT, emul, emul_rev, emul_small
from test_emul_geometry import edge_patterns, family_case

EINVAL = -1
FILL = 0xA5
GUARD = 64
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
FM_NT = int(re.search(r"constexpr uint32_t FM_NT = (\d+);", open(os.path.join(ROOT, "caps-sa_amd", "csrc", "kernels.h")).read()).group(1))


# ---- memory of the *_device entry points: the emulation's "device" is host memory ------------------------------------------------

class HostMem:
    def filled(self, nbytes):
        return np.full(nbytes + GUARD, FILL, dtype=np.uint8)

    def put(self, a):
        return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy() if np.asarray(a).size else np.zeros(8, dtype=np.uint8)

    def ptr(self, buf):
        return buf.ctypes.data

    def get(self, buf):
        return buf


def raw_match(lib, mem, blob, cat, off, max_len=0, intervals=True):
    """caps_sa_*_fm_match_device on buffers preset to 0xA5 with a 64-byte guard behind each: -> (len, first, count); nothing but
    len (and first / count when asked for) is written."""
    q = off.size - 1
    total = int(off[-1] - off[0])
    d_index, d_cat, d_off = mem.put(blob), mem.put(cat), mem.put(off)
    d_len, d_first, d_count = mem.filled(4 * total), mem.filled(8 * total), mem.filled(8 * total)
    lib.fm_match_device(mem.ptr(d_index), blob.size, mem.ptr(d_cat), mem.ptr(d_off), q, max_len, mem.ptr(d_len),
                        mem.ptr(d_first) if intervals else 0, mem.ptr(d_count) if intervals else 0)
    ln, first, count = mem.get(d_len), mem.get(d_first), mem.get(d_count)
    assert (ln[4 * total:] == FILL).all() and (first[8 * total:] == FILL).all() and (count[8 * total:] == FILL).all(), "a guard was written"
    assert np.array_equal(mem.get(d_index)[:blob.size], blob), "the index was written"
    if not intervals:
        assert (first == FILL).all() and (count == FILL).all(), "first / count were written without being asked for"
        return ln[:4 * total].view(np.uint32).copy(), None, None
    return ln[:4 * total].view(np.uint32).copy(), first[:8 * total].view(np.uint64).copy(), count[:8 * total].view(np.uint64).copy()


def raw_mems(lib, mem, blob, cat, off, min_len=1, workspace=True):
    """caps_sa_*_fm_mems_device, the counting call and then the writing call, on guarded buffers: -> (records, mem_off)."""
    q = off.size - 1
    total = int(off[-1] - off[0])
    d_index, d_cat, d_off = mem.put(blob), mem.put(cat), mem.put(off)
    ws_bytes = lib.fm_mems_workspace_bytes(total, q)
    d_ws = mem.filled(ws_bytes)
    ws = (mem.ptr(d_ws), ws_bytes) if workspace else (0, 0)
    d_moff = mem.filled(8 * (q + 1))
    lib.fm_mems_device(mem.ptr(d_index), blob.size, mem.ptr(d_cat), mem.ptr(d_off), q, min_len, mem.ptr(d_moff), 0, 0, *ws)
    moff = mem.get(d_moff)
    assert (moff[8 * (q + 1):] == FILL).all() and (mem.get(d_ws)[ws_bytes:] == FILL).all(), "a guard was written"
    moff = moff[:8 * (q + 1)].view(np.uint64).copy()
    found = int(moff[-1])
    d_mems, d_moff2 = mem.filled(32 * found), mem.filled(8 * (q + 1))
    lib.fm_mems_device(mem.ptr(d_index), blob.size, mem.ptr(d_cat), mem.ptr(d_off), q, min_len, mem.ptr(d_moff2), mem.ptr(d_mems), found, *ws)
    rec, moff2 = mem.get(d_mems), mem.get(d_moff2)
    assert (rec[32 * found:] == FILL).all() and (moff2[8 * (q + 1):] == FILL).all() and (mem.get(d_ws)[ws_bytes:] == FILL).all()
    assert np.array_equal(moff2[:8 * (q + 1)].view(np.uint64), moff), "the counting call and the writing call disagree"
    assert np.array_equal(mem.get(d_index)[:blob.size], blob), "the index was written"
    return rec[:32 * found].view(M.MEM_DTYPE).copy(), moff


class DeviceForm:
    """fm_match and fm_mems through the *_device entry points on preset, guarded buffers; everything else is the library's."""

    def __init__(self, lib, mem):
        self.lib, self.mem = lib, mem
        self.calls = 0

    def __getattr__(self, name):
        return getattr(self.lib, name)

    def fm_match(self, blob, patterns, max_len=0, intervals=False):
        cat, off = patterns if isinstance(patterns, tuple) else self.lib._patterns(patterns)
        return raw_match(self.lib, self.mem, blob, cat, off, max_len, intervals) + (off,)

    def fm_mems(self, blob, patterns, min_len=1):
        cat, off = patterns if isinstance(patterns, tuple) else self.lib._patterns(patterns)
        self.calls += 1
        return raw_mems(self.lib, self.mem, blob, cat, off, min_len, workspace=self.calls % 2 == 0)


# ---- the checker of a batch --------------------------------------------------------------------------------------------------

_texts = {}


def text_of(T, SA):
    key = T.tobytes()
    if key not in _texts:
        ref = M.Text(T, SA)
        ref.memo = {}
        _texts[key] = ref
    return _texts[key]


def answers(ref, P, max_len=0):
    """(L, first, count) of one pattern from the reference, kept per text."""
    key = (bytes(P), max_len)
    if key not in ref.memo:
        L = ref.lengths(P, max_len)
        ref.memo[key] = (L,) + ref.intervals(P, L)
    return ref.memo[key]


def mems_of(ref, P, min_len):
    key = (bytes(P), "mems", min_len)
    if key not in ref.memo:
        ref.memo[key] = ref.mems(P, min_len, answers(ref, P)[0])
    return ref.memo[key]


def mems_in_one_call(lib, blob, patterns, min_len):
    """The host form's writing call alone, with room for one record per pattern byte (there cannot be more)."""
    cat, off = lib._patterns(patterns)
    q, room = off.size - 1, int(off[-1])
    moff = np.zeros(q + 1, dtype=np.uint64)
    rec = np.zeros(room, dtype=M.MEM_DTYPE)
    lib._check(lib._f("fm_mems")(blob.ctypes.data, blob.size, cat.ctypes.data, off.ctypes.data, q, min_len, moff.ctypes.data, rec.ctypes.data, room, 0))
    assert not rec[int(moff[-1]):].view(np.uint8).any(), "records beyond mem_off[q] were written"
    return rec[:int(moff[-1])], moff


def check_batch(lib, blob, ref, pats, what, max_len=0, min_lens=(1, 2), packed=None, once=False):
    """L, the intervals and (without a cap) the MEM records of a batch against the reference.  packed: the (bytes, offsets) to send
    instead of the list (offsets that do not start at 0).  once: each call once (long patterns in the emulation: a lane per end
    walks its whole piece, sum(L) steps per run)."""
    send = packed if packed is not None else pats
    ln, first, count, off = lib.fm_match(blob, send, max_len, True)
    assert ln.dtype == np.uint32 and first.dtype == count.dtype == np.uint64, what
    if not once:
        only, f0, c0, _ = lib.fm_match(blob, send, max_len, False)
        assert f0 is None and c0 is None, what
        assert np.array_equal(only, ln), (what, "lengths differ with and without intervals")
    want = [answers(ref, P, max_len) for P in pats]
    total = sum(len(P) for P in pats)
    assert ln.size == first.size == count.size == total == int(off[-1] - off[0]), what
    for name, got, k in (("len", ln, 0), ("first", first, 1), ("count", count, 2)):
        exp = np.concatenate([w[k] for w in want]) if total else np.zeros(0, dtype=got.dtype)
        assert np.array_equal(got, exp), (what, name, np.flatnonzero(got != exp)[:8])
    if max_len == 0:
        for min_len in min_lens:
            rec, moff = mems_in_one_call(lib, blob, send, min_len) if once and hasattr(lib, "_f") else lib.fm_mems(blob, send, min_len)
            exp, eoff = M.records([mems_of(ref, P, min_len) for P in pats])
            assert np.array_equal(moff, eoff), (what, min_len, "mem_off")
            assert rec.dtype == M.MEM_DTYPE and rec.tobytes() == exp.tobytes(), (what, min_len, rec[:4], exp[:4])
    return total


# ---- 1. every short text x every short pattern ---------------------------------------------------------------------------------

def test_every_short_text_and_every_short_pattern():
    """All texts over {A, C} with 1 <= n <= 7 against all patterns over {A, C, G} with 0 <= m <= 5 (G is no letter of any of the
    indices): L, the intervals and the MEMs for min_len 1 and 2.  The MEMs come from trying every (start, end)."""
    E = emul()
    pats = [bytes(p) for m in range(6) for p in itertools.product(b"ACG", repeat=m)]
    assert len(pats) == sum(3 ** m for m in range(6))
    texts = 0
    for n in range(1, 8):
        for letters in itertools.product(b"AC", repeat=n):
            T = np.array(letters, dtype=np.uint8)
            SA = R.naive_sa(T)
            B, primary = R.bwt_of(T, SA)
            blob = E.fm_build(B, primary, SA if n % 2 else None, 1, 32 if texts % 2 else 64)
            ref = text_of(T, SA)
            for P in pats:
                for min_len in (1, 2):
                    brute = ref.mems_brute(P, min_len)
                    assert brute == ref.mems(P, min_len), (bytes(T), P, min_len)
                    ref.memo[(P, "mems", min_len)] = brute
            check_batch(E, blob, ref, pats, bytes(T))
            del _texts[T.tobytes()]
            texts += 1
    assert texts == sum(2 ** n for n in range(1, 8))


# ---- 2. geometry: intervals at the '$' row and at the block edges ----------------------------------------------------------------

def geometry_patterns(T, SA, primary, longest=64, long_ones=2):
    """The patterns of test_emul_geometry.edge_patterns -- their intervals start or end at row primary, primary + 1 and beside
    every block edge -- (those above `longest` bytes: the first `long_ones` only), T itself, T + one byte, one byte, the empty one."""
    pats, _, _ = edge_patterns(T, SA, primary)
    keep = []
    for p in dict.fromkeys(pats):
        if len(p) <= longest:
            keep.append(p)
        elif long_ones:
            keep.append(p)
            long_ones -= 1
    tb = T.tobytes()
    return keep + [tb, tb + tb[:1], tb[-1:], b""]


def small_edge_sizes():
    return [n for n in R.EDGE_SIZES if n <= 4096]


def geometry_sweep(lib, sizes, primaries=R.edge_primaries, widths=(32, 64), forms=None):
    """Every n x primary x width, through every form (the library itself unless given): the reference is computed once per text."""
    done = 0
    for n in sizes:
        for j in primaries(n):
            T, SA, B, primary = family_case(lib, n, j)
            ref = text_of(T, SA)
            pats = geometry_patterns(T, SA, primary)
            for bits in widths:
                blob = lib.fm_build(B, primary, SA, 32, bits)
                short, long = [p for p in pats if len(p) <= 64], [p for p in pats if len(p) > 64]
                for form in forms or (lib,):
                    check_batch(form, blob, ref, short, (n, j, bits), min_lens=(1,))
                    if long:
                        check_batch(form, blob, ref, long, (n, j, bits, "long"), min_lens=(1,), once=True)
                done += 1
            del _texts[T.tobytes()]
    return done


def test_geometry_small():
    E = emul()
    assert geometry_sweep(E, [n for n in small_edge_sizes() if n < 4000]) >= 150


@pytest.mark.slow
@pytest.mark.parametrize("n", [n for n in R.EDGE_SIZES if 4000 <= n <= 4096])
def test_geometry_4096(n):
    """(T itself and T + one byte are n lanes of up to n steps each, at every primary and width: about 100 s per size in the
    emulation, which runs one lane after the other.)"""
    assert geometry_sweep(emul(), [n]) == 2 * len(R.edge_primaries(n))


# ---- 3. lanes to patterns --------------------------------------------------------------------------------------------------------

def mapping_batch(T, rs, nt=FM_NT):
    """Patterns cut from T (every third with one byte replaced by a non-letter or another letter) whose boundaries, counted from
    the batch's first byte, fall one below, on and one above the multiples of nt, with empty patterns in between."""
    bounds = sorted({k * nt + d for k in (1, 2, 3) for d in (-1, 0, 1)} | {3 * nt + 7})
    lengths, at = [], 0
    for i, b in enumerate(bounds):
        lengths += [b - at] + [0] * (i % 3)
        at = b
    pats = []
    for i, ln in enumerate(lengths):
        a = int(rs.randint(0, T.size - ln + 1))
        p = bytearray(T[a:a + ln].tobytes())
        if ln and i % 3 == 0:
            p[int(rs.randint(0, ln))] = ord("N") if i % 2 else int(T[int(rs.randint(0, T.size))])
        pats.append(bytes(p))
    return pats


def mapping_sweep(lib, n=1500, bases=(0, 5)):
    T = np.random.RandomState(n).choice(DNA, size=n)
    SA = R.naive_sa(T)
    B, primary = R.bwt_of(T, SA)
    ref = text_of(T, SA)
    pats = mapping_batch(T, np.random.RandomState(7))
    assert [len(p) for p in pats].count(0) >= 6
    cat, off = lib._patterns(pats)
    for bits in (32, 64):
        blob = lib.fm_build(B, primary, SA, 32, bits)
        for base in bases:
            packed = (np.concatenate([np.full(base, ord("A"), dtype=np.uint8), cat]), off + np.uint64(base))
            check_batch(lib, blob, ref, pats, ("mapping", bits, base), min_lens=(1, 20), packed=packed)
    return T, SA, B, primary, pats


def test_lane_to_pattern_mapping():
    mapping_sweep(emul())


# ---- 4. the cap ----------------------------------------------------------------------------------------------------------------

def reads_of(T, rs, count, shortest, longest, every=2):
    """Reads cut from T; every `every`-th with one base replaced by another letter of T."""
    out = []
    for i in range(count):
        ln = int(rs.randint(shortest, longest + 1))
        a = int(rs.randint(0, T.size - ln + 1))
        p = T[a:a + ln].copy()
        if i % every == 1:
            k = int(rs.randint(0, ln))
            p[k] = DNA[(int(np.flatnonzero(DNA == p[k])[0]) + 1 + int(rs.randint(0, 3))) % 4]
        out.append(p.tobytes())
    return out


def cap_sweep(lib, n=2000):
    T = np.random.RandomState(n).choice(DNA, size=n)
    SA = R.naive_sa(T)
    B, primary = R.bwt_of(T, SA)
    ref = text_of(T, SA)
    pats = reads_of(T, np.random.RandomState(3), 12, 40, 90) + [b"", b"ACGTNACGT", T[:34].tobytes()]
    blob = lib.fm_build(B, primary, None)
    full = np.concatenate([answers(ref, P)[0] for P in pats])
    for max_len in (1, 2, 31, 32, 33):
        check_batch(lib, blob, ref, pats, ("cap", max_len), max_len=max_len)
        ln, _, _, _ = lib.fm_match(blob, pats, max_len)
        assert np.array_equal(ln, np.minimum(full, np.uint32(max_len))), max_len
    assert int(full.max()) > 33


def test_cap():
    cap_sweep(emul())


# ---- 5. count is the witness -------------------------------------------------------------------------------------------------------

def self_consistency(lib, blob, pats, max_len=0):
    """For every (pattern, end): fm_count of the reported piece gives the reported interval; without a cap, the piece one byte
    longer to the left (when there is one) counts 0."""
    ln, first, count, off = lib.fm_match(blob, pats, max_len, True)
    pieces, longer = [], []
    t = 0
    for P in pats:
        for e in range(1, len(P) + 1):
            l = int(ln[t])
            pieces.append(P[e - l:e])
            if l < e and max_len == 0:
                longer.append(P[e - l - 1:e])
            t += 1
    f, c = lib.fm_count(blob, pieces)
    hit = ln > 0
    assert np.array_equal(f[hit], first[hit]) and np.array_equal(c[hit], count[hit]) and (c[hit] > 0).all()
    assert not first[~hit].any() and not count[~hit].any()
    if longer:
        assert not lib.fm_count(blob, longer)[1].any()
    return t


def test_self_consistency():
    E = emul()
    T, SA, B, primary = family_case(E, 4095, 127)
    rs = np.random.RandomState(11)
    pats = reads_of(T, rs, 30, 20, 70) + geometry_patterns(T, SA, primary)[:40]
    for bits in (32, 64):
        blob = E.fm_build(B, primary, SA, 32, bits)
        assert self_consistency(E, blob, pats) == sum(len(p) for p in pats)
        self_consistency(E, blob, pats, max_len=17)


# ---- 6. output buffers -----------------------------------------------------------------------------------------------------------

def buffer_sweep(lib, mem):
    """The device entry points on 0xA5-filled buffers with guards: see raw_match and raw_mems for what must stay untouched."""
    T = np.random.RandomState(21).choice(DNA, size=1200)
    SA = R.naive_sa(T)
    B, primary = R.bwt_of(T, SA)
    ref = text_of(T, SA)
    pats = reads_of(T, np.random.RandomState(5), 9, 1, 70) + [b"", b"N"]
    cat, off = lib._patterns(pats)
    want = [np.concatenate([answers(ref, P)[k] for P in pats]) for k in range(3)]
    for bits in (32, 64):
        blob = lib.fm_build(B, primary, SA, 32, bits)
        ln, first, count = raw_match(lib, mem, blob, cat, off, 0, True)
        assert np.array_equal(ln, want[0]) and np.array_equal(first, want[1]) and np.array_equal(count, want[2])
        ln, _, _ = raw_match(lib, mem, blob, cat, off, 0, False)
        assert np.array_equal(ln, want[0])
        exp, eoff = M.records([mems_of(ref, P, 1) for P in pats])
        for ws in (True, False):
            rec, moff = raw_mems(lib, mem, blob, cat, off, 1, ws)
            assert rec.tobytes() == exp.tobytes() and np.array_equal(moff, eoff)


def test_output_buffers():
    buffer_sweep(emul(), HostMem())


# ---- 7. MEMs: the counting call, the capacity, min_len ---------------------------------------------------------------------------

def _err(E):
    return E._f("last_error")().decode()


def mems_sweep(lib, mem):
    T = np.random.RandomState(31).choice(DNA, size=1800)
    SA = R.naive_sa(T)
    B, primary = R.bwt_of(T, SA)
    ref = text_of(T, SA)
    pats = reads_of(T, np.random.RandomState(6), 10, 30, 80) + [b"", b"NN", T[100:101].tobytes()]
    cat, off = lib._patterns(pats)
    q = len(pats)
    for bits in (32, 64):
        blob = lib.fm_build(B, primary, None, 0, bits)
        check_batch(DeviceForm(lib, mem), blob, ref, pats, ("mems, device form", bits), min_lens=(1, 2, 12))
        check_batch(lib, blob, ref, pats, ("mems, host form", bits), min_lens=(1, 12))
        exp, eoff = M.records([mems_of(ref, P, 1) for P in pats])
        found = int(eoff[-1])
        assert found >= 10
        # the counting call of the host form
        moff = np.full(q + 1, 7, dtype=np.uint64)
        assert lib._f("fm_mems")(blob.ctypes.data, blob.size, cat.ctypes.data, off.ctypes.data, q, 1, moff.ctypes.data, None, 0, 0) == 0
        assert np.array_equal(moff, eoff)
        # capacity one below the total: EINVAL, mem_off intact, the records untouched -- both forms
        rec = np.full(32 * found + GUARD, FILL, dtype=np.uint8)
        moff[:] = 7
        rc = lib._f("fm_mems")(blob.ctypes.data, blob.size, cat.ctypes.data, off.ctypes.data, q, 1, moff.ctypes.data, rec.ctypes.data, found - 1, 0)
        assert rc == EINVAL and "mem_capacity" in _err(lib), _err(lib)
        assert np.array_equal(moff, eoff) and (rec == FILL).all()
        d_index, d_cat, d_off = mem.put(blob), mem.put(cat), mem.put(off)
        d_moff, d_rec = mem.filled(8 * (q + 1)), mem.filled(32 * found)
        rc = lib._f("fm_mems_device")(mem.ptr(d_index), blob.size, mem.ptr(d_cat), mem.ptr(d_off), q, 1, mem.ptr(d_moff), mem.ptr(d_rec), found - 1,
                                      None, 0, None)
        assert rc == EINVAL and "mem_capacity" in _err(lib), _err(lib)
        assert np.array_equal(mem.get(d_moff)[:8 * (q + 1)].view(np.uint64), eoff) and (mem.get(d_rec) == FILL).all()
        # the exact capacity and a larger one
        for cap in (found, found + 5):
            rec[:] = FILL
            assert lib._f("fm_mems")(blob.ctypes.data, blob.size, cat.ctypes.data, off.ctypes.data, q, 1, moff.ctypes.data, rec.ctypes.data, cap, 0) == 0
            assert rec[:32 * found].tobytes() == exp.tobytes() and (rec[32 * found:] == FILL).all()
        # min_len above every length: no MEM; min_len 0 is 1
        top = max(len(p) for p in pats) + 1
        for form in (lib, DeviceForm(lib, mem)):
            none, noff = form.fm_mems(blob, pats, top)
            assert none.size == 0 and not noff.any() and noff.size == q + 1
            zero, zoff = form.fm_mems(blob, pats, 0)
            assert zero.tobytes() == exp.tobytes() and np.array_equal(zoff, eoff)


def test_mems():
    mems_sweep(emul(), HostMem())


def columns_sweep(lib, lanes):
    """A batch of more than `lanes` pattern bytes: the flags are scanned in more than one column (capi_impl.h FM_MEM_COL_MIN)."""
    T = np.random.RandomState(41).choice(DNA, size=2500)
    SA = R.naive_sa(T)
    B, primary = R.bwt_of(T, SA)
    ref = text_of(T, SA)
    pats = reads_of(T, np.random.RandomState(8), lanes // 80 + 2, 80, 100, every=3) + [b""]
    assert sum(len(p) for p in pats) > lanes
    check_batch(lib, lib.fm_build(B, primary, None), ref, pats, "columns", min_lens=(12,))
    del _texts[T.tobytes()]


def test_mems_across_scan_columns():
    src = open(os.path.join(ROOT, "caps-sa_amd", "csrc", "capi_impl.h")).read()
    col = re.search(r"FM_MEM_COL_MIN = 1u << (\d+)", src)
    columns_sweep(emul(), 2 * (1 << int(col.group(1))) + 100)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals():
    E = emul()
    T, SA, B, primary = family_case(E, 1000, 0)
    cat, off = E._patterns([T[:20].tobytes(), T[500:530].tobytes(), b"", T[990:].tobytes()])
    total, q = int(off[-1]), 4
    for bits in (32, 64):
        blob = E.fm_build(B, primary, SA, 32, bits)
        ln = np.full(4 * total + GUARD, FILL, dtype=np.uint8)
        moff = np.full(8 * (q + 1) + GUARD, FILL, dtype=np.uint8)
        rec = np.full(32 * total + GUARD, FILL, dtype=np.uint8)

        def both(index, code, word, nbytes=None, c=cat, o=off, out=True):
            nbytes = index.size if nbytes is None else nbytes
            cp, op = (c.ctypes.data if c is not None else None), (o.ctypes.data if o is not None else None)
            lp, mp = (ln.ctypes.data if out else None), (moff.ctypes.data if out else None)
            for rc in (E._f("fm_match")(index.ctypes.data, nbytes, cp, op, q, 0, lp, None, None, 0),
                       E._f("fm_match_device")(index.ctypes.data, nbytes, cp, op, q, 0, lp, None, None, None),
                       E._f("fm_mems")(index.ctypes.data, nbytes, cp, op, q, 1, mp, rec.ctypes.data, total, 0),
                       E._f("fm_mems_device")(index.ctypes.data, nbytes, cp, op, q, 1, mp, rec.ctypes.data, total, None, 0, None)):
                assert rc == code and word in _err(E), (bits, word, rc, _err(E))
            assert (ln == FILL).all() and (moff == FILL).all() and (rec == FILL).all(), word

        bad_off = off.copy()
        bad_off[2] = off[1] - np.uint64(1)
        both(blob, EINVAL, "not monotone", o=bad_off)
        both(blob, EINVAL, "null pointer", o=None)
        both(blob, EINVAL, "null pointer", c=None)
        both(blob, EINVAL, "null pointer", out=False)
        both(blob, EINVAL, "truncated", nbytes=blob.size - 1)
        both(blob, EINVAL, "smaller than an FM-index header", nbytes=255)
        for word, value in ((0, 1), (1, 9), (4, 5), (7, 2), (14, int(blob[:256].view(np.uint64)[14]) + 1)):
            bad = blob.copy()
            bad[:256].view(np.uint64)[word] = value
            both(bad, EINVAL, "")
        assert E._f("fm_match_device")(None, blob.size, cat.ctypes.data, off.ctypes.data, q, 0, ln.ctypes.data, None, None, None) == EINVAL
        assert E._f("fm_mems_device")(blob.ctypes.data, blob.size, cat.ctypes.data, off.ctypes.data, q, 1, moff.ctypes.data, rec.ctypes.data + 4, total,
                                      None, 0, None) == EINVAL and "aligned" in _err(E)
        ws = np.zeros(E.fm_mems_workspace_bytes(total, q), dtype=np.uint8)
        assert E._f("fm_mems_device")(blob.ctypes.data, blob.size, cat.ctypes.data, off.ctypes.data, q, 1, moff.ctypes.data, None, 0, ws.ctypes.data, 64,
                                      None) == EINVAL and "workspace too small" in _err(E)
        moff[:] = FILL
        # a pattern above 2^32 - 1 bytes is refused from its offsets alone (no byte of it is read)
        long_off = np.array([0, 2**32], dtype=np.uint64)
        assert E._f("fm_match")(blob.ctypes.data, blob.size, cat.ctypes.data, long_off.ctypes.data, 1, 0, ln.ctypes.data, None, None, 0) == EINVAL
        assert "2^32 - 1" in _err(E)
        assert E._f("fm_match_device")(blob.ctypes.data, blob.size, cat.ctypes.data, long_off.ctypes.data, 1, 0, ln.ctypes.data, None, None, None) == EINVAL
        assert "2^32 - 1" in _err(E)
        assert E._f("fm_mems_device")(blob.ctypes.data, blob.size, cat.ctypes.data, long_off.ctypes.data, 1, 1, moff.ctypes.data, None, 0, None, 0,
                                      None) == EINVAL and "2^32 - 1" in _err(E)
        assert (ln == FILL).all() and (moff == FILL).all()
        # ... and the valid call on the same buffers
        assert E._f("fm_match")(blob.ctypes.data, blob.size, cat.ctypes.data, off.ctypes.data, q, 0, ln.ctypes.data, None, None, 0) == 0
        assert ln[:4 * total].view(np.uint32).tolist() == list(range(1, 21)) + list(range(1, 31)) + list(range(1, 11))
    out = ctypes.c_uint64(0)
    assert E._f("fm_mems_workspace_bytes")(10, 1, None) == EINVAL and E._f("fm_mems_workspace_bytes")(2**60, 1, ctypes.byref(out)) == EINVAL
    assert E._f("fm_mems_workspace_bytes")(2**20, 2**10, ctypes.byref(out)) == 0 and out.value <= 28 * 2**20 + 24 * 1024


# ---- 9. degenerate inputs ----------------------------------------------------------------------------------------------------------

def test_empty_text_and_empty_batch():
    import caps_sa_amd
    E = emul()
    empty = np.zeros(0, dtype=np.uint8)
    for bits in (32, 64):
        blob = E.fm_build(empty, 0, None, 0, bits)
        ln, first, count, off = E.fm_match(blob, [b"ACGT", b"", b"A"], 0, True)
        assert ln.tolist() == [0] * 5 and not first.any() and not count.any()
        rec, moff = E.fm_mems(blob, [b"ACGT", b"", b"A"])
        assert rec.size == 0 and moff.tolist() == [0, 0, 0, 0]
        D = DeviceForm(E, HostMem())
        assert D.fm_match(blob, [b"ACGT", b"", b"A"], 0, True)[0].tolist() == [0] * 5
        assert D.fm_mems(blob, [b"ACGT", b"", b"A"])[1].tolist() == [0, 0, 0, 0]
    T, SA, B, primary = family_case(E, 1000, 0)
    blob = E.fm_build(B, primary, None)                                   # (no samples: neither call needs them)
    assert int(blob[:256].view(np.uint64)[12]) == 0
    # q = 0
    ln, first, count, off = E.fm_match(blob, [], 0, True)
    assert ln.size == 0 and off.tolist() == [0]
    rec, moff = E.fm_mems(blob, [])
    assert rec.size == 0 and moff.tolist() == [0]
    one = np.full(1, 7, dtype=np.uint64)
    assert E._f("fm_mems_device")(blob.ctypes.data, blob.size, None, None, 0, 1, one.ctypes.data, None, 0, None, 0, None) == 0 and one[0] == 0
    assert E._f("fm_match_device")(blob.ctypes.data, blob.size, None, None, 0, 0, None, None, None, None) == 0
    assert E._f("fm_match")(blob.ctypes.data, blob.size, None, None, 0, 0, None, None, None, 0) == 0
    # a batch of empty patterns
    ln, _, _, off = E.fm_match(blob, [b"", b""])
    assert ln.size == 0 and E.fm_mems(blob, [b"", b""])[1].tolist() == [0, 0, 0]
    # the Python surface on the count-only index
    fm = caps_sa_amd.FMIndex(blob, _lib=E)
    tb = T.tobytes()
    P = tb[10:40] + b"N" + tb[700:720]
    L = fm.matching_statistics([P, b""])
    assert len(L) == 2 and L[0].dtype == np.uint32 and L[0].tolist() == list(range(1, 31)) + [0] + list(range(1, 21)) and L[1].size == 0
    L2, first, count = fm.matching_statistics([P], intervals=True)
    assert np.array_equal(L2[0], L[0]) and int(count[0][29]) >= 1 and int(count[0][30]) == 0
    ms = fm.mems([P, b"", tb[:5]], min_len=5)
    assert [m.dtype.names for m in ms] == [("start", "length", "first", "count")] * 3
    assert ms[0]["start"].tolist() == [0, 31] and ms[0]["length"].tolist() == [30, 20] and ms[1].size == 0 and ms[2]["length"].tolist() == [5]
    assert fm.matching_statistics([P], max_len=7)[0].max() == 7


# ---- 10. corrupted body: a child process, the emulation only ------------------------------------------------------------------------

_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [%(tests)r, %(root)r]
import caps_sa_amd
import fm_reference as R
E = caps_sa_amd.CapsLib(%(so)r, "caps_sa_emul_")
n = 5000
T = np.random.RandomState(5).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
SA = R.naive_sa(T)
B, primary = R.bwt_of(T, SA)
rs = np.random.RandomState(77)
pats = [T[a:a + ln].tobytes() for a, ln in ((0, 300), (63, 64), (2000, 700), (4990, 10), (100, 1), (0, 0))] + [b"ACGTN" * 20]
for bits in (32, 64):
    for s in (0, 32):
        good = E.fm_build(B, primary, SA if s else None, s, bits)
        for trial in range(6):
            bad = good.copy()
            at = rs.randint(256, bad.size, size=1000)
            bad[at] ^= rs.randint(1, 256, size=1000).astype(np.uint8)
            ln, first, count, off = E.fm_match(bad, pats, 0, True)
            assert ln.size == int(off[-1]) and int(ln.max()) <= 700
            E.fm_match(bad, pats, 33, False)
            rec, moff = E.fm_mems(bad, pats, 1)
            assert rec.size == int(moff[-1]) <= ln.size
print("done")
"""


def test_corrupted_body_terminates():
    """1,000 flipped body bytes of a valid blob, 24 blobs: both calls read inside the blob, end after at most one step per pattern
    byte and lane, and return.  In a child process, so that a read outside the blob ends the child and not the suite.  Never on a
    GPU."""
    emul()
    code = _CHILD % {"tests": os.path.join(ROOT, "tests"), "root": ROOT, "so": os.path.join(EMUL_DIR, "libcaps_sa_emul.so")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("done"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- 11. the other emulation builds -------------------------------------------------------------------------------------------------

def test_other_builds_give_the_same_answers():
    """The lane-to-pattern sweep and a few geometry sizes once more with the threads of every phase in descending order and with
    64-thread workgroups."""
    for E in (emul_rev(False), emul_small()):
        mapping_sweep(E)
        assert geometry_sweep(E, [127, 129, 255], primaries=lambda n: sorted({0, n // 2, n - 1})) == 3 * 3 * 2
