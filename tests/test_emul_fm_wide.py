"""CPU: the wide FM-index (include/caps_sa_hip.h "FM-index: the wide format") through the host emulation of the kernels.

Every check is exact.  Blobs are compared byte for byte with fm_wide_reference.encode (numpy, written from the header's format
table); a blob does not ask its (BWT, primary, SA) to belong to a text, so those sweeps use random bytes, any primary and a random
permutation.  Answers are compared with the naive suffix array (count, locate) and with fm_match_reference (matching statistics,
MEMs), and on 4-letter texts with the narrow index."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import fm_match_reference as M
import fm_wide_reference as W
from emul_util import EMUL_DIR, ROOT, emul, emul_rev, emul_small

EINVAL, EUNSUPPORTED, EALPHABET = -1, -2, -6
FILL, GUARD = 0xA5, 64
SIZES = (0, 1, 2, 127, 128, 129, 255, 256, 257, 16383, 16384, 16385, 32769)
SIGMAS = (1, 2, 4, 5, 16, 17, 64, 65, 256)
COMBOS = [(bits, s) for bits in (32, 64) for s in (0, 1, 32, 1024)]          # s = 0: without an SA


def _caps():
    import caps_sa_amd
    return caps_sa_amd


def _fmw(E, B, primary, SA=None, s=32, bits=None):
    return _caps().FMIndex.from_bwt(B, primary, SA, s, bits, _lib=E, wide=True)


def blob_case(E, n, sigma, primary, bits, s, seed=0):
    """One build against the encoder.  Returns the blob."""
    rs = np.random.RandomState(seed + 7 * n + sigma)
    B = W.text_with_sigma(n, sigma, seed) if n else np.zeros(0, dtype=np.uint8)
    SA = rs.permutation(n) if s else None
    blob = E.fm_build_wide(B, primary, SA, s or 32, bits)
    ref = W.encode(B, primary, SA, s, bits // 8)
    assert blob.size == ref.size == E.fm_wide_index_bytes(n, sigma, s, bits), (n, sigma, primary, bits, s)
    if not np.array_equal(blob, ref):
        at = np.flatnonzero(blob != ref)
        raise AssertionError((n, sigma, primary, bits, s, "first differing bytes", at[:8].tolist()))
    return blob


def blob_sweep(E, sizes=SIZES, sigmas=SIGMAS, all_primaries_up_to=257, every_pair=True):
    """n x sigma (n >= sigma): at the edge primaries every (width, sample distance) pair; for n <= 257 every other primary too,
    the pairs taken in turn.  Bytes >= 0x80 are among the letters from sigma = 2 on (fm_wide_reference.text_with_sigma)."""
    done = 0
    for n in sizes:
        for sigma in sigmas:
            if n == 0:
                if sigma == 1:
                    for bits, s in COMBOS:
                        blob_case(E, 0, 1, 0, bits, s)
                        done += 1
                continue
            if n < sigma:
                continue
            edges = W.edge_primaries(n)
            for k, primary in enumerate(edges):
                for bits, s in (COMBOS if every_pair else [COMBOS[(k + sigma + n) % len(COMBOS)]]):
                    blob_case(E, n, sigma, primary, bits, s)
                    done += 1
            if n <= all_primaries_up_to:
                for k, primary in enumerate(p for p in range(n) if p not in edges):
                    bits, s = COMBOS[(k + sigma) % len(COMBOS)]
                    blob_case(E, n, sigma, primary, bits, s)
                    done += 1
    return done


def test_blobs_small_sizes_quick():
    """n <= 257 at the edge primaries, the (width, sample distance) pairs taken in turn: the default run's share of the sweep below."""
    assert blob_sweep(emul(), [n for n in SIZES if n <= 257], all_primaries_up_to=2, every_pair=False) > 300


@pytest.mark.slow
def test_blobs_small_sizes():
    """Every primary of every n <= 257 (about 11,500 builds, 2 to 3 minutes)."""
    assert blob_sweep(emul(), [n for n in SIZES if n <= 257]) > 5000


@pytest.mark.slow
def test_blobs_tile_sizes():
    """16,383 .. 32,769 rows: one, two and three tiles, a scatter that crosses tiles on up to three levels."""
    assert blob_sweep(emul(), [n for n in SIZES if n > 257]) > 1000


def test_blobs_tile_sizes_quick():
    """The same sizes at one primary and one pair per alphabet, for the default run."""
    E = emul()
    for k, (n, sigma) in enumerate(itertools.product([n for n in SIZES if n > 257], SIGMAS)):
        bits, s = COMBOS[k % len(COMBOS)]
        blob_case(E, n, sigma, W.edge_primaries(n)[k % 5], bits, s)


def test_index_bytes_and_sigma_at_most_4_is_the_narrow_section():
    E = emul()
    assert E.fm_wide_index_bytes(1000, 0, 32, 32) == E.fm_wide_index_bytes(1000, 256, 32, 32) > E.fm_wide_index_bytes(1000, 64, 32, 32)
    n = 1 << 20
    per_base = [(E.fm_wide_index_bytes(n, sg, 32, 32) - 5056) / n for sg in (5, 17, 65)]
    assert all(abs(b - (0.5 * lv + 0.16)) < 0.01 for b, lv in zip(per_base, (2, 3, 4))), per_base
    rs = np.random.RandomState(2)
    for n, bits, s in ((1, 32, 1), (300, 32, 32), (300, 64, 0), (16385, 64, 32), (20000, 32, 0)):
        B = rs.choice(np.array([0x80, 0xFE, 0x05, 0x7F], dtype=np.uint8), size=n)
        SA = rs.permutation(n) if s else None
        primary = n // 3
        wide, narrow = E.fm_build_wide(B, primary, SA, s or 32, bits), E.fm_build(B, primary, SA, s or 32, bits)
        hw, hn = wide[:256].view(np.uint64), narrow[:256].view(np.uint64)
        assert int(hw[6]) == 1 and int(hw[15]) == 5056
        assert np.array_equal(wide[5056:], narrow[256:]), (n, bits, s)              # level 0 | mark ranks | samples
        assert [int(hw[k]) for k in (2, 3, 4, 12, 13, 14)] == [int(hn[k]) for k in (2, 3, 4, 12, 13, 14)]


# ---- answers -----------------------------------------------------------------------------------------------------------------------

def check_all(fm, T, SA, pats, R=None, min_len=1):
    """count and locate against the SA, matching statistics and MEMs against fm_match_reference, for every pattern."""
    n, tb = T.size, T.tobytes()
    R = R or M.Text(T, SA)
    first, count = fm.count(pats)
    hits = fm.locate(pats) if fm.sa_sample else None
    for j, P in enumerate(pats):
        f, c = int(first[j]), int(count[j])
        want = R.interval(bytes(P)) if len(P) else (0, n)
        assert (f, c) == want, (tb[:40], bytes(P)[:40], f, c, want)
        if hits is not None:
            assert hits[j].dtype == np.uint64 and np.array_equal(hits[j], SA[f:f + c].astype(np.uint64)), (tb[:40], bytes(P)[:40])
    L, F, C = fm.matching_statistics(pats, intervals=True)
    mems = fm.mems(pats, min_len)
    for j, P in enumerate(pats):
        rl = R.lengths(P)
        rf, rc = R.intervals(P, rl)
        assert np.array_equal(L[j], rl) and np.array_equal(F[j], rf) and np.array_equal(C[j], rc), (tb[:40], bytes(P)[:40])
        want = R.mems(P, min_len, rl)
        got = [tuple(int(x) for x in r) for r in mems[j]]
        assert got == want, (tb[:40], bytes(P)[:40], got, want)
    return first, count


def exhaustive(E, lengths):
    letters, foreign = bytes([0x80, 0xFE, 0x05, 0x41, 0x7F]), b"N"                  # ascending in signed-char order
    pats = [bytes(p) for m in range(4) for p in itertools.product(letters + foreign, repeat=m)]
    done = 0
    for n in lengths:
        for t in itertools.product(letters, repeat=n):
            T = np.array(t, dtype=np.uint8)
            SA = W.naive_sa(T)
            B, primary = W.bwt_of(T, SA)
            fm = _fmw(E, B, primary, SA, 2 if n % 2 else 1, 32 if done % 2 else 64)
            assert fm.sigma == len(set(t))
            check_all(fm, T, SA, pats)
            done += 1
    return done


def test_exhaustive_short_texts():
    """Every text of length 1 .. 4 over 5 letters, every pattern of length 0 .. 3 over those letters and one byte that is none."""
    assert exhaustive(emul(), range(1, 5)) == 5 + 25 + 125 + 625


@pytest.mark.slow
def test_exhaustive_short_texts_5_and_6():
    assert exhaustive(emul(), (5, 6)) == 5 ** 5 + 5 ** 6


def make_patterns(T, rs, foreign, k=40):
    """(The whole text as a pattern only for short texts: matching statistics walk from every end, quadratic in the emulation.)"""
    n = T.size
    whole = T[:min(n, 1200)].tobytes() if n > 1200 else T.tobytes()
    pats = [b"", whole, whole + T[:1].tobytes(), bytes([foreign]), T[n - min(n, 7):].tobytes()]
    for _ in range(k):
        m = int(rs.choice([1, 2, 3, 8, 31, 32, 33, 100]))
        if m > n:
            continue
        a = int(rs.randint(0, n - m + 1))
        P = T[a:a + m].copy()
        pats.append(P.tobytes())
        Q = P.copy()
        Q[int(rs.randint(0, m))] = T[int(rs.randint(0, n))]
        pats.append(Q.tobytes())
        Q = P.copy()
        Q[int(rs.randint(0, m))] = foreign
        pats.append(Q.tobytes())
    return list(dict.fromkeys(pats))


@pytest.mark.parametrize("sigma", [5, 16, 17, 65, 255])
def test_random_texts(sigma):
    """Texts of about a thousand bytes at every number of levels, both widths, three sample distances."""
    E = emul()
    rs = np.random.RandomState(sigma)
    T = W.text_with_sigma(900 + sigma, sigma, 3)
    foreign = next(b for b in range(255, -1, -1) if b not in set(T.tolist()))
    SA = W.naive_sa(T)
    B, primary = W.bwt_of(T, SA)
    R = M.Text(T, SA)
    pats = make_patterns(T, rs, foreign)
    ref = None
    for bits, s in ((32, 1), (64, 32), (32, 1024), (64, 0)):
        fm = _fmw(E, B, primary, SA if s else None, s or 32, bits)
        assert (fm.wide, fm.sigma, fm.n, fm.sa_sample) == (True, sigma, T.size, s)
        got = check_all(fm, T, SA, pats, R, min_len=2)
        ref = ref or got
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    with pytest.raises(_caps().CapsSaError) as e:
        fm.locate(pats)                                                              # (the last one: no samples)
    assert e.value.code == EUNSUPPORTED


def test_four_letter_differential():
    """On 4-letter texts the wide blob (one level) answers what the narrow blob answers, and its level 0 is the narrow Occ section."""
    E = emul()
    rs = np.random.RandomState(11)
    for n, letters in ((1, b"A"), (700, b"AC"), (5000, b"ACGT"), (20001, bytes([0x80, 0xFE, 0x05, 0x7F]))):
        T = rs.choice(np.frombuffer(letters, dtype=np.uint8), size=n)
        SA, _, B, primary, _ = E.build_bwt(T)
        pats = make_patterns(T, rs, ord("N"))
        for bits in (32, 64):
            wide = _fmw(E, B, primary, SA, 32, bits)
            narrow = _caps().FMIndex.from_bwt(B, primary, SA, 32, bits, _lib=E)
            nb = narrow.blob.size
            assert np.array_equal(wide.blob[5056:5056 + nb - 256], narrow.blob[256:])
            for a, b in zip(wide.count(pats), narrow.count(pats)):
                assert np.array_equal(a, b)
            for a, b in zip(wide.locate(pats, 50), narrow.locate(pats, 50)):
                assert np.array_equal(a, b)
            for a, b in zip(wide.matching_statistics(pats, 40, True), narrow.matching_statistics(pats, 40, True)):
                assert all(np.array_equal(x, y) for x, y in zip(a, b))
            for a, b in zip(wide.mems(pats, 3), narrow.mems(pats, 3)):
                assert np.array_equal(a, b)


def test_lane_and_tile_mapping():
    """2 * 16,384 + 1 rows over 17 letters (three levels, every scatter crosses tiles), and a batch of 3 * 256 + 5 patterns, so
    that patterns and (pattern, end) pairs straddle workgroup boundaries: each answer is its own pattern's."""
    E = emul()
    n = 2 * 16384
    T = W.text_with_sigma(n, 17, 9)
    SA, _, B, primary, _ = E.build_bwt(T)
    assert np.array_equal(W.bwt_of(T, SA)[0], B)
    fm = _fmw(E, B, primary, SA, 32, 32)
    assert np.array_equal(fm.blob, W.encode(B, primary, SA, 32, 4))
    rs = np.random.RandomState(4)
    q = 3 * 256 + 5
    starts, lens = rs.randint(0, n - 40, size=q), rs.randint(1, 40, size=q)
    pats = [T[a:a + m].tobytes() for a, m in zip(starts, lens)]
    first, count = fm.count(pats)
    rank = np.empty(n, dtype=np.int64)
    rank[SA.astype(np.int64)] = np.arange(n)
    tb = T.tobytes()
    for j, P in enumerate(pats):
        f, c, m = int(first[j]), int(count[j]), len(P)
        assert c >= 1 and f <= rank[starts[j]] < f + c
        assert tb[int(SA[f]):int(SA[f]) + m] == P == tb[int(SA[f + c - 1]):int(SA[f + c - 1]) + m]
        assert f == 0 or tb[int(SA[f - 1]):int(SA[f - 1]) + m] != P
        assert f + c == n or tb[int(SA[f + c]):int(SA[f + c]) + m] != P
    for h, f, c in zip(fm.locate(pats, 3), first.tolist(), count.tolist()):
        assert np.array_equal(h, SA[f:f + min(c, 3)].astype(np.uint64))
    L = fm.matching_statistics(pats)
    for j in range(0, q, 97):
        assert L[j][-1] == lens[j] and (L[j] == np.arange(1, lens[j] + 1)).all()       # (every prefix of a piece of T occurs)


# ---- the device entry points on guarded buffers --------------------------------------------------------------------------------------

def _guarded(nbytes, odd=1, elem=8):
    """A buffer of nbytes inside a 0xA5-filled array, an ODD number of elements behind an 8-byte boundary: (whole array, view)."""
    whole = np.full(nbytes + 2 * GUARD + 64, FILL, dtype=np.uint8)
    o = (-whole.ctypes.data) % 8 + GUARD + odd * elem
    return whole, whole[o:o + nbytes]


def _untouched(whole, view):
    lo = view.ctypes.data - whole.ctypes.data
    return (whole[:lo] == FILL).all() and (whole[lo + view.size:] == FILL).all()


def test_device_entry_points_write_nothing_outside():
    """Build with a caller's workspace, count, locate and match on 0xA5-filled buffers: index and workspace 64-byte aligned as the
    header asks, every output array at an odd byte offset; nothing outside them is written."""
    E = emul()
    n, sigma = 16385, 17
    T = W.text_with_sigma(n, sigma, 5)
    SA, _, B, primary, _ = E.build_bwt(T)
    for bits in (32, 64):
        SAw = np.ascontiguousarray(SA, dtype=np.uint32 if bits == 32 else np.uint64)
        cap = E.fm_wide_index_bytes(n, 0, 32, bits)
        need = E.fm_wide_index_bytes(n, sigma, 32, bits)
        whole_i = np.full(cap + 3 * GUARD, FILL, dtype=np.uint8)
        o = (-whole_i.ctypes.data) % 64 + GUARD
        idx = whole_i[o:o + cap]
        ws_bytes = E.fm_wide_workspace_bytes(n, bits)
        whole_w, ws = _guarded(ws_bytes, 3, 1)
        E.fm_build_wide_device(B.ctypes.data, n, primary, SAw.ctypes.data, 32, idx.ctypes.data, cap, ws.ctypes.data, ws_bytes, bits)
        assert _untouched(whole_w, ws) and _untouched(whole_i, idx)
        assert int(idx[:256].view(np.uint64)[18]) == need and (idx[need:] == FILL).all()
        assert np.array_equal(idx[:need], W.encode(B, primary, SA, 32, bits // 8))
        # without a workspace: the same bytes
        idx2 = np.zeros(need, dtype=np.uint8)
        E.fm_build_wide_device(B.ctypes.data, n, primary, SAw.ctypes.data, 32, idx2.ctypes.data, need, 0, 0, bits)
        assert np.array_equal(idx2, idx[:need])
        blob = idx[:need].copy()
        rs = np.random.RandomState(bits)
        pats = make_patterns(T, rs, 0x7E, 20)
        cat, off = E._patterns(pats)
        q = len(pats)
        wf, first = _guarded(8 * q, 1)
        wc, count = _guarded(8 * q, 3)
        E.fm_count_device(blob.ctypes.data, blob.size, cat.ctypes.data, off.ctypes.data, q, first.ctypes.data, count.ctypes.data)
        assert _untouched(wf, first) and _untouched(wc, count)
        f, c = first.copy().view(np.uint64), count.copy().view(np.uint64)
        rf, rc = E.fm_count(blob, pats)
        assert np.array_equal(f, rf) and np.array_equal(c, rc)
        take = np.minimum(c, 5)
        ooff = np.concatenate([[0], np.cumsum(take)]).astype(np.uint64)
        wp, pos = _guarded(8 * int(ooff[-1]), 5)
        E.fm_locate_device(blob.ctypes.data, blob.size, f.ctypes.data, c.ctypes.data, ooff.ctypes.data, q, pos.ctypes.data)
        assert _untouched(wp, pos)
        pos = pos.copy().view(np.uint64)
        for j in range(q):
            assert np.array_equal(pos[int(ooff[j]):int(ooff[j + 1])], SA[int(f[j]):int(f[j]) + int(take[j])].astype(np.uint64))
        total = int(off[-1])
        wl, ln = _guarded(4 * total, 1, 4)
        E.fm_match_device(blob.ctypes.data, blob.size, cat.ctypes.data, off.ctypes.data, q, 0, ln.ctypes.data, 0, 0)
        assert _untouched(wl, ln)
        assert np.array_equal(ln.copy().view(np.uint32), E.fm_match(blob, pats)[0])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def _rc(E, name, *args):
    rc = E._f(name)(*args)
    return rc, E._f("last_error")().decode(errors="replace")


def test_build_refusals_and_n_0():
    E = emul()
    rs = np.random.RandomState(1)
    n = 1000
    T = W.text_with_sigma(n, 5, 1)
    SA, _, B, primary, _ = E.build_bwt(T)
    SA32 = np.ascontiguousarray(SA, dtype=np.uint32)
    need = E.fm_wide_index_bytes(n, 5, 32, 32)
    blob = np.zeros(need, dtype=np.uint8)
    ws_bytes = E.fm_wide_workspace_bytes(n, 32)
    ws = np.zeros(ws_bytes, dtype=np.uint8)
    good = dict(b=B.ctypes.data, n=n, primary=primary, sa=SA32.ctypes.data, s=32, idx=blob.ctypes.data, cap=need, ws=ws.ctypes.data, wsb=ws_bytes)

    def dev(sfx="u32", **kw):
        a = dict(good, **kw)
        return _rc(E, f"fm_build_wide_device_{sfx}", a["b"], a["n"], a["primary"], a["sa"], a["s"], a["idx"], a["cap"], a["ws"], a["wsb"], None)

    def host(sfx="u32", **kw):
        a = dict(good, **kw)
        return _rc(E, f"fm_build_wide_{sfx}", a["b"], a["n"], a["primary"], a["sa"], a["s"], a["idx"], a["cap"], 0)

    for call in (dev, host):
        assert call()[0] == 0
        assert np.array_equal(blob, W.encode(B, primary, SA, 32, 4))
        blob[:] = 0
        for kw, word in ((dict(b=None), "null"), (dict(idx=None), "null"), (dict(primary=n), "primary"), (dict(primary=2 ** 40), "primary"),
                         (dict(n=2 ** 32), "32-bit"), (dict(s=3), "sa_sample"), (dict(s=2048), "sa_sample"), (dict(cap=need - 1), "too small"),
                         (dict(cap=100), "too small")):
            rc, msg = call(**kw)
            assert rc == EINVAL and word in msg, (call.__name__, kw, rc, msg)
            assert not blob.any()                                                      # nothing written
        blob[:] = 0
    rc, msg = dev(wsb=ws_bytes - 1)
    assert rc == EINVAL and "workspace" in msg and not blob.any()
    # an SA that is no permutation: too many multiples of sa_sample
    bad = SA32.copy()
    bad[bad % 32 == 1] = 0
    rc, msg = dev(sa=bad.ctypes.data)
    assert rc == EINVAL and "multiples of sa_sample" in msg
    # the size calls
    for args in ((10, 257, 32, 32), (10, 5, 3, 32), (2 ** 32, 5, 32, 32)):
        with pytest.raises(_caps().CapsSaError) as e:
            E.fm_wide_index_bytes(*args)
        assert e.value.code == EINVAL
    with pytest.raises(_caps().CapsSaError):
        E.fm_wide_workspace_bytes(2 ** 32, 32)
    # the narrow build still refuses five letters, and now names the wide build
    rc, msg = _rc(E, "fm_build_u32", B.ctypes.data, n, primary, SA32.ctypes.data, 32, blob.ctypes.data, blob.size, 0)
    assert rc == EALPHABET and "fm_build_wide" in msg
    # n = 0 builds and counts 0
    for bits in (32, 64):
        fm = _fmw(E, np.zeros(0, dtype=np.uint8), 0, None, 32, bits)
        assert (fm.n, fm.sigma, fm.wide) == (0, 0, True)
        first, count = fm.count([b"", b"A", b"\x00\xff"])
        assert not first.any() and not count.any()
        assert all(x.size == 0 for x in fm.locate([b""])) and [m.size for m in fm.mems([b"AB"])] == [0]
        assert [x.tolist() for x in fm.matching_statistics([b"AB"])] == [[0, 0]]
    with pytest.raises(_caps().CapsSaError) as e:
        _caps().FMIndex.from_bwt_only(B, primary, 32, _lib=E, wide=True)
    assert e.value.code == EUNSUPPORTED
    del rs


def _set64(blob, byte_off, value):
    out = blob.copy()
    out[byte_off:byte_off + 8] = np.array([value], dtype="<u8").view(np.uint8)
    return out


def test_query_refusals_and_damaged_headers():
    E = emul()
    caps = _caps()
    n = 3000
    T = W.text_with_sigma(n, 17, 2)
    SA, _, B, primary, _ = E.build_bwt(T)
    fm = _fmw(E, B, primary, SA, 32, 32)
    blob = fm.blob
    pats = [T[5:25].tobytes(), b""]
    first, count = fm.count(pats)
    # extract and text samples: not built for the wide format, nothing written
    for call in (lambda: fm.with_text_samples(32), lambda: fm.extract([0], [5]), lambda: E.fm_extract_device(blob.ctypes.data, blob.size, 0, 0, 0, 0),
                 lambda: E.fm_add_text_samples_device(blob.ctypes.data, blob.size, 32)):
        keep = blob.copy()
        with pytest.raises(caps.CapsSaError) as e:
            call()
        assert e.value.code == EUNSUPPORTED and "wide" in str(e.value)
        assert np.array_equal(blob, keep)
    # header words, each off by one: Lv, the table offset, the level size, n_blocks, the three offsets, the total, the samples, sigma
    h = blob[:256].view(np.uint64)
    for word in (5, 6, 7, 8, 13, 14, 15, 16, 17, 18):
        for delta in (1, -1):
            bad = _set64(blob, 8 * word, int(h[word]) + delta)
            for call in (lambda b: E.fm_count(b, pats), lambda b: E.fm_locate(b, first, count), lambda b: E.fm_match(b, pats), lambda b: E.fm_mems(b, pats),
                         lambda b: E.fm_count_device(b.ctypes.data, b.size, 0, 0, 0, 0, 0)):
                with pytest.raises(caps.CapsSaError) as e:
                    call(bad)
                assert e.value.code == EINVAL, (word, delta)
    for word, value in ((1, 0), (1, 2), (2, 2 ** 33), (3, n), (4, 5), (12, 3)):
        with pytest.raises(caps.CapsSaError) as e:
            E.fm_count(_set64(blob, 8 * word, value), pats)
        assert e.value.code == EINVAL, word
    # the table: one entry of C, zone, Z off by one (first, middle, last of each), a letter, a code
    t0 = 256
    spots = [(W.OFF_C + 8 * k, "C") for k in (0, 1, 9, 16, 17, 256)] + [(W.OFF_ZONE + 8 * k, "zone") for k in (1, 7, 16)] + \
            [(W.OFF_Z + 8 * k, "Z") for k in (1, 3, 5, 9, 11)]
    for at, what in spots:
        cur = int(blob[t0 + at:t0 + at + 8].view(np.uint64)[0])
        for delta in (1, -1):
            if cur + delta < 0:
                continue
            bad = _set64(blob, t0 + at, cur + delta)
            for call in (lambda b: E.fm_count(b, pats), lambda b: E.fm_count_device(b.ctypes.data, b.size, 0, 0, 0, 0, 0)):
                with pytest.raises(caps.CapsSaError) as e:
                    call(bad)
                assert e.value.code == EINVAL and what in str(e.value), (what, at, delta, str(e.value))
    for at in (W.OFF_LETTERS + 3, W.OFF_LETTERS + 20, W.OFF_CODE_OF + 0x41, W.OFF_CODE_OF + 0xFF):
        bad = blob.copy()
        bad[t0 + at] ^= 1
        with pytest.raises(caps.CapsSaError) as e:
            E.fm_count(bad, pats)
        assert e.value.code == EINVAL
    # truncated blobs, null pointers, bad offsets, first + count > n
    for size in (0, 255, 256, 5055, blob.size - 1):
        with pytest.raises(caps.CapsSaError) as e:
            E.fm_count(blob[:size].copy() if size else np.zeros(0, dtype=np.uint8), pats)
        assert e.value.code == EINVAL
    off = np.array([0, 5, 3], dtype=np.uint64)
    with pytest.raises(caps.CapsSaError) as e:
        E.fm_count(blob, (np.zeros(8, dtype=np.uint8), off))
    assert e.value.code == EINVAL and "monotone" in str(e.value)
    with pytest.raises(caps.CapsSaError) as e:
        E.fm_locate(blob, np.array([n - 1], dtype=np.uint64), np.array([2], dtype=np.uint64))
    assert e.value.code == EINVAL
    assert _rc(E, "fm_count", blob.ctypes.data, blob.size, None, None, 1, None, None, 0)[0] == EINVAL
    # the good blob still answers
    f2, c2 = E.fm_count(blob, pats)
    assert np.array_equal(f2, first) and np.array_equal(c2, count) and int(count[0]) >= 1 and int(count[1]) == n


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [%(tests)r, %(root)r]
import caps_sa_amd
import fm_wide_reference as W
E = caps_sa_amd.CapsLib(%(so)r, "caps_sa_emul_")
rs = np.random.RandomState(77)
for n, sigma in ((5000, 5), (4000, 17), (3000, 200)):
    T = W.text_with_sigma(n, sigma, 1)
    SA, _, B, primary, _ = E.build_bwt(T)
    pats = [T[a:a + ln].tobytes() for a, ln in ((0, 300), (63, 64), (2000, 700), (n - 10, 10), (100, 1), (0, 0))] + [bytes(T[:40]) + b"\x7e" * 3]
    for bits in (32, 64):
        for s in (0, 32):
            good = E.fm_build_wide(B, primary, SA if s else None, 32, bits)
            for trial in range(4):
                bad = good.copy()
                at = rs.randint(5056, bad.size, size=1000)
                bad[at] ^= rs.randint(1, 256, size=1000).astype(np.uint8)
                first, count = E.fm_count(bad, pats)
                assert int((first + count).max()) <= n
                if s:
                    try:
                        E.fm_locate(bad, first, np.minimum(count, 20))
                    except caps_sa_amd.CapsSaError as e:
                        assert e.code == -1 and "walk" in str(e)
                ln, _, _, off = E.fm_match(bad, pats, 0, True)
                assert ln.size == int(off[-1]) and int(ln.max()) <= 700
                rec, moff = E.fm_mems(bad, pats, 1)
                assert rec.size == int(moff[-1]) <= ln.size
print("done")
"""


def test_corrupted_body_terminates():
    """1,000 flipped bytes behind the table section of a valid blob, 48 blobs at 2, 3 and 4 levels: every query reads inside the
    blob, ends and returns.  In a child process, so that a read outside the blob ends the child and not the suite.  Never on a GPU."""
    emul()
    code = _CHILD % {"tests": os.path.join(ROOT, "tests"), "root": ROOT, "so": os.path.join(EMUL_DIR, "libcaps_sa_emul.so")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("done"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- the other emulation builds ------------------------------------------------------------------------------------------------------

def small_sweep(E):
    done = blob_sweep(E, (129, 16385), (5, 17, 256), all_primaries_up_to=0)
    T = W.text_with_sigma(2 * 16384 + 7, 17, 6)
    SA, _, B, primary, _ = emul().build_bwt(T)
    fm = _fmw(E, B, primary, SA, 32, 32)
    assert np.array_equal(fm.blob, W.encode(B, primary, SA, 32, 4))
    pats = make_patterns(T, np.random.RandomState(8), 0x7E, 12)
    first, count = fm.count(pats)
    return done, fm.blob.tobytes(), first.tobytes(), count.tobytes(), b"".join(h.tobytes() for h in fm.locate(pats, 4)), \
        b"".join(x.tobytes() for x in fm.matching_statistics(pats, 50)), b"".join(m.tobytes() for m in fm.mems(pats, 2))


def test_other_builds_give_the_same_answers():
    """Descending thread order and 64-thread pipeline tiles: the plain build's blobs and answers."""
    ref = small_sweep(emul())
    for E in (emul_rev(False), emul_small()):
        assert small_sweep(E) == ref


@pytest.mark.slow
def test_poison_and_race_builds():
    """The same through the poison-filled build (LDS and registers start as 0xA5, scattered thread order) and the barrier-race
    detector: the plain build's blobs and answers, and no race."""
    import ctypes
    from test_emul_inverse_bwt import _load
    poison, _ = _load("libcaps_sa_emul_small_poison.so")
    race, raw = _load("libcaps_sa_emul_small_race.so")
    raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
    raw.caps_sa_emul_races_reset()
    ref = small_sweep(emul())
    assert small_sweep(poison) == ref
    assert small_sweep(race) == ref
    assert int(raw.caps_sa_emul_races_found()) == 0
