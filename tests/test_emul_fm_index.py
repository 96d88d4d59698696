"""CPU: the FM-index (include/caps_sa_hip.h caps_sa_hip_fm_*) through the host emulation of the kernels (tests/emul).

Truth is independent of the index: the suffix array (the fixtures' recorded one, or the emulated build's) and the text.  An answer
(first, count) with count > 0 is exact iff T[SA[k] .. + m) == P at k = first and k = first + count - 1 and != P at k = first - 1 and
k = first + count where those ranks exist (the SA is sorted: the matches are one interval); count == 0 is right iff P occurs
nowhere (brute force over the text) and first == 0.  locate must equal SA[first : first + count] entry by entry.  Every pattern
of every batch is checked."""
import itertools
import subprocess
import sys

import numpy as np
import pytest

from conftest import LARGE_GOLDEN, large_golden, text_bytes
from emul_util import ROOT, emul, emul_rev, emul_small

EINVAL, EUNSUPPORTED, EALPHABET = -1, -2, -6
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
FM_LARGE = [name for name in LARGE_GOLDEN if name != "latin1_signed_136k"]
SAMPLES = (1, 2, 32, 64, 1024)
LENGTHS = (1, 2, 3, 8, 31, 32, 33, 100, 5000)


def _fm(E, B, primary, SA=None, s=32, bits=None):
    import caps_sa_amd
    return caps_sa_amd.FMIndex.from_bwt(B, primary, SA, s, bits, _lib=E)


def _bwt_of(T, SA):
    """(BWT, primary) in the header's convention, from the suffix array."""
    n = T.size
    SA = SA.astype(np.int64)
    return T[(SA + n - 1) % n], int(np.flatnonzero(SA == 0)[0])


def _occurs(tb: bytes, P: bytes) -> bool:
    return tb.find(P) >= 0


def check_answers(T, SA, pats, first, count):
    """The four-rank condition for every pattern."""
    n, tb = T.size, T.tobytes()
    assert first.dtype == np.uint64 and count.dtype == np.uint64 and first.size == len(pats) == count.size
    for P, f, c in zip(pats, first.tolist(), count.tolist()):
        P = bytes(P)
        m = len(P)
        if m == 0:
            assert (f, c) == (0, n), (P, f, c)
            continue
        if c == 0:
            assert f == 0 and not _occurs(tb, P), (P[:40], f, c)
            continue
        assert f + c <= n, (P[:40], f, c)
        at = lambda k: tb[int(SA[k]):int(SA[k]) + m]        # noqa: E731
        assert at(f) == P and at(f + c - 1) == P, (P[:40], f, c)
        if f > 0:
            assert at(f - 1) != P, (P[:40], f, c)
        if f + c < n:
            assert at(f + c) != P, (P[:40], f, c)


def check_locate(SA, first, count, hits):
    assert len(hits) == first.size
    for f, c, h in zip(first.tolist(), count.tolist(), hits):
        assert h.dtype == np.uint64 and np.array_equal(h, SA[f:f + c].astype(np.uint64)), (f, c)


def make_patterns(T, rs, foreign=ord("N"), per_length=3):
    """Substrings at random positions with the lengths of LENGTHS, mutated copies (mostly absent), a foreign byte at the first /
    middle / last position, the empty pattern, the whole text, the whole text + one byte."""
    n = T.size
    letters = np.unique(T)
    pats = [b"", T.tobytes(), T.tobytes() + bytes([int(letters[0])])]
    for m in LENGTHS:
        if m > n:
            continue
        for _ in range(per_length if m > 3 else 1):          # (a short pattern has hits by the ten thousand: one of each)
            a = int(rs.randint(0, n - m + 1))
            P = T[a:a + m].copy()
            pats.append(P.tobytes())
            Q = P.copy()
            k = int(rs.randint(0, m))
            Q[k] = letters[(int(np.searchsorted(letters, Q[k])) + 1) % letters.size]
            pats.append(Q.tobytes())
            for k in (0, m // 2, m - 1):
                Q = P.copy()
                Q[k] = foreign
                pats.append(Q.tobytes())
    pats.append(T[n - min(n, 7):].tobytes())                 # a suffix of the text
    return list(dict.fromkeys(pats))                         # (each pattern once, in order)


def full_check(E, T, SA, rs, samples=SAMPLES, foreign=ord("N")):
    """count exact and locate == the SA slices, for every sample distance; both index widths give identical answers."""
    B, primary = _bwt_of(T, SA)
    pats = make_patterns(T, rs, foreign)
    ref = None
    for s in samples:
        for bits in (32, 64):
            fm = _fm(E, B, primary, SA, s, bits)
            assert fm.n == T.size and fm.sa_sample == s and fm.nbytes == E.fm_index_bytes(T.size, s, bits)
            first, count = fm.count(pats)
            if ref is None:
                check_answers(T, SA, pats, first, count)
                ref = (first, count)
            assert np.array_equal(first, ref[0]) and np.array_equal(count, ref[1]), (s, bits)
            check_locate(SA, first, count, fm.locate(pats))
    return pats, ref


def test_golden_cases(golden_cases):
    E = emul()
    rs = np.random.RandomState(1)
    done = 0
    for c in golden_cases:
        T = text_bytes(c["text"])
        if T.size == 0 or np.unique(T).size > 4:
            continue
        SA, _, B, primary, _ = E.build_bwt(T)
        B2, p2 = _bwt_of(T, SA)
        assert np.array_equal(B, B2) and primary == p2
        foreign = next(b for b in range(1, 256) if b not in set(T.tolist()))
        full_check(E, T, SA, rs, foreign=foreign)
        done += 1
    assert done >= 3


@pytest.mark.parametrize("name", FM_LARGE)
def test_large_golden_cases(name):
    T, SA, _ = large_golden(name)
    assert np.unique(T).size <= 4
    full_check(emul(), T, SA, np.random.RandomState(len(name)))


def test_exhaustive_short_texts():
    """Every text over {A, C} of length 1 .. 8 and over {A, C, G} up to length 5, every pattern of length 0 .. 4 over the same
    letters plus one foreign letter, against brute force."""
    E = emul()
    for letters, max_n, foreign in ((b"AC", 8, b"G"), (b"ACG", 5, b"T")):
        pats = [bytes(p) for m in range(5) for p in itertools.product(letters + foreign, repeat=m)]
        for n in range(1, max_n + 1):
            for t in itertools.product(letters, repeat=n):
                T = np.array(t, dtype=np.uint8)
                tb = T.tobytes()
                SA, _, B, primary, _ = E.build_bwt(T)
                fm = _fm(E, B, primary, SA, 2)
                first, count = fm.count(pats)
                hits = fm.locate(pats)
                for P, f, c, h in zip(pats, first.tolist(), count.tolist(), hits):
                    occ = [i for i in range(n - len(P) + 1) if tb[i:i + len(P)] == P] if P else list(range(n))
                    assert c == len(occ), (tb, P, f, c)
                    assert sorted(h.tolist()) == occ and np.array_equal(h, SA[f:f + c].astype(np.uint64)), (tb, P)
                    if c == 0:
                        assert f == 0


def test_other_texts():
    """Bytes on both sides of 0x80 (the codes follow the signed order: compared with the SA), a^40000, (ACGT)^9000, a tandem repeat."""
    E = emul()
    rs = np.random.RandomState(3)
    texts = [
        rs.choice(np.array([0x05, 0x7F, 0x80, 0xFE], dtype=np.uint8), size=30_000),
        text_bytes("a" * 40_000),
        np.tile(DNA, 9_000),
        np.tile(rs.choice(DNA, size=171), 200),
    ]
    for T in texts:
        SA, _, B, primary, _ = E.build_bwt(T)
        full_check(E, T, SA, rs, samples=(1, 32, 1024), foreign=0x41 if T[0] != 0x41 and 0x41 not in T else 0x4E)


def test_refusals():
    import caps_sa_amd
    E = emul()
    rs = np.random.RandomState(5)
    T = rs.choice(DNA, size=5000)
    SA, _, B, primary, _ = E.build_bwt(T)
    # five distinct bytes
    T5 = rs.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=3000)
    SA5, _, B5, p5, _ = E.build_bwt(T5)
    blob = np.zeros(E.fm_index_bytes(T5.size, 32, 32), dtype=np.uint8)
    assert E._f("fm_build_u32")(B5.ctypes.data, T5.size, p5, SA5.ctypes.data, 32, blob.ctypes.data, blob.size, 0) == EALPHABET
    assert not blob.any()                                                          # nothing written
    T9, SA9, _ = large_golden("latin1_signed_136k")
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        _fm(E, *_bwt_of(T9, SA9), SA9)
    assert e.value.code == EALPHABET
    # locate without samples
    fm0 = _fm(E, B, primary)
    assert fm0.sa_sample == 0 and fm0.nbytes == E.fm_index_bytes(T.size, 0, 32)
    pats = make_patterns(T, rs)
    first, count = fm0.count(pats)
    check_answers(T, SA, pats, first, count)
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        fm0.locate(pats)
    assert e.value.code == EUNSUPPORTED
    # broken blobs and arguments
    fm = _fm(E, B, primary, SA, 32)
    first, count = fm.count(pats)
    cat, off = E._patterns(pats)
    q = len(pats)
    f_out, c_out = np.zeros(q, dtype=np.uint64), np.zeros(q, dtype=np.uint64)

    def count_rc(blob, nbytes, off_=off):
        return E._f("fm_count")(blob.ctypes.data, nbytes, cat.ctypes.data, off_.ctypes.data, q, f_out.ctypes.data, c_out.ctypes.data, 0)

    assert count_rc(fm.blob, fm.nbytes) == 0 and np.array_equal(f_out, first) and np.array_equal(c_out, count)
    assert count_rc(fm.blob, fm.nbytes - 1) == EINVAL                              # truncated
    assert count_rc(fm.blob, 100) == EINVAL                                        # shorter than a header
    bad = fm.blob.copy()
    bad[0] ^= 1
    assert count_rc(bad, bad.size) == EINVAL and "magic" in E._f("last_error")().decode()
    bad = fm.blob.copy()
    bad[8] = 9                                                                     # format version
    assert count_rc(bad, bad.size) == EINVAL
    bad = fm.blob.copy()
    bad[:256].view(np.uint64)[3] = T.size                                          # primary >= n
    assert count_rc(bad, bad.size) == EINVAL
    off_bad = off.copy()
    off_bad[4] = off_bad[3] - 1
    assert off_bad[4] < off_bad[3] and count_rc(fm.blob, fm.nbytes, off_bad) == EINVAL
    out_off = np.zeros(q + 1, dtype=np.uint64)
    out_off[1:] = np.cumsum(count)
    pos = np.zeros(int(out_off[-1]), dtype=np.uint64)

    def locate_rc(first_, count_, off_, fn="fm_locate"):
        return E._f(fn)(fm.blob.ctypes.data, fm.nbytes, first_.ctypes.data, count_.ctypes.data, off_.ctypes.data, q, pos.ctypes.data, 0)

    assert locate_rc(first, count, out_off) == 0
    big = count.copy()
    big[1] = T.size + 1
    assert locate_rc(first, big, out_off) == EINVAL and locate_rc(first, big, out_off, "fm_locate_device") == EINVAL
    far = first.copy()
    far[2] = T.size
    one = np.ones(q, dtype=np.uint64)
    assert locate_rc(far, one, out_off) == EINVAL
    rev = out_off.copy()
    rev[5] = rev[6] + 1
    assert locate_rc(first, count, rev) == EINVAL and locate_rc(first, count, rev, "fm_locate_device") == EINVAL
    assert E._f("fm_count")(None, 1000, cat.ctypes.data, off.ctypes.data, q, f_out.ctypes.data, c_out.ctypes.data, 0) == EINVAL
    assert E._f("fm_count")(fm.blob.ctypes.data, fm.nbytes, cat.ctypes.data, None, q, f_out.ctypes.data, c_out.ctypes.data, 0) == EINVAL
    assert E._f("fm_count_device")(fm.blob.ctypes.data, fm.nbytes, cat.ctypes.data, off.ctypes.data, q, None, c_out.ctypes.data, None) == EINVAL
    # build arguments: sample distances, sizes, widths
    blob = np.zeros(fm.nbytes, dtype=np.uint8)
    build = E._f("fm_build_u32")
    for s in (0, 3, 2048):
        assert build(B.ctypes.data, T.size, primary, SA.ctypes.data, s, blob.ctypes.data, blob.size, 0) == EINVAL
    assert build(B.ctypes.data, T.size, primary, SA.ctypes.data, 32, blob.ctypes.data, blob.size - 1, 0) == EINVAL
    assert build(B.ctypes.data, T.size, T.size, SA.ctypes.data, 32, blob.ctypes.data, blob.size, 0) == EINVAL
    assert build(B.ctypes.data, (1 << 32) + 5, 0, None, 0, blob.ctypes.data, 1 << 62, 0) == EINVAL      # before any allocation
    assert E._f("fm_build_device_u32")(B.ctypes.data, (1 << 32) + 5, 0, None, 0, blob.ctypes.data, 1 << 62, None) == EINVAL
    notsa = SA.copy()
    notsa[:] = 0                                                                   # every row a multiple of 32: not a permutation
    assert build(B.ctypes.data, T.size, primary, notsa.ctypes.data, 32, blob.ctypes.data, blob.size, 0) == EINVAL
    assert build(B.ctypes.data, T.size, primary, SA.ctypes.data, 32, blob.ctypes.data, blob.size, 0) == 0
    assert np.array_equal(blob, fm.blob)                                           # a valid call afterwards, the same bytes


def test_empty_text():
    E = emul()
    for bits in (32, 64):
        fm = _fm(E, np.zeros(0, dtype=np.uint8), 0, None, 32, bits)
        assert fm.n == 0
        first, count = fm.count([b"", b"A", b"ACGT"])
        assert not first.any() and not count.any()
        assert all(h.size == 0 for h in fm.locate([b"", b"A"]))


def test_sizes():
    """The point of packing: at most 0.75 bytes per base with 32-bit indices and 1.0 with 64-bit ones (s = 32)."""
    E = emul()
    n4, n8 = 3_000_000_001, 1 << 33
    assert E.fm_index_bytes(n4, 32, 32) <= 0.75 * n4 + (64 << 10)
    assert E.fm_index_bytes(n8, 32, 64) <= 1.0 * n8 + (64 << 10)
    assert E.fm_index_bytes(n4, 0, 32) <= 0.5 * n4 + (64 << 10)
    assert E.fm_index_bytes(n4, 32, 32) > E.fm_index_bytes(n4, 64, 32) > E.fm_index_bytes(n4, 0, 32)


def test_save_load_round_trip(tmp_path):
    import caps_sa_amd
    E = emul()
    rs = np.random.RandomState(9)
    T = rs.choice(DNA, size=20_000)
    SA, _, B, primary, _ = E.build_bwt(T)
    fm = _fm(E, B, primary, SA, 64)
    path = str(tmp_path / "x.fm")
    fm.save(path)
    assert (tmp_path / "x.fm").stat().st_size == fm.nbytes
    fm2 = caps_sa_amd.FMIndex.load(path, _lib=E)
    assert np.array_equal(fm.blob, fm2.blob) and fm2.n == T.size and fm2.sa_sample == 64
    pats = make_patterns(T, rs)
    a, b = fm.count(pats), fm2.count(pats)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    check_answers(T, SA, pats, *b)
    check_locate(SA, b[0], b[1], fm2.locate(pats))
    capped = fm2.locate(pats, max_hits=5)
    for f, c, h in zip(b[0].tolist(), b[1].tolist(), capped):
        assert np.array_equal(h, SA[f:f + min(c, 5)].astype(np.uint64))


@pytest.mark.slow
def test_other_builds_give_the_same_bytes():
    """The small-tile and the reversed-order builds of the emulation: the same blob, the same answers."""
    rs = np.random.RandomState(23)
    T = rs.choice(DNA, size=40_000)
    T[10_000:18_000] = np.tile(rs.choice(DNA, size=40), 200)
    SA, _, B, primary, _ = emul().build_bwt(T)
    pats = make_patterns(T, rs)
    ref = None
    for E in (emul(), emul_small(), emul_rev(True), emul_rev(False)):
        for bits in (32, 64):
            fm = _fm(E, B, primary, SA, 32, bits)
            first, count = fm.count(pats)
            hits = fm.locate(pats)
            got = (fm.blob.tobytes() if bits == 32 else None, first.tobytes(), count.tobytes(), b"".join(h.tobytes() for h in hits))
            if bits == 32:
                if ref is None:
                    check_answers(T, SA, pats, first, count)
                    check_locate(SA, first, count, hits)
                    ref = got
                assert got == ref
            else:
                assert got[1:] == ref[1:]


@pytest.mark.slow
def test_poison_and_race_builds_at_the_geometry_edges():
    """FM build, count and locate, build_bwt and bwt_device through the poison-filled build (LDS and registers start as 0xA5,
    scattered order) and the barrier-race detector, at sizes on a block edge (127, 128), a tile edge of the FM kernels (16,383,
    16,384) and beyond two tiles (40,001), both widths, s = 1 and 32: the plain build's blobs and answers, and no race."""
    import ctypes
    from test_emul_inverse_bwt import _load
    plain = emul()
    poison, _ = _load("libcaps_sa_emul_small_poison.so")
    race, raw = _load("libcaps_sa_emul_small_race.so")
    raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
    raw.caps_sa_emul_races_reset()
    rs = np.random.RandomState(29)
    runs = 0
    for n in (127, 128, 16_383, 16_384, 40_001):
        T = rs.choice(DNA, size=n)
        pats = make_patterns(T, rs)
        ref = {}
        for E in (plain, poison, race):
            for bits in (32, 64):
                SA, LCP, B, primary, _ = E.build_bwt(T, idx_bits=bits)
                got = {"sa": SA.astype(np.uint64).tobytes(), "lcp": LCP.astype(np.uint64).tobytes(), "bwt": B.tobytes(), "primary": primary}
                for first, cnt in ((0, n), (1, n - 1), (primary, 1), (max(primary - 1, 0), 2), (n // 2, 0)):
                    out = np.full(cnt + 2, 0xA5, dtype=np.uint8)
                    p = E.bwt_device(T.ctypes.data, n, SA[first:].ctypes.data, first, cnt, out[1:].ctypes.data, idx_bits=bits)
                    assert out[0] == 0xA5 and out[-1] == 0xA5
                    got["slice", first, cnt] = (out[1:-1].tobytes(), p)
                for s in (1, 32):
                    blob = E.fm_build(B, primary, SA, s, bits)
                    first, count = E.fm_count(blob, pats)
                    pos, _ = E.fm_locate(blob, first, count)
                    got["fm", s] = (blob.tobytes(), first.tobytes(), count.tobytes(), pos.tobytes())
                    if E is plain and bits == 32 and s == 1:
                        check_answers(T, SA, pats, first, count)
                        out_off = np.concatenate([[0], np.cumsum(count.astype(np.int64))])
                        check_locate(SA, first, count, [pos[out_off[j]:out_off[j + 1]] for j in range(len(pats))])
                    runs += 1
                if E is plain:
                    ref[bits] = got
                    assert got["bwt"] == _bwt_of(T, SA)[0].tobytes() and primary == _bwt_of(T, SA)[1]
                assert got.keys() == ref[bits].keys()
                for key in got:
                    assert got[key] == ref[bits][key], (n, bits, key)
    assert runs == 5 * 3 * 2 * 2
    assert int(raw.caps_sa_emul_races_found()) == 0


ANY_BLOB_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from emul_util import emul
import caps_sa_amd
E = emul()
rs = np.random.RandomState(77)
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
T = rs.choice(DNA, size=100_000)
SA, _, B, primary, _ = E.build_bwt(T)
for bits in (32, 64):
    blob = E.fm_build(B, primary, SA, 32, bits).copy()
    at = rs.randint(256, blob.size, size=1000)
    blob[at] ^= rs.randint(1, 256, size=1000).astype(np.uint8)
    pats = [T[a:a + m].tobytes() for a, m in zip(rs.randint(0, T.size - 64, size=1000), rs.randint(1, 64, size=1000))]
    fm = caps_sa_amd.FMIndex(blob, _lib=E)
    first, count = fm.count(pats)                       # CAPS_SA_OK: count has no error to report, only bounds to keep
    assert (first + count <= T.size).all()
    try:
        hits = fm.locate(pats, max_hits=50)
    except caps_sa_amd.CapsSaError as e:
        assert e.code == -1, e
print("returned")
"""


def test_any_blob_terminates_inside_the_blob():
    """A valid blob with 1,000 random byte flips in its body (header intact): count and locate over 1,000 queries return
    (CAPS_SA_OK or CAPS_SA_EINVAL) -- on the CPU emulation only."""
    r = subprocess.run([sys.executable, "-c", ANY_BLOB_CHILD, ROOT], timeout=120, capture_output=True, text=True)
    assert r.returncode == 0 and "returned" in r.stdout, r.stderr[-2000:]
