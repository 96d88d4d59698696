"""CPU: BWT, inverse BWT and FM-index with sizes and `primary` ON the edges of the kernels' geometry, through the host emulation.

The geometry (kernels.h fm_*, ibwt_*): 16 rows per code word, 32 per mark word, 128 (_u32) / 256 (_u64) rows per Occ block, 16,384
rows per tile, a splitter every 64 rows, ranking levels that switch at 16,384 and 1,048,576 rows, and ONE '$' row at primary + 1
with a slow path of its own.  Every fast path is guarded by a comparison with n, n + 1 or primary + 1; fm_reference.EDGE_SIZES and
edge_primaries put n + 1 and primary + 1 one below, on and one above every such modulus.

Truth never comes from the library:
  * the FM blob is compared BYTE FOR BYTE with fm_reference.encode, a numpy encoder written from the format table of
    include/caps_sa_hip.h;
  * queries: a pattern made to match ONE chosen rank k must come back as (k, 1); every answer meets the four-rank condition of
    test_emul_fm_index.check_answers; locate of the empty pattern is the whole suffix array;
  * BWT against T[(SA + n - 1) mod n], the inverse BWT against T; texts of fm_reference.text_with_primary have the primary they
    were built for, and below 4,097 bytes the suffix array is also the naive one.
The sweeps take the library as an argument: test_gpu_geometry.py runs the same ones on the MI355X."""
import functools

import numpy as np
import pytest

import fm_reference as R
from emul_util import emul
from test_emul_fm_index import check_answers

NOT_FOUND = 2**64 - 1
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
# 1, 2, 3 and 4 letters; the last one has two bytes on each side of 0x80 and is NOT in byte order
ALPHABETS = (b"A", b"AC", b"ACG", bytes([0x05, 0x7F, 0x80, 0xFE]))
SAMPLES = (1, 2, 32, 64, 1024)
NAIVE_MAX = 4096                       # the naive suffix array up to here, the library's own above
SMALL = tuple(n for n in R.EDGE_SIZES if n <= NAIVE_MAX)
LARGE = tuple(n for n in R.EDGE_SIZES if n > NAIVE_MAX)
MILLION = (1_048_575, 1_048_576, 1_048_577)


# ---- blobs without samples: any (BWT, primary) builds -------------------------------------------------------------------------

def blobs_without_samples(lib, sizes=R.EDGE_SIZES):
    """Every n of `sizes` x the four alphabets x both widths x every primary (n <= 257) or edge_primaries(n) -> blobs compared."""
    done = 0
    for n in sizes:
        rs = np.random.RandomState(n)
        primaries = range(n) if n <= 257 else R.edge_primaries(n)
        for letters in ALPHABETS:
            B = rs.choice(np.frombuffer(letters, dtype=np.uint8), size=n)
            for primary in primaries:
                for bits in (32, 64):
                    blob = lib.fm_build(B, primary, None, 0, bits)
                    want = R.encode(B, primary, None, 0, bits // 8)
                    assert blob.size == want.size == lib.fm_index_bytes(n, 0, bits), (n, letters, primary, bits)
                    assert np.array_equal(blob, want), (n, letters, primary, bits, np.flatnonzero(blob != want)[:8])
                    done += 1
    return done


def test_blob_bytes_without_samples():
    assert blobs_without_samples(emul()) >= 5000


# ---- texts with a chosen primary ----------------------------------------------------------------------------------------------

def chosen_primaries(n):
    """0, n - 1, the word edge (row 16 = primary + 1), the block edges of both widths and the tile edge, where they are < n."""
    return sorted(p for p in {0, n - 1, 15, 127, 255, 16_383} if 0 <= p <= n - 1)


def family_letters(n, j):
    return R.SIGNED_LETTERS if (n + j) % 2 else R.DNA_LETTERS


@functools.lru_cache(maxsize=None)
def _family_text(n, j):
    return R.text_with_primary(n, j, seed=n + j, letters=family_letters(n, j))


_built = {}


def family_case(lib, n, j):
    """(T, SA, BWT, primary) of the text with primary j; SA naive for n <= NAIVE_MAX, else the library's.  Kept per library."""
    key = (id(lib), n, j)
    if key not in _built:
        T = _family_text(n, j)
        SA, _, B, primary, _ = lib.build_bwt(T)
        assert primary == j, (n, j, primary)                      # what the construction promises
        if n <= NAIVE_MAX:
            naive = R.naive_sa(T)
            assert np.array_equal(SA.astype(np.int64), naive), (n, j)
            SA = naive.astype(np.uint32)
        B2, p2 = R.bwt_of(T, SA)
        assert np.array_equal(B, B2) and p2 == j, (n, j)
        _built[key] = (T, SA, B, j)
    return _built[key]


def blobs_with_samples(lib, sizes):
    done = 0
    for n in sizes:
        for j in chosen_primaries(n):
            T, SA, B, primary = family_case(lib, n, j)
            for s in SAMPLES:
                for bits in (32, 64):
                    blob = lib.fm_build(B, primary, SA, s, bits)
                    want = R.encode(B, primary, SA, s, bits // 8)
                    assert blob.size == want.size == lib.fm_index_bytes(n, s, bits), (n, j, s, bits)
                    assert np.array_equal(blob, want), (n, j, s, bits, np.flatnonzero(blob != want)[:8])
                    done += 1
    return done


def test_blob_bytes_with_samples():
    """Both halves of the size list in one test, so that the count of the whole sweep is asserted."""
    E = emul()
    assert sum(len(chosen_primaries(n)) for n in R.EDGE_SIZES) * len(SAMPLES) * 2 >= 400
    assert blobs_with_samples(E, SMALL) + blobs_with_samples(E, LARGE) >= 400


# ---- queries whose interval starts or ends at a rank of interest --------------------------------------------------------------

def ranks_of_interest(n, primary):
    ks = {0, n - 1, primary - 1, primary, primary + 1}
    for m in (128, 256, 16_384):
        for x in range(m, n + 2, m):
            ks |= {x - 2, x - 1, x, x + 1}
    return sorted(k for k in ks if 0 <= k <= n - 1)


def _lcp(T, a, b):
    ln = T.size - max(a, b)
    d = np.flatnonzero(T[a:a + ln] != T[b:b + ln])
    return int(d[0]) if d.size else ln


def edge_patterns(T, SA, primary):
    """For every rank of interest k: P = T[SA[k] : SA[k] + m), m = max(LCP[k], LCP[k + 1]) + 1, cut at the text end -- when it is
    not cut ("fits") it occurs at rank k and nowhere else -- and the pattern one byte shorter, whose interval reaches a
    neighbour.  -> (patterns, [(index of P, k)] of the fitting ones, number of ranks of interest)."""
    n = T.size
    ranks = ranks_of_interest(n, primary)
    pats, exact = [], []
    for k in ranks:
        a = int(SA[k])
        below = _lcp(T, int(SA[k - 1]), a) if k > 0 else 0
        above = _lcp(T, a, int(SA[k + 1])) if k + 1 < n else 0
        m = max(below, above) + 1
        if a + m <= n:
            exact.append((len(pats), k))
        pats.append(T[a:a + m].tobytes())
        pats.append(T[a:a + m - 1].tobytes())
    return pats, exact, len(ranks)


def _locate_capped(lib, blob, first, count, cap):
    take = np.minimum(count, np.uint64(cap))
    out_off = np.zeros(first.size + 1, dtype=np.uint64)
    out_off[1:] = np.cumsum(take, dtype=np.uint64)
    pos, _ = lib.fm_locate(blob, first, count, out_off)
    return pos, out_off


def query_case(lib, n, j, samples=SAMPLES):
    """-> (ranks of interest, ranks whose exact pattern fitted)"""
    T, SA, B, primary = family_case(lib, n, j)
    pats, exact, n_ranks = edge_patterns(T, SA, primary)
    whole = SA.astype(np.uint64)
    ref = None
    for s in samples:
        for bits in (32, 64):
            blob = lib.fm_build(B, primary, SA, s, bits)
            if s == 32:                                                       # count does not read the samples: one distance
                first, count = lib.fm_count(blob, pats)
                if ref is None:
                    check_answers(T, SA, pats, first, count)
                    for i, k in exact:
                        assert (int(first[i]), int(count[i])) == (k, 1), (n, j, k, pats[i][:40])
                    ref = (first, count)
                assert np.array_equal(first, ref[0]) and np.array_equal(count, ref[1]), (n, j, bits)
                pos, off = _locate_capped(lib, blob, first, count, 3)
                for q, (f, c) in enumerate(zip(first.tolist(), count.tolist())):
                    assert np.array_equal(pos[int(off[q]):int(off[q + 1])], whole[f:f + min(c, 3)]), (n, j, bits, q)
            f0, c0 = lib.fm_count(blob, [b""])
            assert (int(f0[0]), int(c0[0])) == (0, n)
            pos, _ = lib.fm_locate(blob, f0, c0)
            assert np.array_equal(pos, whole), (n, j, s, bits)
    return n_ranks, len(exact)


def queries(lib, sizes, samples=SAMPLES):
    """Every rank of interest is queried.  The pattern that matches it alone exists unless the suffix at that rank is a prefix
    of a neighbour's, which in this family happens for the last byte of the text and, when primary = n - 1 (T = c . a^(n-1), R
    empty), for every suffix a^i: over the texts with a non-empty R at least nine tenths of the ranks have it."""
    ranks = fitted = ranks_r = fitted_r = 0
    for n in sizes:
        for j in chosen_primaries(n):
            a, b = query_case(lib, n, j, samples)
            ranks, fitted = ranks + a, fitted + b
            if j < n - 1 and n >= 14:
                ranks_r, fitted_r = ranks_r + a, fitted_r + b
    assert ranks_r and fitted_r * 10 >= ranks_r * 9, (fitted_r, ranks_r)
    return ranks, fitted


def test_queries_at_the_edges_small():
    ranks, fitted = queries(emul(), SMALL)
    assert ranks >= 400 and fitted >= 300, (ranks, fitted)


def test_queries_at_the_edges_large():
    """The sizes above 4,096 with the samples of distance 32 (the whole-SA locate of the other distances: the slow test below)."""
    ranks, fitted = queries(emul(), LARGE, samples=(32,))
    assert ranks >= 10_000 and fitted >= 9000, (ranks, fitted)


@pytest.mark.slow
def test_queries_at_the_edges_large_every_sample_distance():
    ranks, fitted = queries(emul(), LARGE)
    assert ranks >= 10_000 and fitted >= 9000, (ranks, fitted)


# ---- BWT and inverse BWT ------------------------------------------------------------------------------------------------------

def shapes(n):
    rs = np.random.RandomState(n + 1)
    return [rs.choice(DNA, size=n),
            rs.randint(0, 256, size=n).astype(np.uint8),                     # all 256 byte values
            np.full(n, ord("a"), dtype=np.uint8),
            rs.choice(np.array([0x7F, 0x80], dtype=np.uint8), size=n)]      # two bytes across 0x80


def bwt_round_trip(lib, T, primary=None):
    n = T.size
    SA, _, B, p, _ = lib.build_bwt(T)
    S = SA.astype(np.int64)
    assert B.dtype == np.uint8 and np.array_equal(B, T[(S + n - 1) % n]), n
    assert p == int(np.flatnonzero(S == 0)[0]) and (primary is None or p == primary), (n, p, primary)
    if n <= NAIVE_MAX:
        assert np.array_equal(S, R.naive_sa(T)), n
    for bits in (32, 64):
        out = lib.inverse_bwt(B, p, idx_bits=bits)
        assert out.dtype == np.uint8 and np.array_equal(out, T), (n, bits)


def bwt_sweep(lib, sizes, family=True):
    done = 0
    for n in sizes:
        for T in shapes(n):
            bwt_round_trip(lib, T)
            done += 1
        if family:
            for j in R.edge_primaries(n):
                T, SA, B, primary = family_case(lib, n, j)                    # (build_bwt against the gather and j: family_case)
                for bits in (32, 64):
                    assert np.array_equal(lib.inverse_bwt(B, primary, idx_bits=bits), T), (n, j, bits)
                done += 1
    return done


def test_bwt_and_inverse_small():
    assert bwt_sweep(emul(), SMALL) >= 4 * len(SMALL) + 100


def test_bwt_and_inverse_large():
    assert bwt_sweep(emul(), LARGE) >= 4 * len(LARGE) + 50


@pytest.mark.slow
@pytest.mark.parametrize("n", MILLION)
def test_bwt_and_inverse_at_the_second_ranking_level(n):
    rs = np.random.RandomState(n)
    bwt_round_trip(emul(), rs.choice(DNA, size=n))


# ---- bwt_device on slices ------------------------------------------------------------------------------------------------------

def slice_list(primary, n):
    out = [(first, cnt) for first in range(17) for cnt in range(34)]
    for first in (primary - 1, primary, primary + 1):
        for end in (primary - 1, primary, primary + 1, primary + 2):
            if 0 <= first <= end <= n:
                out.append((first, end - first))
    return out


def test_bwt_device_slices():
    E = emul()
    rs = np.random.RandomState(50)
    T = rs.choice(DNA, size=5000)
    n = T.size
    for bits in (32, 64):
        SA, _ = E.build(T, idx_bits=bits)[:2]
        S = SA.astype(np.int64)
        want = T[(S + n - 1) % n]
        primary = int(np.flatnonzero(S == 0)[0])
        assert 17 < primary < n - 2                                           # (the slices around it are not those of the grid)
        cases = slice_list(primary, n)
        assert len(cases) == 17 * 34 + 9
        for first, cnt in cases:
            out = np.full(cnt + 8, 0xA5, dtype=np.uint8)
            p = E.bwt_device(T.ctypes.data, n, SA[first:].ctypes.data, first, cnt, out[4:].ctypes.data, idx_bits=bits)
            assert np.array_equal(out[4:4 + cnt], want[first:first + cnt]), (bits, first, cnt)
            assert (out[:4] == 0xA5).all() and (out[4 + cnt:] == 0xA5).all(), (bits, first, cnt)
            assert p == (primary if first <= primary < first + cnt else NOT_FOUND), (bits, first, cnt, p)
