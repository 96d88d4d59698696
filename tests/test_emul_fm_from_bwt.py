"""CPU: the FM-index with its SA samples from (BWT, primary) ALONE (include/caps_sa_hip.h "FM-index from the BWT alone",
caps_sa_hip_fm_build_from_bwt_*) through the host emulation of the kernels.

The blob must be, byte for byte, the one the build with the suffix array writes: every case is compared with fm_reference.encode
(the independent numpy encoder) and, in the sweep, with lib.fm_build given the SA.  Truth never comes from the new path.

Ranking levels: the splitter constants are the inverse BWT's (a splitter every 64 rows, a list level per 64 nodes, at most 256
nodes in the top workgroup), so n < 16,384 ranks the splitters in the top workgroup, n = 16,384 adds the second level and
n = 1,048,576 the third: the sizes one below, on and one above each are below."""
import ctypes
import itertools

import numpy as np
import pytest

import fm_reference as R
from conftest import large_golden, text_bytes
from emul_util import emul, emul_rev, emul_small
from test_emul_fm_index import check_answers, check_locate, make_patterns
from test_emul_geometry import ALPHABETS, LARGE, MILLION, SAMPLES, SMALL, chosen_primaries, family_case

EINVAL, EALPHABET = -1, -6
FILL = 0xA5
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


def _same(blob, want, what):
    assert blob.dtype == np.uint8 and blob.size == want.size, what
    assert np.array_equal(blob, want), (what, np.flatnonzero(blob != want)[:8])


# ---- 1. blob bytes over the geometry's sizes ----------------------------------------------------------------------------------

def blobs_from_bwt(lib, sizes, samples=SAMPLES, with_fm_build=True):
    """Every n of `sizes` x chosen_primaries(n) x `samples` x both widths: the blob from the BWT alone against the encoder and
    against the build with the SA.  test_gpu_fm_from_bwt.py runs the same sweep on the device forms."""
    done = 0
    for n in sizes:
        for j in chosen_primaries(n):
            T, SA, B, primary = family_case(lib, n, j)
            for s in samples:
                for bits in (32, 64):
                    blob = lib.fm_build_from_bwt(B, primary, s, bits)
                    assert blob.size == lib.fm_index_bytes(n, s, bits), (n, j, s, bits)
                    _same(blob, R.encode(B, primary, SA, s, bits // 8), (n, j, s, bits))
                    if with_fm_build:
                        _same(blob, lib.fm_build(B, primary, SA, s, bits), (n, j, s, bits, "fm_build"))
                    done += 1
    return done


def test_blob_bytes():
    E = emul()
    assert blobs_from_bwt(E, SMALL) + blobs_from_bwt(E, LARGE) >= 400


# ---- 2. the walk's own edges ---------------------------------------------------------------------------------------------------

SPLITTER_SIZES = (1, 2, 62, 63, 64, 65, 127, 128)
LEVEL_SIZES = (16_382, 16_383, 16_384, 16_385)


def walk_primaries(n):
    """0, n - 1 and the '$' row (primary + 1) next to, on and behind the first splitter edge (row 64)."""
    return sorted(p for p in {0, n - 1, 62, 63, 64} if 0 <= p <= n - 1)


def walk_edges(lib, sizes, samples, widths=(32, 64)):
    done = 0
    for n in sizes:
        for j in walk_primaries(n):
            T, SA, B, primary = family_case(lib, n, j)
            for s in samples:
                for bits in widths:
                    _same(lib.fm_build_from_bwt(B, primary, s, bits), R.encode(B, primary, SA, s, bits // 8), (n, j, s, bits))
                    done += 1
    return done


def test_first_splitter_edge():
    done = walk_edges(emul(), SPLITTER_SIZES, SAMPLES)
    assert done == sum(len(walk_primaries(n)) for n in SPLITTER_SIZES) * len(SAMPLES) * 2 == 240


def test_second_ranking_level():
    assert walk_edges(emul(), LEVEL_SIZES, (1, 32, 1024)) == len(LEVEL_SIZES) * 5 * 3 * 2


@pytest.mark.parametrize("n", MILLION)
def test_third_ranking_level(n):
    """The SA comes from the emulated build; s = 32, 32-bit indices."""
    E = emul()
    T = np.random.RandomState(n).choice(DNA, size=n)
    SA, _, B, primary, _ = E.build_bwt(T)
    _same(E.fm_build_from_bwt(B, primary, 32, 32), R.encode(B, primary, SA, 32, 4), n)


# ---- 3. long and degenerate walks ----------------------------------------------------------------------------------------------

def _naive_case(T):
    SA = R.naive_sa(T)
    B, primary = R.bwt_of(T, SA)
    return SA, B, primary


def _both(E, B, primary, SA, what):
    for s in (1, 32):
        for bits in (32, 64):
            _same(E.fm_build_from_bwt(B, primary, s, bits), R.encode(B, primary, SA, s, bits // 8), (what, s, bits))


@pytest.mark.parametrize("n", [1, 64, 65, 5000])
def test_one_letter(n):
    """a^n: SA = n - 1 .. 0, LF is r -> r + 1, every segment is exactly 64 steps."""
    T = np.full(n, ord("a"), dtype=np.uint8)
    SA = np.arange(n - 1, -1, -1, dtype=np.int64)
    B, primary = R.bwt_of(T, SA)
    assert primary == n - 1
    _both(emul(), B, primary, SA, ("a^n", n))


def test_ab_repeated():
    T = np.tile(text_bytes("ab"), 2500)
    SA, B, primary = _naive_case(T)
    _both(emul(), B, primary, SA, "(ab)^2500")


@pytest.mark.parametrize("name", ["two_letters_skewed_150k", "planted_repeat_145k", "markov_skewed_250k"])
def test_goldens(name):
    T, SA, _ = large_golden(name)
    B, primary = R.bwt_of(T, SA)
    _both(emul(), B, primary, SA, name)


def test_signed_alphabet():
    """05 7F 80 FE: two letters on each side of 0x80, codes in signed-char order."""
    letters = np.frombuffer(ALPHABETS[3], dtype=np.uint8)
    assert bytes(letters) == bytes([0x05, 0x7F, 0x80, 0xFE])
    T = np.random.RandomState(4).choice(letters, size=3000)
    SA, B, primary = _naive_case(T)
    _both(emul(), B, primary, SA, "signed")


# ---- 4. every short pair -------------------------------------------------------------------------------------------------------

def test_every_short_pair_over_two_letters():
    """Every B over {A, C} with 1 <= n <= 10 and every primary < n: the call succeeds exactly when the emulated inverse BWT does,
    then with the blob of the inverse's text; else -1 and the message of the LF cycle.  No case left out."""
    import caps_sa_amd
    E = emul()
    pairs = ok = 0
    for n in range(1, 11):
        for letters in itertools.product(b"AC", repeat=n):
            B = np.array(letters, dtype=np.uint8)
            for primary in range(n):
                pairs += 1
                try:
                    T = E.inverse_bwt(B, primary)
                except caps_sa_amd.CapsSaError:
                    T = None
                try:
                    blob = E.fm_build_from_bwt(B, primary, 1)
                except caps_sa_amd.CapsSaError as e:
                    assert T is None, (bytes(B), primary)
                    assert e.code == EINVAL and "LF mapping is not one cycle" in str(e), str(e)
                    continue
                assert T is not None, (bytes(B), primary)
                ok += 1
                _same(blob, R.encode(B, primary, R.naive_sa(T), 1, 4), (bytes(B), primary))
    assert pairs == sum(n * 2 ** n for n in range(1, 11)) and ok == sum(2 ** n for n in range(1, 11)), (pairs, ok)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals():
    E = emul()
    T = np.random.RandomState(6).choice(DNA, size=1000)
    SA, B, primary = _naive_case(T)
    n = B.size
    for sfx, bits in (("u32", 32), ("u64", 64)):
        nbytes = E.fm_index_bytes(n, 32, bits)
        ws_bytes = E.fm_from_bwt_workspace_bytes(n, 32, bits)
        index = np.full(nbytes, FILL, dtype=np.uint8)
        ws = np.zeros(ws_bytes, dtype=np.uint8)
        host, dev = E._f(f"fm_build_from_bwt_{sfx}"), E._f(f"fm_build_from_bwt_device_{sfx}")

        def refused(rc, word, code=EINVAL):
            assert rc == code, (sfx, word, rc)
            assert word in E._f("last_error")().decode(), (sfx, word, E._f("last_error")().decode())
            assert (index == FILL).all(), (sfx, word)

        for form in ("host", "device"):
            def call(b=B.ctypes.data, n_=n, p=primary, s=32, ib=nbytes, w=ws.ctypes.data, wb=ws_bytes):
                if form == "host":
                    return host(b, n_, p, s, index.ctypes.data, ib, 0)
                return dev(b, n_, p, s, index.ctypes.data, ib, w, wb, None)
            refused(call(s=0), "caps_sa_hip_fm_build_")            # points to the build with a null SA
            refused(call(s=0), "null SA")
            refused(call(s=3), "power of two")
            refused(call(s=2048), "power of two")
            refused(call(p=n), "primary >= n")
            refused(call(b=None), "null BWT")
            refused(call(ib=nbytes - 1), "index_bytes too small")
            if bits == 32:
                refused(call(n_=1 << 32, p=0, ib=1 << 62), "does not fit 32-bit")
            B5 = B.copy()
            B5[n // 2] = ord("N")
            refused(call(b=B5.ctypes.data), "more than 4 distinct bytes", EALPHABET)
        refused(dev(B.ctypes.data, n, primary, 32, index.ctypes.data, nbytes, ws.ctypes.data, ws_bytes - 1, None), "workspace too small")
        if sfx == "u32":
            assert host(B.ctypes.data, n, primary, 32, None, nbytes, 0) == EINVAL
        # the same buffers then build: the caller's workspace, and a null one (allocated by the call)
        want = R.encode(B, primary, SA, 32, bits // 8)
        for w, wb in ((ws.ctypes.data, ws_bytes), (None, 0)):
            index[:] = FILL
            assert dev(B.ctypes.data, n, primary, 32, index.ctypes.data, nbytes, w, wb, None) == 0
            _same(index, want, (sfx, "after the refusals"))
        index[:] = FILL
        assert host(B.ctypes.data, n, primary, 32, index.ctypes.data, nbytes, 0) == 0
        _same(index, want, (sfx, "host form"))


def test_empty_text():
    E = emul()
    empty = np.zeros(0, dtype=np.uint8)
    for s in SAMPLES:
        for bits in (32, 64):
            want = R.encode(empty, 0, np.zeros(0, dtype=np.int64), s, bits // 8)
            assert int(want[:256].view(np.uint64)[12]) == s and int(want[:256].view(np.uint64)[13]) == 0
            _same(E.fm_build_from_bwt(empty, 0, s, bits), want, (s, bits))
            index = np.full(want.size, FILL, dtype=np.uint8)
            E.fm_build_from_bwt_device(0, 0, 0, s, index.ctypes.data, index.size, idx_bits=bits)
            _same(index, want, (s, bits, "device"))


# ---- 6. the workspace bound ----------------------------------------------------------------------------------------------------

def test_workspace_bound():
    """No array of n entries: at most one index per sample, 32 bytes per 64 rows and 1 MiB."""
    E = emul()
    for n in (0, 1, 64, 10**6, 3 * 10**9 + 1, 2**33):
        for s in SAMPLES:
            for W in (4, 8):
                out = ctypes.c_uint64(0)
                rc = E._f("fm_from_bwt_workspace_bytes")(n, s, W, ctypes.byref(out))
                if n == 2**33 and W == 4:
                    assert rc == EINVAL
                    continue
                assert rc == 0
                n_samples = (n - 1) // s + 1 if n else 0
                assert out.value <= n_samples * W + 32 * (n // 64 + 1) + 2**20, (n, s, W, out.value)
                assert E.fm_from_bwt_workspace_bytes(n, s, 8 * W) == out.value
    out = ctypes.c_uint64(0)
    for s in (0, 3, 2048):
        assert E._f("fm_from_bwt_workspace_bytes")(1000, s, 4, ctypes.byref(out)) == EINVAL
    assert E._f("fm_from_bwt_workspace_bytes")(1000, 32, 3, ctypes.byref(out)) == EINVAL
    assert E._f("fm_from_bwt_workspace_bytes")(1000, 32, 4, None) == EINVAL


# ---- 7. queries end to end -----------------------------------------------------------------------------------------------------

def _queries(E, T, SA, B, primary, seed):
    import caps_sa_amd
    pats = make_patterns(T, np.random.RandomState(seed))
    for s, bits in ((32, None), (1, 64)):
        fm = caps_sa_amd.FMIndex.from_bwt_only(B, primary, s, bits, _lib=E)
        assert fm.n == T.size and fm.sa_sample == s
        first, count = fm.count(pats)
        check_answers(T, SA, pats, first, count)
        check_locate(SA, first, count, fm.locate(pats))


def test_queries_on_a_golden():
    T, SA, _ = large_golden("dna_cli_140k")
    B, primary = R.bwt_of(T, SA)
    _queries(emul(), T, SA, B, primary, 11)


def test_queries_on_a_family_case():
    E = emul()
    T, SA, B, primary = family_case(E, 16_385, 127)
    _queries(E, T, SA, B, primary, 12)


# ---- 8. the other emulation builds ---------------------------------------------------------------------------------------------

@pytest.mark.slow
def test_other_builds_give_the_same_bytes():
    """Small tiles, descending thread order, poison-filled LDS and registers (scattered order) and the barrier-race detector, one
    small case each (two list levels, both widths, s = 1 and 32): the encoder's bytes, and no hand-off reported for the new kernels."""
    from test_emul_inverse_bwt import _load
    rs = np.random.RandomState(31)
    T = rs.choice(DNA, size=17_001)
    T[4000:9000] = np.tile(rs.choice(DNA, size=25), 200)
    SA, _, B, primary, _ = emul().build_bwt(T)
    want = {(s, bits): R.encode(B, primary, SA, s, bits // 8) for s in (1, 32) for bits in (32, 64)}
    poison, _ = _load("libcaps_sa_emul_small_poison.so")
    race, raw = _load("libcaps_sa_emul_small_race.so")
    raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
    raw.caps_sa_emul_races_reset()
    for name, E in (("small", emul_small()), ("rev", emul_rev()), ("poison", poison), ("race", race)):
        for (s, bits), blob in want.items():
            _same(E.fm_build_from_bwt(B, primary, s, bits), blob, (name, s, bits))
    assert int(raw.caps_sa_emul_races_found()) == 0
