"""CPU: format version 2 of the FM-index blob (text-position samples) and extract (include/caps_sa_hip.h "FM-index: extract",
caps_sa_hip_fm_add_text_samples_*, caps_sa_hip_fm_extract_*) through the host emulation of the kernels.

Every comparison is exact.  The version-2 bytes are compared with fm_extract_reference.add_text_samples (numpy, from the format
table and the naive inverse of the suffix array); the truth of extract is the text itself.  The sweeps are functions of a library
object, so that test_gpu_fm_extract.py runs the same ones through the device entry points."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import fm_extract_reference as X
import fm_reference as R
from emul_util import EMUL_DIR, ROOT, emul, emul_rev, emul_small
from test_emul_geometry import family_case

EINVAL, EUNSUPPORTED = -1, -2
FILL = 0xA5
GUARD = 64
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


def _same(blob, want, what):
    assert blob.dtype == np.uint8 and blob.size == want.size, (what, blob.size, want.size)
    assert np.array_equal(blob, want), (what, np.flatnonzero(blob != want)[:8])


def _hdr(blob):
    return blob[:256].view(np.uint64)


def other_distance(s, t):
    return 1024 if t < 1024 else s


# ---- 1. blob bytes and extract over the geometry's sizes -----------------------------------------------------------------------

def few_primaries(n):
    return sorted({0, n // 2, n - 1})


def sizes_of(t, small_only=False):
    """The sizes on the kernels' edges and those on the edges of the chunks of t positions."""
    sizes = set(R.EDGE_SIZES) | set(X.chunk_edge_sizes(t))
    return sorted(n for n in sizes if not small_only or n <= 4096)


def check_extract(lib, blob, T, ranges, what):
    text, off = lib.fm_extract(blob, [a for a, _ in ranges], [ln for _, ln in ranges])
    want = X.expected(T, ranges)
    assert text.dtype == np.uint8 and text.size == want.size == int(off[-1]), what
    assert np.array_equal(text, want), (what, np.flatnonzero(text != want)[:8])


def mixed_batch(n, t, rs):
    """Empty, one-byte and long queries in one batch, in random order."""
    rg = [(int(rs.randint(0, n + 1)), 0) for _ in range(3)] + [(int(rs.randint(0, n)), 1) for _ in range(5)]
    for _ in range(4):
        a = int(rs.randint(0, n))
        rg.append((a, int(rs.randint(1, n - a + 1))))
    rg += [(0, n), (n, 0), (n - 1, 1)]
    return [rg[i] for i in rs.permutation(len(rg))]


def sweep(lib, sizes_for, distances=X.DISTANCES, widths=(32, 64), primaries=R.edge_primaries, from_bwt=True, queries=True):
    """Every n x primary x (s, t) x width: the version-2 bytes against the encoder -- from the build with the SA, from the BWT alone
    and from a version-2 blob at another distance --, the version-1 part unchanged, and extract on the chunk edges, the whole text
    and a mixed batch against the text; count and locate as on the version-1 blob.  Returns the number of blobs checked."""
    done = 0
    for s, t in distances:
        for n in sizes_for(t):
            for j in (primaries(n) if n <= 4096 else few_primaries(n)):
                T, SA, B, primary = family_case(lib, n, j)
                for bits in widths:
                    what = (n, j, s, t, bits)
                    v1 = lib.fm_build(B, primary, SA, s, bits)
                    want1 = R.encode(B, primary, SA, s, bits // 8)
                    _same(v1, want1, what)
                    want = X.add_text_samples(want1, SA, t)
                    v2 = lib.fm_add_text_samples(v1, t)
                    _same(v2, want, what)
                    assert v2.size == lib.fm_index_bytes_ex(n, s, t, bits) == int(_hdr(v2)[22]), what
                    assert np.array_equal(v2[16:152], v1[16:152]) and np.array_equal(v2[256:v1.size], v1[256:]), what
                    assert int(_hdr(v2)[1]) == 2 and int(_hdr(v2)[0]) == int(_hdr(v1)[0]), what
                    if from_bwt:
                        _same(lib.fm_add_text_samples(lib.fm_build_from_bwt(B, primary, s, bits), t), want, what + ("from the BWT",))
                    t2 = other_distance(s, t)
                    _same(lib.fm_add_text_samples(v2, t2), X.add_text_samples(want1, SA, t2), what + ("again at", t2))
                    check_extract(lib, v2, T, X.edge_ranges(n, t), what)
                    check_extract(lib, v2, T, mixed_batch(n, t, np.random.RandomState(n + j + t)), what + ("mixed",))
                    if queries:
                        pats = [b"", T[:5].tobytes(), T[n // 2:n // 2 + 9].tobytes(), T[n - min(n, 3):].tobytes(), b"N"]
                        f1, c1 = lib.fm_count(v1, pats)
                        f2, c2 = lib.fm_count(v2, pats)
                        assert np.array_equal(f1, f2) and np.array_equal(c1, c2), what
                        take = np.minimum(c1, np.uint64(20))
                        off = np.zeros(take.size + 1, dtype=np.uint64)
                        off[1:] = np.cumsum(take, dtype=np.uint64)
                        assert np.array_equal(lib.fm_locate(v1, f1, c1, off)[0], lib.fm_locate(v2, f2, c2, off)[0]), what
                    done += 1
    return done


def test_blob_bytes_and_extract_small():
    """n <= 4096 of the edge sizes and k t - 1, k t, k t + 1, every edge primary, DNA and the signed letters (the family alternates),
    both widths; the whole text in one query is also the inverse BWT's."""
    E = emul()
    assert sweep(E, lambda t: sizes_of(t, small_only=True)) >= 1800
    for n, j in ((129, 127), (4096, 255)):
        T, SA, B, primary = family_case(E, n, j)
        v2 = E.fm_add_text_samples(E.fm_build(B, primary, SA, 32, 32), 64)
        text, _ = E.fm_extract(v2, [0], [n])
        assert np.array_equal(text, E.inverse_bwt(B, primary)) and np.array_equal(text, T)


def test_blob_bytes_and_extract_large():
    """The tile edges (16,384 +- 1, 32,768) at three primaries each."""
    assert sweep(emul(), lambda t: [n for n in sizes_of(t) if n > 4096], distances=((1, 1), (32, 64), (32, 1024), (1024, 1024))) >= 100


# ---- 2. adjacent ranges at odd offsets, through the device entry point -----------------------------------------------------------

def raw_extract(lib, blob, ranges, base, workspace=True):
    """caps_sa_*_fm_extract_device on host memory (the emulation's 'device'): the output starts at the odd offset `base` of a buffer
    preset to 0xA5 with a guard behind it; returns the buffer."""
    starts, off = X.pack(ranges)
    off = off + np.uint64(base)
    total = int(off[-1])
    text = np.full(total + GUARD, FILL, dtype=np.uint8)
    ws_bytes = lib.fm_extract_workspace_bytes(len(ranges))
    ws = np.full(ws_bytes + GUARD, FILL, dtype=np.uint8)
    lib.fm_extract_device(blob.ctypes.data, blob.size, starts.ctypes.data, off.ctypes.data, len(ranges), text.ctypes.data,
                          ws.ctypes.data if workspace else 0, ws_bytes if workspace else 0)
    assert (ws[ws_bytes:] == FILL).all()
    return text, total


def odd_ranges(n, rs, count=200, longest=11):
    rg = []
    for _ in range(count):
        ln = int(rs.randint(0, min(longest, n) + 1))
        rg.append((int(rs.randint(0, n - ln + 1)), ln))
    return rg


def test_adjacent_ranges_at_odd_offsets():
    E = emul()
    T, SA, B, primary = family_case(E, 4097, 127)
    for s, t, bits in ((1, 1, 32), (32, 64, 32), (32, 32, 64)):
        v2 = E.fm_add_text_samples(E.fm_build(B, primary, SA, s, bits), t)
        rg = odd_ranges(T.size, np.random.RandomState(t))
        for base in (1, 3, 64):
            for ws in (True, False):
                text, total = raw_extract(E, v2, rg, base, ws)
                assert (text[:base] == FILL).all() and (text[total:] == FILL).all()
                assert np.array_equal(text[base:total], X.expected(T, rg)), (s, t, bits, base)


# ---- 3. every short text x every range ----------------------------------------------------------------------------------------

def test_every_short_text_and_every_range():
    """All texts over {A, C} with 1 <= n <= 8, every (start, length) with start + length <= n, t = 1, 2, 4: one batch per text."""
    E = emul()
    texts = ranges = 0
    for n in range(1, 9):
        rg = [(a, ln) for a in range(n + 1) for ln in range(n - a + 1)]
        for letters in itertools.product(b"AC", repeat=n):
            T = np.array(letters, dtype=np.uint8)
            SA = R.naive_sa(T)
            B, primary = R.bwt_of(T, SA)
            v1 = E.fm_build(B, primary, SA, 1, 32)
            for t in (1, 2, 4):
                v2 = E.fm_add_text_samples(v1, t)
                _same(v2, X.add_text_samples(R.encode(B, primary, SA, 1, 4), SA, t), (bytes(T), t))
                check_extract(E, v2, T, rg, (bytes(T), t))
            texts += 1
            ranges += len(rg)
    assert texts == sum(2 ** n for n in range(1, 9)) and ranges == sum(2 ** n * (n + 1) * (n + 2) // 2 for n in range(1, 9))


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------

def _err(E):
    return E._f("last_error")().decode()


def test_refusals_of_the_upgrade():
    import caps_sa_amd
    E = emul()
    T, SA, B, primary = family_case(E, 1000, 0)
    out = ctypes.c_uint64(0)
    for s, t, W in ((32, 16, 4), (32, 48, 4), (32, 2048, 4), (32, 0, 4), (0, 32, 4), (3, 32, 4), (32, 32, 3)):
        assert E._f("fm_index_bytes_ex")(1000, s, t, W, ctypes.byref(out)) == EINVAL, (s, t, W)
    assert E._f("fm_index_bytes_ex")(1000, 32, 64, 4, None) == EINVAL
    assert E._f("fm_index_bytes_ex")(1 << 32, 32, 64, 4, ctypes.byref(out)) == EINVAL
    assert E._f("fm_index_bytes_ex")(0, 32, 64, 4, ctypes.byref(out)) == 0 and out.value == E.fm_index_bytes(0, 32, 32)
    for bits in (32, 64):
        v1 = E.fm_build(B, primary, SA, 32, bits)
        need = E.fm_index_bytes_ex(1000, 32, 64, bits)
        for form in ("host", "device"):
            def call(buf, cap, t):
                if form == "host":
                    return E._f("fm_add_text_samples")(buf.ctypes.data if buf is not None else None, cap, t, 0)
                return E._f("fm_add_text_samples_device")(buf.ctypes.data if buf is not None else None, cap, t, None)
            buf = np.full(need + GUARD, FILL, dtype=np.uint8)
            buf[:v1.size] = v1
            before = buf.copy()
            for t, word in ((16, "sa_sample .. 1024"), (48, "power of two"), (2048, "power of two"), (0, "power of two")):
                assert call(buf, need, t) == EINVAL and word in _err(E), (form, t, _err(E))
                assert np.array_equal(buf, before), (form, t)
            assert call(buf, need - 1, 64) == EINVAL and "index_bytes too small" in _err(E), _err(E)      # one byte short
            assert np.array_equal(buf, before), form
            assert call(buf, 255, 64) == EINVAL and call(None, need, 64) == EINVAL
            assert np.array_equal(buf, before), form
            # without samples: EUNSUPPORTED, whatever n is
            for B0, p0 in ((B, primary), (np.zeros(0, dtype=np.uint8), 0)):
                plain = E.fm_build(B0, p0, None, 0, bits)
                big = np.zeros(plain.size + 4096, dtype=np.uint8)
                big[:plain.size] = plain
                keep = big.copy()
                assert call(big, big.size, 64) == EUNSUPPORTED and "without SA samples" in _err(E), (form, _err(E))
                assert np.array_equal(big, keep)
            # an unknown version, and then the valid call on the same buffer
            buf[8] = 9
            assert call(buf, need, 64) == EINVAL and "format version" in _err(E)
            buf[8] = 1
            assert call(buf, need, 64) == 0
            _same(buf[:need], X.add_text_samples(R.encode(B, primary, SA, 32, bits // 8), SA, 64), (form, bits))
            assert (buf[need:] == FILL).all()
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        E.fm_add_text_samples(E.fm_build(B, primary, None), 64)
    assert e.value.code == EUNSUPPORTED


def test_refusals_of_extract():
    E = emul()
    n = 1000
    T, SA, B, primary = family_case(E, n, 0)
    for bits in (32, 64):
        v1 = E.fm_build(B, primary, SA, 32, bits)
        v2 = E.fm_add_text_samples(v1, 64)
        text = np.full(4096 + GUARD, FILL, dtype=np.uint8)
        ws_bytes = E.fm_extract_workspace_bytes(4)
        ws = np.zeros(ws_bytes, dtype=np.uint8)
        good_s, good_o = np.array([0, 10, 990, 1000], dtype=np.uint64), np.array([0, 5, 5, 15, 15], dtype=np.uint64)

        def both(blob, starts, off, code, word, nbytes=None, q=None, txt=text, w=ws, wb=ws_bytes):
            q = (off.size - 1 if off is not None else 4) if q is None else q
            nbytes = blob.size if nbytes is None else nbytes
            sp = starts.ctypes.data if starts is not None else None
            op = off.ctypes.data if off is not None else None
            tp = txt.ctypes.data if txt is not None else None
            for rc in (E._f("fm_extract_device")(blob.ctypes.data, nbytes, sp, op, q, tp, w.ctypes.data if w is not None else None, wb, None),
                       E._f("fm_extract")(blob.ctypes.data, nbytes, sp, op, q, tp, 0)):
                assert rc == code and word in _err(E), (bits, word, rc, _err(E))
            assert (text == FILL).all(), word

        both(v1, good_s, good_o, EUNSUPPORTED, "format version 1")
        both(v1, good_s, good_o, EUNSUPPORTED, "format version 1", q=0)
        both(v2, np.array([0, 991], dtype=np.uint64), np.array([0, 5, 15], dtype=np.uint64), EINVAL, "start + length > n")
        both(v2, np.array([1001], dtype=np.uint64), np.array([7, 7], dtype=np.uint64), EINVAL, "start + length > n")
        both(v2, np.array([2**64 - 3, 0], dtype=np.uint64), np.array([0, 5, 6], dtype=np.uint64), EINVAL, "start + length > n")
        both(v2, np.array([2**64 - 1], dtype=np.uint64), np.array([0, 1], dtype=np.uint64), EINVAL, "start + length > n")
        both(v2, good_s, np.array([0, 5, 4, 15, 15], dtype=np.uint64), EINVAL, "not monotone")
        both(v2, None, good_o, EINVAL, "null pointer")
        both(v2, good_s, None, EINVAL, "null pointer")
        both(v2, good_s, good_o, EINVAL, "null pointer", txt=None)
        both(v2, good_s, good_o, EINVAL, "truncated", nbytes=v2.size - 1)
        both(v2, good_s, good_o, EINVAL, "smaller than an FM-index header", nbytes=255)
        assert E._f("fm_extract_device")(v2.ctypes.data, v2.size, good_s.ctypes.data, good_o.ctypes.data, 4, text.ctypes.data, ws.ctypes.data,
                                         ws_bytes - 1, None) == EINVAL and "workspace too small" in _err(E)
        assert E._f("fm_extract_device")(None, v2.size, good_s.ctypes.data, good_o.ctypes.data, 4, text.ctypes.data, None, 0, None) == EINVAL
        for word in (19, 20, 21, 22):                                   # each header word of the section off by one, both ways
            for d in (1, -1):
                bad = v2.copy()
                _hdr(bad)[word] = int(_hdr(v2)[word]) + d
                both(bad, good_s, good_o, EINVAL, "FM-index header")
                for rc in (E._f("fm_count")(bad.ctypes.data, bad.size, None, good_o.ctypes.data, 0, None, None, 0),):
                    assert rc == EINVAL
        for version in (0, 3, 9):
            bad = v2.copy()
            _hdr(bad)[1] = version
            both(bad, good_s, good_o, EINVAL, "format version")
        # q = 0, an all-empty batch (a null text), and the valid call after all of it
        assert E._f("fm_extract_device")(v2.ctypes.data, v2.size, None, None, 0, None, None, 0, None) == 0
        assert E._f("fm_extract")(v2.ctypes.data, v2.size, None, None, 0, None, 0) == 0
        empty_s, empty_o = np.array([0, 500, 1000], dtype=np.uint64), np.array([9, 9, 9, 9], dtype=np.uint64)
        assert E._f("fm_extract_device")(v2.ctypes.data, v2.size, empty_s.ctypes.data, empty_o.ctypes.data, 3, None, None, 0, None) == 0
        assert E._f("fm_extract")(v2.ctypes.data, v2.size, empty_s.ctypes.data, empty_o.ctypes.data, 3, None, 0) == 0
        assert (text == FILL).all()
        assert E._f("fm_extract_device")(v2.ctypes.data, v2.size, good_s.ctypes.data, good_o.ctypes.data, 4, text.ctypes.data, ws.ctypes.data,
                                         ws_bytes, None) == 0
        assert np.array_equal(text[:15], np.concatenate([T[0:5], T[990:1000]])) and (text[15:] == FILL).all()
    out = ctypes.c_uint64(0)
    assert E._f("fm_extract_workspace_bytes")(4, None) == EINVAL and E._f("fm_extract_workspace_bytes")(2**63, ctypes.byref(out)) == EINVAL
    assert E._f("fm_extract_workspace_bytes")(2**22, ctypes.byref(out)) == 0 and out.value <= 8 * (2**22 + 1) + 512


def test_empty_text():
    E = emul()
    empty = np.zeros(0, dtype=np.uint8)
    for s, t in X.DISTANCES:
        for bits in (32, 64):
            want1 = R.encode(empty, 0, np.zeros(0, dtype=np.int64), s, bits // 8)
            want = X.add_text_samples(want1, np.zeros(0, dtype=np.int64), t)
            assert want.size == want1.size and int(_hdr(want)[20]) == 0 and int(_hdr(want)[19]) == t
            v2 = E.fm_add_text_samples(E.fm_build_from_bwt(empty, 0, s, bits), t)
            _same(v2, want, (s, t, bits))
            text, off = E.fm_extract(v2, [0, 0], [0, 0])
            assert text.size == 0 and off.tolist() == [0, 0, 0]
            st, of = np.array([0], dtype=np.uint64), np.array([0, 1], dtype=np.uint64)
            one = np.zeros(8, dtype=np.uint8)
            assert E._f("fm_extract")(v2.ctypes.data, v2.size, st.ctypes.data, of.ctypes.data, 1, one.ctypes.data, 0) == EINVAL
            f, c = E.fm_count(v2, [b"", b"A"])
            assert f.tolist() == [0, 0] and c.tolist() == [0, 0]


# ---- 5. corrupted samples ------------------------------------------------------------------------------------------------------

def test_a_duplicated_sample_is_refused():
    """One sample value overwritten by its neighbour's: a multiple of t is missing, its rowof slot stays empty.  EINVAL, and the
    header still says version 1; from a version-2 blob the header falls back to version 1."""
    E = emul()
    T, SA, B, primary = family_case(E, 4097, 127)
    for bits, dt in ((32, np.uint32), (64, np.uint64)):
        for s, t, victim in ((32, 32, 5), (32, 64, 6), (1, 1, 4000)):
            v1 = E.fm_build(B, primary, SA, s, bits)
            h = _hdr(v1)
            samples = v1[int(h[17]):int(h[17]) + int(h[13]) * (bits // 8)].view(dt)
            k = next(i for i in range(victim, samples.size) if int(samples[i]) % t == 0)     # a sample the section needs
            samples[k] = samples[k - 1]
            need = E.fm_index_bytes_ex(T.size, s, t, bits)
            for form in ("fm_add_text_samples", "fm_add_text_samples_device"):
                buf = np.zeros(need, dtype=np.uint8)
                buf[:v1.size] = v1
                rc = E._f(form)(buf.ctypes.data, need, t, 0 if form == "fm_add_text_samples" else None)
                assert rc == EINVAL and "not an index this library built" in _err(E), (form, _err(E))
                assert np.array_equal(buf[:v1.size], v1), form
            # ... and from a valid version-2 blob whose sample section is then damaged
            v2 = E.fm_add_text_samples(E.fm_build(B, primary, SA, s, bits), t)
            v2[int(h[17]):int(h[17]) + samples.nbytes] = samples.view(np.uint8)
            buf = np.zeros(max(need, v2.size), dtype=np.uint8)
            buf[:v2.size] = v2
            assert E._f("fm_add_text_samples")(buf.ctypes.data, buf.size, t, 0) == EINVAL
            assert int(_hdr(buf)[1]) == 1 and not _hdr(buf)[19:].any()


# ---- 6. corrupted body: a child process, the emulation only -----------------------------------------------------------------------

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
starts = np.array([0, 1, 63, 64, 65, 2000, 4990, 0], dtype=np.uint64)
off = np.zeros(9, dtype=np.uint64)
off[1:] = np.cumsum([5, 64, 2, 129, 0, 700, 10, n])
seen = set()
for bits in (32, 64):
    for s, t in ((1, 1), (32, 64), (32, 1024)):
        v2 = E.fm_add_text_samples(E.fm_build(B, primary, SA, s, bits), t)
        for trial in range(4):
            bad = v2.copy()
            at = rs.randint(256, bad.size, size=1000)
            bad[at] ^= rs.randint(1, 256, size=1000).astype(np.uint8)
            text = np.zeros(int(off[-1]) + 64, dtype=np.uint8)
            rc = E._f("fm_extract")(bad.ctypes.data, bad.size, starts.ctypes.data, off.ctypes.data, 8, text.ctypes.data, 0)
            assert rc in (0, -1), rc
            seen.add(rc)
            rc = E._f("fm_add_text_samples")(bad.ctypes.data, bad.size, t, 0)
            assert rc in (0, -1), rc
            seen.add(rc)
print("done", sorted(seen))
"""


def test_corrupted_body_terminates():
    """1,000 flipped body bytes of a valid version-2 blob, 24 blobs: extract and the upgrade read inside the blob, end, and return
    0 or EINVAL.  In a child process, so that a read outside the blob ends the child and not the suite.  Never on a GPU."""
    emul()
    code = _CHILD % {"tests": os.path.join(ROOT, "tests"), "root": ROOT, "so": os.path.join(EMUL_DIR, "libcaps_sa_emul.so")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("done"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- 7. the other emulation builds ---------------------------------------------------------------------------------------------

@pytest.mark.slow
def test_other_builds_give_the_same_answers():
    """256-element tiles, descending thread order, poison-filled LDS and registers (scattered order) and the barrier-race detector:
    one sweep each (a few sizes, two distances, both widths), and no hand-off reported for the new kernels."""
    from test_emul_inverse_bwt import _load
    poison, _ = _load("libcaps_sa_emul_small_poison.so")
    race, raw = _load("libcaps_sa_emul_small_race.so")
    raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
    raw.caps_sa_emul_races_reset()
    for name, E in (("small", emul_small()), ("rev", emul_rev()), ("poison", poison), ("race", race)):
        done = sweep(E, lambda t: [63, 129, 1025, 4097], distances=((1, 1), (32, 64)), primaries=few_primaries, queries=False)
        assert done == 4 * 3 * 2 * 2, name
    assert int(raw.caps_sa_emul_races_found()) == 0
