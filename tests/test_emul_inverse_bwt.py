"""CPU: the inverse Burrows-Wheeler transform (include/caps_sa_hip.h caps_sa_hip_inverse_bwt_*) through the host emulation of the
kernels (tests/emul): (BWT, primary) from E.build_bwt back to T, against T itself and _lf_invert of test_emul_bwt.py; inputs that
are not the BWT of any text; argument errors; the same bytes from the small-tile, reversed-order, poison and race builds.

Ranking levels (kernels.h: a splitter every 64 rows, every 64 nodes of a list above that, a list of at most 256 nodes ranked in
one workgroup): n < 16,384 ranks the splitters of the LF walk directly in the top workgroup; 16,384 <= n < 1,048,576 (70,001,
the large fixtures) adds one list level; n >= 1,048,576 (1,100,000 below) adds a second."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import LARGE_GOLDEN, large_golden, text_bytes
from emul_util import EMUL_DIR, emul, emul_rev, emul_small
from test_emul_bwt import _lf_invert

DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
EINVAL = -1


def _bwt(E, T, bits=32):
    _, _, B, primary, _ = E.build_bwt(T, idx_bits=bits)
    return B, primary


def _round_trip(E, T, widths=(32, 64)):
    B, primary = _bwt(E, T)
    for bits in widths:
        out = E.inverse_bwt(B, primary, idx_bits=bits)
        assert out.dtype == np.uint8 and np.array_equal(out, T), (T.size, bits)
    return B, primary


def test_golden_cases(golden_cases):
    E = emul()
    for c in golden_cases:
        T = text_bytes(c["text"])
        if T.size:
            _round_trip(E, T)


@pytest.mark.parametrize("name", LARGE_GOLDEN)
def test_large_golden_cases(name):
    """Both index widths of the build give the same (BWT, primary), and both widths of the inverse give T back; latin1_signed_136k
    pins bytes >= 0x80."""
    E = emul()
    T, _, _ = large_golden(name)
    B, primary = _round_trip(E, T)
    B64, primary64 = _bwt(E, T, 64)
    assert np.array_equal(B, B64) and primary == primary64
    if name == "latin1_signed_136k":
        assert (B >= 0x80).any()


@pytest.mark.parametrize("n", [1, 2, 3, 31, 4097, 70_001, 1_100_000])
def test_random_dna(n):
    rs = np.random.RandomState(n)
    T = rs.choice(DNA, size=n)
    B, primary = _round_trip(emul(), T, widths=(32, 64) if n < 1_000_000 else (32,))
    if n <= 4097:
        assert np.array_equal(_lf_invert(B, primary), T)


def test_other_texts():
    E = emul()
    rs = np.random.RandomState(3)
    T = rs.choice(DNA, size=60_000)
    for _ in range(4):                                                   # planted repeats
        ln = int(rs.randint(500, 6000))
        a, b = rs.randint(0, T.size - ln, size=2)
        T[b:b + ln] = T[a:a + ln]
    texts = [
        rs.randint(0, 256, size=50_000).astype(np.uint8),              # every byte value
        np.arange(256, dtype=np.uint8),
        text_bytes("a" * 40_000),
        np.tile(DNA, 9_000),                                           # (ACGT)^k
        np.tile(rs.choice(DNA, size=171), 200),                        # a tandem repeat
        T,
        text_bytes("mississippi"),
    ]
    for T in texts:
        _round_trip(E, T)


def test_every_short_pair_over_two_letters():
    """n = 1 .. 8 over {A, C}: of the n * 2^n pairs (BWT, primary) exactly 2^n invert, each to a text whose build_bwt is that pair;
    every other pair is refused with EINVAL."""
    import caps_sa_amd
    E = emul()
    for n in range(1, 9):
        ok = 0
        for letters in itertools.product(b"AC", repeat=n):
            B = np.array(letters, dtype=np.uint8)
            for primary in range(n):
                try:
                    T = E.inverse_bwt(B, primary)
                except caps_sa_amd.CapsSaError as e:
                    assert e.code == EINVAL
                    assert "not the BWT" in str(e)
                    continue
                ok += 1
                B2, p2 = _bwt(E, T)
                assert np.array_equal(B2, B) and p2 == primary, (bytes(B), primary, bytes(T))
        assert ok == 2 ** n, (n, ok)


def test_not_a_bwt():
    import caps_sa_amd
    E = emul()
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        E.inverse_bwt(b"aa", 0)
    assert e.value.code == EINVAL and "not the BWT" in str(e.value)
    rs = np.random.RandomState(17)
    B = rs.randint(0, 256, size=1 << 16).astype(np.uint8)
    primary = int(rs.randint(0, B.size))
    try:
        T = E.inverse_bwt(B, primary)
    except caps_sa_amd.CapsSaError as e:
        assert e.code == EINVAL
    else:                                                              # (1 pair in n is a BWT)
        B2, p2 = _bwt(E, T)
        assert np.array_equal(B2, B) and p2 == primary
    T = rs.choice(DNA, size=5000)                                      # a valid call afterwards still works
    _round_trip(E, T)


def test_errors():
    E = emul()
    T = np.frombuffer(b"ACGTTGCA" * 125, dtype=np.uint8)
    B, primary = _bwt(E, T)
    n = B.size
    out = np.empty(n, dtype=np.uint8)
    for sfx in ("u32", "u64"):
        f = E._f(f"inverse_bwt_{sfx}")
        assert f(None, n, primary, out.ctypes.data, 0) == EINVAL                  # null BWT
        assert f(B.ctypes.data, n, primary, None, 0) == EINVAL                    # null T
        assert f(B.ctypes.data, n, n, out.ctypes.data, 0) == EINVAL               # primary >= n
        assert f(B.ctypes.data, n, n + 7, out.ctypes.data, 0) == EINVAL
        assert f(None, 0, 12345, None, 0) == 0                                    # n = 0: nothing read, primary not looked at
        assert f(B.ctypes.data, n, primary, out.ctypes.data, 0) == 0 and np.array_equal(out, T)
        bits = 32 if sfx == "u32" else 64
        ws_bytes = E.inverse_bwt_workspace_bytes(n, bits)
        ws = np.zeros(ws_bytes, dtype=np.uint8)
        dev = E._f(f"inverse_bwt_device_{sfx}")
        out[:] = 0
        assert dev(B.ctypes.data, n, primary, out.ctypes.data, ws.ctypes.data, ws_bytes - 1, None) == EINVAL   # one byte short
        assert dev(B.ctypes.data, n, primary, out.ctypes.data, None, ws_bytes, None) == EINVAL
        assert dev(None, 0, 99, None, None, 0, None) == 0
        E.inverse_bwt_device(B.ctypes.data, n, primary, out.ctypes.data, ws.ctypes.data, ws_bytes, idx_bits=bits)
        assert np.array_equal(out, T)
    # _u32 with n > UINT32_MAX: refused before anything is allocated or read (the buffers here are 1000 bytes)
    big = (1 << 32) + 5
    assert E._f("inverse_bwt_u32")(B.ctypes.data, big, 0, out.ctypes.data, 0) == EINVAL
    assert E._f("inverse_bwt_device_u32")(B.ctypes.data, big, 0, out.ctypes.data, out.ctypes.data, 1 << 62, None) == EINVAL
    wb = ctypes.c_uint64(0)
    assert E._f("inverse_bwt_workspace_bytes")(big, 4, ctypes.byref(wb)) == EINVAL
    assert E._f("inverse_bwt_workspace_bytes")(big, 8, ctypes.byref(wb)) == 0 and wb.value > big * 8
    assert E._f("inverse_bwt_workspace_bytes")(100, 3, ctypes.byref(wb)) == EINVAL
    assert E._f("inverse_bwt_workspace_bytes")(100, 4, None) == EINVAL


def _load(name):
    import caps_sa_amd
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, name])
    path = os.path.join(EMUL_DIR, name)
    return caps_sa_amd.CapsLib(path, "caps_sa_emul_"), ctypes.CDLL(path)


@pytest.mark.slow
def test_other_builds_give_the_same_bytes():
    """Small tiles, descending thread order, poison-filled LDS and registers (scattered order), and the barrier-race detector:
    the same T, and no race in any LDS hand-off of the new kernels."""
    rs = np.random.RandomState(23)
    T1 = rs.choice(DNA, size=40_000)
    T1[10_000:18_000] = np.tile(rs.choice(DNA, size=40), 200)
    texts = [T1, rs.randint(0, 256, size=20_000).astype(np.uint8), text_bytes("a" * 17_000)]
    pairs = [_bwt(emul(), T) for T in texts]
    poison, _ = _load("libcaps_sa_emul_small_poison.so")
    race, raw = _load("libcaps_sa_emul_small_race.so")
    raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
    raw.caps_sa_emul_races_reset()
    for E in (emul_small(), emul_rev(True), emul_rev(False), poison, race):
        for T, (B, primary) in zip(texts, pairs):
            for bits in (32, 64):
                assert np.array_equal(E.inverse_bwt(B, primary, idx_bits=bits), T)
    assert int(raw.caps_sa_emul_races_found()) == 0
