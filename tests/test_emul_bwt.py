"""CPU: the Burrows-Wheeler transform output (include/caps_sa_hip.h caps_sa_hip_build_bwt_* / caps_sa_hip_bwt_device_*) through the
host emulation of the kernels (tests/emul), against np.where on the oracle's SA or on a golden SA:
BWT[k] = T[(SA[k] + n - 1) mod n], primary = the k with SA[k] == 0."""
import ctypes

import numpy as np
import pytest

from conftest import LARGE_GOLDEN, large_golden, text_bytes
from emul_util import emul, emul_small

DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
NONE = (1 << 64) - 1


def _expect(T, SA):
    """(BWT, primary) from a suffix array by np.where -- the definition, independent of the library."""
    SA = np.asarray(SA).astype(np.int64)
    n = T.size
    bwt = T[np.where(SA == 0, n - 1, SA - 1)] if n else np.zeros(0, dtype=np.uint8)
    zero = np.where(SA == 0)[0]
    return bwt, (int(zero[0]) if zero.size else NONE)


def _check(E, T, SAo, LCPo=None, **kw):
    SA, LCP, BWT, primary, st = E.build_bwt(T, **kw)
    assert np.array_equal(SA, SAo)
    if LCPo is not None:
        assert np.array_equal(LCP, LCPo)
    bwt, pr = _expect(T, SAo)
    assert BWT.dtype == np.uint8 and np.array_equal(BWT, bwt)
    assert primary == pr
    return st


def _lf_invert(bwt: np.ndarray, primary: int) -> np.ndarray:
    """T back from (BWT, primary) by an LF walk over L = BWT[primary], BWT[0 .. primary), '$', BWT[primary + 1 .. n): the last
    column of the sorted rotations of T$, bytes in signed-char order, $ below every byte."""
    n = bwt.size
    L = np.concatenate([bwt[primary:primary + 1], bwt[:primary], np.zeros(1, dtype=np.uint8), bwt[primary + 1:]])
    key = (L ^ 0x80).astype(np.int32)                 # signed char order as unsigned keys
    key[primary + 1] = -1                             # '$'
    order = np.argsort(key, kind="stable")
    LF = np.empty(n + 1, dtype=np.int64)
    LF[order] = np.arange(n + 1)
    out = np.empty(n, dtype=np.uint8)
    i = 0                                             # row 0 is $T: its last char is T[n - 1]
    for j in range(n - 1, -1, -1):
        out[j] = L[i]
        i = LF[i]
    return out


def test_golden_cases(golden_cases):
    E = emul()
    for c in golden_cases:
        T = text_bytes(c["text"])
        for p in (0, 2):
            _check(E, T, np.array(c["sa"]), np.array(c["lcp"]), p=p)


@pytest.mark.parametrize("name", LARGE_GOLDEN)
def test_large_golden_cases(name, monkeypatch):
    """The default construction (direct path); latin1_signed_136k pins bytes >= 0x80 in the BWT."""
    monkeypatch.delenv("CAPS_SA_PATH", raising=False)
    T, sa, lcp = large_golden(name)
    st = _check(emul(), T, sa, lcp)
    assert st["path_direct"] == 1
    if name == "latin1_signed_136k":
        assert (T >= 0x80).any() and (_expect(T, sa)[0] >= 0x80).any()


@pytest.mark.parametrize("n", [1, 2, 3, 31, 4097, 70_001])
def test_random_dna_both_constructions(oracle, sa_path, n):
    rs = np.random.RandomState(n)
    T = rs.choice(DNA, size=n)
    SAo, LCPo = oracle.naive_sa_lcp(T)
    _check(emul(), T, SAo, LCPo)


def test_index_widths_and_small_tiles(oracle):
    rs = np.random.RandomState(12)
    T = rs.choice(DNA, size=90_001)
    for bits in (32, 64):
        SAo, LCPo = oracle.naive_sa_lcp(T, idx_bits=bits)
        _check(emul(), T, SAo, LCPo, idx_bits=bits)
        _check(emul_small(), T, SAo, LCPo, idx_bits=bits)
    B = rs.randint(0, 256, size=30_000).astype(np.uint8)          # the byte alphabet (8-bit codes)
    SAo, _ = oracle.naive_sa_lcp(B)
    _check(emul_small(), B, SAo)


def test_empty_text():
    SA, LCP, BWT, primary, _ = emul().build_bwt(np.zeros(0, dtype=np.uint8))
    assert SA.size == LCP.size == BWT.size == 0 and primary == NONE


def test_host_path_in_waves(oracle, monkeypatch):
    """The BWT leaves the device slice by slice (HostCopySink::wave_done) with SA and LCP."""
    E = emul_small()
    rs = np.random.RandomState(31)
    T = rs.choice(DNA, size=200_000)
    SAo, LCPo = oracle.build_sa_lcp(T, p=64)
    for waves in ("3", "1"):
        monkeypatch.setenv("CAPS_SA_HOST_WAVES", waves)
        st = _check(E, T, SAo, LCPo)
        assert st["path_direct"] == 1
        if waves == "3":
            assert st["result_waves"] >= 2, st["result_waves"]
    monkeypatch.setenv("CAPS_SA_PATH", "classic")                  # nothing streamed: one gather over the whole SA after the build
    monkeypatch.setenv("CAPS_SA_HOST_WAVES", "3")
    st = _check(E, T, SAo, LCPo)
    assert st["result_waves"] == 1


def _tandem(rs, T, at, unit_len, copies, rate):
    seg = np.tile(rs.choice(DNA, size=unit_len), copies)
    m = rs.rand(seg.size) < rate
    seg[m] = rs.choice(DNA, size=int(m.sum()))
    T[at:at + seg.size] = seg


def test_host_path_restart_rewrites_the_bwt(monkeypatch):
    """A build that starts over (the deferred ties do not fit: CAPS_SA_TEST_MSD_FAIL) after slices have gone out: the BWT copied so
    far is rewritten and primary re-armed.  tie_groups_deferred == 0 shows the restart happened (it is > 0 without the variable)."""
    from sa_check import sa_lcp
    E = emul_small()
    rs = np.random.RandomState(71)
    T = rs.choice(DNA, size=120_000)
    _tandem(rs, T, 40_000, 23, 700, 0.003)
    SAo, LCPo = sa_lcp(T)
    monkeypatch.setenv("CAPS_SA_HOST_WAVES", "3")
    st = _check(E, T, SAo, LCPo)
    assert st["path_direct"] == 1 and st["tie_groups_deferred"] > 0
    monkeypatch.setenv("CAPS_SA_TEST_MSD_FAIL", "1")
    st = _check(E, T, SAo, LCPo)
    assert st["path_direct"] == 1 and st["tie_groups_deferred"] == 0


def test_bwt_device_on_slices(oracle):
    """bwt_device over slices of an SA (the emulation's device memory is host memory): first > 0, with and without rank 0, cnt = 0;
    the slices agree with the full-array call."""
    E = emul()
    rs = np.random.RandomState(5)
    T = rs.choice(DNA, size=50_003)
    n = T.size
    for bits, dt in ((32, np.uint32), (64, np.uint64)):
        SA = np.ascontiguousarray(oracle.naive_sa_lcp(T, idx_bits=bits)[0], dtype=dt)
        bwt, pr = _expect(T, SA)
        full = np.empty(n, dtype=np.uint8)
        assert E.bwt_device(T.ctypes.data, n, SA.ctypes.data, 0, n, full.ctypes.data, idx_bits=bits) == pr
        assert np.array_equal(full, bwt)
        lo = max(0, pr - 17)
        for first, cnt in ((lo, min(4_000, n - lo)), (pr + 1, n - pr - 1), (3, 17), (n - 5, 5), (1000, 0), (pr, 1), (0, pr)):
            out = np.full(max(cnt, 1), 0xEE, dtype=np.uint8)
            got = E.bwt_device(T.ctypes.data, n, SA[first:].ctypes.data, first, cnt, out.ctypes.data, idx_bits=bits)
            assert np.array_equal(out[:cnt], full[first:first + cnt]), (bits, first, cnt)
            assert got == (pr if first <= pr < first + cnt else NONE), (bits, first, cnt, got)


def test_lf_walk_inverts_the_bwt():
    """Independent of any SA: the BWT and primary alone give T back (the convention of include/caps_sa_hip.h)."""
    E = emul()
    rs = np.random.RandomState(9)
    for T in (rs.choice(DNA, size=100_000), rs.randint(0, 256, size=20_000).astype(np.uint8), text_bytes("mississippi"),
              text_bytes("a" * 500), text_bytes("\x80\xff\x00\x7f" * 50 + "x")):
        _, _, BWT, primary, _ = E.build_bwt(T)
        assert np.array_equal(_lf_invert(BWT, primary), T)


def test_errors():
    import caps_sa_amd
    E = emul()
    T = np.frombuffer(b"ACGTTGCA" * 125, dtype=np.uint8)
    n = T.size
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        E.build_bwt(T, max_context=5)                                # a bounded-context order has no BWT
    assert e.value.code == -2
    SA = np.empty(n, dtype=np.uint32)
    LCP = np.empty(n, dtype=np.uint32)
    primary = ctypes.c_uint64(0)
    st = caps_sa_amd.Stats()
    rc = E._f("build_bwt_u32")(T.ctypes.data, n, 0, 0, SA.ctypes.data, LCP.ctypes.data, None, ctypes.byref(primary), 0, ctypes.byref(st))
    assert rc == -1                                                  # null BWT
    BWT = np.empty(n, dtype=np.uint8)
    rc = E._f("build_bwt_u32")(T.ctypes.data, n, 0, 0, SA.ctypes.data, LCP.ctypes.data, BWT.ctypes.data, None, 0, ctypes.byref(st))
    assert rc == -1                                                  # null primary
    SA, _, _, _, _ = E.build_bwt(T)
    out = np.empty(n, dtype=np.uint8)
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        E.bwt_device(T.ctypes.data, n, SA[n - 5:].ctypes.data, n - 5, 10, out.ctypes.data)    # first + cnt > n
    assert e.value.code == -1
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        E.bwt_device(T.ctypes.data, n, SA.ctypes.data, 0, n, 0)       # null dBWT
    assert e.value.code == -1
    with pytest.raises(ValueError):
        caps_sa_amd.SuffixArray(T, bwt=True, devices=[0, 0])
    sa = caps_sa_amd.SuffixArray(T, bwt=True)
    with pytest.raises(RuntimeError):
        sa.BWT()
    with pytest.raises(RuntimeError):
        sa.primary()
    with pytest.raises(RuntimeError):                                # not asked for
        caps_sa_amd.SuffixArray(T).BWT()
