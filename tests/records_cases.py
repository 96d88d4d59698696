"""Shared by test_emul_records.py and test_gpu_records.py: the direct path with 12-byte (key, index) records between its passes
(kernels.h KeySaRec, pipeline.h run_direct; CAPS_SA_RECORDS: bit 0 = level A -> level B, the one hand-over that ships as records)
against the two-array layout and the oracle."""
import numpy as np

DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
RECORDS_ON = "1"            # the mask of the hand-overs that ship as records
ENV = ("CAPS_SA_DIRECT_MODE", "CAPS_SA_DIRECT_SUB", "CAPS_SA_TEST_SPILL_SLOT", "CAPS_SA_TEST_STREAM_CAP", "CAPS_SA_HOST_WAVES",
       "CAPS_SA_RECORDS", "CAPS_SA_KEYS", "CAPS_SA_PATH")

_refs = {}


def reference(oracle, key, T, bits=32):
    """The oracle's SA and LCP of a text, computed once per session and shared (never modified)."""
    if key not in _refs:
        SA, LCP = oracle.build_sa_lcp(T, p=64, idx_bits=bits)
        SA.setflags(write=False)
        LCP.setflags(write=False)
        _refs[key] = (SA, LCP)
    return _refs[key]


def markov(rs, n, order=3, skew=0.3):
    """The skewed text of test_emul_pipeline.py test_direct_path_modes_and_fallbacks (same generator, same seed there: 5)."""
    trans = rs.dirichlet([skew] * 4, size=4 ** order)
    cdf = np.cumsum(trans, 1)
    m = np.zeros(n, dtype=np.int64)
    u = rs.rand(n)
    st = 0
    for i in range(n):
        c = min(3, int(np.searchsorted(cdf[st], u[i])))
        m[i] = c
        st = (st * 4 + c) % (4 ** order)
    return DNA[m]


def both_layouts(lib, monkeypatch, T, want, bits=32, p=0, direct=True, **env):
    """Builds T with CAPS_SA_RECORDS = 0 and = RECORDS_ON under the given CAPS_SA_* settings: both equal `want` (SA, LCP) and each
    other bit for bit, and the statistic names the layout each build used.  direct: the path the builds must take (None: either,
    the same for both).  -> the statistics of the records build."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("CAPS_SA_" + k, v)
    out = {}
    for mask in ("0", RECORDS_ON):
        monkeypatch.setenv("CAPS_SA_RECORDS", mask)
        SA, LCP, st = lib.build(T, p=p, idx_bits=bits)
        assert np.array_equal(SA, want[0]), ("SA", mask, env)
        assert np.array_equal(LCP, want[1]), ("LCP", mask, env)
        if direct is not None:
            assert st["path_direct"] == (1 if direct else 0), (mask, env, st["path_fallback"])
        # records: 32-bit indices on the direct path; 64-bit indices stay on two arrays
        expect = int(mask) if st["path_direct"] and bits == 32 else 0
        assert st["direct_records"] == expect, (mask, env, st["direct_records"])
        out[mask] = (SA, LCP, st)
    assert np.array_equal(out["0"][0], out[RECORDS_ON][0]) and np.array_equal(out["0"][1], out[RECORDS_ON][1]), env
    assert out["0"][2]["path_direct"] == out[RECORDS_ON][2]["path_direct"], env
    monkeypatch.delenv("CAPS_SA_RECORDS")
    return out[RECORDS_ON][2]
