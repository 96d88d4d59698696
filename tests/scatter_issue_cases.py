"""Shared by test_emul_scatter_issue.py and test_gpu_scatter_issue.py: the scatter kernels of the direct path that issue a tile's
memory traffic together (kernels.h bucket_scatter_kernel ISSUE, pipeline.h run_direct; level A's tiles are cases too;
CAPS_SA_SCATTER_ISSUE: bit 0 = level B; bit 1, level A, is read and not built) against the plain kernels and the oracle."""
import re

import numpy as np

from tile_chain_cases import DNA, uniform  # noqa: F401  (the texts of the tile-chain cases serve here too)

KEPT = ("1",)               # the masks of the kept stages, each built beside mask 0 (bit 1, level A, was dropped: DESIGN 5.3)
DEFAULT = 1                 # what a build runs with when the variable is not set
ENV = ("CAPS_SA_DIRECT_MODE", "CAPS_SA_DIRECT_SUB", "CAPS_SA_DIRECT_K1", "CAPS_SA_TEST_SPILL_SLOT", "CAPS_SA_TEST_STREAM_CAP",
       "CAPS_SA_HOST_WAVES", "CAPS_SA_RECORDS", "CAPS_SA_KEYS", "CAPS_SA_PATH", "CAPS_SA_TILE_CHAIN", "CAPS_SA_SCATTER_ISSUE")

_refs = {}


def reference(oracle, key, T, bits=32):
    """The oracle's SA and LCP of a text, computed once per session and shared (never modified)."""
    if key not in _refs:
        SA, LCP = oracle.build_sa_lcp(T, p=64, idx_bits=bits)
        SA.setflags(write=False)
        LCP.setflags(write=False)
        _refs[key] = (SA, LCP)
    return _refs[key]


_INPUT = re.compile(r"\[direct\] level B input: (\d+) streams, (\d+) full tiles, last tiles that end in load((?: \d+: \d+)+) "
                    r"\(tiles of (\d+), (\d+) threads\)")


def level_b_input(lib, monkeypatch, capfd, T, p=0, **env):
    """One build with CAPS_SA_DEBUG=1, which makes the library describe the streams level A handed to level B (pipeline.h
    run_direct, read back from the device).  -> streams, full (full tiles), tails (tails[k] = streams whose last tile ends inside
    the (k + 1)-th load of a thread, i.e. holds k * threads + 1 .. (k + 1) * threads elements), tile, threads."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("CAPS_SA_" + k, v)
    monkeypatch.setenv("CAPS_SA_DEBUG", "1")
    capfd.readouterr()
    lib.build(T, p=p)
    err = capfd.readouterr().err
    monkeypatch.delenv("CAPS_SA_DEBUG")
    m = _INPUT.findall(err)
    assert len(m) == 1, err[-2000:]
    streams, full, tails, tile, threads = m[0]
    tails = [int(x) for x in re.findall(r"\d+: (\d+)", tails)]
    return dict(streams=int(streams), full=int(full), tails=tails, tile=int(tile), threads=int(threads))


def all_masks(lib, monkeypatch, T, want, bits=32, p=0, taken=1, direct=True, **env):
    """Builds T with CAPS_SA_SCATTER_ISSUE = 0 and = every mask of KEPT under the given CAPS_SA_* settings: all equal `want` (SA,
    LCP) and each other bit for bit, and the statistic names the stages the build ran with -- the ones asked for among `taken`
    (a mask: the stages this build has a launch for), 0 where none can be taken.  -> the statistics of the last build."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("CAPS_SA_" + k, v)
    out = {}
    for mask in ("0",) + KEPT:
        monkeypatch.setenv("CAPS_SA_SCATTER_ISSUE", mask)
        SA, LCP, st = lib.build(T, p=p, idx_bits=bits)
        assert np.array_equal(SA, want[0]), ("SA", mask, env)
        assert np.array_equal(LCP, want[1]), ("LCP", mask, env)
        if direct is not None:
            assert st["path_direct"] == (1 if direct else 0), (mask, env, st["path_fallback"])
        assert st["scatter_issue"] == (int(mask) & taken), (mask, env, st["scatter_issue"])
        out[mask] = (SA, LCP, st)
    for mask in KEPT:
        assert np.array_equal(out["0"][0], out[mask][0]) and np.array_equal(out["0"][1], out[mask][1]), (mask, env)
        assert out["0"][2]["path_direct"] == out[mask][2]["path_direct"], (mask, env)
    monkeypatch.delenv("CAPS_SA_SCATTER_ISSUE")
    # without the variable: the default
    SA, LCP, st = lib.build(T, p=p, idx_bits=bits)
    assert np.array_equal(SA, want[0]) and np.array_equal(LCP, want[1]), ("default", env)
    assert st["scatter_issue"] == (DEFAULT & taken), ("default", env, st["scatter_issue"])
    return st
