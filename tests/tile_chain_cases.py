"""Shared by test_emul_tile_chain.py and test_gpu_tile_chain.py: the shortened start of a tile of the direct path's final sort
(kernels.h tile_sort_kernel CHAIN, pipeline.h segmented_sort / run_direct; CAPS_SA_TILE_CHAIN: bit 0 = the bucket-indexed launch)
against the launch over the tile table and the oracle."""
import re

import numpy as np

DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
STAGES = ("1",)             # the masks of the kept stages, each built beside mask 0
ENV = ("CAPS_SA_DIRECT_MODE", "CAPS_SA_DIRECT_SUB", "CAPS_SA_TEST_SPILL_SLOT", "CAPS_SA_TEST_STREAM_CAP", "CAPS_SA_HOST_WAVES",
       "CAPS_SA_RECORDS", "CAPS_SA_KEYS", "CAPS_SA_PATH", "CAPS_SA_TILE_CHAIN")

_refs = {}


def reference(oracle, key, T, bits=32):
    """The oracle's SA and LCP of a text, computed once per session and shared (never modified)."""
    if key not in _refs:
        SA, LCP = oracle.build_sa_lcp(T, p=64, idx_bits=bits)
        SA.setflags(write=False)
        LCP.setflags(write=False)
        _refs[key] = (SA, LCP)
    return _refs[key]


def uniform(n, letters=DNA):
    return np.random.RandomState(n % 9973).choice(letters, size=n)


def with_repeat(n, length=80, copies=2, seed=3):
    """Uniform text with `copies` copies of one random stretch of `length` bases: the suffixes that start inside them tie on their
    keys (32 bases); whether tile_sort_kernel settles them depends on `length` (its bounded tie-break reads 64 windows of 32 bases) and on
    `copies` (a bin takes 48 elements)."""
    rs = np.random.RandomState(seed)
    T = rs.choice(DNA, size=n)
    rep = rs.choice(DNA, size=length)
    for c in range(copies):
        at = (c * 2 + 1) * n // (2 * copies) + 7 * c
        T[at:at + length] = rep
    return T


def no_kmer(n, kmer, seed=11):
    """Uniform text over ACGT in which the word `kmer` (letter codes) never occurs: every occurrence has its last letter drawn again."""
    rs = np.random.RandomState(seed)
    m = rs.randint(0, 4, size=n)
    k = len(kmer)
    while True:
        hit = np.ones(n - k + 1, dtype=bool)
        for j in range(k):
            hit &= m[j:n - k + 1 + j] == kmer[j]
        idx = np.flatnonzero(hit)
        if idx.size == 0:
            break
        m[idx + k - 1] = rs.randint(0, 4, size=idx.size)
    return DNA[m]


def no_kmer_with_repeat(n, kmer, length=80, copies=64, seed=11):
    """no_kmer(n, kmer) with `copies` copies of one of its own stretches planted as in with_repeat.  The stretch begins and ends
    with T: planting it cuts runs of other letters and joins none, so a `kmer` without T stays absent -- the empty slot stays --
    while the copies crowd the bins of their suffixes (64 in a bin that takes 48), in the buckets before AND behind that slot."""
    assert 3 not in kmer
    T = no_kmer(n, kmer, seed)
    rep = T[n // 3:n // 3 + length].copy()
    rep[0] = rep[-1] = DNA[3]
    for c in range(copies):
        at = (c * 2 + 1) * n // (2 * copies) + 7 * c
        T[at:at + length] = rep
    return T


_LAUNCH = re.compile(r"\[sort\] bucket-indexed launch: (\d+) slots for (\d+) tiles, (\d+) empty slots before the last full one "
                     r"\(slot (\d+), (\d+) elements\), (\d+) buckets below (\d+) elements, (\d+) below (\d+), smallest (\d+)")
_QUEUED = re.compile(r"\[sort\] bucket-indexed launch: (\d+) tiles queued, (\d+) behind an empty slot, (\d+) not tiles of the launch")


def launch_shape(lib, monkeypatch, capfd, T, p=0, **env):
    """One build with the bucket-indexed launch and CAPS_SA_DEBUG=1, which makes the library describe the launch on stderr (pipeline.h
    segmented_sort: the bounds of the buckets and the queue of flagged tiles, read back from the device).  -> what a case relies
    on: slots, tiles, inner_empty (empty slots before the last full one), below_nt / below_early (buckets smaller than ONE early
    load per thread / than all of them: lanes of the early loads lie beyond the bucket), smallest, queued, queued_moved (flagged
    tiles whose tile index is not their slot's number), queued_bad."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("CAPS_SA_" + k, v)
    monkeypatch.setenv("CAPS_SA_TILE_CHAIN", STAGES[-1])
    monkeypatch.setenv("CAPS_SA_DEBUG", "1")
    capfd.readouterr()
    _, _, st = lib.build(T, p=p)
    err = capfd.readouterr().err
    monkeypatch.delenv("CAPS_SA_DEBUG")
    monkeypatch.delenv("CAPS_SA_TILE_CHAIN")
    assert st["tile_chain"] == int(STAGES[-1]), st["tile_chain"]
    a, b = _LAUNCH.findall(err), _QUEUED.findall(err)
    assert len(a) == 1 and len(b) == 1, err[-2000:]
    a, b = [int(x) for x in a[0]], [int(x) for x in b[0]]
    return dict(slots=a[0], tiles=a[1], inner_empty=a[2], last_slot=a[3], last_size=a[4], below_nt=a[5], tile_nt=a[6],
                below_early=a[7], early=a[8], smallest=a[9], queued=b[0], queued_moved=b[1], queued_bad=b[2])


def all_masks(lib, monkeypatch, T, want, bits=32, p=0, taken=True, direct=True, **env):
    """Builds T with CAPS_SA_TILE_CHAIN = 0 and = every mask of STAGES under the given CAPS_SA_* settings: all equal `want` (SA,
    LCP) and each other bit for bit, and the statistic names the mask the final sort ran with -- the one asked for when `taken`
    (the build qualifies for the bucket-indexed launch), 0 otherwise.  -> the statistics of the last build."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("CAPS_SA_" + k, v)
    out = {}
    for mask in ("0",) + STAGES:
        monkeypatch.setenv("CAPS_SA_TILE_CHAIN", mask)
        SA, LCP, st = lib.build(T, p=p, idx_bits=bits)
        assert np.array_equal(SA, want[0]), ("SA", mask, env)
        assert np.array_equal(LCP, want[1]), ("LCP", mask, env)
        if direct is not None:
            assert st["path_direct"] == (1 if direct else 0), (mask, env, st["path_fallback"])
        assert st["tile_chain"] == (int(mask) if taken else 0), (mask, env, st["tile_chain"])
        out[mask] = (SA, LCP, st)
    for mask in STAGES:
        assert np.array_equal(out["0"][0], out[mask][0]) and np.array_equal(out["0"][1], out[mask][1]), (mask, env)
        assert out["0"][2]["path_direct"] == out[mask][2]["path_direct"], (mask, env)
    monkeypatch.delenv("CAPS_SA_TILE_CHAIN")
    # without the variable: the default is the last kept stage
    SA, LCP, st = lib.build(T, p=p, idx_bits=bits)
    assert np.array_equal(SA, want[0]) and np.array_equal(LCP, want[1]), ("default", env)
    assert st["tile_chain"] == (int(STAGES[-1]) if taken else 0), ("default", env, st["tile_chain"])
    return st
