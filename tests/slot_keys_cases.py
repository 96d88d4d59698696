"""Shared by test_emul_slot_keys.py and test_gpu_slot_keys.py: level B of the direct path handing the tile sort 8-byte records of
bucket-relative 32-bit keys (kernels.h "slot keys", bucket_scatter_kernel SLOT32, tile_sort_kernel SLOTREC; pipeline.h
segmented_sort / run_direct; CAPS_SA_SLOT_KEYS: bit 0 = the records; bit 1, the sort itself on 32 bits, is read and not built)
against the two-array slots of 64-bit keys and the oracle.  Everything is compared bit for bit."""
import re

import numpy as np

from slot_keys_model import bucket_of, make_bucket_params, slot_key_shift
from tile_chain_cases import DNA, no_kmer, no_kmer_with_repeat, uniform, with_repeat  # noqa: F401  (the tile-chain texts serve here too)

KEPT = ("1",)               # the masks of the kept stages, each built beside mask 0
DEFAULT = 1                 # what a build runs with when the variable is not set
ENV = ("CAPS_SA_DIRECT_MODE", "CAPS_SA_DIRECT_SUB", "CAPS_SA_DIRECT_K1", "CAPS_SA_TEST_SPILL_SLOT", "CAPS_SA_TEST_STREAM_CAP",
       "CAPS_SA_HOST_WAVES", "CAPS_SA_RECORDS", "CAPS_SA_KEYS", "CAPS_SA_PATH", "CAPS_SA_TILE_CHAIN", "CAPS_SA_SCATTER_ISSUE",
       "CAPS_SA_SLOT_KEYS")

_refs = {}


def reference(oracle, key, T, bits=32):
    """The oracle's SA and LCP of a text, computed once per session and shared (never modified)."""
    if key not in _refs:
        SA, LCP = oracle.build_sa_lcp(T, p=64, idx_bits=bits)
        SA.setflags(write=False)
        LCP.setflags(write=False)
        _refs[key] = (SA, LCP)
    return _refs[key]


def ends_inside_a_copy(n, seed=21):
    """Uniform text with a 60-base stretch planted in its middle -- 30 random bases, nine A (the lowest letter: what the key of a
    suffix is padded with beyond the end of the text), 21 random bases -- whose first 30 bases are also the END of the text.  The
    suffix of the last 30 bases (longer than the chars a slot key stands for, shorter than a key) and the suffix of the last 10
    (shorter than either; its padded key reads like the planted bases 20 .. 38) tie on their slot keys with the longer suffixes
    in the middle."""
    rs = np.random.RandomState(seed)
    T = rs.choice(DNA, size=n)
    rep = np.concatenate([rs.choice(DNA, size=30), np.repeat(DNA[0], 9), rs.choice(DNA, size=21)])
    T[n // 2:n // 2 + 60] = rep
    T[n - 30:] = rep[:30]
    return T


def tail_repeats_head(n, seed=22):
    """Uniform text whose last 40 bases repeat its first 40."""
    T = np.random.RandomState(seed).choice(DNA, size=n)
    T[n - 40:] = T[:40]
    return T


_SLOT_KEYS = re.compile(r"\[sort\] slot keys: shifts (\d+) \.\. (\d+), (\d+) of (\d+) buckets whose window wraps, (\d+) neighbour pairs "
                        r"with equal slot keys, (\d+) bucket heads tied with the element before them")
_MAP = re.compile(r"\[sort\] slot keys: group map kmin (\d+) kmax (\d+) B (\d+) first bucket (\d+)")
_QUEUED = re.compile(r"\[sort\] bucket-indexed launch: (\d+) tiles queued, (\d+) behind an empty slot, (\d+) not tiles of the launch")
_LAUNCH = re.compile(r"\[sort\] bucket-indexed launch: (\d+) slots for (\d+) tiles, (\d+) empty slots before the last full one "
                     r"\(slot (\d+), (\d+) elements\), (\d+) buckets below (\d+) elements, (\d+) below (\d+), smallest (\d+)")


def slot_keys_shape(lib, monkeypatch, capfd, T, p=0, **env):
    """One build with the last kept mask and CAPS_SA_DEBUG=1, which makes the library describe its slot keys on stderr (pipeline.h
    segmented_sort, read back from the device).  -> smin / smax (the shifts of the non-empty buckets), wraps (buckets whose key
    range straddles a multiple of the window 2^(32 + shift)), buckets, ties (neighbours of the result inside a bucket with equal
    slot keys), head_ties (bucket heads tied with the last element of the bucket below), queued (tiles the plain kernel passed
    on), inner_empty / below_early (empty slots between full ones, buckets that end inside the early loads), maps (the groups'
    linear maps: kmin, kmax, B, first bucket)."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("CAPS_SA_" + k, v)
    monkeypatch.setenv("CAPS_SA_SLOT_KEYS", KEPT[-1])
    monkeypatch.setenv("CAPS_SA_DEBUG", "1")
    capfd.readouterr()
    _, _, st = lib.build(T, p=p)
    err = capfd.readouterr().err
    monkeypatch.delenv("CAPS_SA_DEBUG")
    monkeypatch.delenv("CAPS_SA_SLOT_KEYS")
    assert st["slot_keys"] == int(KEPT[-1]) and st["tile_chain"] == 1 and st["scatter_issue"] == 1, st
    a, b, c = _SLOT_KEYS.findall(err), _QUEUED.findall(err), _LAUNCH.findall(err)
    assert len(a) == 1 and len(b) == 1 and len(c) == 1, err[-2000:]
    a, c = [int(x) for x in a[0]], [int(x) for x in c[0]]
    maps = [tuple(int(x) for x in m) for m in _MAP.findall(err)]
    return dict(smin=a[0], smax=a[1], wraps=a[2], buckets=a[3], ties=a[4], head_ties=a[5], queued=int(b[0][0]), inner_empty=c[2],
                below_early=c[7], maps=maps)


def all_masks(lib, monkeypatch, T, want, bits=32, p=0, taken=True, direct=True, **env):
    """Builds T with CAPS_SA_SLOT_KEYS = 0 and = every mask of KEPT under the given CAPS_SA_* settings, and without the variable:
    all equal `want` (SA, LCP) and each other bit for bit, and the statistic names the mask the final sort ran with -- the one
    asked for when `taken` (the build qualifies), 0 otherwise.  -> the statistics of the last build."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("CAPS_SA_" + k, v)
    out = {}
    for mask in ("0",) + KEPT:
        monkeypatch.setenv("CAPS_SA_SLOT_KEYS", mask)
        SA, LCP, st = lib.build(T, p=p, idx_bits=bits)
        assert np.array_equal(SA, want[0]), ("SA", mask, env)
        assert np.array_equal(LCP, want[1]), ("LCP", mask, env)
        if direct is not None:
            assert st["path_direct"] == (1 if direct else 0), (mask, env, st["path_fallback"])
        assert st["slot_keys"] == (int(mask) if taken else 0), (mask, env, st["slot_keys"])
        out[mask] = (SA, LCP, st)
    for mask in KEPT:
        assert np.array_equal(out["0"][0], out[mask][0]) and np.array_equal(out["0"][1], out[mask][1]), (mask, env)
        assert out["0"][2]["path_direct"] == out[mask][2]["path_direct"], (mask, env)
        # the rest of the route is the same: the records change what the slots hold, not which kernels run
        for k in ("tile_chain", "scatter_issue", "direct_records", "slot_splits", "slot_splits_redone", "direct_quantile"):
            assert out["0"][2][k] == out[mask][2][k], (k, mask, env)
    monkeypatch.delenv("CAPS_SA_SLOT_KEYS")
    SA, LCP, st = lib.build(T, p=p, idx_bits=bits)
    assert np.array_equal(SA, want[0]) and np.array_equal(LCP, want[1]), ("default", env)
    assert st["slot_keys"] == (DEFAULT if taken else 0), ("default", env, st["slot_keys"])
    return st


def _edge(bp, b):
    """Smallest key that bucket_of sends to bucket b or above (b >= 1): the true edge between the buckets b - 1 and b."""
    lo, hi = bp["kmin"], bp["kmin"] + bp["range"]             # bucket_of(lo) = 0 < b <= bucket_of(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if bucket_of(bp, mid) >= b:
            hi = mid
        else:
            lo = mid
    return hi


def _bases(key):
    return DNA[[(key >> (62 - 2 * i)) & 3 for i in range(32)]]


def tie_across_a_boundary(lib, monkeypatch, capfd, n=1_000_003, p=20, seed=23, first=0):
    """A uniform text with two planted 32-base words whose keys are the last key of one bucket and the first key of the next and
    agree above the group's shift: a tie on the slot keys ACROSS a bucket boundary.  The edge comes from the library's own
    description of its groups' maps on the text without the words (slot_keys_shape), followed through the copy of bucket_of in
    slot_keys_model.py.  Planting moves the pivots -- and with them the maps -- when a sampled suffix reads the planted bases,
    so the pair is planted at one place after the other until the library reports the tie (fixed seeds: the same places every
    time; `first` = the place to begin with).  -> (text, shape of the build that reported the tie, the two positions)."""
    T0 = np.random.RandomState(seed).choice(DNA, size=n)
    sh = slot_keys_shape(lib, monkeypatch, capfd, T0, p=p)
    assert sh["head_ties"] == 0 and sh["maps"], sh
    kmin, kmax, B, _first = sh["maps"][len(sh["maps"]) // 2]
    bp = make_bucket_params(kmin, kmax, B)
    s = slot_key_shift(bp["range"], B)
    for b in range(B // 2, B):
        E = _edge(bp, b)
        if (E - 1) >> s == E >> s and bucket_of(bp, E - 1) == b - 1 and bucket_of(bp, E) == b:
            break
    else:
        raise AssertionError("no bucket edge inside an aligned block of slot keys")
    for j in range(first, first + 24):
        at = (n // 3 + 5 + 97 * j, 2 * n // 3 + 11 + 89 * j)
        T = T0.copy()
        T[at[0]:at[0] + 32] = _bases(E - 1)
        T[at[1]:at[1] + 32] = _bases(E)
        sh = slot_keys_shape(lib, monkeypatch, capfd, T, p=p)
        if sh["head_ties"] >= 1:
            return T, sh, at
    raise AssertionError(("the planted tie did not land on a bucket boundary", sh))
