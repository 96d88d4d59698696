"""CPU: slot keys -- level B of the direct path handing the tile sort 8-byte records of bucket-relative 32-bit keys (kernels.h "slot
keys", CAPS_SA_SLOT_KEYS) -- through the host emulation of the kernels.  Every case is built with today's two-array slots (mask 0),
with every kept mask and without the variable: equal to the oracle, equal to each other, and the statistic names the mask the
final sort ran with.  Each case asserts the corner it is there for from the library's own description of its slot keys
(slot_keys_cases.slot_keys_shape).

The records exist only in a linear slot split that is KEPT, which the 256-element-tile build never has (test_emul_tile_chain.py):
the cases run on the 4096-element-tile build, on texts of a million bases; the small-tile build serves the redone split."""
import os
import subprocess

import numpy as np
import pytest

from emul_util import EMUL_DIR, emul, emul_rev, emul_small
from records_cases import markov
from slot_keys_cases import (DNA, all_masks, ends_inside_a_copy, no_kmer, no_kmer_with_repeat, reference, slot_keys_shape,
                             tail_repeats_head, tie_across_a_boundary, uniform, with_repeat)

TIE_FROM = 19               # (64 - 26) / 2: the chars a slot key stands for at a million bases in 20 groups


@pytest.mark.parametrize("n,p", [(1_000_003, 20), (1_100_001, 20), (1_200_007, 300)])
def test_uniform_text_and_odd_bucket_counts(oracle, monkeypatch, capfd, n, p):
    T = uniform(n)
    sh = slot_keys_shape(emul(), monkeypatch, capfd, T, p=p)
    assert sh["wraps"] >= 1 and sh["queued"] == 0 and sh["smin"] >= 20 and (64 - sh["smax"]) // 2 >= 16, sh
    st = all_masks(emul(), monkeypatch, T, reference(oracle, ("uni", n), T), p=p)
    assert st["direct_quantile"] == 0 and st["slot_splits"] == 1 and st["slot_splits_redone"] == 0, st


@pytest.mark.parametrize("length,copies", [(TIE_FROM + 1, 2), (24, 8), (31, 2), (31, 8)])
def test_ties_on_the_slot_key_but_not_on_the_key(oracle, monkeypatch, capfd, length, copies):
    """Repeats longer than the chars a slot key stands for and shorter than a key: the 64-bit keys differ, the slot keys tie, and
    the plain kernel settles every pair from the text -- no tile is queued."""
    T = with_repeat(1_000_003, length=length, copies=copies)
    sh = slot_keys_shape(emul(), monkeypatch, capfd, T, p=20)
    assert (64 - sh["smin"]) // 2 == TIE_FROM and sh["smin"] == sh["smax"], sh
    assert sh["ties"] >= (copies - 1) * (length - TIE_FROM) and sh["queued"] == 0, sh
    all_masks(emul(), monkeypatch, T, reference(oracle, ("rep", length, copies), T), p=20)


@pytest.mark.parametrize("length,copies", [(80, 2), (80, 64), (2400, 2)])
def test_deep_ties_reach_the_queue_kernels_through_the_records(oracle, monkeypatch, capfd, length, copies):
    """80 bases twice: settled in place.  64 copies (a bin beyond its limit) and 2,400 bases twice (beyond the bounded tie-break):
    flagged tiles, whose indices the queue kernels get out of the records."""
    T = with_repeat(1_000_003, length=length, copies=copies)
    sh = slot_keys_shape(emul(), monkeypatch, capfd, T, p=20)
    assert sh["ties"] >= 1 and (sh["queued"] >= 1) == ((length, copies) != (80, 2)), sh
    all_masks(emul(), monkeypatch, T, reference(oracle, ("rep", length, copies), T), p=20)


@pytest.mark.parametrize("seed,length,copies", [(11, 80, 56), (12, 2500, 2)])
def test_flagged_tiles_behind_an_empty_slot(oracle, monkeypatch, capfd, seed, length, copies):
    T = no_kmer_with_repeat(1_200_007, [1, 1, 1, 1], length=length, copies=copies, seed=seed)
    sh = slot_keys_shape(emul(), monkeypatch, capfd, T, p=8)
    assert sh["inner_empty"] >= 1 and sh["queued"] >= 1 and sh["ties"] >= 1, sh
    all_masks(emul(), monkeypatch, T, reference(oracle, ("behind", seed, length, copies), T), p=8)


def test_ties_at_the_end_of_the_text(oracle, monkeypatch, capfd):
    """A text that ends inside a planted copy (suffixes shorter than a slot key's chars, and between those and a key's, tie with
    longer ones), and one whose last 40 bases repeat its first 40."""
    T = ends_inside_a_copy(1_000_003)
    sh = slot_keys_shape(emul(), monkeypatch, capfd, T, p=20)
    assert sh["ties"] >= 30 - TIE_FROM + 1 and sh["queued"] == 0, sh
    want = reference(oracle, "ends_inside", T)
    SA, LCP = want
    n = T.size
    for short in (n - 30, n - 10):                      # the two short suffixes stand next to a suffix of the planted copy
        r = int(np.flatnonzero(SA == short)[0])
        assert abs(int(SA[r + 1]) - n // 2) < 60 and int(LCP[r + 1]) == n - short, (short, SA[r - 1:r + 2], LCP[r:r + 2])
    all_masks(emul(), monkeypatch, T, want, p=20)
    H = tail_repeats_head(1_000_003)
    sh = slot_keys_shape(emul(), monkeypatch, capfd, H, p=20)
    assert sh["ties"] >= 40 - TIE_FROM and sh["queued"] == 0, sh
    all_masks(emul(), monkeypatch, H, reference(oracle, "tail_head", H), p=20)


def test_a_tie_across_a_bucket_boundary(oracle, monkeypatch, capfd):
    """Two planted words on the two sides of a bucket's edge that agree above the shift: the head LCP comes from the text."""
    T, sh, (a, b) = tie_across_a_boundary(emul(), monkeypatch, capfd)
    assert sh["head_ties"] >= 1, sh
    want = reference(oracle, "boundary_tie", T)
    SA, LCP = want
    r = int(np.flatnonzero(SA == b)[0])
    assert int(SA[r - 1]) == a and TIE_FROM <= int(LCP[r]) < 32, (SA[r - 1:r + 1], LCP[r])       # the pair, neighbours, tied above the shift
    all_masks(emul(), monkeypatch, T, want, p=20)


def test_empty_slots_and_small_buckets(oracle, monkeypatch, capfd):
    """Empty slots and small buckets come from the texts without a word: their split is kept, with an empty slot between full
    ones (no CCCC) and buckets whose early loads have lanes beyond their size (both).  The three-letter text cannot serve for them
    -- its key ranges are empty at every scale, a slot overflows and the split is redone: it is a case that must report 0."""
    T = uniform(1_000_001, DNA[:3])
    st = all_masks(emul(), monkeypatch, T, reference(oracle, "acg1m", T), p=20, taken=False)
    assert st["slot_splits_redone"] >= 1, st
    for key, kmer, p in (("no_cccc", [1, 1, 1, 1], 8), ("no_gggg_p20", [2, 2, 2, 2], 20)):
        T = no_kmer(1_200_007, kmer)
        sh = slot_keys_shape(emul(), monkeypatch, capfd, T, p=p)
        assert sh["below_early"] >= 1 and (key != "no_cccc" or sh["inner_empty"] >= 1), sh
        all_masks(emul(), monkeypatch, T, reference(oracle, key, T), p=p)


def test_a_redone_split_reports_zero(oracle, monkeypatch):
    """Skewed Markov text, linear mode forced: a slot overflows, the split is redone from level A's untouched 64-bit records."""
    T = markov(np.random.RandomState(5), 200_000)
    st = all_masks(emul_small(), monkeypatch, T, reference(oracle, "markov200k", T), taken=False, DIRECT_MODE="linear")
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] >= 1 and st["tile_chain"] == 0, st


def test_builds_that_keep_todays_slots_report_zero(oracle, monkeypatch):
    """64-bit indices, quantile mode, an 8-bit text, 32-bit keys, two-array streams, the plain scatter, the table launch and the
    samplesort path."""
    T = uniform(1_000_003)
    want = reference(oracle, ("uni", T.size), T)
    all_masks(emul(), monkeypatch, T, reference(oracle, ("uni64", T.size), T, bits=64), bits=64, p=20, taken=False)
    st = all_masks(emul(), monkeypatch, T, want, p=20, taken=False, DIRECT_MODE="quantile")
    assert st["direct_quantile"] == 1, st
    st = all_masks(emul(), monkeypatch, T, want, p=20, taken=False, KEYS="32")
    assert st["direct_key_bits"] == 32, st
    st = all_masks(emul(), monkeypatch, T, want, p=20, taken=False, RECORDS="0")
    assert st["direct_records"] == 0, st
    all_masks(emul(), monkeypatch, T, want, p=20, taken=False, SCATTER_ISSUE="0")
    all_masks(emul(), monkeypatch, T, want, p=20, taken=False, TILE_CHAIN="0")
    all_masks(emul(), monkeypatch, T, want, p=20, taken=False, direct=False, PATH="classic")
    B = np.random.RandomState(7).randint(32, 127, size=1_000_003).astype(np.uint8)
    st = all_masks(emul(), monkeypatch, B, reference(oracle, "bytes1m", B), p=20, taken=False, direct=None)
    assert st["bits_per_char"] == 8, st


def test_reversed_thread_order_and_poisoned_memory(oracle, monkeypatch):
    """The uniform text and a tie on the slot keys with the threads of every phase in descending order, and with LDS and registers
    that start as 0xA5 bytes and threads in a scattered order."""
    import caps_sa_amd
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, "libcaps_sa_emul_poison.so"])
    poison = caps_sa_amd.CapsLib(os.path.join(EMUL_DIR, "libcaps_sa_emul_poison.so"), "caps_sa_emul_")
    T = uniform(1_000_003)
    R = with_repeat(1_000_003, length=31, copies=8)
    D = with_repeat(1_000_003, length=80, copies=64)
    for E in (emul_rev(False), poison):
        all_masks(E, monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20)
        all_masks(E, monkeypatch, R, reference(oracle, ("rep", 31, 8), R), p=20)
        all_masks(E, monkeypatch, D, reference(oracle, ("rep", 80, 64), D), p=20)


def test_barrier_race_detector_on_the_record_builds(oracle, monkeypatch):
    """The uniform text and the tie on the slot keys through the emulation with the barrier-race detector (tests/emul/race_rt.h)."""
    import ctypes
    import caps_sa_amd
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, "libcaps_sa_emul_race.so"])
    path = os.path.join(EMUL_DIR, "libcaps_sa_emul_race.so")
    race = caps_sa_amd.CapsLib(path, "caps_sa_emul_")
    raw = ctypes.CDLL(path)
    raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
    raw.caps_sa_emul_races_reset()
    for k in ("CAPS_SA_SLOT_KEYS", "CAPS_SA_TILE_CHAIN", "CAPS_SA_SCATTER_ISSUE"):
        monkeypatch.delenv(k, raising=False)
    for key, T in ((("uni", 1_000_003), uniform(1_000_003)), (("rep", 31, 8), with_repeat(1_000_003, length=31, copies=8))):
        SA, LCP, st = race.build(T, p=20)
        want = reference(oracle, key, T)
        assert st["slot_keys"] == 1 and np.array_equal(SA, want[0]) and np.array_equal(LCP, want[1]), key
        races = int(raw.caps_sa_emul_races_found())
        raw.caps_sa_emul_races_reset()
        assert races == 0, (key, races)
