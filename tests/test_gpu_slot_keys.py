"""GPU (-m gpu): slot keys -- level B of the direct path handing the tile sort 8-byte records of bucket-relative 32-bit keys
(kernels.h "slot keys", bucket_scatter_kernel SLOT32, tile_sort_kernel SLOTREC, CAPS_SA_SLOT_KEYS) -- on the real kernels.  Every
case is built with today's two-array slots (mask 0), with every kept mask and without the variable: equal to the oracle, equal to
each other, and the statistic names the mask the final sort ran with.  Texts of 1.0 to 1.2 M bases (the smallest whose linear slot
split is kept); they are those of test_emul_slot_keys.py, and each case asserts its corner from the library's own description of
its slot keys (slot_keys_cases.slot_keys_shape)."""
import numpy as np
import pytest

from records_cases import markov
from slot_keys_cases import (DNA, all_masks, ends_inside_a_copy, no_kmer, no_kmer_with_repeat, reference, slot_keys_shape,
                             tail_repeats_head, tie_across_a_boundary, uniform, with_repeat)

pytestmark = pytest.mark.gpu

TIE_FROM = 19               # (64 - 26) / 2: the chars a slot key stands for at a million bases in 20 groups


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


@pytest.mark.parametrize("n,p", [(1_000_003, 20), (1_100_001, 20), (1_200_007, 300)])
def test_uniform_text_and_odd_bucket_counts(L, oracle, monkeypatch, capfd, n, p):
    T = uniform(n)
    sh = slot_keys_shape(L, monkeypatch, capfd, T, p=p)
    assert sh["wraps"] >= 1 and sh["queued"] == 0 and sh["smin"] >= 20 and (64 - sh["smax"]) // 2 >= 16, sh
    st = all_masks(L, monkeypatch, T, reference(oracle, ("uni", n), T), p=p)
    assert st["direct_quantile"] == 0 and st["slot_splits"] == 1 and st["slot_splits_redone"] == 0, st


@pytest.mark.parametrize("length,copies", [(TIE_FROM + 1, 2), (24, 8), (31, 2), (31, 8)])
def test_ties_on_the_slot_key_but_not_on_the_key(L, oracle, monkeypatch, capfd, length, copies):
    """Repeats longer than the chars a slot key stands for and shorter than a key: the slot keys tie, the plain kernel settles
    every pair from the text, no tile is queued."""
    T = with_repeat(1_000_003, length=length, copies=copies)
    sh = slot_keys_shape(L, monkeypatch, capfd, T, p=20)
    assert (64 - sh["smin"]) // 2 == TIE_FROM and sh["smin"] == sh["smax"], sh
    assert sh["ties"] >= (copies - 1) * (length - TIE_FROM) and sh["queued"] == 0, sh
    all_masks(L, monkeypatch, T, reference(oracle, ("rep", length, copies), T), p=20)


@pytest.mark.parametrize("length,copies", [(80, 2), (80, 64), (2400, 2)])
def test_deep_ties_reach_the_queue_kernels_through_the_records(L, oracle, monkeypatch, capfd, length, copies):
    T = with_repeat(1_000_003, length=length, copies=copies)
    sh = slot_keys_shape(L, monkeypatch, capfd, T, p=20)
    assert sh["ties"] >= 1 and (sh["queued"] >= 1) == ((length, copies) != (80, 2)), sh
    all_masks(L, monkeypatch, T, reference(oracle, ("rep", length, copies), T), p=20)


@pytest.mark.parametrize("seed,length,copies", [(11, 80, 56), (12, 2500, 2)])
def test_flagged_tiles_behind_an_empty_slot(L, oracle, monkeypatch, capfd, seed, length, copies):
    T = no_kmer_with_repeat(1_200_007, [1, 1, 1, 1], length=length, copies=copies, seed=seed)
    sh = slot_keys_shape(L, monkeypatch, capfd, T, p=8)
    assert sh["inner_empty"] >= 1 and sh["queued"] >= 1 and sh["ties"] >= 1, sh
    all_masks(L, monkeypatch, T, reference(oracle, ("behind", seed, length, copies), T), p=8)


def test_ties_at_the_end_of_the_text(L, oracle, monkeypatch, capfd):
    T = ends_inside_a_copy(1_000_003)
    sh = slot_keys_shape(L, monkeypatch, capfd, T, p=20)
    assert sh["ties"] >= 30 - TIE_FROM + 1 and sh["queued"] == 0, sh
    all_masks(L, monkeypatch, T, reference(oracle, "ends_inside", T), p=20)
    H = tail_repeats_head(1_000_003)
    sh = slot_keys_shape(L, monkeypatch, capfd, H, p=20)
    assert sh["ties"] >= 40 - TIE_FROM and sh["queued"] == 0, sh
    all_masks(L, monkeypatch, H, reference(oracle, "tail_head", H), p=20)


def test_a_tie_across_a_bucket_boundary(L, oracle, monkeypatch, capfd):
    """Two planted words on the two sides of a bucket's edge that agree above the shift: the head LCP comes from the text."""
    T, sh, (a, b) = tie_across_a_boundary(L, monkeypatch, capfd)
    assert sh["head_ties"] >= 1, sh
    want = reference(oracle, "boundary_tie", T)
    SA, LCP = want
    r = int(np.flatnonzero(SA == b)[0])
    assert int(SA[r - 1]) == a and TIE_FROM <= int(LCP[r]) < 32, (SA[r - 1:r + 1], LCP[r])
    all_masks(L, monkeypatch, T, want, p=20)


def test_empty_slots_and_small_buckets(L, oracle, monkeypatch, capfd):
    """Empty slots and small buckets come from the texts without a word (kept splits with an empty slot between full ones and
    buckets whose early loads have lanes beyond their size); the three-letter text's split is redone: a case that must report 0."""
    T = uniform(1_000_001, DNA[:3])
    st = all_masks(L, monkeypatch, T, reference(oracle, "acg1m", T), p=20, taken=False)
    assert st["slot_splits_redone"] >= 1, st
    for key, kmer, p in (("no_cccc", [1, 1, 1, 1], 8), ("no_gggg_p20", [2, 2, 2, 2], 20)):
        T = no_kmer(1_200_007, kmer)
        sh = slot_keys_shape(L, monkeypatch, capfd, T, p=p)
        assert sh["below_early"] >= 1 and (key != "no_cccc" or sh["inner_empty"] >= 1), sh
        all_masks(L, monkeypatch, T, reference(oracle, key, T), p=p)


def test_a_redone_split_reports_zero(L, oracle, monkeypatch):
    """Skewed Markov text, linear mode forced: a slot overflows, the split is redone from level A's untouched 64-bit records."""
    T = markov(np.random.RandomState(5), 1_000_000)
    st = all_masks(L, monkeypatch, T, reference(oracle, "markov1m", T), p=20, taken=False, DIRECT_MODE="linear")
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] >= 1 and st["tile_chain"] == 0, st


def test_builds_that_keep_todays_slots_report_zero(L, oracle, monkeypatch):
    """64-bit indices, quantile mode, an 8-bit text, 32-bit keys, two-array streams, the plain scatter, the table launch and the
    samplesort path."""
    T = uniform(1_000_003)
    want = reference(oracle, ("uni", T.size), T)
    all_masks(L, monkeypatch, T, reference(oracle, ("uni64", T.size), T, bits=64), bits=64, p=20, taken=False)
    st = all_masks(L, monkeypatch, T, want, p=20, taken=False, DIRECT_MODE="quantile")
    assert st["direct_quantile"] == 1, st
    st = all_masks(L, monkeypatch, T, want, p=20, taken=False, KEYS="32")
    assert st["direct_key_bits"] == 32, st
    st = all_masks(L, monkeypatch, T, want, p=20, taken=False, RECORDS="0")
    assert st["direct_records"] == 0, st
    all_masks(L, monkeypatch, T, want, p=20, taken=False, SCATTER_ISSUE="0")
    all_masks(L, monkeypatch, T, want, p=20, taken=False, TILE_CHAIN="0")
    all_masks(L, monkeypatch, T, want, p=20, taken=False, direct=False, PATH="classic")
    B = np.random.RandomState(7).randint(32, 127, size=1_000_003).astype(np.uint8)
    st = all_masks(L, monkeypatch, B, reference(oracle, "bytes1m", B), p=20, taken=False, direct=None)
    assert st["bits_per_char"] == 8, st
