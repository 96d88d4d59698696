"""GPU (-m gpu): the bucket-indexed launch of tile_sort_kernel (kernels.h CHAIN, pipeline.h segmented_sort / run_direct,
CAPS_SA_TILE_CHAIN) on the real kernels.  Every case is built with the launch over the tile table (mask 0) and with every kept
stage: equal to the oracle, equal to each other, and the statistic names the mask the final sort ran with.  Texts of 1.0 to 1.2 M
bases: the smallest whose linear slot split finds room for its slots (at 0.6 M the split is not tried).  The texts are those of
test_emul_tile_chain.py, and each case asserts the corner it is there for from the library's own description of its launch
(tile_chain_cases.launch_shape)."""
import numpy as np
import pytest

from records_cases import markov
from tile_chain_cases import DNA, all_masks, launch_shape, no_kmer, no_kmer_with_repeat, reference, uniform, with_repeat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


def test_uniform_text_takes_the_bucket_indexed_launch(L, oracle, monkeypatch, capfd):
    T = uniform(1_000_003)
    sh = launch_shape(L, monkeypatch, capfd, T, p=20)
    assert sh["tiles"] > 1 and sh["below_early"] == 0 and sh["queued"] == 0 and sh["queued_bad"] == 0, sh     # the plain case
    st = all_masks(L, monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20)
    assert st["direct_quantile"] == 0 and st["slot_splits"] == 1 and st["slot_splits_redone"] == 0, st


@pytest.mark.parametrize("n,p", [(1_100_001, 20), (1_200_007, 20), (1_200_007, 300)])
def test_odd_sizes_and_bucket_counts(L, oracle, monkeypatch, capfd, n, p):
    """317, 344 and 342 buckets (odd and even) in 348, 376 and 374 slots: the slots behind the last bucket are empty and return."""
    T = uniform(n)
    sh = launch_shape(L, monkeypatch, capfd, T, p=p)
    assert sh["slots"] > sh["last_slot"] + 1 and sh["tiles"] % 2 == (1 if (n, p) == (1_100_001, 20) else 0), sh
    all_masks(L, monkeypatch, T, reference(oracle, ("uni", n), T), p=p)


def test_three_letters_only(L, oracle, monkeypatch):
    """Key ranges empty at every scale: the split is redone and the sort keeps the table launch."""
    T = uniform(1_000_001, DNA[:3])
    st = all_masks(L, monkeypatch, T, reference(oracle, "acg1m", T), p=20, taken=False)
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] >= 1, st


def test_an_empty_bucket_between_full_ones(L, oracle, monkeypatch, capfd):
    """Four letters without the word CCCC, eight groups: kept, with an empty slot between full ones -- bucket and tile index
    differ behind it -- and a bucket at the hole's edge that ends inside the third early load."""
    T = no_kmer(1_200_007, [1, 1, 1, 1])
    sh = launch_shape(L, monkeypatch, capfd, T, p=8)
    assert sh["inner_empty"] >= 1 and sh["tiles"] < sh["last_slot"] + 1 and sh["below_early"] >= 1, sh
    st = all_masks(L, monkeypatch, T, reference(oracle, "no_cccc", T), p=8)
    assert st["slot_splits"] == 1 and st["slot_splits_redone"] == 0, st


SMALL = {"no_gggg_p8": (lambda: no_kmer(1_200_007, [2, 2, 2, 2]), 8),
         "no_gggg_p20": (lambda: no_kmer(1_200_007, [2, 2, 2, 2]), 20),
         "no_cccc_rep": (lambda: no_kmer_with_repeat(1_200_007, [1, 1, 1, 1], length=80, copies=56, seed=12), 8)}


@pytest.mark.parametrize("case", sorted(SMALL))
def test_small_buckets_mask_the_early_loads(L, oracle, monkeypatch, capfd, case):
    """A bucket that a hole in the key range leaves a sliver (fewer elements than ONE early load per thread covers): lanes of all
    three early loads lie at or beyond cnt and keep what the slot held; others end inside the second or third early load."""
    make, p = SMALL[case]
    T = make()
    sh = launch_shape(L, monkeypatch, capfd, T, p=p)
    assert sh["tile_nt"] == 1024 and sh["early"] == 3 * 1024, sh
    assert sh["below_nt"] >= 1 and sh["smallest"] < sh["tile_nt"] and sh["below_early"] > sh["below_nt"], sh
    all_masks(L, monkeypatch, T, reference(oracle, ("small", case), T), p=p)


@pytest.mark.parametrize("seed,length,copies", [(11, 80, 56), (12, 2500, 2)])
def test_flagged_tiles_behind_an_empty_slot(L, oracle, monkeypatch, capfd, seed, length, copies):
    """Tiles flagged in buckets BEHIND an empty slot (a crowded and a deep repeat planted into the text without CCCC): the tile
    index a bucket queues, tile_off[g], is not its own number there."""
    T = no_kmer_with_repeat(1_200_007, [1, 1, 1, 1], length=length, copies=copies, seed=seed)
    sh = launch_shape(L, monkeypatch, capfd, T, p=8)
    assert sh["inner_empty"] >= 1 and sh["queued"] >= 1 and sh["queued_moved"] >= 1 and sh["queued_bad"] == 0, sh
    all_masks(L, monkeypatch, T, reference(oracle, ("behind", seed, length, copies), T), p=8)


@pytest.mark.parametrize("length,copies", [(80, 2), (80, 64), (2500, 2)])
def test_planted_repeats_reach_the_queue_kernels(L, oracle, monkeypatch, capfd, length, copies):
    """80 bases twice: settled by the plain kernel's bounded tie-break.  64 copies (a bin beyond its limit) and 2,500 bases twice
    (ties beyond the 64 windows): flagged tiles reach the eq / general kernels through the queued tile index."""
    T = with_repeat(1_000_003, length=length, copies=copies)
    sh = launch_shape(L, monkeypatch, capfd, T, p=20)
    assert (sh["queued"] >= 1) == ((length, copies) != (80, 2)) and sh["queued_bad"] == 0, sh
    all_masks(L, monkeypatch, T, reference(oracle, ("rep", length, copies), T), p=20)


def test_a_redone_split_keeps_the_table_launch(L, oracle, monkeypatch):
    """Skewed Markov text, linear mode forced: a slot overflows, the split is redone with the count pass.  (The emulation case
    runs the 256-element-tile build on 200,000 bases; with 4096-element tiles the slot split is first tried near a million.)"""
    T = markov(np.random.RandomState(5), 1_000_000)
    st = all_masks(L, monkeypatch, T, reference(oracle, "markov1m", T), p=20, taken=False, DIRECT_MODE="linear")
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] >= 1, st


def test_unchanged_paths_report_zero(L, oracle, monkeypatch):
    """64-bit indices, quantile mode, and a host build whose results leave in waves."""
    T = uniform(1_000_003)
    all_masks(L, monkeypatch, T, reference(oracle, ("uni64", T.size), T, bits=64), bits=64, p=20, taken=False)
    st = all_masks(L, monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20, taken=False, DIRECT_MODE="quantile")
    assert st["direct_quantile"] == 1, st
    L.release_cache()
    st = all_masks(L, monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20, taken=False, HOST_WAVES="2")
    assert st["result_waves"] >= 2, st
    L.release_cache()
