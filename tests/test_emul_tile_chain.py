"""CPU: the bucket-indexed launch of tile_sort_kernel (kernels.h CHAIN, pipeline.h segmented_sort / run_direct,
CAPS_SA_TILE_CHAIN) through the host emulation of the kernels.  Every case is built with the launch over the tile table (mask 0)
and with every kept stage: equal to the oracle, equal to each other, and the statistic names the mask the final sort ran with.

The launch needs a linear slot split that is KEPT (every bucket fits its slot).  The 256-element-tile build never keeps one -- the
spread of its bucket sizes is a quarter of the slots' headroom per sigma -- so the cases that take the launch run on the
4096-element-tile build, on the texts of the GPU cases; the small-tile build serves the paths that must stay on the table launch.
Buckets of a kept split of a uniform text hold 7/8 of a tile give or take a few per cent: more than the three loads per thread
that are issued ahead of the bounds cover, so only the fourth, guarded load is cut there.  Lanes of the EARLY loads beyond a bucket's
size, an empty slot between full ones and a flagged tile behind it need texts with a hole in their key range (tile_chain_cases
no_kmer): each such case asks the library what its launch looked like (launch_shape) and asserts the corner it is there for."""
import os
import subprocess

import numpy as np
import pytest

from emul_util import EMUL_DIR, emul, emul_rev, emul_small
from records_cases import markov
from tile_chain_cases import DNA, all_masks, launch_shape, no_kmer, no_kmer_with_repeat, reference, uniform, with_repeat


def test_uniform_text_takes_the_bucket_indexed_launch(oracle, monkeypatch, capfd):
    T = uniform(1_000_003)
    sh = launch_shape(emul(), monkeypatch, capfd, T, p=20)
    assert sh["tiles"] > 1 and sh["below_early"] == 0 and sh["queued"] == 0 and sh["queued_bad"] == 0, sh     # the plain case
    st = all_masks(emul(), monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20)
    assert st["direct_quantile"] == 0 and st["slot_splits"] == 1 and st["slot_splits_redone"] == 0, st


@pytest.mark.parametrize("n,p", [(1_100_001, 20), (1_200_007, 20), (1_200_007, 300)])
def test_odd_sizes_and_bucket_counts(oracle, monkeypatch, capfd, n, p):
    """317, 344 and 342 buckets (odd and even) in 348, 376 and 374 slots: the slots behind the last bucket are empty and return."""
    T = uniform(n)
    sh = launch_shape(emul(), monkeypatch, capfd, T, p=p)
    assert sh["slots"] > sh["last_slot"] + 1 and sh["tiles"] % 2 == (1 if (n, p) == (1_100_001, 20) else 0), sh
    all_masks(emul(), monkeypatch, T, reference(oracle, ("uni", n), T), p=p)


def test_three_letters_only(oracle, monkeypatch):
    """Whole key ranges are empty at every scale: some buckets get nothing, others more than a slot holds -- the split is redone
    with the count pass and the sort keeps the table launch."""
    T = uniform(1_000_001, DNA[:3])
    st = all_masks(emul(), monkeypatch, T, reference(oracle, "acg1m", T), p=20, taken=False)
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] >= 1, st


def test_an_empty_bucket_between_full_ones(oracle, monkeypatch, capfd):
    """Four letters without the word CCCC, eight groups: the hole in the key range is wider than a bucket and small against its
    group -- the split is kept with an empty slot in the middle, so bucket and tile index differ behind it (the boundary records
    and the output offsets of the buckets behind the hole), and the bucket at the hole's edge ends inside the third early load."""
    T = no_kmer(1_200_007, [1, 1, 1, 1])
    sh = launch_shape(emul(), monkeypatch, capfd, T, p=8)
    assert sh["inner_empty"] >= 1 and sh["tiles"] < sh["last_slot"] + 1 and sh["below_early"] >= 1, sh
    st = all_masks(emul(), monkeypatch, T, reference(oracle, "no_cccc", T), p=8)
    assert st["slot_splits"] == 1 and st["slot_splits_redone"] == 0, st


SMALL = {"no_gggg_p8": (lambda: no_kmer(1_200_007, [2, 2, 2, 2]), 8),
         "no_gggg_p20": (lambda: no_kmer(1_200_007, [2, 2, 2, 2]), 20),
         "no_cccc_rep": (lambda: no_kmer_with_repeat(1_200_007, [1, 1, 1, 1], length=80, copies=56, seed=12), 8)}


@pytest.mark.parametrize("case", sorted(SMALL))
def test_small_buckets_mask_the_early_loads(oracle, monkeypatch, capfd, case):
    """A hole in the key range that ends inside a bucket leaves that bucket a sliver (839, 211 and 69 elements when this was
    written): fewer elements than ONE early load per thread covers, so lanes of all three early loads lie at or beyond cnt and keep
    what the slot held; other buckets at a hole's edge end inside the second or third early load.  The third text also has tiles
    flagged (56 copies of an 80-base stretch), a sliver's neighbours among them."""
    make, p = SMALL[case]
    T = make()
    sh = launch_shape(emul(), monkeypatch, capfd, T, p=p)
    assert sh["tile_nt"] == 1024 and sh["early"] == 3 * 1024, sh
    assert sh["below_nt"] >= 1 and sh["smallest"] < sh["tile_nt"] and sh["below_early"] > sh["below_nt"], sh
    all_masks(emul(), monkeypatch, T, reference(oracle, ("small", case), T), p=p)


BEHIND = [(11, 80, 56), (12, 2500, 2)]


@pytest.mark.parametrize("seed,length,copies", BEHIND)
def test_flagged_tiles_behind_an_empty_slot(oracle, monkeypatch, capfd, seed, length, copies):
    """The text without CCCC with a crowded repeat (56 copies in bins that take 48) or a deep one (2,500 bases twice) planted:
    tiles are flagged in buckets BEHIND the empty slot, where the tile index a bucket must queue (tile_off[g]) is not its own
    number -- a kernel that queued g would hand the kernels behind it the wrong tiles, leave the flagged ones unsorted and
    sort others twice."""
    T = no_kmer_with_repeat(1_200_007, [1, 1, 1, 1], length=length, copies=copies, seed=seed)
    sh = launch_shape(emul(), monkeypatch, capfd, T, p=8)
    assert sh["inner_empty"] >= 1 and sh["queued"] >= 1 and sh["queued_moved"] >= 1 and sh["queued_bad"] == 0, sh
    all_masks(emul(), monkeypatch, T, reference(oracle, ("behind", seed, length, copies), T), p=8)


@pytest.mark.parametrize("length,copies", [(80, 2), (80, 64), (2500, 2)])
def test_planted_repeats_reach_the_queue_kernels(oracle, monkeypatch, capfd, length, copies):
    """An 80-base repeat in two copies ties on the keys (32 bases) but inside what the plain kernel reads (64 windows past the
    key): settled in place.  64 copies crowd one bin beyond its limit, and two copies of 2,500 bases tie beyond the 64 windows:
    those tiles are flagged and reach tile_sort_eq_kernel (and the kernels behind it) through the tile index the bucket-indexed
    build queues for its bucket."""
    T = with_repeat(1_000_003, length=length, copies=copies)
    sh = launch_shape(emul(), monkeypatch, capfd, T, p=20)
    assert (sh["queued"] >= 1) == ((length, copies) != (80, 2)) and sh["queued_bad"] == 0, sh
    all_masks(emul(), monkeypatch, T, reference(oracle, ("rep", length, copies), T), p=20)


def test_a_redone_split_keeps_the_table_launch(oracle, monkeypatch):
    """Skewed Markov text, linear mode forced: a slot overflows, the split is redone with the count pass."""
    T = markov(np.random.RandomState(5), 200_000)
    st = all_masks(emul_small(), monkeypatch, T, reference(oracle, "markov200k", T), taken=False, DIRECT_MODE="linear")
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] >= 1, st


def test_unchanged_paths_report_zero(oracle, monkeypatch):
    """64-bit indices, quantile mode, and a build whose results leave in waves."""
    T = uniform(1_000_003)
    all_masks(emul(), monkeypatch, T, reference(oracle, ("uni64", T.size), T, bits=64), bits=64, p=20, taken=False)
    st = all_masks(emul(), monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20, taken=False, DIRECT_MODE="quantile")
    assert st["direct_quantile"] == 1, st
    S = uniform(200_000)
    st = all_masks(emul_small(), monkeypatch, S, reference(oracle, ("uni", S.size), S), taken=False, HOST_WAVES="2")
    assert st["result_waves"] >= 2, st


def test_reversed_thread_order_and_poisoned_memory(oracle, monkeypatch):
    """The first case and the crowded repeat with the threads of every phase in descending order, and with LDS and registers that
    start as 0xA5 bytes and threads in a scattered order (lanes beyond a bucket's size hold whatever the slot held)."""
    import caps_sa_amd
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, "libcaps_sa_emul_poison.so"])
    poison = caps_sa_amd.CapsLib(os.path.join(EMUL_DIR, "libcaps_sa_emul_poison.so"), "caps_sa_emul_")
    T = uniform(1_000_003)
    R = with_repeat(1_000_003, length=80, copies=64)
    for E in (emul_rev(False), poison):
        all_masks(E, monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20)
        all_masks(E, monkeypatch, R, reference(oracle, ("rep", 80, 64), R), p=20)
