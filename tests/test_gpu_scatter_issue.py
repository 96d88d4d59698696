"""GPU (-m gpu): the scatter kernels that issue a tile's memory traffic together (kernels.h bucket_scatter_kernel
ISSUE, pipeline.h run_direct, CAPS_SA_SCATTER_ISSUE; the corners of level A's tiles stay as cases) on the real kernels.  Every case is built with the plain
kernels (mask 0) and with every kept mask: equal to the oracle, equal to each other, and the statistic names the stages the build
ran with.  The smallest texts that reach the code; a case that is there for a corner of the tiles (a last tile that ends inside a
given load of a thread) asserts the corner from the library's own description of its streams (scatter_issue_cases.level_b_input)."""
import numpy as np
import pytest

from records_cases import markov
from scatter_issue_cases import DNA, all_masks, level_b_input, reference, uniform

pytestmark = pytest.mark.gpu

GA_E = 4 * 4096             # positions per tile of level A (kernels.h GA_E)


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


def test_level_b_last_tiles_end_inside_every_load(L, oracle, monkeypatch, capfd):
    """Linear mode, uniform DNA: 150,001 bases in one sub-stream per group (seven streams; at this size level B splits by
    counting, with the grouped map: no flagged build), 4,200,003 in eight (the smallest text that keeps them) and
    5,300,003 in eight.  The streams of one text are all about as long, so their last tiles end inside the same one or two loads
    of a thread -- the first, third and fourth at 4.2 M, the first, second and fourth at 5.3 M: together a tile that ends inside
    each of the four loads (1 .. 1024, 1025 .. 2048, 2049 .. 3072, 3073 .. 4095 elements), beside a thousand full tiles."""
    seen = np.zeros(4, dtype=np.int64)
    full = 0
    for n, sub, taken in ((150_001, "1", 0), (4_200_003, "8", 1), (5_300_003, "8", 1)):
        T = uniform(n)
        sh = level_b_input(L, monkeypatch, capfd, T, DIRECT_MODE="linear", DIRECT_SUB=sub)
        assert sh["tile"] == 4096 and sh["threads"] == 1024 and len(sh["tails"]) == 4, sh
        print(n, sub, sh)
        if taken & 1:
            seen += np.array(sh["tails"])
            full += sh["full"]
        st = all_masks(L, monkeypatch, T, reference(oracle, ("uni", n), T), taken=taken, DIRECT_MODE="linear", DIRECT_SUB=sub)
        assert st["direct_quantile"] == 0, st
    assert full >= 100 and seen.sum() >= 200 and (seen >= 1).all(), (full, seen)


def test_slot_split_kept_and_the_bucket_indexed_sort_behind_it(L, oracle, monkeypatch):
    T = uniform(1_000_003)
    st = all_masks(L, monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20)
    assert st["direct_quantile"] == 0 and st["slot_splits"] == 1 and st["slot_splits_redone"] == 0 and st["tile_chain"] == 1, st


def test_three_letters_only(L, oracle, monkeypatch):
    """Key ranges empty at every scale: groups whose segments get one bucket (the route without the LDS histogram, in the same
    launch as the flagged one) and a split that is redone with the count pass."""
    T = uniform(1_000_001, DNA[:3])
    st = all_masks(L, monkeypatch, T, reference(oracle, "acg1m", T), p=20)
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] >= 1, st


def test_a_redone_split_of_a_skewed_text(L, oracle, monkeypatch):
    """Skewed Markov text, linear mode forced: a slot overflows, the count pass and the second scatter read the records again."""
    T = markov(np.random.RandomState(5), 1_000_000)
    st = all_masks(L, monkeypatch, T, reference(oracle, "markov1m", T), p=20, DIRECT_MODE="linear")
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] >= 1, st


@pytest.mark.parametrize("last", [1, 15, 16, 17, GA_E - 1])
def test_level_a_last_tile(L, oracle, monkeypatch, last):
    """Nine full tiles of level A and a last one of 1, 15, 16 (one packed word), 17 and 16,383 positions: the packed text ends
    inside the last tile's window, in its first word, its second, or its last but one."""
    n = 9 * GA_E + last
    T = uniform(n)
    all_masks(L, monkeypatch, T, reference(oracle, ("uni", n), T), taken=0, DIRECT_MODE="linear")     # (level B: the grouped map)


@pytest.mark.parametrize("k1", [1024, 1025, 1026])
def test_level_a_splitter_table_around_one_load_per_thread(L, oracle, monkeypatch, k1):
    """K1 - 1 = 1023, 1024 and 1025 splitters: the second load of a thread from the splitter table is empty, empty, one entry.
    (A group is then less than a tile: level B has nothing to split, no flagged build runs.)"""
    T = uniform(1_000_003)
    st = all_masks(L, monkeypatch, T, reference(oracle, ("uni", T.size), T), p=k1, taken=0, DIRECT_MODE="linear", DIRECT_K1=str(k1))
    assert st["direct_groups"] == k1, st


def test_unchanged_paths_report_zero(L, oracle, monkeypatch):
    """64-bit indices, quantile mode, 32-bit keys, a host build whose results leave in waves, the classic path."""
    T = uniform(1_000_003)
    all_masks(L, monkeypatch, T, reference(oracle, ("uni64", T.size), T, bits=64), bits=64, p=20, taken=0)
    want = reference(oracle, ("uni", T.size), T)
    st = all_masks(L, monkeypatch, T, want, p=20, taken=0, DIRECT_MODE="quantile")
    assert st["direct_quantile"] == 1, st
    st = all_masks(L, monkeypatch, T, want, p=20, taken=0, direct=None, KEYS="32")
    assert st["direct_key_bits"] == 32 or st["path_direct"] == 0, st
    all_masks(L, monkeypatch, T, want, p=20, taken=0, direct=False, PATH="classic")
    L.release_cache()
    st = all_masks(L, monkeypatch, T, want, p=20, taken=0, HOST_WAVES="2")
    assert st["result_waves"] >= 2, st
    L.release_cache()
