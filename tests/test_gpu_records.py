"""GPU (-m gpu): the direct path with records between level A and level B (kernels.h KeySaRec, group_scatter_kernel REC_OUT,
bucket_scatter_kernel / bucket_count_kernel REC_IN; pipeline.h run_direct, CAPS_SA_RECORDS) on the real kernels.  Every case is
built with two arrays and with records: equal to the oracle, equal to each other, and the statistic names the layout.  The
smallest texts that reach the code: the direct path starts at 32 tiles of 4096."""
import os
import sys

import numpy as np
import pytest

from conftest import LARGE_GOLDEN, large_golden
from records_cases import DNA, both_layouts, markov, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


def _uniform(n):
    return np.random.RandomState(n % 9973).choice(DNA, size=n)


@pytest.mark.parametrize("n", [150_001, 142_867, 4_200_003])
def test_linear_mode_odd_sizes_and_substreams(L, oracle, monkeypatch, n):
    """Stream lengths and tails that are no multiple of anything, one, two and eight sub-streams per group.  (Ten tiles of level A
    dealt to eight sub-streams overload some of them: the small texts then leave the direct path, with either layout; the text
    of 257 such tiles is the smallest that keeps eight sub-streams.)"""
    T = _uniform(n)
    for sub in ("1", "2", "8"):
        st = both_layouts(L, monkeypatch, T, reference(oracle, ("uni", n), T), direct=True if sub == "1" or n > 4_000_000 else None,
                          DIRECT_MODE="linear", DIRECT_SUB=sub)
        assert st["direct_quantile"] == 0


def test_several_tiles_per_stream_slot_split_kept(L, oracle, monkeypatch):
    """20 groups of 18 tiles each, one stream per group."""
    T = _uniform(1_500_000)
    st = both_layouts(L, monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20)
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] == 0, st


def test_skewed_keys_in_both_level_b_modes(L, oracle, monkeypatch):
    """The skewed text of the emulation's tests at 200,000 (whichever mode its pivots choose at 4096-element tiles, small slots,
    linear forced), and one long enough for quantile buckets at this tile size: records feed the scatter with the spill stream;
    linear forced, a slot overflows and the count pass and the second scatter read the records again."""
    small = markov(np.random.RandomState(5), 200_000)
    want = reference(oracle, "markov200k", small)
    both_layouts(L, monkeypatch, small, want)
    both_layouts(L, monkeypatch, small, want, TEST_SPILL_SLOT="160")
    both_layouts(L, monkeypatch, small, want, DIRECT_MODE="linear")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    from genome_like import markov_dna
    skew = markov_dna(2_000_000, seed=23).cpu().numpy()
    want = reference(oracle, "markov2m", skew)
    st = both_layouts(L, monkeypatch, skew, want, p=1000)
    assert st["direct_quantile"] == 1 and st["knot_slot_splits"] == 1, st
    st = both_layouts(L, monkeypatch, skew, want, p=1000, TEST_SPILL_SLOT="2816")         # slots below the mean bucket
    assert st["direct_quantile"] == 1 and st["spill_entries"] > 0, st
    st = both_layouts(L, monkeypatch, skew, want, p=1000, DIRECT_MODE="linear")
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] >= 1, st


def test_a_stream_that_outgrows_its_region(L, oracle, monkeypatch):
    T = _uniform(150_001)
    st = both_layouts(L, monkeypatch, T, reference(oracle, ("uni", T.size), T), direct=False, TEST_STREAM_CAP="80")
    assert st["path_fallback"] == 5


def test_eight_bit_codes(L, oracle, monkeypatch):
    rs = np.random.RandomState(8)
    T = rs.choice(np.frombuffer(b"abcdefgh", dtype=np.uint8), size=150_000, p=[.5, .2, .1, .1, .05, .03, .01, .01])
    st = both_layouts(L, monkeypatch, T, reference(oracle, "text8_150k", T))
    assert st["bits_per_char"] == 8
    # (120,000 chars, the emulation's size, are 30 tiles of 4096: below the direct path -- either setting is the same build)
    st = both_layouts(L, monkeypatch, T[:120_000], reference(oracle, "text8_120k", T[:120_000]), direct=False)
    assert st["bits_per_char"] == 8 and st["path_fallback"] == 2


def test_64_bit_indices_stay_on_two_arrays(L, oracle, monkeypatch):
    T = _uniform(600_001)
    both_layouts(L, monkeypatch, T, reference(oracle, ("uni64", T.size), T, bits=64), bits=64)


@pytest.mark.parametrize("name", LARGE_GOLDEN)
def test_large_golden_cases(L, monkeypatch, name):
    T, sa, lcp = large_golden(name)
    both_layouts(L, monkeypatch, T, (sa, lcp))


def test_results_leave_in_waves_host_path(L, oracle, monkeypatch):
    """Later waves' records still sit in buffer A while earlier waves are sorted (pipeline.h set_waves)."""
    T = _uniform(1_500_000)
    L.release_cache()
    st = both_layouts(L, monkeypatch, T, reference(oracle, ("uni", T.size), T), HOST_WAVES="3")
    assert 2 <= st["result_waves"] <= 4
    L.release_cache()
