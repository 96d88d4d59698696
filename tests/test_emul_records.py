"""CPU: the direct path with records between level A and level B (kernels.h KeySaRec, group_scatter_kernel REC_OUT,
bucket_scatter_kernel / bucket_count_kernel REC_IN; pipeline.h run_direct, CAPS_SA_RECORDS), through the host emulation of the
kernels -- the 256-element-tile build, where texts of 150,000 chars have streams of several tiles.  Every case is built with
two arrays and with records: equal to the oracle, equal to each other, and the statistic names the layout."""
import numpy as np
import pytest

from conftest import LARGE_GOLDEN, large_golden
from emul_util import EMUL_DIR, emul, emul_rev, emul_small
from records_cases import DNA, both_layouts, markov, reference


def _uniform(n):
    return np.random.RandomState(n % 9973).choice(DNA, size=n)


@pytest.mark.parametrize("n", [150_001, 142_867])
@pytest.mark.parametrize("sub", ["1", "2", "8"])
def test_linear_mode_odd_sizes_and_substreams(oracle, monkeypatch, n, sub):
    """Stream lengths and tails that are no multiple of anything, one, two and eight sub-streams per group."""
    T = _uniform(n)
    st = both_layouts(emul_small(), monkeypatch, T, reference(oracle, ("uni", n), T), DIRECT_MODE="linear", DIRECT_SUB=sub)
    assert st["direct_quantile"] == 0


def test_several_tiles_per_stream_slot_split_kept(oracle, monkeypatch):
    """The 4096-element-tile build (1,500,000 chars are too many for the group tables of the small one): 20 groups of 18 tiles."""
    T = _uniform(1_500_000)
    st = both_layouts(emul(), monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20)
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] == 0, st


@pytest.fixture(scope="module")
def skewed():
    return markov(np.random.RandomState(5), 200_000)


def test_quantile_mode_reads_records_in_the_spill_scatter(oracle, monkeypatch, skewed):
    want = reference(oracle, "markov200k", skewed)
    st = both_layouts(emul_small(), monkeypatch, skewed, want)
    assert st["direct_quantile"] == 1 and st["knot_slot_splits"] == 1, st
    st = both_layouts(emul_small(), monkeypatch, skewed, want, TEST_SPILL_SLOT="160")       # most buckets outgrow their slots
    assert st["direct_quantile"] == 1 and st["spill_entries"] > 0, st


def test_linear_mode_on_skewed_keys_reads_the_records_twice(oracle, monkeypatch, skewed):
    """A slot overflows: count pass and scatter read the record stream again."""
    st = both_layouts(emul_small(), monkeypatch, skewed, reference(oracle, "markov200k", skewed), DIRECT_MODE="linear")
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] >= 1, st


def test_a_stream_that_outgrows_its_region(oracle, monkeypatch):
    T = _uniform(150_001)
    st = both_layouts(emul_small(), monkeypatch, T, reference(oracle, ("uni", T.size), T), direct=False, TEST_STREAM_CAP="80")
    assert st["path_fallback"] == 5


def test_eight_bit_codes(oracle, monkeypatch):
    rs = np.random.RandomState(8)
    T = rs.choice(np.frombuffer(b"abcdefgh", dtype=np.uint8), size=120_000, p=[.5, .2, .1, .1, .05, .03, .01, .01])
    st = both_layouts(emul_small(), monkeypatch, T, reference(oracle, "text8", T))
    assert st["bits_per_char"] == 8


def test_64_bit_indices_stay_on_two_arrays(oracle, monkeypatch):
    T = _uniform(600_001)
    both_layouts(emul_small(), monkeypatch, T, reference(oracle, ("uni64", T.size), T, bits=64), bits=64)


@pytest.mark.parametrize("name", LARGE_GOLDEN)
def test_large_golden_cases(monkeypatch, name):
    T, sa, lcp = large_golden(name)
    both_layouts(emul_small(), monkeypatch, T, (sa, lcp))


def test_results_leave_in_waves(oracle, monkeypatch):
    """Later waves' records still sit in buffer A while earlier waves are sorted (pipeline.h set_waves)."""
    T = _uniform(200_000)
    st = both_layouts(emul_small(), monkeypatch, T, reference(oracle, ("uni", T.size), T), HOST_WAVES="3")
    assert 2 <= st["result_waves"] <= 4


def test_reversed_thread_order_and_poisoned_memory(oracle, monkeypatch):
    """The first case again with the threads of every phase in descending order, and with LDS and registers that start as
    0xA5 bytes and threads in a scattered order."""
    import subprocess
    import os
    import caps_sa_amd
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, "libcaps_sa_emul_small_poison.so"])
    poison = caps_sa_amd.CapsLib(os.path.join(EMUL_DIR, "libcaps_sa_emul_small_poison.so"), "caps_sa_emul_")
    T = _uniform(142_867)
    want = reference(oracle, ("uni", T.size), T)
    for E in (emul_rev(True), poison):
        for sub in ("1", "8"):
            both_layouts(E, monkeypatch, T, want, DIRECT_MODE="linear", DIRECT_SUB=sub)
