"""CPU: the scatter kernels that issue a tile's memory traffic together (kernels.h bucket_scatter_kernel
ISSUE, pipeline.h run_direct, CAPS_SA_SCATTER_ISSUE; the corners of level A's tiles stay as cases) through the host emulation of the kernels.  Every case is
built with the plain kernels (mask 0) and with every kept mask: equal to the oracle, equal to each other, and the statistic names
the stages the build ran with.

The cases of test_gpu_scatter_issue.py run on the 4096-element-tile build (a slot split is only KEPT there); the same corners at
the scale of the 256-element-tile build (64 threads, tiles of level A of 1,024 positions, 128 buckets in LDS) run with the threads of
every phase ascending, descending and scattered over poisoned LDS and registers, and under the barrier-race detector: in the flagged
build of level B a barrier changes its kind and the zeroing of the histogram moves relative to the loads."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from emul_util import EMUL_DIR, emul, emul_rev, emul_small
from records_cases import markov
from scatter_issue_cases import DNA, all_masks, level_b_input, reference, uniform

GA_E = 4 * 4096             # positions per tile of level A (kernels.h GA_E), 4096-element tiles
GA_S = 4 * 256              #   ... and in the 256-element-tile build


def _lib(name):
    import caps_sa_amd
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, name])
    path = os.path.join(EMUL_DIR, name)
    return caps_sa_amd.CapsLib(path, "caps_sa_emul_"), path


def test_level_b_last_tiles_end_inside_every_load(oracle, monkeypatch, capfd):
    """The texts of the GPU case (see there): together their streams have last tiles that end inside each of the four loads."""
    seen = np.zeros(4, dtype=np.int64)
    full = 0
    for n, sub, taken in ((150_001, "1", 0), (4_200_003, "8", 1), (5_300_003, "8", 1)):
        T = uniform(n)
        sh = level_b_input(emul(), monkeypatch, capfd, T, DIRECT_MODE="linear", DIRECT_SUB=sub)
        assert sh["tile"] == 4096 and sh["threads"] == 1024 and len(sh["tails"]) == 4, sh
        if taken & 1:
            seen += np.array(sh["tails"])
            full += sh["full"]
        st = all_masks(emul(), monkeypatch, T, reference(oracle, ("uni", n), T), taken=taken, DIRECT_MODE="linear", DIRECT_SUB=sub)
        assert st["direct_quantile"] == 0, st
    assert full >= 100 and seen.sum() >= 200 and (seen >= 1).all(), (full, seen)


def test_slot_split_kept_and_the_bucket_indexed_sort_behind_it(oracle, monkeypatch):
    T = uniform(1_000_003)
    st = all_masks(emul(), monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20)
    assert st["direct_quantile"] == 0 and st["slot_splits"] == 1 and st["slot_splits_redone"] == 0 and st["tile_chain"] == 1, st


def test_three_letters_only(oracle, monkeypatch):
    """Key ranges empty at every scale: groups whose segments get one bucket (the route without the LDS histogram, in the same
    launch as the flagged one) and a split that is redone with the count pass."""
    T = uniform(1_000_001, DNA[:3])
    st = all_masks(emul(), monkeypatch, T, reference(oracle, "acg1m", T), p=20)
    assert st["direct_quantile"] == 0 and st["slot_splits_redone"] >= 1, st


@pytest.mark.parametrize("last", [1, 15, 16, 17, GA_E - 1])
def test_level_a_last_tile(oracle, monkeypatch, last):
    n = 9 * GA_E + last
    T = uniform(n)
    all_masks(emul(), monkeypatch, T, reference(oracle, ("uni", n), T), taken=0, DIRECT_MODE="linear")


@pytest.mark.parametrize("k1", [1024, 1025, 1026])
def test_level_a_splitter_table_around_one_load_per_thread(oracle, monkeypatch, k1):
    T = uniform(1_000_003)
    st = all_masks(emul(), monkeypatch, T, reference(oracle, ("uni", T.size), T), p=k1, taken=0, DIRECT_MODE="linear", DIRECT_K1=str(k1))
    assert st["direct_groups"] == k1, st


def test_unchanged_paths_report_zero(oracle, monkeypatch):
    """64-bit indices, quantile mode, 32-bit keys, results that leave in waves, the classic path."""
    T = uniform(1_000_003)
    all_masks(emul(), monkeypatch, T, reference(oracle, ("uni64", T.size), T, bits=64), bits=64, p=20, taken=0)
    want = reference(oracle, ("uni", T.size), T)
    st = all_masks(emul(), monkeypatch, T, want, p=20, taken=0, DIRECT_MODE="quantile")
    assert st["direct_quantile"] == 1, st
    st = all_masks(emul(), monkeypatch, T, want, p=20, taken=0, KEYS="32")
    assert st["direct_key_bits"] == 32, st
    st = all_masks(emul(), monkeypatch, T, want, p=20, taken=0, HOST_WAVES="2")
    assert st["result_waves"] >= 2, st
    S = uniform(200_000)
    all_masks(emul_small(), monkeypatch, S, reference(oracle, ("uni", S.size), S), taken=0, direct=False, PATH="classic")


def _small_cases(oracle):
    """(text, reference, p, taken, settings) at the scale of the 256-element-tile build: last tiles of level B inside every load of
    a thread (see test_small_tiles_...), the route without the LDS histogram and a redone split, last tiles of level A of 1, 15, 16,
    17 and 1,023 positions, 63, 64 and 65 splitters (one load per thread from the splitter table is 64)."""
    for n, sub in ((150_001, "8"), (300_001, "8")):
        T = uniform(n)
        yield T, reference(oracle, ("uni", n), T), 0, 1, dict(DIRECT_MODE="linear", DIRECT_SUB=sub)
    T = uniform(200_001, DNA[:3])
    yield T, reference(oracle, "acg200k", T), 20, 1, dict()
    T = markov(np.random.RandomState(5), 200_000)
    yield T, reference(oracle, "markov200k", T), 0, 1, dict(DIRECT_MODE="linear")
    for last in (1, 15, 16, 17, GA_S - 1):
        n = 9 * GA_S + last
        T = uniform(n)
        yield T, reference(oracle, ("uni", n), T), 0, 0, dict(DIRECT_MODE="linear")
    T = uniform(100_003)
    for k1 in (64, 65, 66):
        yield T, reference(oracle, ("uni", T.size), T), k1, 0, dict(DIRECT_MODE="linear", DIRECT_K1=str(k1))


def test_small_tiles_level_b_last_tiles_end_inside_every_load(oracle, monkeypatch, capfd):
    """What the cases below rely on: the streams of the two uniform texts have last tiles of 1 .. 64, 65 .. 128, 129 .. 192 and
    193 .. 255 elements, and full tiles."""
    seen = np.zeros(4, dtype=np.int64)
    for n in (150_001, 300_001):
        sh = level_b_input(emul_small(), monkeypatch, capfd, uniform(n), DIRECT_MODE="linear", DIRECT_SUB="8")
        assert sh["tile"] == 256 and sh["threads"] == 64 and sh["full"] >= 100, sh
        seen += np.array(sh["tails"])
    assert (seen >= 1).all(), seen


def test_small_tiles_threads_ascending_and_descending(oracle, monkeypatch):
    for E in (emul_small(), emul_rev(True)):
        for T, want, p, taken, env in _small_cases(oracle):
            st = all_masks(E, monkeypatch, T, want, p=p, taken=taken, **env)
            assert st["direct_quantile"] == 0, (env, st)


def test_small_tiles_threads_scattered_over_poisoned_memory(oracle, monkeypatch):
    """LDS and registers start as 0xA5 bytes: the lanes of the early loads beyond a tile's size, the histogram before its zeroing."""
    E, _ = _lib("libcaps_sa_emul_small_poison.so")
    for T, want, p, taken, env in _small_cases(oracle):
        all_masks(E, monkeypatch, T, want, p=p, taken=taken, **env)


def test_small_tiles_free_of_barrier_races(oracle, monkeypatch):
    E, path = _lib("libcaps_sa_emul_small_race.so")
    raw = ctypes.CDLL(path)
    raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
    raw.caps_sa_emul_races_reset()
    for T, want, p, taken, env in _small_cases(oracle):
        all_masks(E, monkeypatch, T, want, p=p, taken=taken, **env)
        races = int(raw.caps_sa_emul_races_found())
        raw.caps_sa_emul_races_reset()
        assert races == 0, (env, races)


def test_full_size_tiles_reversed_and_poisoned(oracle, monkeypatch):
    """The kept slot split with the threads of every phase in descending order, and over poisoned LDS and registers."""
    poison, _ = _lib("libcaps_sa_emul_poison.so")
    T = uniform(1_000_003)
    for E in (emul_rev(False), poison):
        all_masks(E, monkeypatch, T, reference(oracle, ("uni", T.size), T), p=20)
