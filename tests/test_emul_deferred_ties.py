"""CPU: the deferred-tie refinement (kernels.h "Deferred ties, resolved", pipeline.h msd_refine) at every route, size and window
edge, on the host emulation of the kernels.  The texts and the witnesses are tests/deferred_tie_cases.py's: every case proves from
the library's own output (the sentinels a build with CAPS_SA_DEBUG_NO_MSD leaves, the "[msd]" lines of CAPS_SA_DEBUG) that a
group of exactly the intended size existed at the intended level, and compares SA and LCP entry by entry with tests/sa_check.py.

The small emulation has tiles of 256 elements: finish <= 32, quick classes <= 16 (EMPTY: below MSD_FIN_MAX) / 64 / 256, the loop
above.  Level 0 = left open by the sort (generation 0), level 1 = left open by the first level of the loop (generation 1)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import deferred_tie_cases as C
from emul_util import EMUL_DIR, emul, emul_rev, emul_small

TILE = 256
ALPHABETS = {"dna": C.DNA, "wide": C.WIDE}
# (n, segment length) per alphabet: families up to TIE_BIG_CAP members need hundreds of chars to be left open, larger ones do not
SMALL = {"dna": (600_000, 400), "wide": (400_000, 120)}
BIG = {"dna": (600_000, 100), "wide": (400_000, 40)}
NESTED = {"dna": (400_000, 100, 40), "wide": (200_000, 40, 20)}          # n, L, q
JUMP = {"dna": (600_000, 384), "wide": (600_000, 320)}                     # n, L: 12 / 40 windows
SMALL_SIZES = [2, 16, 17, 31, 32, 33, 64, 65]
BIG_SIZES = [255, 256, 257, 513]

AB = pytest.mark.parametrize("alpha,bits", [("dna", 32), ("dna", 64), ("wide", 32), ("wide", 64)])


def _small(alpha):
    """Eight families, one per size."""
    def make():
        n, L = SMALL[alpha]
        return C.families(n, [(k, L) for k in SMALL_SIZES], alphabet=ALPHABETS[alpha])
    return C.reference(("small", alpha), make)


@AB
def test_sizes_up_to_a_quarter_tile_at_level_0(alpha, bits, monkeypatch, capfd):
    """Level 0: groups of exactly 2, 31, 32 (msd_finish_kernel), 33, 64 (msd_quick_kernel, class 1) and 65 members (class 2)."""
    T, want, _ = _small(alpha)
    groups, gens, st = C.check(emul_small(), monkeypatch, capfd, T, want[bits], TILE, bits=bits)
    sizes = C.size_counts(groups)
    for s in (2, 31, 32, 33, 64, 65):
        assert sizes.get(s, 0) >= 1, (s, sizes)
    assert gens[0]["quick"][0] == 0 and gens[0]["quick"][1] >= 2 and gens[0]["quick"][2] >= 1, gens[0]
    assert st["tie_levels"] == 0


def _big(alpha):
    """Four families; the one of TILE_E + 1 starts with 3/4 KCH times the smallest letter, the one of 2 TILE_E + 1 with 3/4 KCH times
    the largest (a whole key of one letter would not do: the char before a copy may not be that letter, and it is random)."""
    def make():
        A = ALPHABETS[alpha]
        n, L = BIG[alpha]
        order, K = C.signed_order(A), C.kch(A)
        return C.families(n, [(k, L) for k in BIG_SIZES], alphabet=A, seed=5, head=[None, None, (order[0], K - K // 4), (order[-1], K - K // 4)])
    return C.reference(("big", alpha), make)


@AB
def test_sizes_around_a_tile_at_level_0_and_both_ends_of_the_rank_range(alpha, bits, monkeypatch, capfd):
    """Level 0: groups of exactly TILE_E - 1 and TILE_E members (the largest class of msd_quick_kernel, full to its last member)
    and of TILE_E + 1 and 2 TILE_E + 1 (the level loop: one and two tiles above).  The group of the smallest letter's head starts
    at rank 0 -- LCP[0] stays 0, msd_fix_edges_kernel skips that edge -- and the group of the largest letter's head ends at rank
    n - 1: the edge behind it is no entry of LCP."""
    T, want, _ = _big(alpha)
    groups, gens, st = C.check(emul_small(), monkeypatch, capfd, T, want[bits], TILE, bits=bits)
    sizes = C.size_counts(groups)
    for s in BIG_SIZES:
        assert sizes.get(s, 0) >= 8, (s, sizes)
    assert gens[0]["above_tile"] == sizes[257] + sizes[513] and gens[0]["largest"] == 513, gens[0]
    assert min(groups) == (0, 257), min(groups)
    assert max((f + s, s) for f, s in groups) == (T.size, 513), (max(groups), T.size)
    assert st["tie_levels"] >= 1


def _nested(alpha):
    def make():
        n, L, q = NESTED[alpha]
        return C.nested(n, C.edge_sizes(TILE), L, q, alphabet=ALPHABETS[alpha])
    return C.reference(("nested", alpha), make)


@AB
def test_every_size_at_level_1(alpha, bits, monkeypatch, capfd):
    """Level 1: one family of 1,541 copies is one group at level 0 (the loop) and splits in the first level into groups of exactly
    2, 16, 17, 31, 32, 33, 64, 65, 255, 256, 257 and 513 members -- every route chosen again from the tables of generation 1,
    at depth 2 KCH.  The groups of 257 and 513 stay whole for another level: the loop has at least three."""
    T, want, _ = _nested(alpha)
    groups, gens, st = C.check(emul_small(), monkeypatch, capfd, T, want[bits], TILE, bits=bits)
    K = sum(C.edge_sizes(TILE))
    assert C.size_counts(groups).get(K, 0) >= 1, C.size_counts(groups)
    assert len(gens) >= 3 and gens[1]["depth_min"] == 2 * C.kch(ALPHABETS[alpha]), gens[1]
    for s in C.edge_sizes(TILE):
        assert gens[1]["sizes"].get(s, 0) >= 1, (s, gens[1]["sizes"])
    assert gens[1]["quick"][0] == 0 and gens[1]["quick"][1] >= 2 and gens[1]["quick"][2] >= 2 and gens[1]["above_tile"] >= 2
    assert st["tie_levels"] == len(gens) - 1 >= 2


def _jump(alpha, run):
    def make():
        A = ALPHABETS[alpha]
        n, L = JUMP[alpha]
        if run:
            n, L = 1_200_000, 40 + run + 30
        return C.long_agreement(n, 260 if run else 300, L, run=run, alphabet=A)
    return C.reference(("jump", alpha, run), make)


@pytest.mark.parametrize("run", [0, C.RUN_TABLE_MIN - 1, C.RUN_TABLE_MIN, C.RUN_TABLE_MIN + 6])
@AB
def test_groups_above_a_tile_that_agree_for_tens_of_windows_jump(alpha, bits, run, monkeypatch, capfd):
    """300 copies (above a tile) that agree for 12 (40) windows, or 260 that agree through a single-letter run of 1,023 chars (just
    below the run table's threshold: long_runs stays 0, the plain builds of msd_jump_kernel, msd_finish_kernel and msd_quick_kernel
    walk the run window by window), of 1,024 and of 1,030 chars (a stretch of the run table: long_runs, the <LONG = true> builds).  A level
    that leaves a group whole makes it jump to the whole windows of what its members share (msd_jump_apply_kernel rounds down:
    offset j shares L - j chars, every residue modulo KCH): some generation stands deeper than a window per level could have
    brought it, and the loop is over after a handful of levels instead of one per window."""
    T, want, _ = _jump(alpha, run)
    K = C.kch(ALPHABETS[alpha])
    groups, gens, st = C.check(emul_small(), monkeypatch, capfd, T, want[bits], TILE, bits=bits)
    assert st["long_runs"] == (1 if run >= C.RUN_TABLE_MIN else 0)
    assert C.size_counts(groups).get(260 if run else 300, 0) >= K, C.size_counts(groups)
    assert any(g["depth_max"] > (lvl + 3) * K for lvl, g in enumerate(gens)), [(g["depth_min"], g["depth_max"]) for g in gens]
    assert 2 <= st["tie_levels"] <= 8, st["tie_levels"]
    if run:                     # the groups the jump leaves are finished by finish and quick, in the same build (<LONG> or plain)
        assert any(g["depth_max"] > run for g in gens), [(g["depth_min"], g["depth_max"]) for g in gens]    # jumped through the run
        assert any(s <= C.FIN_MAX for s in gens[-1]["sizes"]), gens[-1]
        if alpha == "dna":      # (over 64 letters the family's parts are all of at most 32 members: no group for msd_quick_kernel)
            assert any(g["in_lds"] for g in gens), gens


def _cuts(alpha):
    """The lengths of the text's last suffix inside a family: D + KCH - 1, D + KCH, D + KCH + 1 for D = KCH, 2 KCH, 3 KCH (msd_ending's
    bound at levels 0, 1 and 2), and at 8 chars per window every length in between for the first window."""
    K = C.kch(ALPHABETS[alpha])
    cuts = {D + K + d for D in (K, 2 * K, 3 * K) for d in (-1, 0, 1)}
    if K == 8:
        cuts |= set(range(2 * K - 1, 3 * K + 2))
    return sorted(cuts)


def _members_of_a_group(groups, SA, positions, size):
    """Every suffix of `positions` stands inside an open group of exactly `size` members (SA: the reference's)."""
    rank = np.empty(SA.size, dtype=np.int64)
    rank[SA.astype(np.int64)] = np.arange(SA.size)
    first = np.array([f for f, _ in groups])
    for pos in positions:
        g = groups[int(np.searchsorted(first, rank[pos], side="right")) - 1]
        assert g[0] <= rank[pos] < g[0] + g[1] and g[1] == size, (pos, int(rank[pos]), g)


@pytest.mark.parametrize("last", [300, 200])
@AB
def test_a_text_that_ends_inside_a_family(alpha, bits, last, monkeypatch, capfd):
    """The text ends c chars into one more copy of a family of 300 (the loop: msd_classify_kernel's msd_ending) or 200 copies
    (msd_quick_kernel's): that suffix is a prefix of the family's other members, a member of their group at level 0 and must come
    first; its n - sa lands on both sides of msd_ending's bound at levels 0, 1 and 2.  The same holds at every offset j <= c - KCH
    of the cut copy, where n - sa = c - j: asserted from the sentinels for EVERY such offset, so that each text has a member of a
    group of last + 1 at every length from c down to KCH -- at 32 chars per window every residue of three windows per text, where
    the cuts themselves sweep a whole window only at 8 chars per window."""
    A = ALPHABETS[alpha]
    K = C.kch(A)
    E = emul_small()
    for c in _cuts(alpha):
        T, want, fam = C.reference(("cut", alpha, last, c), lambda: C.families(
            420_000 if K == 32 else 120_000, [(500 - last, 5 * K), (last, 5 * K)], alphabet=A, seed=7, cut=c))
        assert T.size - fam[0][-1][-1] == c
        groups, gens, st = C.check(E, monkeypatch, capfd, T, want[bits], TILE, bits=bits)
        _members_of_a_group(groups, want[bits][0], range(T.size - c, T.size - K + 1), last + 1)
        assert st["tie_levels"] >= 1


@pytest.mark.parametrize("last", [300, 200])
@AB
def test_a_suffix_that_ends_inside_the_key_of_a_family(alpha, bits, last, monkeypatch, capfd):
    """The segment is h random chars and then more than KCH times the smallest letter; the text ends h + 2 chars into one more copy.
    Padded with the smallest code that suffix HAS the family's key: it is a member of the group of offset 0 although it is shorter
    than the key (n - sa < KCH), the stable merges may leave it anywhere in the group, and the LCP behind the group is taken from
    the text again once the group is in order (msd_edges_kernel, msd_fix_edges_kernel).  So are its own suffixes at the offsets
    1 .. h - 1."""
    A = ALPHABETS[alpha]
    K = C.kch(A)
    h = K // 4 + 2
    E = emul_small()
    T, want, fam = C.reference(("short", alpha, last), lambda: C.families(
        420_000 if K == 32 else 120_000, [(500 - last, 5 * K), (last, 5 * K)], alphabet=A, seed=9, cut=h + 2,
        head=[None, (C.signed_order(A)[0], K + 8, h)]))
    groups, gens, st = C.check(E, monkeypatch, capfd, T, want[bits], TILE, bits=bits)
    _members_of_a_group(groups, want[bits][0], range(T.size - (h + 2), T.size - 2), last + 1)
    assert st["tie_levels"] >= 1


@AB
def test_results_that_leave_in_waves_and_both_level_b_modes(alpha, bits, monkeypatch, capfd):
    """The nested family under CAPS_SA_HOST_WAVES=3 (every wave refines the groups of its own slice) and the families around a tile
    under CAPS_SA_DIRECT_MODE=quantile, the small families under linear."""
    T, want, _ = _nested(alpha)
    groups, gens, st = C.check(emul_small(), monkeypatch, capfd, T, want[bits], TILE, bits=bits, HOST_WAVES="3")
    assert st["result_waves"] >= 2 and st["tie_levels"] >= 2
    T, want, _ = _big(alpha)
    groups, gens, st = C.check(emul_small(), monkeypatch, capfd, T, want[bits], TILE, bits=bits, DIRECT_MODE="quantile")
    assert st["tie_levels"] >= 1 and C.size_counts(groups).get(256, 0) >= 1, C.size_counts(groups)
    # linear buckets cannot split a key that hundreds of suffixes share: such a text takes the samplesort path (CAPS_SA_FB_PIVOT_TIES,
    # nothing is deferred there); the families of up to 65 members stay on the direct path at 2 bits per char
    T, want, _ = _small(alpha)
    if alpha == "dna":
        groups, gens, st = C.check(emul_small(), monkeypatch, capfd, T, want[bits], TILE, bits=bits, DIRECT_MODE="linear")
        assert all(C.size_counts(groups).get(s, 0) >= 1 for s in (32, 33, 64, 65)), C.size_counts(groups)
    else:
        monkeypatch.setenv("CAPS_SA_DIRECT_MODE", "linear")
        SA, LCP, st = emul_small().build(T, idx_bits=bits)
        assert np.array_equal(SA, want[bits][0]) and np.array_equal(LCP, want[bits][1])
        assert st["path_direct"] == 0 and st["path_fallback"] == 4 and st["tie_groups_deferred"] == 0


def _other(name):
    import caps_sa_amd
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, name])
    path = os.path.join(EMUL_DIR, name)
    return caps_sa_amd.CapsLib(path, "caps_sa_emul_"), ctypes.CDLL(path)


@pytest.mark.slow
@pytest.mark.parametrize("build", ["rev", "poison", "race"])
@AB
def test_every_route_in_the_other_emulation_builds(alpha, bits, build, monkeypatch, capfd):
    """The nested family -- every route at level 0 or level 1, four levels -- with the threads of every phase in descending order,
    with LDS and registers starting as 0xA5 bytes, and under the barrier-race detector (msd_quick_kernel hands its members over
    through LDS three times per round)."""
    T, want, _ = _nested(alpha)
    if build == "rev":
        E, raw = emul_rev(True), None
    else:
        E, raw = _other("libcaps_sa_emul_small_%s.so" % build)
    if build == "race":
        raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
        raw.caps_sa_emul_races_reset()
    groups, gens, st = C.check(E, monkeypatch, capfd, T, want[bits], TILE, bits=bits)
    for s in C.edge_sizes(TILE):
        assert gens[1]["sizes"].get(s, 0) >= 1, (s, gens[1]["sizes"])
    if build == "race":
        assert int(raw.caps_sa_emul_races_found()) == 0


@pytest.mark.slow
@pytest.mark.parametrize("name", sorted(C.FULL))
@pytest.mark.parametrize("bits", [32, 64])
def test_the_edges_at_full_tiles(bits, name, oracle, monkeypatch, capfd):
    """The texts of the GPU file (tiles of 4,096 elements: classes of 256 / 1,024 / 4,096 members) on the full emulation."""
    C.full_case(emul(), monkeypatch, capfd, oracle, name, bits=bits)


def _edge_text():
    rs = np.random.RandomState(101)
    T = rs.choice(C.DNA, size=150_001, p=[0.72, 0.1, 0.1, 0.08])
    T[-40:] = ord("A")
    return T


@pytest.mark.parametrize("bits", [32, 64])
def test_an_lcp_at_the_end_of_a_group_that_the_sort_left_wrong(bits, monkeypatch, capfd):
    """msd_edges_kernel / msd_fix_edges_kernel: in a text of 72 % A's that ends in 40 A's the suffixes near the end have -- padded --
    the keys of longer ones, and with 20 subproblems one group is left with a member shorter than the key where the LCP behind
    the group was emitted from another member: the build without msd_refine has that LCP WRONG (asserted), the build has it right.
    (The one text of test_emul_pipeline.py's six on which a refinement without msd_fix_edges_kernel fails.)"""
    T, want, _ = C.reference(("edge",), _edge_text)
    E = emul_small()
    groups, gens, st = C.check(E, monkeypatch, capfd, T, want[bits], TILE, bits=bits, p=20)
    assert groups and groups.edges_to_fix >= 1, (len(groups), groups.edges_to_fix)
