"""Shared by test_emul_deferred_ties.py and test_gpu_deferred_ties.py: texts whose groups of equal keys take a chosen route of the
deferred-tie refinement (kernels.h "Deferred ties, resolved", pipeline.h msd_refine), and the witnesses that prove from the
library's own output that they did.

A group of equal keys is routed by its member count alone: <= 32 msd_finish_kernel, <= TILE_E / 16, / 4, / 1 msd_quick_kernel in
three capacity classes, larger ones the level loop (rekey, sort, msd_classify_kernel, msd_compact_kernel), where the routes are
chosen again for every generation of groups.  The sizes at the edges of the routes, for a library with tiles of `tile_e` elements
(256 in the small emulation, where the class of TILE_E / 16 = 16 < 32 members is empty by construction: msd_groups_kernel asks for
MSD_FIN_MAX first; 4,096 in the full emulation and on the GPU): see edge_sizes().

Which sizes a text can leave open at level 0 (measured, see DESIGN.md "Deferred ties"): a group is left open only in a tile that
reaches tile_sort_general_kernel, and the tile sorts before it settle a tie themselves when few suffixes share few windows.  The
segmented sort then defers only while the comparison sort's tiles hold at most half the elements (segmented_sort defer_check).
Every size of edge_sizes() that a family leaves open at level 0 is witnessed there by groups_left_open(); every size is witnessed
at level 1 as well, by a nested family whose copies differ in the second window (levels(): the sizes of generation 1)."""
import re

import numpy as np

DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
# 64 letters, five of them >= 0x80: in the order of the text (signed char) 0x80 is the smallest letter and 'z' the largest
WIDE = np.frombuffer(bytes([0x80, 0x81, 0x9c, 0xe9, 0xfe]) + bytes(range(0x30, 0x3a)) + bytes(range(0x41, 0x5b)) +
                     bytes(range(0x61, 0x78)), dtype=np.uint8)
assert WIDE.size == 64 and np.unique(WIDE).size == 64
ENV = ("CAPS_SA_DIRECT_MODE", "CAPS_SA_HOST_WAVES", "CAPS_SA_NO_DEFER", "CAPS_SA_DEBUG", "CAPS_SA_DEBUG_NO_MSD", "CAPS_SA_PATH",
       "CAPS_SA_TEST_MSD_FAIL", "CAPS_SA_TEST_MSD_MAX_LEVELS", "CAPS_SA_TILE_CHAIN")
FIN_MAX = 32                # kernels.h MSD_FIN_MAX
RUN_TABLE_MIN = 1024        # text.h: a single-letter run of at least this many chars enters the run table (stats: long_runs)


def kch(alphabet):
    """Chars per key and per level (text.h TextTraits::KCH): 32 at 2 bits per char, 8 at 8."""
    return 32 if np.unique(alphabet).size <= 4 else 8


def signed_order(alphabet):
    """The letters in the order of the text: bytes as signed char (sa_check.py)."""
    a = np.unique(alphabet)
    return a[np.argsort(a.view(np.int8), kind="stable")]


def edge_sizes(tile_e):
    """The member counts at which a group changes its route, and one far inside the loop."""
    s = [2, FIN_MAX - 1, FIN_MAX, FIN_MAX + 1, tile_e // 16, tile_e // 16 + 1, tile_e // 4, tile_e // 4 + 1, tile_e - 1, tile_e,
         tile_e + 1, 2 * tile_e + 1]
    return sorted(set(s))


def route(size, tile_e):
    """The route msd_groups_kernel gives a group of `size` members: 'finish', 'quick0' .. 'quick2', 'loop'."""
    if size <= FIN_MAX:
        return "finish"
    for c, cap in enumerate((tile_e // 16, tile_e // 4, tile_e)):
        if size <= cap:
            return "quick%d" % c
    return "loop"


# ---- generators (deterministic) -------------------------------------------------------------------------------------------------

def _gap(rs, alphabet):
    return rs.choice(alphabet, size=rs.randint(7, 12))


def _place(rs, T, at, copies, alphabet, avoid=None):
    """Lays the copies out from `at` on, 7 to 11 random chars between them (avoid: a letter the char before a copy must not be);
    -> the starts and the position behind the last one."""
    starts = []
    other = None if avoid is None else np.unique(alphabet)[np.unique(alphabet) != avoid][1]
    for c in copies:
        if at + c.size > T.size:
            raise ValueError("the text is too short for its families")
        T[at:at + c.size] = c
        if other is not None and T[at - 1] == avoid:
            T[at - 1] = other
        starts.append(at)
        g = _gap(rs, alphabet)
        at += c.size
        T[at:at + g.size] = g[:max(0, T.size - at)]
        at += g.size
    return starts, at


def families(n, specs, alphabet=DNA, seed=1, head=(), cut=None):
    """Random text of n chars over `alphabet` with planted families: for every (k, L) of `specs`, k exact copies of one random
    segment of L chars, one after another with gaps of 7 to 11 random chars; the families follow each other from n // 16 on.
    The suffixes at offset j of the copies share L - j chars: k members with one key for every j <= L - KCH.
    head: per family, optionally (letter, count[, at = 0]) -- the segment holds `count` times `letter` from char `at` on, with another
    letter before and behind them; at = 0: when the letter is the smallest (largest) one and the text holds no other run of `count` of them, the suffixes
    at offset 0 are the first (last) of the suffix array.
    cut = c: the text ends c chars into one more copy of the LAST family (that suffix ends inside its group's windows).
    -> T, [starts of the copies per family]."""
    rs = np.random.RandomState(seed)
    if cut is None:
        T = rs.choice(alphabet, size=n)
        at = n // 16
    else:                                                  # (the families behind n random chars: the text ends inside the last one)
        T = rs.choice(alphabet, size=n + sum(k * (L + 12) + 64 for k, L in specs))
        at = n
    out = []
    letters = np.unique(alphabet)
    for f, (k, L) in enumerate(specs):
        seg = rs.choice(alphabet, size=L)
        avoid = None
        if f < len(head) and head[f]:
            letter, count, h0 = (tuple(head[f]) + (0,))[:3]
            seg[h0:h0 + count] = letter
            seg[h0 + count] = letters[letters != letter][f % (letters.size - 1)]
            if h0:
                seg[h0 - 1] = letters[letters != letter][(f + 1) % (letters.size - 1)]
            else:
                avoid = letter
        starts, at = _place(rs, T, at, [seg] * k, alphabet, avoid)
        out.append(starts)
        at += 64
        if cut is not None and f == len(specs) - 1:
            T = np.concatenate([T[:at], seg[:cut]])
            out[-1] = starts + [at]
    if cut is None and at > n - 64:
        raise ValueError("the text is too short for its families")
    if cut is None and any(head):
        T[-1] = signed_order(alphabet)[letters.size // 2]   # (the text's last suffix is one char: not the smallest letter)
    return T, out


def nested(n, sizes, L, q, alphabet=DNA, seed=2, at=None):
    """One family of sum(sizes) copies of a segment of L chars in a random text of n chars; the copies of sub-family i carry the
    digits of i (base = letters of the alphabet) at chars q .. q + w - 1 of the segment and are otherwise equal, and the
    sub-families are shuffled along the text.  The suffixes at offset j share q - j chars as a whole family and L - j chars inside
    a sub-family: for KCH <= q - j and q + w - j <= 2 KCH the family is ONE group at level 0 that the first level of the loop
    splits into groups of exactly `sizes` members (generation 1), which agree to the end of the segment.
    -> T, [the starts of the copies per sub-family], w."""
    rs = np.random.RandomState(seed)
    letters = np.unique(alphabet)
    w = 1
    while letters.size ** w < len(sizes):
        w += 1
    T = rs.choice(alphabet, size=n)
    seg = rs.choice(alphabet, size=L)
    sub = rs.permutation(np.repeat(np.arange(len(sizes)), sizes))
    copies = []
    for i in sub:
        c = seg.copy()
        for d in range(w):
            c[q + d] = letters[(i // letters.size ** d) % letters.size]
        copies.append(c)
    starts, end = _place(rs, T, n // 16 if at is None else at, copies, alphabet)
    if end > n - 64:
        raise ValueError("the text is too short for its family")
    starts = np.array(starts)
    return T, [starts[sub == i] for i in range(len(sizes))], w


def long_agreement(n, k, L, run=0, alphabet=DNA, seed=3):
    """k copies of a segment of L chars (k above a tile, L tens of windows: the level loop leaves the groups unchanged and they
    jump, msd_jump_kernel / msd_jump_apply_kernel, to the whole windows of the L - j chars that offset j shares -- every residue
    modulo KCH over the offsets).  run > 0: chars 40 .. 40 + run - 1 of the segment are one letter (run >= RUN_TABLE_MIN: every copy
    is a stretch of the run table, the <LONG = true> builds of jump, finish and quick run)."""
    rs = np.random.RandomState(seed)
    T = rs.choice(alphabet, size=n)
    seg = rs.choice(alphabet, size=L)
    if run:
        letters = np.unique(alphabet)
        seg[40:40 + run] = letters[1]
        seg[39] = seg[40 + run] = letters[2]
    starts, end = _place(rs, T, n // 16, [seg] * k, alphabet)
    if end > n - 64:
        raise ValueError("the text is too short for its family")
    return T, starts


# ---- witnesses ------------------------------------------------------------------------------------------------------------------

def _clear(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv("CAPS_SA_" + k, v)


class Groups(list):
    """[(first rank, members)] of the groups a sort left open; edges_to_fix = how many LCPs behind a group the sort left wrong."""
    edges_to_fix = 0


def groups_left_open(lib, monkeypatch, T, want, bits=32, p=0, **env):
    """One build with CAPS_SA_DEBUG_NO_MSD=1 (pipeline.h finalize(): msd_refine is skipped, the sentinels stay).  Every maximal run
    of the all-ones LCP value plus the entry before it is one level-0 group.  -> [(first rank, members)], after asserting against
    `want` (the reference's SA, LCP) that the SA entries of every group are, as a set, the reference's at those ranks, and that
    every entry outside the groups is final already -- SA and LCP, except the LCP BEHIND a group with a member that ends inside the
    key (msd_fix_edges_kernel; counted in the result's edges_to_fix).  The LCP at the HEAD of a group is final whichever member stood
    there: the suffix before the group has a smaller padded key, the pad is the smallest code, so the two keys differ before the
    shortest member ends, and that LCP is the same for every member."""
    _clear(monkeypatch, env)
    monkeypatch.setenv("CAPS_SA_DEBUG_NO_MSD", "1")
    SA, LCP, st = lib.build(T, p=p, idx_bits=bits)
    monkeypatch.delenv("CAPS_SA_DEBUG_NO_MSD")
    assert st["path_direct"] == 1, st["path_fallback"]
    sent = np.iinfo(SA.dtype).max
    tied = LCP == sent
    assert not tied[0]
    d = np.diff(np.concatenate([[0], tied.view(np.int8), [0]]))
    first, end = np.flatnonzero(d == 1) - 1, np.flatnonzero(d == -1)
    member = tied.copy()
    member[first] = True
    assert np.array_equal(SA[~member], want[0][~member]), "an entry outside the open groups is not final"
    gid = np.cumsum(member & ~tied) - 1
    # the LCPs that are not sentinels are final -- but the one behind a group with a member that ends inside the key: the sort
    # emitted it from whichever member stood last (msd_edges_kernel; taken from the text again by msd_fix_edges_kernel)
    inner = ~tied
    short = np.zeros(first.size, dtype=bool)
    short[np.unique(gid[member & (T.size - SA.astype(np.int64) <= kch(T))])] = True
    edge = end[short & (end < tied.size)]
    inner[edge] = False
    assert np.array_equal(LCP[inner], want[1][inner]), "an LCP outside the open groups is not final"
    a = np.lexsort((SA[member], gid[member]))
    b = np.lexsort((want[0][member], gid[member]))
    assert np.array_equal(SA[member][a], want[0][member][b]), "a group's members are not the reference's at its ranks"
    out = Groups((int(f), int(e - f)) for f, e in zip(first, end))
    out.edges_to_fix = int((LCP[edge] != want[1][edge]).sum())
    return out


# pipeline.h msd_refine, the two lines per generation of groups (see the comment at the fprintf of "[msd] generation")
_LEVEL = re.compile(r"\[msd\] (?:level 0: \d+ flagged tiles, \d+ elements in them,|depth (\d+):) (\d+) groups of (\d+) members, "
                    r"(\d+) above (\d+) finished in LDS, (\d+) above (\d+) \(largest (\d+)\)")
_SIZES = re.compile(r"\[msd\] generation (\d+): quick classes (\d+) (\d+) (\d+), depths (\d+) to (\d+), sizes((?: \d+x\d+)*)")


def levels(lib, monkeypatch, capfd, T, bits=32, p=0, **env):
    """One build with CAPS_SA_DEBUG=1.  -> (SA, LCP, stats, [per generation of groups: dict(groups, members, in_lds, fin_max,
    above_tile, tile_e, largest, quick = groups per capacity class, depth_min, depth_max = the chars the groups are known to share,
    sizes = {members: groups})]); generation 0 is what the sort left open, generation L what level L of the loop left."""
    _clear(monkeypatch, env)
    monkeypatch.setenv("CAPS_SA_DEBUG", "1")
    capfd.readouterr()
    SA, LCP, st = lib.build(T, p=p, idx_bits=bits)
    err = capfd.readouterr().err
    monkeypatch.delenv("CAPS_SA_DEBUG")
    a, b = _LEVEL.findall(err), _SIZES.findall(err)
    assert len(a) == len(b), err[-3000:]
    out = []
    lvl = -1
    for x, y in zip(a, b):
        lvl = 0 if not x[0] else lvl + 1                  # (results that leave in waves: every wave refines its own groups)
        assert int(y[0]) == lvl, err[-3000:]
        sizes = {int(s): int(c) for s, c in (t.split("x") for t in y[6].split())}
        g = dict(groups=int(x[1]), members=int(x[2]), in_lds=int(x[3]), fin_max=int(x[4]), above_tile=int(x[5]), tile_e=int(x[6]),
                 largest=int(x[7]), quick=tuple(int(v) for v in y[1:4]), depth_min=int(y[4]), depth_max=int(y[5]), sizes=sizes)
        # the log agrees with itself: the routes are a function of the sizes
        assert sum(sizes.values()) == g["groups"] and sum(s * c for s, c in sizes.items()) == g["members"], g
        assert g["fin_max"] == FIN_MAX and sum(g["quick"]) == g["in_lds"], g
        by = {}
        for s, c in sizes.items():
            by[route(s, g["tile_e"])] = by.get(route(s, g["tile_e"]), 0) + c
        assert tuple(by.get("quick%d" % c, 0) for c in range(3)) == g["quick"] and by.get("loop", 0) == g["above_tile"], (g, by)
        assert g["largest"] == (max(sizes) if g["above_tile"] else 0), g
        if lvl == len(out):
            out.append(g)
        else:                                              # another wave's generation `lvl`: added up
            o = out[lvl]
            for k in ("groups", "members", "in_lds", "above_tile"):
                o[k] += g[k]
            o["quick"] = tuple(u + v for u, v in zip(o["quick"], g["quick"]))
            o["largest"], o["depth_max"] = max(o["largest"], g["largest"]), max(o["depth_max"], g["depth_max"])
            o["depth_min"] = min(o["depth_min"], g["depth_min"])
            for k, v in sizes.items():
                o["sizes"][k] = o["sizes"].get(k, 0) + v
    return SA, LCP, st, out


def check(lib, monkeypatch, capfd, T, want, tile_e, bits=32, p=0, **env):
    """The whole check of one text under one setting: the witness build, the logged build and the build without deferring, all equal
    to `want` entry by entry; the statistics equal the witness's counts; generation 0 of the log is the witness's groups.
    -> (groups, generations, stats)."""
    groups = groups_left_open(lib, monkeypatch, T, want, bits=bits, p=p, **env)
    SA, LCP, st, gens = levels(lib, monkeypatch, capfd, T, bits=bits, p=p, **env)
    bad = np.flatnonzero(SA != want[0])
    assert bad.size == 0, ("SA", bad[:8], SA[bad[:8]], want[0][bad[:8]])
    bad = np.flatnonzero(LCP != want[1])
    assert bad.size == 0, ("LCP", bad[:8], LCP[bad[:8]], want[1][bad[:8]], SA[bad[:8]])
    assert st["path_direct"] == 1
    assert st["tie_groups_deferred"] == len(groups) and st["tie_elems_deferred"] == sum(s for _, s in groups), (st, len(groups))
    if groups:
        assert gens and gens[0]["tile_e"] == tile_e, (gens[:1], tile_e)
        sizes = {}
        for _, s in groups:
            sizes[s] = sizes.get(s, 0) + 1
        assert gens[0]["sizes"] == sizes
        assert st["tie_levels"] == len(gens) - 1, (st["tie_levels"], len(gens))
    else:
        assert not gens
    monkeypatch.setenv("CAPS_SA_NO_DEFER", "1")
    SA2, LCP2, st2 = lib.build(T, p=p, idx_bits=bits)
    monkeypatch.delenv("CAPS_SA_NO_DEFER")
    assert st2["tie_groups_deferred"] == 0
    assert np.array_equal(SA2, SA) and np.array_equal(LCP2, LCP), "the build that compares every tie differs"
    for k in env:
        monkeypatch.delenv("CAPS_SA_" + k, raising=False)
    return groups, gens, st


# ---- the texts ------------------------------------------------------------------------------------------------------------------
# Sizes chosen for the deferring floor (segmented_sort defer_check): n exceeds twice the elements of the comparison sort's tiles.
# Families of at most TIE_BIG_CAP members are left open only with segments of hundreds of chars (the tile sorts before the
# comparison sort settle shorter ties), and every (family, offset) pair then costs a tile: at 256-element tiles eight such
# families fit 600,000 chars, at 4,096-element tiles ONE family of 400 chars needs n > 3,000,000 -- there the small sizes are the
# sub-families of a nested family above a tile (level 0 where its digits lie inside the key, level 1 where they lie in the second window).
# Larger families need two keys' length at any tile size.

def _ref(T):
    from sa_check import sa_lcp
    return sa_lcp(T)


_refs = {}


def reference(key, make):
    """(T, (SA, LCP) at 32 bits, (SA, LCP) at 64 bits, extra) of a text, made and solved once per session (tests/sa_check.py),
    never modified."""
    if key not in _refs:
        made = make()
        T, extra = (made[0], made[1:]) if isinstance(made, tuple) else (made, ())
        sa, lcp = _ref(T)
        w32, w64 = (sa, lcp), (sa.astype(np.uint64), lcp.astype(np.uint64))
        for a in (T,) + w32 + w64:
            a.setflags(write=False)
        _refs[key] = (T, {32: w32, 64: w64}, extra)
    return _refs[key]


def size_counts(groups):
    out = {}
    for _, s in groups:
        out[s] = out.get(s, 0) + 1
    return out


# ---- the texts at tiles of 4,096 elements (the full emulation and the GPU) -------------------------------------------------------
FULL_TILE = 4096


def _full_edges(alphabet=DNA, n=3_000_000, L=64):
    order, K = signed_order(alphabet), kch(alphabet)
    return families(n, [(k, L) for k in (1025, 4096, 4097)], alphabet=alphabet, seed=11,
                    head=[None, (order[0], K - K // 4), (order[-1], K - K // 4)])[0]


def _full_long():
    """One family above a tile that agrees for 7 windows, and ONE single-letter run of 1,030 chars: a stretch of the run table, so that
    every kernel of the refinement runs in its <LONG = true> build (at these tiles a family of such runs makes their key frequent
    enough for CAPS_SA_FB_GROUP_OVERFLOW: 8 copies do; the small emulation's text has 260)."""
    T, _ = long_agreement(4_500_000, 4100, 224, seed=13)
    T[3_000_000:3_001_030] = DNA[1]
    T[2_999_999] = T[3_001_030] = DNA[3]
    return T


FULL = {
    # level 0: TILE_E / 4 + 1, TILE_E (msd_quick_kernel's largest class: 128 KB of LDS) and TILE_E + 1 (the loop); the family of
    # TILE_E starts at rank 0, the one of TILE_E + 1 ends at rank n - 1
    "edges": _full_edges,
    # level 0: TILE_E - 1 and 2 TILE_E + 1
    "around": lambda: families(3_200_000, [(k, 64) for k in (4095, 8193)], seed=12)[0],
    # level 1: 2, 31, 32 (finish), 33, 256 (class 0), 257, 1024 (class 1), 1025 (class 2), 4097 (the loop)
    "nested_small": lambda: nested(2_400_000, [2, 31, 32, 33, 256, 257, 1024, 1025, 4097], 72, 40, seed=15)[0],
    # level 1: 4095, 4096 (class 2), 8193 (the loop)
    "nested_big": lambda: nested(3_600_000, [4095, 4096, 8193], 72, 40, seed=16)[0],
    # the jump and the <LONG = true> builds (a run-table stretch: long_runs)
    "long": _full_long,
    # 8 bits per char (KCH = 8): "edges" and "nested_small" over 64 letters
    "edges_wide": lambda: _full_edges(WIDE, 2_000_000, 24),
    "nested_wide": lambda: nested(2_000_000, [2, 31, 32, 33, 256, 257, 1024, 1025, 4097], 40, 20, alphabet=WIDE, seed=17)[0],
}
# (nested_small: at the offsets where the digits lie inside the key the sub-families are groups of level 0 already)
FULL_LEVEL0 = {"edges": (1025, 4096, 4097), "around": (4095, 8193), "nested_small": (6757, 2, 31, 32, 33, 256, 257, 1024, 1025, 4097), "nested_big": (16384,), "long": (4100,),
               "edges_wide": (1025, 4096, 4097), "nested_wide": (6757,)}
FULL_LEVEL1 = {"nested_small": (2, 31, 32, 33, 256, 257, 1024, 1025, 4097), "nested_big": (4095, 4096, 8193),
               "nested_wide": (2, 31, 32, 33, 256, 257, 1024, 1025, 4097)}


def full_text(name, oracle):
    """(T, {bits: (SA, LCP)}) of a text of FULL, solved once per session by the oracle (such families cost it a fraction of a second)."""
    if ("full", name) not in _refs:
        T = np.ascontiguousarray(FULL[name]())
        sa, lcp = oracle.build_sa_lcp(T, p=64)
        w = {32: (sa, lcp), 64: (sa.astype(np.uint64), lcp.astype(np.uint64))}
        for a in (T,) + w[32] + w[64]:
            a.setflags(write=False)
        _refs["full", name] = (T, w)
    return _refs["full", name]


def full_case(lib, monkeypatch, capfd, oracle, name, bits=32, **env):
    """check() of one text of FULL and what the text is for: the sizes at level 0 and level 1, the ends of the rank range, the jump."""
    T, want = full_text(name, oracle)
    groups, gens, st = check(lib, monkeypatch, capfd, T, want[bits], FULL_TILE, bits=bits, **env)
    sizes = size_counts(groups)
    for s in FULL_LEVEL0[name]:
        assert sizes.get(s, 0) >= 1, (name, s, sizes)
    for s in FULL_LEVEL1.get(name, ()):
        assert gens[1]["sizes"].get(s, 0) >= 1 and gens[1]["depth_min"] == 2 * kch(T), (name, s, gens[1])
    if name.startswith("edges"):
        assert gens[0]["quick"][2] >= 2 and gens[0]["above_tile"] >= 1, gens[0]
        assert min(groups) == (0, 4096), min(groups)
        assert max((f + s, s) for f, s in groups) == (T.size, 4097), max(groups)
    if name in ("nested_small", "nested_wide"):
        assert all(q >= 2 for q in gens[1]["quick"]) and gens[1]["above_tile"] >= 1, gens[1]
    if name == "long":
        assert st["long_runs"] == 1
        assert any(g["depth_max"] > (lvl + 3) * 32 for lvl, g in enumerate(gens)), [(g["depth_min"], g["depth_max"]) for g in gens]
        assert any(g["in_lds"] for g in gens[1:]) and any(min(g["sizes"]) <= FIN_MAX for g in gens[1:]), gens[1:]   # <LONG> quick and finish
    return groups, gens, st
