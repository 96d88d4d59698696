"""Texts whose keys tie, and the position lists that drive the five kernel-level entry points (include/caps_sa_hip.h: lcp,
sort_suffixes, merge, upper_bound, sort_segments) over them -- shared by test_emul_kernel_entry.py (the host emulation) and
test_gpu_kernel_entry.py (the compiled kernels), as verifier_cases.py and records_cases.py are shared.

On random DNA two suffixes never share a key, so the comparator of csrc/text.h (deep_scan, the run table, pair_lcp,
suffix_less_tie) is never entered behind a key.  Here it is entered at once, by every kernel: each case is a text plus what it is
built to hit.  Everything is compared, exactly, with suffix_order_reference.Reference.  The list is deterministic (fixed seeds) and
depends only on the tile size E of the library under test (4,096 on the GPU and in emul(), 256 in emul_small())."""
import os

import numpy as np

from suffix_order_reference import Reference

RUN_ENTER = 3                      # csrc/text.h CAPS_RUN_ENTER: plain windows before the run table is asked
RUN_LONG = 1024                    # csrc/text.h: a periodic stretch of this many chars selects the RUNS = true builds
WIDTHS = (32, 64)
BATCHES = (1, 255, 256, 257)       # one block of 256 threads, one short of it, one more

DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
WIDE = np.array([0x80, 0x61, 0xC8, 0x10, 0x7F, 0xFF], dtype=np.uint8)       # 8-bit form; 0x80 is code 0 = the padding behind the text
HEAD8 = np.array([0x7F, 0x00, 0xFF, 0x41, 0x81, 0x20], dtype=np.uint8)      # six distinct bytes: a text behind them is packed to 8 bits
PERIODS = {2: (1, 2, 3, 5, 8, 15, 16, 17), 8: (1, 2, 3, 4, 5)}              # every period the run table knows (<= KCH / 2) and the first it does not


def kch_of(bits: int) -> int:
    return 64 // bits


def tile_size_of_the_sources() -> int:
    """TILE_E of a default build (libcaps_sa_hip.so, tests/emul/libcaps_sa_emul.so): the `#define CAPS_TILE_E` of
    caps-sa_amd/csrc/kernels.h.  There is no ABI query for it, so the lists around E - 1 / E / E + 1 read it where the libraries get
    it from; a build with -DCAPS_TILE_E=... (tests/emul/Makefile: 256 for libcaps_sa_emul_small*.so) states its own."""
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "caps-sa_amd", "csrc", "kernels.h")
    with open(path) as f:
        m = re.search(r"^#define CAPS_TILE_E (\d+)\s*$", f.read(), re.M)
    assert m, "caps-sa_amd/csrc/kernels.h no longer defines CAPS_TILE_E this way"
    return int(m.group(1))


TILE_E = tile_size_of_the_sources()
SMALL_TILE_E = 256                 # tests/emul/Makefile: -DCAPS_TILE_E=256 of the small-tile builds


class Case:
    """name; T; bits_per_char the build must report; long_runs it must report; stretches [(start, end, period)] for the lcp pair
    lists; hits: what the text is built to reach."""

    def __init__(self, name, T, bits, long_runs, stretches=(), hits=""):
        self.name, self.T, self.bits, self.long_runs = name, np.ascontiguousarray(T, dtype=np.uint8), bits, long_runs
        self.stretches, self.hits = list(stretches), hits
        self.n = int(self.T.size)
        self.kch = kch_of(bits)


def _seed(*parts) -> int:
    s = 0
    for p in parts:
        s = (s * 1000003 + int(p)) % (1 << 31)
    return s


def primitive_unit(letters, d: int, seed: int) -> np.ndarray:
    """d letters that are no power of a shorter word (no rotation but the trivial one maps the unit onto itself)."""
    rs = np.random.RandomState(seed)
    while True:
        u = rs.choice(letters, size=d)
        if all(not np.array_equal(np.roll(u, k), u) for k in range(1, d)):
            return u


def _halves(s: int, e: int, d: int):
    """One stretch as two places to take positions from: its front, and its back up to the end of the text."""
    mid = s + (e - s) // 2
    return [(s, mid, d), (mid, e, d)]


def unary_cases(E: int):
    n = 5 * E + 77
    yield Case("unary A", np.full(n, ord("A"), dtype=np.uint8), 2, 1, _halves(0, n, 1),
               "every key but the last 31 equal: each merge-path diagonal, tile halo and bisection step falls inside a tie")
    T = np.concatenate([HEAD8, np.full(n - HEAD8.size, 0x80, dtype=np.uint8)])
    yield Case("unary 0x80, 8-bit", T, 8, 1, _halves(HEAD8.size, n, 1),
               "the letter is code 0 = the padding behind the text: its end is found by length alone")


def period_cases(E: int, full: bool = False):
    """unit^k for every period.  full: the texts of a period the table does not know are 5 tiles + 1 long like the others (every
    comparison walks them window by window: quick on a GPU, half a minute per text and library in the emulation, which keeps them
    at one tile + 1)."""
    for bits in (2, 8):
        kch = kch_of(bits)
        for d in PERIODS[bits]:
            letters = DNA if bits == 2 else WIDE
            u = np.array([ord("G") if bits == 2 else 0x61], dtype=np.uint8) if d == 1 else primitive_unit(letters, d, _seed(bits, d))
            for long in (True, False):
                known = d <= kch // 2
                n = max((5 if known or full else 1) * E + 1 + 2 * kch + 3, RUN_LONG + 4 * kch + HEAD8.size) if long else 1000
                head = HEAD8 if bits == 8 else HEAD8[:0]
                T = np.concatenate([head, np.resize(u, n - head.size)])
                yield Case(f"period {d}, {bits}-bit, {'long' if long else 'short'}", T, bits, int(long and known), _halves(head.size, n, d),
                           ("a period the run table knows" if known else "the first period the run table does not know")
                           + (": the RUNS = true builds" if long and known else ": the plain builds"))


def planted_case(E: int, bits: int):
    """Periodic stretches planted in random text: both ends of a stretch at every offset modulo KCH, the same unit at different
    lengths, the same period with different units, a stretch followed at once by one whose period divides (or does not divide) its
    own, one that starts the text and one that ends it."""
    kch = kch_of(bits)
    letters = DNA if bits == 2 else WIDE
    n = max(6 * E, 9216 if bits == 2 else 6144)
    rs = np.random.RandomState(_seed(4242, bits))
    T = rs.choice(letters, size=n).astype(np.uint8)
    stretches, closed = [], []
    L = [int(x) for x in letters]

    def other(c):
        return L[(L.index(int(c)) + 1) % len(L)]

    def plant(at, unit, length, open_left=False, open_right=False):
        unit = np.asarray(unit, dtype=np.uint8)
        d = unit.size
        assert at + length <= n
        T[at:at + length] = np.resize(unit, length)
        if not open_right and at + length < n:
            T[at + length] = other(T[at + length - d])             # the period breaks right behind the stretch
        if not open_left and at > 0:
            T[at - 1] = other(T[at - 1 + d])                       # ... and does not reach in front of it
        stretches.append((at, at + length, d))
        closed.append((open_left, open_right))
        return at + length

    a_, c_, g_ = L[0], L[1], L[2]
    ac, ag, acg, acag = [a_, c_], [a_, g_], [a_, c_, g_], [a_, c_, a_, g_]
    cur = plant(0, ac, 3 * kch + 5)                               # starts the text
    cur = plant(cur + 37, [a_], RUN_LONG + 76, open_right=True)   # A^k (AC)^k: the next period is a multiple
    cur = plant(cur, ac, 300 + 1, open_left=True)
    cur = plant(cur + 29, ac, RUN_LONG + 177)                     # the same unit, another length
    cur = plant(cur + 41, ag, 500 + 3)                            # the same period, another unit
    cur = plant(cur + 23, ac, 260, open_right=True)               # (ACAC...) then (ACG...): neither period divides the other
    cur = plant(cur, acg, 331, open_left=True)
    cur = plant(cur + 31, ac, 200, open_right=True)               # (AC)^k then (ACAG)^k: 2 divides 4
    cur = plant(cur, acag, 262, open_left=True)
    units = [[a_], ac, ag, acg, [c_], acag]
    first_residue = len(stretches)
    for i in range(kch):                                           # start = i, end = 7 i + 3 (mod KCH): every residue once each
        at = cur + 9
        at += (i - at) % kch
        length = 2 * kch + ((7 * i + 3) - i) % kch
        cur = plant(at, units[i % len(units)], length)
    assert cur + 9 < n - (2 * kch + 11), "the planted stretches do not fit"
    plant(n - (2 * kch + 11), acg, 2 * kch + 11)                   # ends the text
    res = stretches[first_residue:first_residue + kch]
    assert {s % kch for s, _, _ in res} == set(range(kch)) and {e % kch for _, e, _ in res} == set(range(kch))
    for (s, e, d), (open_left, open_right) in zip(stretches, closed):    # as planted: periodic inside, broken on both sides unless left open
        assert np.array_equal(T[s + d:e], T[s:e - d])
        assert open_left or s == 0 or T[s - 1] != T[s - 1 + d], (s, e, d)
        assert open_right or e == n or T[e] != T[e - d], (s, e, d)
    return Case(f"planted stretches, {bits}-bit", T, bits, 1, stretches,
                "the periodic128 test failing while both table entries carry a period; stretch ends at every offset of a window")


def duplicate_case(E: int, bits: int):
    """Aperiodic depth: S S S[:1000] x S S[5:] ... S -- LCPs in the thousands with table entries 0, and the text ends with a copy of
    S: one suffix is a proper prefix of another."""
    letters = DNA if bits == 2 else WIDE
    rs = np.random.RandomState(_seed(777, bits))
    m = 2500 if E >= 4096 else 640
    S = rs.choice(letters, size=m).astype(np.uint8)
    x = np.array([letters[3]], dtype=np.uint8)
    filler = rs.choice(letters, size=m // 3).astype(np.uint8)
    T = np.concatenate([S, S, S[:2 * m // 5], x, S, S[5:], filler, S])
    return Case(f"long duplicates, {bits}-bit", T, bits, 0, (), "LCPs of thousands of chars found window by window; a suffix that is a prefix of another")


def random_case(E: int, bits: int):
    rs = np.random.RandomState(_seed(99, bits))
    return Case(f"random, {bits}-bit", rs.choice(DNA if bits == 2 else WIDE, size=6 * E).astype(np.uint8), bits, 0, (),
                "the control: no two suffixes share a key")


def cases(E: int, full: bool = False):
    out = list(unary_cases(E)) + list(period_cases(E, full))
    for bits in (2, 8):
        out += [planted_case(E, bits), duplicate_case(E, bits), random_case(E, bits)]
    return out


NAMES = [c.name for c in cases(TILE_E)]                               # the same names at every tile size
CLASSIC_NAMES = ["unary A", "unary 0x80, 8-bit", "planted stretches, 2-bit", "planted stretches, 8-bit", "long duplicates, 2-bit",
                 "long duplicates, 8-bit"]

_cache = {}


def case_and_reference(E: int, name: str, full: bool = False):
    """(case, reference), built once per tile size and shared by every test that asks; neither is ever changed."""
    if (E, full, name) not in _cache:
        if (E, full, None) not in _cache:
            _cache[(E, full, None)] = {c.name: c for c in cases(E, full)}
        c = _cache[(E, full, None)][name]
        c.T.setflags(write=False)
        _cache[(E, full, name)] = (c, Reference(c.T))
    return _cache[(E, full, name)]


# ---- the position lists ------------------------------------------------------------------------------------------------------------

def lcp_edge_pairs(c: Case, R: Reference):
    """{(m, delta): (a, b)}: neighbours in the suffix array whose LCP is m KCH + delta, for m = 1 .. RUN_ENTER + 3 and delta = -1, 0,
    1 -- the last char of a window, a whole number of windows, the first char of the next -- in both orders; found by search in the
    reference's LCP array.  A class the text does not hold is absent (the planted texts must hold all 18:
    test_emul_kernel_entry.py asserts it)."""
    out = {}
    for m in range(1, RUN_ENTER + 4):
        for delta in (-1, 0, 1):
            at = np.nonzero(R.lcp_array == m * c.kch + delta)[0]
            at = at[at > 0]
            if at.size:
                pick = at[[0, at.size // 2, at.size - 1]]
                out[(m, delta)] = (np.concatenate([R.sa[pick - 1], R.sa[pick]]), np.concatenate([R.sa[pick], R.sa[pick - 1]]))
    return out


def lcp_pairs(c: Case, R: Reference):
    """(a, b): positions at every residue modulo KCH in every pair of stretches; pairs whose true LCP is one below, on and one above
    every multiple of KCH up to (RUN_ENTER + 3) KCH, found by search in the reference's LCP array; a == b; the last positions of
    the text against everything; 2,000 random pairs."""
    n, kch = c.n, c.kch
    rs = np.random.RandomState(_seed(5, n, c.bits))
    A, B = [], []
    off = np.arange(kch, dtype=np.int64)
    st = c.stretches
    for i in range(len(st)):
        for j in range(i, len(st)):
            a0 = min(st[i][0], max(st[i][1] - kch, 0))
            b0 = min(st[j][0] + (1 if i == j else 0), max(st[j][1] - kch, 0))
            A.append(np.repeat(a0 + off, kch))
            B.append(np.tile(b0 + off, kch))
    for a, b in lcp_edge_pairs(c, R).values():
        A.append(a)
        B.append(b)
    ends = np.array(sorted({p for p in (n - 1, n - 2, n - kch, n - kch - 1, n - kch + 1) if 0 <= p < n}), dtype=np.int64)
    A.append(ends)                                                  # a == b
    B.append(ends)
    A.append(np.array([0, n // 2], dtype=np.int64))
    B.append(np.array([0, n // 2], dtype=np.int64))
    others = np.concatenate([ends, rs.randint(0, n, size=40), np.array([s for s, _, _ in st[:40]], dtype=np.int64),
                             np.array([max(e - 1, 0) for _, e, _ in st[:40]], dtype=np.int64)]).astype(np.int64)
    for e in ends.tolist():
        A += [np.full(others.size, e, dtype=np.int64), others]
        B += [others, np.full(others.size, e, dtype=np.int64)]
    A.append(rs.randint(0, n, size=2000))
    B.append(rs.randint(0, n, size=2000))
    return np.concatenate(A).astype(np.int64), np.concatenate(B).astype(np.int64)


def list_sizes(E: int, n: int):
    return [k for k in (1, 2, E - 1, E, E + 1, 2 * E + 1, 3 * E + 1, 5 * E + 1) if k <= n]


def sort_lists(c: Case, E: int):
    """(what, idx): random subsets of every size around the tile edges, and all positions (in a shuffled order)."""
    for cnt in list_sizes(E, c.n):
        yield f"{cnt} positions", np.random.RandomState(_seed(6, c.n, cnt)).permutation(c.n)[:cnt].astype(np.int64)
    yield "all positions", np.random.RandomState(_seed(7, c.n)).permutation(c.n).astype(np.int64)


def merge_splits(s: np.ndarray, seed: int):
    """(what, X, Y) of a sorted list s."""
    rs = np.random.RandomState(seed)
    cnt = s.size
    for p in (0.5, 0.03):
        m = rs.rand(cnt) < p
        yield f"coin {p}", s[m], s[~m]
    yield "alternating", s[0::2], s[1::2]
    cut = 2 * cnt // 5
    yield "X below Y", s[:cut], s[cut:]
    yield "Y below X", s[cut:], s[:cut]
    yield "X empty", s[:0], s
    yield "Y empty", s, s[:0]
    k = cnt // 2
    yield "one against the rest", s[k:k + 1], np.concatenate([s[:k], s[k + 1:]])


def upper_bound_queries(c: Case, R: Reference, E: int):
    """(what, X, pivots): X a sorted list; pivots = position n - 1, the smallest and the largest suffix of the text, members of X at a
    stride, non-members."""
    n = c.n
    rs = np.random.RandomState(_seed(8, n, c.bits))
    perm = rs.permutation(n).astype(np.int64)
    cnt = min(2 * E + 1, n // 2)
    X, _ = R.sort_suffixes(perm[:cnt])
    members = X[::max(1, cnt // 120)][:125]
    outside = perm[cnt:cnt + 129]
    mixed = np.empty(members.size + outside.size, dtype=np.int64)
    k = min(members.size, outside.size)
    mixed[0:2 * k:2], mixed[1:2 * k:2] = members[:k], outside[:k]
    mixed[2 * k:] = np.concatenate([members[k:], outside[k:]])
    piv = np.concatenate([[n - 1, R.sa[0], R.sa[-1]], mixed])
    piv = np.resize(piv, 257).astype(np.int64)
    for q in BATCHES:
        yield f"{q} pivots in a list of {cnt}", X, piv[:q]
    yield "an empty list", X[:0], piv
    yield "the list of all suffixes", R.sa, piv


def segment_lists(c: Case, E: int):
    """(what, idx, seg_start): the length mix 0, 1, 3, E, E + 1, 2E, 2E + 1, 5E + 1 with empty segments first, last and between, in as
    many calls as the text has positions for.  A segment of <= E / <= 2E / <= 4E / <= 8E elements ends after 0 / 1 / 2 / 3 merge
    passes, in ping-pong buffer 0 / 1 / 0 / 1: the heads behind E -> E + 1, 2E -> 2E + 1 and 5E + 1 -> 3 have their predecessor in
    the other buffer."""
    n = c.n
    mixes = [[0, 5 * E + 1, 0, 3, 0], [0, 1, E, 0, E + 1, 2 * E, 0], [3, 0, 0, 2 * E, 2 * E + 1, 1, 0]]
    mixes = [m for m in mixes if sum(m) <= n] or [[0, 1, 0, 3, n // 2, 0, 7, n // 3, 0]]
    for k, lens in enumerate(mixes):
        seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        idx = np.random.RandomState(_seed(9, n, k)).permutation(n)[:int(seg[-1])].astype(np.int64)
        yield f"segments {lens}", idx, seg


# ---- the checks: an entry point of `lib` against the reference -------------------------------------------------------------------------

def _eq(got, want, what):
    got = np.asarray(got).astype(np.int64)
    want = np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} wrong, the first at {int(bad[0])}: {int(got[bad[0]])} for {int(want[bad[0]])}"


def check_lcp(lib, c: Case, R: Reference, bits: int):
    a, b = lcp_pairs(c, R)
    want = R.lcps(a, b)
    pick = np.random.RandomState(3).randint(0, a.size, size=60)      # the table of minima against the definition
    R.check_against_definition(a[pick], b[pick])
    _eq(lib.lcp(c.T, a, b, idx_bits=bits), want, f"{c.name}: lcp u{bits}")
    for q in BATCHES:                                               # the random pairs stand last
        _eq(lib.lcp(c.T, a[-q:], b[-q:], idx_bits=bits), want[-q:], f"{c.name}: lcp u{bits}, a batch of {q}")
    return a.size


def check_sort_and_merge(lib, c: Case, R: Reference, E: int, bits: int):
    done = 0
    for what, idx in sort_lists(c, E):
        s, l = R.sort_suffixes(idx)
        sa, lcp = lib.sort_suffixes(c.T, idx, idx_bits=bits)
        _eq(sa, s, f"{c.name}: sort_suffixes u{bits}, {what}")
        _eq(lcp, l, f"{c.name}: sort_suffixes u{bits}, {what}, LCP")
        for how, X, Y in merge_splits(s, _seed(10, c.n, s.size)):
            Z, LZ = lib.merge(c.T, X, Y, R.neighbour_lcps(X), R.neighbour_lcps(Y), idx_bits=bits)
            _eq(Z, s, f"{c.name}: merge u{bits}, {what}, {how}")
            _eq(LZ, l, f"{c.name}: merge u{bits}, {what}, {how}, LCP")
            done += 1
    return done


def check_upper_bound(lib, c: Case, R: Reference, E: int, bits: int):
    for what, X, piv in upper_bound_queries(c, R, E):
        want = R.upper_bound(X, piv)
        if X.size == 0:
            assert not want.any()
        _eq(lib.upper_bound(c.T, X, piv, idx_bits=bits), want, f"{c.name}: upper_bound u{bits}, {what}")


def check_segments(lib, c: Case, R: Reference, E: int, bits: int):
    for what, idx, seg in segment_lists(c, E):
        s, l = R.sort_segments(idx, seg)
        sa, lcp = lib.sort_segments(c.T, idx, seg, idx_bits=bits)
        _eq(sa, s, f"{c.name}: sort_segments u{bits}, {what}")
        _eq(lcp, l, f"{c.name}: sort_segments u{bits}, {what}, LCP")


def check_form(lib, c: Case):
    """One build of the text: the code width and the comparator builds the case was made for."""
    st = lib.build(c.T, p=0)[2]
    assert st["bits_per_char"] == c.bits, (c.name, st["bits_per_char"])
    assert st["long_runs"] == c.long_runs, (c.name, st["long_runs"])


def check_case(lib, E: int, name: str, widths=WIDTHS, form=True, full=False):
    """Every entry point over every list of one text, at both index widths."""
    c, R = case_and_reference(E, name, full)
    for bits in widths:
        check_lcp(lib, c, R, bits)
        check_sort_and_merge(lib, c, R, E, bits)
        check_upper_bound(lib, c, R, E, bits)
        check_segments(lib, c, R, E, bits)
    if form:
        check_form(lib, c)


# ---- classic-path builds that take the galloping locate ----------------------------------------------------------------------------------

def gallop_p(n: int):
    """Subproblem counts with 64 < n / p < 8 (p - 1): csrc/pipeline.h then launches locate_kernel<..., GALLOP = true> and its
    subarrays are long enough (len > 64) to gallop."""
    ps = [p for p in (n // 160, n // 72) if p >= 2 and 64 < n // p < 8 * (p - 1) and p <= n // 16]
    assert ps, n
    return ps


def check_classic_builds(lib, E: int, name: str):
    """Whole builds on the samplesort path at both index widths against sa_check.sa_lcp (the reference's sa and lcp_array are its
    output).  The caller has set CAPS_SA_PATH=classic."""
    assert os.environ.get("CAPS_SA_PATH") == "classic"
    c, R = case_and_reference(E, name)
    for p in gallop_p(c.n):
        for bits in WIDTHS:
            SA, LCP, st = lib.build(c.T, p=p, idx_bits=bits)
            assert st["path_direct"] == 0 and st["p_eff"] == p, (c.name, p, st["path_direct"], st["p_eff"])
            assert 64 < c.n // st["p_eff"] < 8 * (st["p_eff"] - 1)
            _eq(SA, R.sa, f"{c.name}: classic build p = {p} u{bits}, SA")
            _eq(LCP, R.lcp_array, f"{c.name}: classic build p = {p} u{bits}, LCP")
