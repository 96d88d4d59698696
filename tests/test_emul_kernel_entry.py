"""CPU: the five kernel-level entry points (include/caps_sa_hip.h: lcp, sort_suffixes, merge, upper_bound, sort_segments) on texts
whose keys tie, through the host emulation of the kernels -- the LOGIC of segmented_sort, merge_partition_kernel / merge_pass_kernel,
locate_kernel, finalize_kernel and lcp_pairs_kernel behind an equal key: deep_scan, the run table, pair_lcp, suffix_less_tie
(csrc/text.h).  The texts and position lists are kernel_entry_cases.py's, the truth is suffix_order_reference.py's, every comparison
is exact; test_gpu_kernel_entry.py runs the same list through the compiled kernels.

Also here: the reference against the oracle (what ties it to the reference project's order), classic-path builds that take the
galloping locate (locate_kernel<..., GALLOP = true>, which no entry point launches), and the refusals of the five entry points."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_entry_cases as K
from emul_util import EMUL_DIR, ROOT, emul, emul_rev, emul_small
from suffix_order_reference import Reference, lcp, rank

EINVAL = -1
FILL = 0xA5


# ---- 1. the reference against the oracle -------------------------------------------------------------------------------------------

def test_the_reference_orders_suffixes_as_the_oracle_does(oracle):
    """Random DNA, and 600 chars of signed bytes with a planted run that also ends the text (shorter suffix first, signed-char
    order): rank, lcp and the four expected answers against oracle.lcp / merge_sort / merge / upper_bound."""
    rs = np.random.RandomState(11)
    dna = rs.choice(K.DNA, size=777).astype(np.uint8)
    wide = rs.choice(K.WIDE, size=600).astype(np.uint8)
    wide[100:340] = np.resize(np.array([0x80, 0x61], dtype=np.uint8), 240)
    wide[520:] = np.resize(np.array([0x80, 0x61], dtype=np.uint8), 80)
    for T in (dna, wide):
        n = T.size
        R = Reference(T)
        assert np.array_equal(R.rank, rank(T))
        a, b = rs.randint(0, n, size=300), rs.randint(0, n, size=300)
        a[:40] = rs.randint(100, 340, size=40) if T is wide else a[:40]
        b[:40] = rs.randint(100, 340, size=40) if T is wide else b[:40]
        a[40:50] = b[40:50]
        got = R.lcps(a, b)
        for x, y, l in zip(a.tolist(), b.tolist(), got.tolist()):
            assert l == oracle.lcp(T, x, y) == lcp(T, x, y), (x, y)
        idx = rs.permutation(n)[:n // 2].astype(np.uint32)
        s, l = R.sort_suffixes(idx)
        so, lo = oracle.merge_sort(T, idx)
        assert np.array_equal(s, so) and np.array_equal(l, lo)
        xa, xl = oracle.merge_sort(T, idx[:100])
        ya, yl = oracle.merge_sort(T, idx[100:])
        Zo, LZo = oracle.merge(T, xa, ya, xl, yl)
        Z, LZ = R.merge(xa, ya)
        assert np.array_equal(Z, Zo) and np.array_equal(LZ, LZo)
        piv = np.concatenate([s[::13], rs.randint(0, n, size=40), [n - 1, R.sa[0], R.sa[-1]]])
        ub = R.upper_bound(s, piv)
        for pv, u in zip(piv.tolist(), ub.tolist()):
            assert u == oracle.upper_bound(T, so, pv), pv
        seg = np.array([0, 0, 5, 5, 130, n // 2, n // 2], dtype=np.uint64)
        ss, sl = R.sort_segments(idx, seg)
        for g in range(seg.size - 1):
            u, v = int(seg[g]), int(seg[g + 1])
            if u < v:
                so, lo = oracle.merge_sort(T, idx[u:v])
                assert np.array_equal(ss[u:v], so) and np.array_equal(sl[u + 1:v], lo[1:])
        assert sl[0] == 0 and sl[5] == oracle.lcp(T, int(ss[4]), int(ss[5])) and sl[130] == oracle.lcp(T, int(ss[129]), int(ss[130]))


def test_the_case_list_is_deterministic_and_says_what_it_hits():
    assert K.TILE_E == 4096                                       # (the sizes quoted in the docstrings; the lists follow the constant)
    for E in (K.TILE_E, K.SMALL_TILE_E):
        one, two = K.cases(E), K.cases(E)
        assert [c.name for c in one] == K.NAMES and len(set(K.NAMES)) == len(K.NAMES)
        assert all(np.array_equal(a.T, b.T) and a.stretches == b.stretches and a.hits for a, b in zip(one, two))
        for c in one:
            distinct = np.unique(c.T).size
            assert (distinct > 4) == (c.bits == 8), c.name
            assert c.n <= max(6 * E + 1, 9216), c.name
        assert [c.name for c in K.cases(E, full=True)] == K.NAMES
        for bits in (2, 8):                                       # every window edge: LCPs of m KCH - 1, m KCH, m KCH + 1 for m = 1 .. 6
            c, R = K.case_and_reference(E, f"planted stretches, {bits}-bit")
            found = K.lcp_edge_pairs(c, R)
            assert set(found) == {(m, d) for m in range(1, K.RUN_ENTER + 4) for d in (-1, 0, 1)}, (E, bits, sorted(found))
            for (m, d), (a, b) in found.items():
                assert all(lcp(c.T, x, y) == m * c.kch + d for x, y in zip(a.tolist(), b.tolist()))
    assert set(K.CLASSIC_NAMES) <= set(K.NAMES)


# ---- 2. the case list through the emulation builds ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.NAMES)
def test_entry_points_on_ties(name):
    K.check_case(emul(), K.TILE_E, name)


@pytest.mark.parametrize("name", K.NAMES)
def test_entry_points_on_ties_small_tiles(name):
    K.check_case(emul_small(), K.SMALL_TILE_E, name)


def test_entry_points_on_ties_do_not_depend_on_the_order_of_the_threads():
    E = emul_rev(True)
    for name in K.NAMES:
        K.check_case(E, K.SMALL_TILE_E, name, form=False)


@pytest.mark.slow
def test_poisoned_and_race_checked_builds_give_the_same_answers():
    """The small-tile half once more with LDS and registers starting as 0xA5 and the threads in a scattered order, and under the
    barrier-race detector (no race may be found)."""
    import caps_sa_amd
    for so in ("libcaps_sa_emul_small_poison.so", "libcaps_sa_emul_small_race.so"):
        subprocess.check_call(["make", "-s", "-C", EMUL_DIR, so])
        path = os.path.join(EMUL_DIR, so)
        lib = caps_sa_amd.CapsLib(path, "caps_sa_emul_")
        for name in K.NAMES:                                    # (the text's form is the plain small-tile build's to check, above)
            K.check_case(lib, K.SMALL_TILE_E, name, form=False)
        if "race" in so:
            raw = ctypes.CDLL(path)
            raw.caps_sa_emul_races_found.restype = ctypes.c_ulonglong
            assert int(raw.caps_sa_emul_races_found()) == 0


# ---- 3. classic-path builds that take the galloping locate -------------------------------------------------------------------------

_CHILD = r"""
import sys
sys.path[:0] = [%(tests)r, %(root)r]
import caps_sa_amd
import kernel_entry_cases as K
for so, E in (("libcaps_sa_emul.so", K.TILE_E), ("libcaps_sa_emul_small.so", K.SMALL_TILE_E)):
    K.check_classic_builds(caps_sa_amd.CapsLib(%(emul)r + "/" + so, "caps_sa_emul_"), E, %(name)r)
print("done")
"""


@pytest.mark.parametrize("name", K.CLASSIC_NAMES)
def test_classic_builds_with_the_galloping_locate(name):
    """CAPS_SA_PATH=classic with 64 < n / p < 8 (p - 1), both tile sizes, both index widths.  In a child process: a locate that
    answers wrongly sends the emulated partition step outside its arrays, which then ends the child and not the suite."""
    emul(), emul_small()
    code = _CHILD % {"tests": os.path.join(ROOT, "tests"), "root": ROOT, "emul": EMUL_DIR, "name": name}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, CAPS_SA_PATH="classic"))
    assert r.returncode == 0 and r.stdout.startswith("done"), (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------

def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


@pytest.mark.parametrize("bits", K.WIDTHS)
def test_refusals_leave_the_outputs_untouched(bits):
    """capi_impl.h: a position >= n in each argument, seg_start that does not start at 0, does not end at cnt or decreases, G = 0 (or
    beyond 2^31 - 1), null pointers with a non-zero count, too many pivots, n beyond the index type: CAPS_SA_EINVAL, and no byte of
    an output buffer is written."""
    E = emul()
    sfx, dt = ("u32" if bits == 32 else "u64"), _dt(bits)
    n, cnt = 5000, 300
    rs = np.random.RandomState(5)
    T = rs.choice(K.DNA, size=n).astype(np.uint8)
    R = Reference(T)
    idx = rs.permutation(n)[:cnt].astype(dt)
    s = R.sort_suffixes(idx)[0].astype(dt)
    X, Y = s[0::2].copy(), s[1::2].copy()
    LX, LY = R.neighbour_lcps(X).astype(dt), R.neighbour_lcps(Y).astype(dt)
    seg = np.array([0, 100, 100, cnt], dtype=np.uint64)
    o1, o2 = np.full(cnt, FILL, dtype=np.uint8).repeat(bits // 8).view(dt), np.full(cnt, FILL, dtype=np.uint8).repeat(bits // 8).view(dt)
    fill = o1.copy()

    def p(a):
        return a.ctypes.data

    def bad(a, at, v):
        b = a.copy()
        b[at] = v
        return b

    sort = E._f(f"sort_suffixes_{sfx}")
    segs = E._f(f"sort_segments_{sfx}")
    merge = E._f(f"merge_{sfx}")
    ub = E._f(f"upper_bound_{sfx}")
    lcpf = E._f(f"lcp_{sfx}")
    top = int(np.iinfo(dt).max)
    keep = []                                                   # (arrays must outlive the calls that read them)

    def k(a):
        keep.append(a)
        return p(a)

    calls = {
        "sort: a position = n": sort(p(T), n, k(bad(idx, 7, n)), cnt, p(o1), p(o2), 0),
        "sort: the last position = the largest value": sort(p(T), n, k(bad(idx, cnt - 1, top)), cnt, p(o1), p(o2), 0),
        "sort: null idx": sort(p(T), n, None, cnt, p(o1), p(o2), 0),
        "sort: null out_sa": sort(p(T), n, p(idx), cnt, None, p(o2), 0),
        "sort: null out_lcp": sort(p(T), n, p(idx), cnt, p(o1), None, 0),
        "sort: null text": sort(None, n, p(idx), cnt, p(o1), p(o2), 0),
        "segments: null text": segs(None, n, p(idx), cnt, p(seg), 3, p(o1), p(o2), 0),
        "merge: null text": merge(None, n, p(X), X.size, p(Y), Y.size, p(LX), p(LY), p(o1), p(o2), 0),
        "upper_bound: null text": ub(None, n, p(s), cnt, p(idx), 10, p(o1), 0),
        "lcp: null text": lcpf(None, n, p(idx), p(s), cnt, p(o1), 0),
        "segments: a position = n": segs(p(T), n, k(bad(idx, 0, n)), cnt, p(seg), 3, p(o1), p(o2), 0),
        "segments: seg_start[0] != 0": segs(p(T), n, p(idx), cnt, k(bad(seg, 0, 1)), 3, p(o1), p(o2), 0),
        "segments: seg_start[G] < cnt": segs(p(T), n, p(idx), cnt, k(bad(seg, 3, cnt - 1)), 3, p(o1), p(o2), 0),
        "segments: seg_start[G] > cnt": segs(p(T), n, p(idx), cnt, k(bad(seg, 3, cnt + 1)), 3, p(o1), p(o2), 0),
        "segments: decreasing": segs(p(T), n, p(idx), cnt, k(bad(seg, 1, 101)), 3, p(o1), p(o2), 0),
        "segments: G = 0": segs(p(T), n, p(idx), cnt, p(seg), 0, p(o1), p(o2), 0),
        "segments: G = 2^31": segs(p(T), n, p(idx), cnt, p(seg), 1 << 31, p(o1), p(o2), 0),
        "segments: null seg_start": segs(p(T), n, p(idx), cnt, None, 3, p(o1), p(o2), 0),
        "segments: null idx": segs(p(T), n, None, cnt, p(seg), 3, p(o1), p(o2), 0),
        "segments: null out_sa": segs(p(T), n, p(idx), cnt, p(seg), 3, None, p(o2), 0),
        "segments: null out_lcp": segs(p(T), n, p(idx), cnt, p(seg), 3, p(o1), None, 0),
        "merge: a position = n in X": merge(p(T), n, k(bad(X, 3, n)), X.size, p(Y), Y.size, p(LX), p(LY), p(o1), p(o2), 0),
        "merge: a position = n in Y": merge(p(T), n, p(X), X.size, k(bad(Y, Y.size - 1, n)), Y.size, p(LX), p(LY), p(o1), p(o2), 0),
        "merge: null X": merge(p(T), n, None, X.size, p(Y), Y.size, p(LX), p(LY), p(o1), p(o2), 0),
        "merge: null Y": merge(p(T), n, p(X), X.size, None, Y.size, p(LX), p(LY), p(o1), p(o2), 0),
        "merge: null LCP_x": merge(p(T), n, p(X), X.size, p(Y), Y.size, None, p(LY), p(o1), p(o2), 0),
        "merge: null LCP_y": merge(p(T), n, p(X), X.size, p(Y), Y.size, p(LX), None, p(o1), p(o2), 0),
        "merge: null Z": merge(p(T), n, p(X), X.size, p(Y), Y.size, p(LX), p(LY), None, p(o2), 0),
        "merge: null LCP_z": merge(p(T), n, p(X), X.size, p(Y), Y.size, p(LX), p(LY), p(o1), None, 0),
        "upper_bound: a position = n in X": ub(p(T), n, k(bad(s, 9, n)), cnt, p(idx), 10, p(o1), 0),
        "upper_bound: a pivot = n": ub(p(T), n, p(s), cnt, k(bad(idx, 9, n)), 10, p(o1), 0),
        "upper_bound: null X": ub(p(T), n, None, cnt, p(idx), 10, p(o1), 0),
        "upper_bound: null pivots": ub(p(T), n, p(s), cnt, None, 10, p(o1), 0),
        "upper_bound: null out": ub(p(T), n, p(s), cnt, p(idx), 10, None, 0),
        "upper_bound: 2^31 pivots": ub(p(T), n, p(s), cnt, p(idx), 1 << 31, p(o1), 0),
        "lcp: a = n": lcpf(p(T), n, k(bad(idx, 5, n)), p(s), cnt, p(o1), 0),
        "lcp: b = n": lcpf(p(T), n, p(idx), k(bad(s, cnt - 1, n)), cnt, p(o1), 0),
        "lcp: null a": lcpf(p(T), n, None, p(s), cnt, p(o1), 0),
        "lcp: null b": lcpf(p(T), n, p(idx), None, cnt, p(o1), 0),
        "lcp: null out": lcpf(p(T), n, p(idx), p(s), cnt, None, 0),
    }
    if bits == 32:                                              # n beyond the index type: refused before anything is read
        big = 1 << 32
        calls["sort: n = 2^32"] = sort(p(T), big, p(idx), cnt, p(o1), p(o2), 0)
        calls["segments: n = 2^32"] = segs(p(T), big, p(idx), cnt, p(seg), 3, p(o1), p(o2), 0)
        calls["merge: n = 2^32"] = merge(p(T), big, p(X), X.size, p(Y), Y.size, p(LX), p(LY), p(o1), p(o2), 0)
        calls["upper_bound: n = 2^32"] = ub(p(T), big, p(s), cnt, p(idx), 10, p(o1), 0)
        calls["lcp: n = 2^32"] = lcpf(p(T), big, p(idx), p(s), cnt, p(o1), 0)
    wrong = {what: rc for what, rc in calls.items() if rc != EINVAL}
    assert not wrong, wrong
    assert np.array_equal(o1, fill) and np.array_equal(o2, fill), "a refused call wrote to an output"
    assert E._f("last_error")()                                 # (a message is there)
    # nothing to do is no error, whatever the pointers: and nothing is written
    assert sort(p(T), n, None, 0, None, None, 0) == 0 and segs(p(T), n, None, 0, None, 0, None, None, 0) == 0
    assert merge(p(T), n, None, 0, None, 0, None, None, None, None, 0) == 0
    assert ub(p(T), n, p(s), cnt, None, 0, None, 0) == 0 and lcpf(p(T), n, None, None, 0, None, 0) == 0
    assert np.array_equal(o1, fill) and np.array_equal(o2, fill)
    # ... and the same arguments without the fault succeed (the refusals above are the faults', not the set-up's)
    assert sort(p(T), n, p(idx), cnt, p(o1), p(o2), 0) == 0 and np.array_equal(o1, s)
    assert segs(p(T), n, p(idx), cnt, p(seg), 3, p(o1), p(o2), 0) == 0
    assert merge(p(T), n, p(X), X.size, p(Y), Y.size, p(LX), p(LY), p(o1), p(o2), 0) == 0 and np.array_equal(o1, s)
    assert ub(p(T), n, p(s), cnt, p(idx), 10, p(o1), 0) == 0 and lcpf(p(T), n, p(idx), p(s), cnt, p(o1), 0) == 0
