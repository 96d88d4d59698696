"""The inputs of the verifier tests (tests/test_emul_verifier.py on the emulation, tests/test_gpu_verifier.py on the MI355X): texts,
their true arrays from fm_reference, and arrays with ONE fault each, built so that exactly one check of the verifier can fire.

A case is (label, T, SA, LCP, cnt, is_head, expect): T np.uint8, SA / LCP lists of non-negative Python ints (the caller puts them
into the index type), the first cnt entries are verified, expect = the count the construction isolates, or None where only the
model (tests/verify_model.py) says it.  Everything is seeded: the same cases on every run and on both sides."""
import numpy as np

from fm_reference import naive_lcp
from verify_model import common_prefix, count, is_true_arrays, true_arrays

ALPHABETS = {
    "one": np.array([0x41], dtype=np.uint8),
    "two": np.frombuffer(b"AC", dtype=np.uint8),
    "four": np.frombuffer(b"ACGT", dtype=np.uint8),
    "high": np.array([0x41, 0xC1], dtype=np.uint8),          # one byte on each side of the sign bit
    "all": np.arange(256, dtype=np.uint8),
}
ACCEPT_SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 600)
EDGES = (1, 2, 63, 64, 65, 255, 256, 257)                    # wave and workgroup edges of the 256-thread launch


def random_text(n, alphabet, seed):
    return np.random.RandomState(seed).choice(ALPHABETS[alphabet], size=n).astype(np.uint8)


def accepted_texts():
    for k, alphabet in enumerate(ALPHABETS):
        for n in ACCEPT_SIZES:
            yield f"{alphabet}/{n}", random_text(n, alphabet, 1000 * k + n)


def _truth(T):
    SA, LCP = true_arrays(T)
    return SA.tolist(), LCP.tolist()


def _lcps_for(T, SA):
    """The exact LCPs of the neighbours of ANY list of in-range positions (a value next to itself: the whole suffix)."""
    return naive_lcp(T, SA).tolist()


def base_text():
    return random_text(600, "four", 7)


def tail_copy_text():
    """Ends in a copy of its own tail: the suffix at n - 24 is a proper prefix of the one at 100, so the pair that holds it runs
    into the end of the text (l == cap in the kernel)."""
    T = random_text(400, "four", 8)
    T[-24:] = T[100:124]
    return T


def prefix_pairs(T, SA, LCP):
    """The i whose pair (SA[i-1], SA[i]) ends at the end of the text: one suffix is a proper prefix of the other."""
    n = T.size
    return [i for i in range(1, n) if LCP[i] == n - max(SA[i - 1], SA[i])]


def single_faults(bits):
    """Every single fault of the list, for one index width."""
    top = (1 << bits) - 1
    T = base_text()
    n = T.size
    SA, LCP = _truth(T)

    # ---- LCP off by one, SA intact: lanes 0 and 1 of a wave, wave and workgroup edges, the last entry
    for i in EDGES + (n - 1,):
        for d in (1, -1):
            bad = list(LCP)
            bad[i] = (bad[i] + d) & top                      # 0 - 1 wraps to the top of the index type: still not the prefix
            yield f"lcp[{i}]{d:+d}", T, SA, bad, n, 1, 1
    Tt = tail_copy_text()
    SAt, LCPt = _truth(Tt)
    pp = prefix_pairs(Tt, SAt, LCPt)
    assert len(pp) >= 2
    for i in (pp[0], pp[-1]):
        for d in (1, -1):
            bad = list(LCPt)
            bad[i] = (bad[i] + d) & top
            yield f"lcp at a prefix pair [{i}]{d:+d}", Tt, SAt, bad, Tt.size, 1, 1

    # ---- head LCP: counted with is_head, not looked at without
    bad = list(LCP)
    bad[0] = 1
    yield "head lcp, is_head", T, SA, bad, n, 1, 1
    yield "head lcp, no head", T, SA, bad, n, 0, 0
    yield "head lcp of a slice, is_head", T, SA[200:], LCP[200:], 300, 1, int(LCP[200] != 0)
    yield "head lcp of a slice, no head", T, SA[200:], [LCP[200] + 1] + LCP[201:], 300, 0, 0

    # ---- one entry out of range: 1, and the two pairs next to it add nothing
    for i in (0, 1, 64, 255, 256, 300, n - 2, n - 1):
        for name, v in (("n", n), ("n+1", n + 1), ("max", top)) + ((("+2^32", SA[i] + (1 << 32)),) if bits == 64 else ()):
            bad = list(SA)
            bad[i] = v
            yield f"sa[{i}]={name}", T, bad, LCP, n, 1, 1

    # ---- a value twice, next to itself: the pair's LCP is the whole suffix, the next pair's is recomputed -- only the repeat counts
    for i in (1, 2, 64, 256, 300, n - 2, n - 1):
        bs, bl = repeat_at(T, SA, LCP, i)
        yield f"repeat sa[{i}]=sa[{i - 1}]", T, bs, bl, n, 1, 1
    # ... and 32 and 32 k positions apart (entries of one wave, of other waves and workgroups), every LCP exact for the new
    # neighbours.  No true array has a place for an earlier value further on, so this cannot be isolated: the copy is a repeat (1)
    # and lies below its left neighbour (1); its right neighbour is above it.  And a value put in place of the one 32 k above or
    # below it (the same bit of another word of the bit set): the repeat and the order of its two pairs, whatever that comes to.
    for i, back in ((300, 32), (300, 64), (300, 256), (599, 32 * 17)):
        bs = list(SA)
        bs[i] = bs[i - back]
        yield f"repeat sa[{i}]=sa[{i - back}]", T, bs, _lcps_for(T, bs), n, 1, 2
    rank = {v: k for k, v in enumerate(SA)}
    for v, up in ((5, 32), (5, 64), (100, 32 * 9), (567, -32 * 16)):
        bs = list(SA)
        bs[rank[v + up]] = v
        yield f"repeat value {v} in place of {v + up}", T, bs, _lcps_for(T, bs), n, 1, None

    # ---- unsigned byte order: bytes on both sides of 0x80, sorted as unsigned chars, LCPs exact for that order
    H = random_text(400, "high", 9)
    hb = H.tobytes()
    su = sorted(range(H.size), key=lambda i: hb[i:])
    yield "unsigned order", H, su, _lcps_for(H, su), H.size, 1, None

    # ---- the longer suffix before its own prefix: 'A'^300 ascending
    U = np.full(300, 0x41, dtype=np.uint8)
    asc = list(range(300))
    yield "prefix order", U, asc, _lcps_for(U, asc), 300, 1, 299

    # ---- two neighbours swapped, the three touched LCPs recomputed: only that pair's order
    for i in (0, 1, 63, 64, 255, 256, 300, n - 2):
        bs = list(SA)
        bs[i], bs[i + 1] = bs[i + 1], bs[i]
        bl = _lcps_for(T, bs)
        assert sum(x != y for x, y in zip(bl, LCP)) <= 3
        yield f"swap sa[{i}], sa[{i + 1}]", T, bs, bl, n, 1, 1


FUZZ_CASES = 2000


def fuzz_cases(count=FUZZ_CASES, seed=2024):
    """count cases of n <= 48: the true arrays with 0, 1 or 2 random edits (an SA entry set to a value in [0, n + 1], or an LCP entry
    to one in [0, n]); an edit may write the value that is there.  expect is None: the model says."""
    rs = np.random.RandomState(seed)
    names = list(ALPHABETS)
    for k in range(count):
        n = int(rs.randint(1, 49))
        alphabet = names[k % len(names)]
        T = rs.choice(ALPHABETS[alphabet], size=n).astype(np.uint8)
        SA, LCP = _truth(T)
        for _ in range(int(rs.randint(0, 3))):
            i = int(rs.randint(0, n))
            if rs.randint(0, 2):
                SA[i] = int(rs.randint(0, n + 2))
            else:
                LCP[i] = int(rs.randint(0, n + 1))
        yield f"fuzz {k} {alphabet}/{n}", T, SA, LCP, n, 1, None


def slice_text():
    return random_text(70, "two", 10)


def repeat_at(T, SA, LCP, i):
    """SA[i] = SA[i-1], LCP[i] = the whole suffix, LCP[i+1] exact for the new pair: only the repeat can count."""
    n = T.size
    bs, bl = list(SA), list(LCP)
    bs[i] = bs[i - 1]
    bl[i] = n - bs[i]
    if i + 1 < n:
        bl[i + 1] = common_prefix(T.tobytes(), bs[i], bs[i + 1])
    return bs, bl


def slice_windows(T, SA, LCP, windows, heads=(0, 1)):
    """(label, T, SA[first:], LCP[first:], cnt, is_head, None) for every window and is_head."""
    for first, cnt in windows:
        for head in heads:
            yield f"window [{first}, +{cnt}) head={head}", T, SA[first:], LCP[first:], cnt, head, None


def all_windows(n):
    return [(first, cnt) for first in range(n + 1) for cnt in range(n - first + 1)]


def edge_windows(n):
    """first = 0, first = 1, cnt = 1, cnt = n - 1 and the whole array."""
    return [(0, 1), (0, n - 1), (0, n), (1, 1), (1, n - 1), (n - 1, 1), (n // 2, 1), (n // 2, n - n // 2)]


def slice_cases(every_window=True):
    """The windows of a 70-character text over two letters (LCPs rarely 0, so is_head on a window that is not the head counts 1) and
    the edge windows of the 600-character one, both is_head; then arrays with one repeat, whose first copy a window may leave out.
    every_window = False: each first with cnt = 1 and cnt = all that follows, and for the repeat the windows that begin around it
    (the MI355X file has a budget of verifier calls; the CPU file runs every window)."""
    T = slice_text()
    n = T.size
    SA, LCP = _truth(T)
    some = [(first, cnt) for first in range(n) for cnt in (1, n - first)]
    yield from slice_windows(T, SA, LCP, all_windows(n) if every_window else some)
    bs, bl = repeat_at(T, SA, LCP, 30)
    near = [(first, cnt) for first in (28, 29, 30, 31) for cnt in range(n - first + 1)]
    for c in slice_windows(T, bs, bl, all_windows(n) if every_window else near, (0, 1) if every_window else (0,)):
        yield ("repeat at 30, " + c[0],) + c[1:]
    T = base_text()
    SA, LCP = _truth(T)
    yield from (("600: " + c[0],) + c[1:] for c in slice_windows(T, SA, LCP, edge_windows(T.size)))
    bs, bl = repeat_at(T, SA, LCP, 300)
    yield "600: second copy heads the window", T, bs[300:], bl[300:], 300, 0, 0
    yield "600: both copies in the window", T, bs[299:], bl[299:], 301, 0, 1


def check_slice_counts(got):
    """What the counts of slice_cases() must show, whichever windows were run: got = {label: count}."""
    assert got["repeat at 30, window [30, +40) head=0"] == 0          # "none twice WITHIN THE SLICE"
    assert got["repeat at 30, window [29, +41) head=0"] == 1
    assert got["window [0, +70) head=1"] == 0 and got["window [0, +70) head=0"] == 0
    plain = {k: v for k, v in got.items() if k.startswith("window")}
    assert sum(v for k, v in plain.items() if k.endswith("head=0")) == 0
    heads = [v for k, v in plain.items() if k.endswith("head=1")]
    assert set(heads) == {0, 1} and sum(heads) > len(heads) * 3 // 4          # LCP != 0 at most window heads


GRID_N = 4_194_304 + 513          # one entry per thread up to 16,384 x 256 threads: beyond it the kernel's loop goes round again
GRID_SINGLE = (4_194_303, 4_194_304, 4_194_305, GRID_N - 1)


def grid_text():
    return np.random.RandomState(12).choice(ALPHABETS["four"], size=GRID_N).astype(np.uint8)


def grid_many():
    """1,000 distinct entries (entry 0 left out: its LCP is the head's)."""
    return np.sort(np.random.RandomState(13).choice(np.arange(1, GRID_N), size=1000, replace=False))


# ---- the checks both files make ------------------------------------------------------------------------------------------------
_model = {}


def model(group, case):
    """(verify_model.count of a case, whether whole arrays are the naive ones or None for a slice): worked out once per label."""
    label, T, SA, LCP, cnt, is_head, _ = case
    key = (group, label)
    if key not in _model:
        whole = cnt == T.size and is_head and len(SA) == cnt
        _model[key] = (count(T, T.size, SA, LCP, cnt, is_head), is_true_arrays(T, SA, LCP) if whole else None)
    return _model[key]


def check(verify, bits, group, case):
    """verify(bits, T, SA, LCP, cnt, is_head) -> *n_errors must be the model's count, the count the case was built for, and for
    whole arrays 0 exactly when they are the naive ones."""
    label, T, SA, LCP, cnt, is_head, expect = case
    want, true = model(group, case)
    got = verify(bits, T, SA, LCP, cnt, is_head)
    print(f"{group} u{bits} {label}: {got} (model {want})")
    assert got == want, f"{label}: the verifier counts {got}, the model {want}"
    if expect is not None:
        assert got == expect, f"{label}: {got}, built to give {expect}"
    if true is not None:
        assert (got == 0) == true, f"{label}: {got} errors, arrays {'are' if true else 'are not'} the naive ones"
    return got


_lists = {}


def cases(name, make):
    """list(make()), made once per name."""
    if name not in _lists:
        _lists[name] = list(make())
    return _lists[name]


def accepted_cases():
    for label, T in accepted_texts():
        SA, LCP = _truth(T)
        yield label, T, SA, LCP, T.size, 1, 0


EINVAL = -1


def check_refusals(lib, bits, n, t, s, l):
    """The calls that must be refused, and the empty ones that must not: t, s, l are the addresses of a text of n bytes and its true
    arrays (host memory for the emulation, device memory for the product library)."""
    import ctypes
    sfx = "u32" if bits == 32 else "u64"
    whole, part = lib._f(f"verify_device_{sfx}"), lib._f(f"verify_slice_device_{sfx}")
    err = ctypes.c_uint64(77)
    out = ctypes.byref(err)
    for cnt in (n + 1, 2 * n, (1 << 64) - 1):
        assert part(t, n, s, l, cnt, 0, None, out) == EINVAL
        assert b"more entries than suffixes" in lib._f("last_error")()
    assert whole(t, n, s, l, None, None) == EINVAL and part(t, n, s, l, n, 1, None, None) == EINVAL
    for args in ((None, s, l), (t, None, l), (t, s, None)):
        assert whole(args[0], n, args[1], args[2], None, out) == EINVAL
        assert part(args[0], n, args[1], args[2], 1, 1, None, out) == EINVAL
    for args in ((None, 0, None, None, 0), (t, 0, s, l, 0), (None, n, None, None, 0), (t, n, s, l, 0)):
        err.value = 77
        assert part(*args, 1, None, out) == 0 and err.value == 0
    err.value = 77
    assert whole(None, 0, None, None, None, out) == 0 and err.value == 0
    assert whole(t, n, s, l, None, out) == 0 and err.value == 0        # ... and the next call is served as usual
