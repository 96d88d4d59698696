"""GPU (-m gpu): the FM-index on the MI355X (include/caps_sa_hip.h caps_sa_hip_fm_*).

Truth is the suffix array and the text, never the index: the four-rank condition of test_emul_fm_index.py for every query, locate
against the SA slices entry by entry.  The fixtures through SuffixArray(bwt=True) -> FMIndex.from_suffix_array; 256 Mi random DNA
through the host path at both widths; C3 device-resident with a million patterns checked on the device; rows beyond 2^32 against a
suffix array in closed form; header refusals on the device entry points; the CLI round trip."""
import os
import subprocess

import numpy as np
import pytest

from conftest import LARGE_GOLDEN, large_golden, text_bytes
from test_emul_fm_index import check_answers, check_locate, make_patterns

pytestmark = pytest.mark.gpu
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


def _random_dna(torch, n, seed, letters=b"ACGT"):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    lut = torch.tensor(list(letters), dtype=torch.uint8, device="cuda")
    T = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for o in range(0, n, step):
        m = min(step, n - o)
        T[o:o + m] = lut[torch.randint(0, len(letters), (m,), device="cuda", generator=g, dtype=torch.int64)]
    return T


def test_golden_and_large_fixtures(L, golden_cases):
    import caps_sa_amd
    rs = np.random.RandomState(2)
    texts = [text_bytes(c["text"]) for c in golden_cases] + [large_golden(name)[0] for name in LARGE_GOLDEN]
    done = 0
    for T in texts:
        if T.size == 0 or np.unique(T).size > 4:
            continue
        s = caps_sa_amd.SuffixArray(T, bwt=True)
        s.construct()
        fm = caps_sa_amd.FMIndex.from_suffix_array(s)
        assert fm.n == T.size and fm.sa_sample == 32
        foreign = next(b for b in range(1, 256) if b not in set(np.unique(T).tolist()))
        pats = make_patterns(T, rs, foreign)
        first, count = fm.count(pats)
        check_answers(T, s.SA(), pats, first, count)
        check_locate(s.SA(), first, count, fm.locate(pats))
        done += 1
    assert done >= 8


def test_host_path_256mi(L):
    import caps_sa_amd
    import torch
    n = 256 << 20
    T = _random_dna(torch, n, 19).cpu().numpy()
    SA, _, B, primary, _ = L.build_bwt(T, p=8000, idx_bits=32)
    rs = np.random.RandomState(4)
    pats = make_patterns(T, rs, per_length=2)[1:]                        # (without the whole text and the whole text + 1: 256 MiB each)
    pats = [p for p in pats if len(p) <= 5000] + [b""]
    ref = None
    for bits in (32, 64):
        fm = caps_sa_amd.FMIndex.from_bwt(B, primary, SA if bits == 32 else SA.astype(np.uint64), 32, bits)
        assert fm.nbytes == L.fm_index_bytes(n, 32, bits)
        first, count = fm.count(pats)
        if ref is None:
            check_answers(T, SA, pats, first, count)
            ref = (first, count)
        assert np.array_equal(first, ref[0]) and np.array_equal(count, ref[1])
        hits = fm.locate(pats, max_hits=100_000)
        for f, c, h in zip(first.tolist(), count.tolist(), hits):
            assert np.array_equal(h, SA[f:f + min(c, 100_000)].astype(np.uint64)), (f, c)
    L.release_cache()


def _u32(torch, x):
    """int32 tensor holding uint32 values -> int64"""
    return x.to(torch.int64) & 0xFFFFFFFF


def test_c3_device_resident(L):
    """C3: build_device -> bwt_device -> fm_build_device (with the SA, s = 32), T and SA kept in HBM; 1,000,000 patterns = 900,000
    substrings of T (lengths uniform in 1 .. 64) + 100,000 random 24-mers; the four-rank condition for EVERY query with gathers on
    the device, an absent pattern confirmed by bisection over the SA on the device; locate in full for every query with
    count <= 1000 and for the first 1000 ranks of the others, torch.equal against the SA slices."""
    import torch
    n = 3_000_000_001
    W = 64
    T = _random_dna(torch, n, 42)
    SA = torch.empty(n, dtype=torch.int32, device="cuda")
    LCP = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
    del LCP
    torch.cuda.empty_cache()
    B = torch.empty(n, dtype=torch.uint8, device="cuda")
    primary = L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, B.data_ptr())
    nbytes = L.fm_index_bytes(n, 32, 32)
    index = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.fm_build_device(B.data_ptr(), n, primary, SA.data_ptr(), 32, index.data_ptr(), nbytes)
    del B
    torch.cuda.empty_cache()

    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    q_sub, q_rnd = 900_000, 100_000
    q = q_sub + q_rnd
    lens = torch.cat([torch.randint(1, W + 1, (q_sub,), device="cuda", generator=g), torch.full((q_rnd,), 24, device="cuda")])
    starts = torch.randint(0, n - W, (q_sub,), device="cuda", generator=g)
    ar = torch.arange(W, device="cuda")
    M = torch.empty((q, W), dtype=torch.uint8, device="cuda")                 # the patterns, one per row, lens[j] bytes of it
    M[:q_sub] = T[starts[:, None] + ar]
    M[q_sub:] = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[torch.randint(0, 4, (q_rnd, W), device="cuda", generator=g)]
    inpat = ar[None, :] < lens[:, None]
    pat = M[inpat].contiguous()
    off = torch.zeros(q + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(lens, 0)
    first = torch.full((q,), -1, dtype=torch.int64, device="cuda")
    count = torch.full((q,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L.fm_count_device(index.data_ptr(), nbytes, pat.data_ptr(), off.data_ptr(), q, first.data_ptr(), count.data_ptr())
    assert bool((first >= 0).all()) and bool((count >= 0).all()) and bool((first + count <= n).all())

    def compare(rank, rows):
        """suffix SA[rank] against the patterns of `rows` over their lengths: -1 / 0 / +1 (0: the pattern is a prefix of it)"""
        s = _u32(torch, SA[rank])
        p = s[:, None] + ar
        inside = p < n
        ch = T[p.clamp(max=n - 1)]
        diff = ((ch != M[rows]) | ~inside) & inpat[rows]
        any_diff = diff.any(1)
        k = diff.to(torch.uint8).argmax(1)
        a = ch.gather(1, k[:, None])[:, 0].to(torch.int64)
        b = M[rows].gather(1, k[:, None])[:, 0].to(torch.int64)
        short = ~inside.gather(1, k[:, None])[:, 0]
        sign = torch.where(short | (a < b), -1, 1)
        return torch.where(any_diff, sign, 0)

    hit = torch.nonzero(count > 0)[:, 0]
    miss = torch.nonzero(count == 0)[:, 0]
    assert hit.numel() >= q_sub and miss.numel() > 90_000                      # (nearly every random 24-mer is absent)
    assert bool((first[miss] == 0).all())
    assert bool((compare(first[hit], hit) == 0).all())
    assert bool((compare(first[hit] + count[hit] - 1, hit) == 0).all())
    lo_rows = hit[first[hit] > 0]
    assert bool((compare(first[lo_rows] - 1, lo_rows) != 0).all())
    hi_rows = hit[first[hit] + count[hit] < n]
    assert bool((compare(first[hi_rows] + count[hi_rows], hi_rows) != 0).all())
    # absent: the lower bound of the pattern among the suffixes is no match
    lo = torch.zeros(miss.numel(), dtype=torch.int64, device="cuda")
    hi = torch.full((miss.numel(),), n, dtype=torch.int64, device="cuda")
    for _ in range(33):
        mid = (lo + hi) // 2
        live = lo < hi
        c = compare(mid.clamp(max=n - 1), miss)
        lo = torch.where(live & (c < 0), mid + 1, lo)
        hi = torch.where(live & (c >= 0), mid, hi)
    assert bool((lo == hi).all())
    at_end = lo >= n
    assert bool((at_end | (compare(lo.clamp(max=n - 1), miss) != 0)).all())

    # locate: every hit up to 1000 per query
    take = count.clamp(max=1000)
    out_off = torch.zeros(q + 1, dtype=torch.int64, device="cuda")
    out_off[1:] = torch.cumsum(take, 0)
    total = int(out_off[-1])
    pos = torch.full((total,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L.fm_locate_device(index.data_ptr(), nbytes, first.data_ptr(), count.data_ptr(), out_off.data_ptr(), q, pos.data_ptr())
    rank = torch.repeat_interleave(first - out_off[:-1], take) + torch.arange(total, device="cuda")
    assert torch.equal(pos, _u32(torch, SA[rank]))


def test_u64_rows_beyond_2_pow_32(L):
    """T = 'A' * m + R, m = 2^32 + 1000, R = 1e7 letters over {C, G, T} (the text of the inverse BWT's test): BWT and SA in closed
    form from the library's SA of R (SA[k] = k for k < m, SA[m + i] = m + SA_R[i]).  'A' * k counts m - k + 1 at first = 0;
    patterns cut from R count as they do in R, at first >= m; locate returns positions >= 2^32 equal to the closed-form SA."""
    import torch
    m = (1 << 32) + 1000
    Rd = _random_dna(torch, 10_000_000, 7, b"CGT")
    R = Rd.cpu().numpy()
    SA_R, _, _ = L.build(R, p=256)
    tail = np.where(SA_R > 0, R[SA_R.astype(np.int64) - 1], ord("A")).astype(np.uint8)
    n = m + R.size
    B = torch.empty(n, dtype=torch.uint8, device="cuda")
    B[0] = int(R[-1])
    B[1:m] = ord("A")
    B[m:] = torch.from_numpy(tail).cuda()
    SA = torch.empty(n, dtype=torch.int64, device="cuda")
    step = 1 << 30                                                       # (in pieces: one arange of more than 2^32 elements is not relied on)
    for o in range(0, m, step):
        SA[o:min(m, o + step)] = torch.arange(o, min(m, o + step), dtype=torch.int64, device="cuda")
    SA[m:] = torch.from_numpy(SA_R.astype(np.int64)).cuda() + m
    assert int(SA[m - 1]) == m - 1 and int(SA[1 << 32]) == 1 << 32
    nbytes = L.fm_index_bytes(n, 32, 64)
    index = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.fm_build_device(B.data_ptr(), n, 0, SA.data_ptr(), 32, index.data_ptr(), nbytes, idx_bits=64)
    del B
    rs = np.random.RandomState(12)
    ks = [1, 2, 5, 64, 1000]
    pats = [b"A" * k for k in ks] + [p for p in make_patterns(R, rs, foreign=ord("N"))[3:] if p]
    cat, off = L._patterns(pats)
    q = len(pats)
    d_cat, d_off = torch.from_numpy(cat).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    first = torch.zeros(q, dtype=torch.int64, device="cuda")
    count = torch.zeros(q, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L.fm_count_device(index.data_ptr(), nbytes, d_cat.data_ptr(), d_off.data_ptr(), q, first.data_ptr(), count.data_ptr())
    f, c = first.cpu().numpy(), count.cpu().numpy()
    for j, k in enumerate(ks):
        assert (f[j], c[j]) == (0, m - k + 1), (k, f[j], c[j])
    fr, cr = f[len(ks):], c[len(ks):]
    assert (fr[cr > 0] >= m).all() and (fr[cr == 0] == 0).all() and (cr > 0).sum() >= 20
    check_answers(R, SA_R, pats[len(ks):], np.where(cr > 0, fr - m, 0).astype(np.uint64), cr.astype(np.uint64))
    take = count.clamp(max=5000)
    out_off = torch.zeros(q + 1, dtype=torch.int64, device="cuda")
    out_off[1:] = torch.cumsum(take, 0)
    total = int(out_off[-1])
    pos = torch.full((total,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L.fm_locate_device(index.data_ptr(), nbytes, first.data_ptr(), count.data_ptr(), out_off.data_ptr(), q, pos.data_ptr())
    rank = torch.repeat_interleave(first - out_off[:-1], take) + torch.arange(total, device="cuda")
    assert torch.equal(pos, SA[rank])
    beyond = pos[int(out_off[len(ks)]):]
    assert beyond.numel() > 1000 and bool((beyond >= (1 << 32)).all())


def test_header_refusals_on_the_device_entry_points(L):
    """Host-side checks only (the body stays a valid index): wrong magic, short index_bytes; a valid call afterwards."""
    import caps_sa_amd
    import torch
    rs = np.random.RandomState(6)
    T = rs.choice(DNA, size=200_000)
    SA, _, B, primary, _ = L.build_bwt(T)
    blob = L.fm_build(B, primary, SA, 32)
    pats = make_patterns(T, rs)
    cat, off = L._patterns(pats)
    q = len(pats)
    d_cat, d_off = torch.from_numpy(cat).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    first = torch.zeros(q, dtype=torch.int64, device="cuda")
    count = torch.zeros(q, dtype=torch.int64, device="cuda")
    good = torch.from_numpy(blob).cuda()
    bad = good.clone()
    bad[0] ^= 1
    torch.cuda.synchronize()
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        L.fm_count_device(bad.data_ptr(), bad.numel(), d_cat.data_ptr(), d_off.data_ptr(), q, first.data_ptr(), count.data_ptr())
    assert e.value.code == EINVAL and "magic" in str(e.value)
    for short in (100, blob.size - 1):
        with pytest.raises(caps_sa_amd.CapsSaError) as e:
            L.fm_count_device(good.data_ptr(), short, d_cat.data_ptr(), d_off.data_ptr(), q, first.data_ptr(), count.data_ptr())
        assert e.value.code == EINVAL
        with pytest.raises(caps_sa_amd.CapsSaError) as e:
            L.fm_locate_device(good.data_ptr(), short, first.data_ptr(), count.data_ptr(), d_off.data_ptr(), q, 0)
        assert e.value.code == EINVAL
    L.fm_count_device(good.data_ptr(), good.numel(), d_cat.data_ptr(), d_off.data_ptr(), q, first.data_ptr(), count.data_ptr())
    f, c = first.cpu().numpy().astype(np.uint64), count.cpu().numpy().astype(np.uint64)
    check_answers(T, SA, pats, f, c)
    out_off = np.zeros(q + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(c.astype(np.int64))
    pos = torch.zeros(int(out_off[-1]), dtype=torch.int64, device="cuda")
    d_out = torch.from_numpy(out_off).cuda()
    torch.cuda.synchronize()
    L.fm_locate_device(good.data_ptr(), good.numel(), first.data_ptr(), count.data_ptr(), d_out.data_ptr(), q, pos.data_ptr())
    pos = pos.cpu().numpy().astype(np.uint64)
    check_locate(SA, f, c, [pos[out_off[j]:out_off[j + 1]] for j in range(q)])


def test_cli_round_trip(L, tmp_path):
    """caps_sa in.fa out.bin --fm-index x.fm, then caps_sa --fm-search x.fm pats.txt --locate 5 against the dump's SA."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    exe = os.path.join(ROOT, "caps-sa_amd", "caps_sa")
    rs = np.random.RandomState(8)
    lines = [b">chr1 test"] + [bytes(rs.choice(list(b"ACGTNacgt"), size=60).tolist()) for _ in range(2000)]
    raw = b"\n".join(lines) + b"\n"
    inp, out, fm, pt = tmp_path / "in.fa", tmp_path / "out.bin", tmp_path / "x.fm", tmp_path / "pats.txt"
    inp.write_bytes(raw)
    subprocess.check_call([exe, str(inp), str(out), "--fm-index", str(fm), "--fm-sample", "16"])
    dump = out.read_bytes()
    n = int(np.frombuffer(dump[:8], dtype=np.uint64)[0])
    assert n == len(raw)
    SA = np.frombuffer(dump[8:8 + 4 * n], dtype=np.uint32)
    remap = np.frombuffer(b"ACTG", dtype=np.uint8)
    T = remap[(np.frombuffer(raw.upper(), dtype=np.uint8) & 0x6) >> 1]
    assert fm.stat().st_size == L.fm_index_bytes(n, 16, 32)
    queries = [raw[a:a + m] for a, m in zip(rs.randint(0, n - 40, size=300), rs.randint(1, 40, size=300))]
    queries = [p for p in queries if b"\n" not in p and b"\r" not in p] + [b"acgtacgtacgtacgtacgtacgtacgtacgtacgt", b"A", b"GATTACA"]
    pt.write_bytes(b"\n".join(queries) + b"\n")
    r = subprocess.run([exe, "--fm-search", str(fm), str(pt), "--locate", "5"], capture_output=True, text=True, check=True)
    rows = r.stdout.splitlines()
    assert len(rows) == len(queries)
    pats = [remap[(np.frombuffer(p.upper(), dtype=np.uint8) & 0x6) >> 1].tobytes() for p in queries]
    tb = T.tobytes()
    for P, row in zip(pats, rows):
        vals = [int(x) for x in row.split()]
        cnt, pos = vals[0], vals[1:]
        occ, i = 0, tb.find(P)
        while i >= 0:
            occ, i = occ + 1, tb.find(P, i + 1)
        assert cnt == occ and len(pos) == min(cnt, 5), (P, row)
        if cnt:
            k = int(np.flatnonzero(SA == pos[0])[0])
            assert pos == SA[k:k + len(pos)].tolist() and tb[pos[0]:pos[0] + len(P)] == P
            assert k == 0 or tb[int(SA[k - 1]):int(SA[k - 1]) + len(P)] != P          # the first rank of the interval
