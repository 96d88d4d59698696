"""GPU (-m gpu): the wide FM-index on the MI355X (include/caps_sa_hip.h "FM-index: the wide format").

The emulation's blob and answer sweeps through the host and the device entry points at a trimmed size list; texts of 8 Mi rows (more
than 256 tiles) device-resident, locate and count checked on the device against the SA and the text; the 4-letter differential at
2^20 + 1 rows; the Python class with save / load.  Every check is exact.  No damaged bodies here."""
import os

import numpy as np
import pytest

import fm_match_reference as M
import fm_wide_reference as W
from test_emul_fm_wide import blob_case, check_all, make_patterns

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -2
SIZES = (0, 1, 127, 128, 129, 16383, 16384, 16385)
SIGMAS = (5, 17, 256)


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


def _device_blob(L, torch, B, primary, SA, s, bits, workspace=True):
    """fm_build_wide_device on torch tensors -> the blob as np.uint8 (header word 18 bytes of the capacity)."""
    n = int(B.size)
    dB = torch.from_numpy(np.ascontiguousarray(B)).cuda() if n else torch.zeros(1, dtype=torch.uint8, device="cuda")
    dSA = None
    if SA is not None:
        dSA = torch.zeros(max(n, 1), dtype=torch.int32 if bits == 32 else torch.int64, device="cuda")   # (n = 0: an SA of no entries, not NULL)
        dSA[:n] = torch.from_numpy(np.ascontiguousarray(SA).astype(np.int32 if bits == 32 else np.int64)).cuda()
    cap = L.fm_wide_index_bytes(n, 0, s, bits)
    idx = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ws_bytes = L.fm_wide_workspace_bytes(n, bits) if workspace else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda") if workspace else None
    torch.cuda.synchronize()
    L.fm_build_wide_device(dB.data_ptr() if n else 0, n, primary, dSA.data_ptr() if dSA is not None else 0, s or 32, idx.data_ptr(), cap,
                           ws.data_ptr() if workspace else 0, ws_bytes, bits)
    out = idx.cpu().numpy()
    total = int(out[:256].view(np.uint64)[18])
    assert total <= cap and (out[total:] == 0xA5).all()
    return out[:total].copy()


def test_blobs_host_and_device_entry_points(L):
    import torch
    k = 0
    for n in SIZES:
        for sigma in ((1,) if n == 0 else SIGMAS):
            if n and n < sigma:
                continue
            for bits in (32, 64):
                for s in (0, 32):
                    primary = W.edge_primaries(n)[k % len(W.edge_primaries(n))] if n else 0
                    blob = blob_case(L, n, sigma, primary, bits, s)                  # the host form against the encoder
                    rs = np.random.RandomState(7 * n + sigma)
                    B = W.text_with_sigma(n, sigma, 0) if n else np.zeros(0, dtype=np.uint8)
                    SA = rs.permutation(n) if s else None
                    assert np.array_equal(_device_blob(L, torch, B, primary, SA, s, bits, workspace=bool(k % 2)), blob), (n, sigma, bits, s)
                    k += 1
    assert k == 4 + 3 * 2 * 4 + 3 * 3 * 4


@pytest.mark.parametrize("sigma", SIGMAS)
def test_answers_against_the_references(L, sigma):
    import caps_sa_amd
    T = W.text_with_sigma(700 + sigma, sigma, 3)
    SA = W.naive_sa(T)
    B, primary = W.bwt_of(T, SA)
    R = M.Text(T, SA)
    foreign = next((b for b in range(255, -1, -1) if b not in set(T.tolist())), int(T[0]))       # (256 letters: no byte is foreign)
    pats = make_patterns(T, np.random.RandomState(sigma), foreign, 25)
    for bits, s in ((32, 1), (64, 32), (32, 0)):
        fm = caps_sa_amd.FMIndex.from_bwt(B, primary, SA if s else None, s or 32, bits, wide=True)
        assert (fm.wide, fm.sigma, fm.sa_sample) == (True, sigma, s)
        check_all(fm, T, SA, pats, R, min_len=2)


def _random_text(torch, n, letters, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    lut = torch.tensor(list(letters), dtype=torch.uint8, device="cuda")
    return lut[torch.randint(0, len(letters), (n,), device="cuda", generator=g, dtype=torch.int64)]


def _device_case(L, torch, T, bits, sigma):
    """build_device -> bwt_device -> fm_build_wide_device, then on the device: locate of 2^16 random ranks equals the SA, count of
    2^16 pieces of T: the interval holds the piece's rank, its ends start with the piece, the ranks just outside do not."""
    n = int(T.numel())
    it = torch.int32 if bits == 32 else torch.int64
    SA = torch.empty(n, dtype=it, device="cuda")
    LCP = torch.empty(n, dtype=it, device="cuda")
    torch.cuda.synchronize()
    L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), idx_bits=bits)
    del LCP
    B = torch.empty(n, dtype=torch.uint8, device="cuda")
    primary = L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, B.data_ptr(), idx_bits=bits)
    cap = L.fm_wide_index_bytes(n, sigma, 32, bits)
    index = torch.empty(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.fm_build_wide_device(B.data_ptr(), n, primary, SA.data_ptr(), 32, index.data_ptr(), cap, 0, 0, bits)
    hdr = index[:256].cpu().numpy().view(np.uint64)
    assert bytes(index[:8].cpu().numpy()) == b"CAPSFMW1" and int(hdr[18]) == cap and int(hdr[5]) == sigma and int(hdr[2]) == n
    sa64 = SA.to(torch.int64) & (0xFFFFFFFF if bits == 32 else -1)
    g = torch.Generator(device="cuda")
    g.manual_seed(n % 1000 + sigma)
    q = 1 << 16
    # locate: q random ranks, one hit each
    ranks = torch.randint(0, n, (q,), device="cuda", generator=g)
    ones = torch.ones(q, dtype=torch.int64, device="cuda")
    off = torch.arange(q + 1, dtype=torch.int64, device="cuda")
    pos = torch.full((q,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L.fm_locate_device(index.data_ptr(), cap, ranks.data_ptr(), ones.data_ptr(), off.data_ptr(), q, pos.data_ptr())
    assert torch.equal(pos, sa64[ranks])
    # count: q pieces of T
    Wd = 24
    lens = torch.randint(1, Wd + 1, (q,), device="cuda", generator=g)
    starts = torch.randint(0, n - Wd, (q,), device="cuda", generator=g)
    ar = torch.arange(Wd, device="cuda")
    P = T[starts[:, None] + ar]
    inpat = ar[None, :] < lens[:, None]
    pat = P[inpat].contiguous()
    poff = torch.zeros(q + 1, dtype=torch.int64, device="cuda")
    poff[1:] = torch.cumsum(lens, 0)
    first = torch.full((q,), -1, dtype=torch.int64, device="cuda")
    count = torch.full((q,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    L.fm_count_device(index.data_ptr(), cap, pat.data_ptr(), poff.data_ptr(), q, first.data_ptr(), count.data_ptr())
    rank = torch.empty(n, dtype=torch.int64, device="cuda")
    rank[sa64] = torch.arange(n, device="cuda")
    r = rank[starts]
    assert bool((count >= 1).all()) and bool((first <= r).all()) and bool((r < first + count).all()) and bool((first + count <= n).all())

    def starts_with(rk):
        p = sa64[rk][:, None] + ar
        same = (T[p.clamp(max=n - 1)] == P) & (p < n)
        return (same | ~inpat).all(1)

    assert bool(starts_with(first).all()) and bool(starts_with(first + count - 1).all())
    lo = first > 0
    assert not bool(starts_with((first - 1).clamp(min=0))[lo].any())
    hi = first + count < n
    assert not bool(starts_with((first + count).clamp(max=n - 1))[hi].any())


@pytest.mark.parametrize("n,bits", [((8 << 20) - 2, 32), ((8 << 20) - 1, 32), (8 << 20, 32), ((8 << 20) - 2, 64)])
def test_8mi_rows_five_letters(L, n, bits):
    """8 Mi - 1, 8 Mi and 8 Mi + 1 rows (rows = n + 1): 512 tiles, two levels."""
    import torch
    T = _random_text(torch, n, b"ACGTN", 5)
    _device_case(L, torch, T, bits, 5)


def test_8mi_rows_all_bytes(L):
    """8 Mi + 1 rows over all 256 bytes: four levels, three scatters."""
    import torch
    n = 8 << 20
    T = _random_text(torch, n, bytes(range(256)), 6)
    assert int(torch.unique(T).numel()) == 256
    _device_case(L, torch, T, 32, 256)


def test_four_letter_differential_2_20(L):
    import caps_sa_amd
    import torch
    n = 1 << 20                                                                      # 2^20 + 1 rows
    T = _random_text(torch, n, bytes([0x80, 0xFE, 0x05, 0x7F]), 8).cpu().numpy()
    SA, _, B, primary, _ = L.build_bwt(T)
    rs = np.random.RandomState(3)
    pats = make_patterns(T, rs, ord("N"))
    for bits in (32, 64):
        wide = caps_sa_amd.FMIndex.from_bwt(B, primary, SA, 32, bits, wide=True)
        narrow = caps_sa_amd.FMIndex.from_bwt(B, primary, SA, 32, bits)
        assert np.array_equal(wide.blob[5056:], narrow.blob[256:])
        for a, b in zip(wide.count(pats), narrow.count(pats)):
            assert np.array_equal(a, b)
        for a, b in zip(wide.locate(pats, 50), narrow.locate(pats, 50)):
            assert np.array_equal(a, b)
        for a, b in zip(wide.matching_statistics(pats, 40, True), narrow.matching_statistics(pats, 40, True)):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        for a, b in zip(wide.mems(pats, 3), narrow.mems(pats, 3)):
            assert np.array_equal(a, b)


def test_python_class_save_load(L, tmp_path):
    import caps_sa_amd
    T = np.frombuffer(b"the quick brown fox jumps over the lazy dog; THE QUICK BROWN FOX \xe9\xe8\x80\xff" * 40, dtype=np.uint8)
    s = caps_sa_amd.SuffixArray(T, bwt=True)
    s.construct()
    with pytest.raises(caps_sa_amd.CapsSaError):
        caps_sa_amd.FMIndex.from_suffix_array(s)                                     # (the default stays the narrow build)
    fm = caps_sa_amd.FMIndex.from_suffix_array(s, 16, wide=True)
    assert fm.wide and fm.sigma == np.unique(T).size and fm.n == T.size and fm.sa_sample == 16
    path = os.path.join(tmp_path, "wide.fmi")
    fm.save(path)
    fm2 = caps_sa_amd.FMIndex.load(path)
    assert fm2.wide and np.array_equal(fm2.blob, fm.blob)
    pats = [b"quick", b"QUICK", b"\xe9\xe8", b"zebra", b"", b"the lazy dog; THE"]
    first, count = fm2.count(pats)
    assert count.tolist() == [40, 40, 40, 0, T.size, 40]
    SA = s.SA()
    for h, f, c in zip(fm2.locate(pats), first.tolist(), count.tolist()):
        assert np.array_equal(h, SA[f:f + c].astype(np.uint64))
    assert [m["length"].tolist() for m in fm2.mems([b"quick~brown"], 5)] == [[5, 5]]
    for call in (lambda: fm2.with_text_samples(32), lambda: fm2.extract([0], [4]),
                 lambda: caps_sa_amd.FMIndex.from_bwt_only(s.BWT(), s.primary(), 32, wide=True)):
        with pytest.raises(caps_sa_amd.CapsSaError) as e:
            call()
        assert e.value.code == EUNSUPPORTED


def test_cli_raw_round_trip(L, tmp_path):
    """caps_sa in.txt out.bin --raw --bwt x.bwt --fm-index w.fm on the device: the text's own SA / LCP, BWT and the wide blob byte
    for byte, then --fm-search and --fm-mems with the pattern lines as bytes (tests/test_cli_fm_wide.py has the expectations)."""
    import subprocess
    import fm_reference as R
    import test_cli_fm_wide as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "caps-sa_amd"), "caps_sa"], timeout=600)
    exe = os.path.join(root, "caps-sa_amd", "caps_sa")
    T = C.make_text()
    SA = R.naive_sa(T)
    (tmp_path / "in.txt").write_bytes(T.tobytes())
    (tmp_path / "p.txt").write_bytes(b"\n".join(C.PATTERN_LINES) + b"\n")

    def run(*args):
        return subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=60)
    r = run(tmp_path / "in.txt", tmp_path / "out.bin", "--raw", "--bwt", tmp_path / "x.bwt", "--fm-index", tmp_path / "w.fm", "--fm-sample", "4")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.bin").read_bytes() == C.dump_of(T, SA)
    bwt_bytes, B, primary = C.bwt_file_of(T, SA)
    assert (tmp_path / "x.bwt").read_bytes() == bwt_bytes
    assert (tmp_path / "w.fm").read_bytes() == W.encode(B, primary, SA, 4, 4).tobytes()
    lines = [p.rstrip(b"\r") for p in C.PATTERN_LINES]
    r = run("--fm-search", tmp_path / "w.fm", tmp_path / "p.txt", "--locate", "1000")
    assert r.returncode == 0 and r.stdout == C.expected_search(T, SA, lines, 1000), r.stderr
    r = run("--fm-mems", tmp_path / "w.fm", tmp_path / "p.txt", "--min-len", "2")
    assert r.returncode == 0 and r.stdout == C.expected_mems(T, SA, lines, 2), r.stderr
    r = run("--fm-extract", tmp_path / "w.fm", tmp_path / "p.txt")
    assert r.returncode != 0 and r.stdout == b""
