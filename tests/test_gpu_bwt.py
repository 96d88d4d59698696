"""GPU (-m gpu): the Burrows-Wheeler transform output on the MI355X (include/caps_sa_hip.h caps_sa_hip_build_bwt_* /
caps_sa_hip_bwt_device_*): BWT[k] = T[(SA[k] + n - 1) mod n], primary = the k with SA[k] == 0.

Small inputs against np.where on golden / oracle suffix arrays; the host path in waves; C3 through build_device -> verify_device
-> bwt_device against a chunked torch gather; 64-bit positions beyond 2^32; the CLI's --bwt file."""
import os
import subprocess

import numpy as np
import pytest

from conftest import LARGE_GOLDEN, large_golden, text_bytes

pytestmark = pytest.mark.gpu
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
NONE = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


def _expect(T, SA):
    SA = np.asarray(SA).astype(np.int64)
    n = T.size
    zero = np.where(SA == 0)[0]
    return T[np.where(SA == 0, n - 1, SA - 1)], (int(zero[0]) if zero.size else NONE)


def _class_check(T, sa, lcp=None):
    import caps_sa_amd
    s = caps_sa_amd.SuffixArray(T, bwt=True)
    s.construct()
    assert np.array_equal(s.SA(), sa)
    if lcp is not None:
        assert np.array_equal(s.LCP(), lcp)
    bwt, pr = _expect(T, sa)
    assert np.array_equal(s.BWT(), bwt) and s.primary() == pr


def test_golden_and_large_fixtures(L, golden_cases):
    for c in golden_cases:
        _class_check(text_bytes(c["text"]), np.array(c["sa"]), np.array(c["lcp"]))
    for name in LARGE_GOLDEN:
        T, sa, lcp = large_golden(name)
        _class_check(T, sa, lcp)


def _torch_gather(torch, T, SA, n, step=1 << 28):
    """The baseline: T[(SA + n - 1) % n], in chunks of int64 indices."""
    out = torch.empty(SA.numel(), dtype=torch.uint8, device=T.device)
    for o in range(0, SA.numel(), step):
        s = SA[o:o + step].to(torch.int64)
        if SA.dtype == torch.int32:
            s &= 0xFFFFFFFF                               # (u32 entries held in int32: the ones >= 2^31 read back negative)
        out[o:o + step] = T[(s + (n - 1)) % n]
    return out


def _rank_of_zero(torch, SA, step=1 << 28):
    """torch.nonzero(SA == 0), chunk by chunk (one nonzero over more than 2^31 entries does not fit its own index arithmetic)."""
    for o in range(0, SA.numel(), step):
        z = torch.nonzero(SA[o:o + step] == 0)
        if z.numel():
            return o + int(z[0, 0])
    return NONE


def _random_dna(torch, n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    T = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for o in range(0, n, step):
        m = min(step, n - o)
        T[o:o + m] = lut[torch.randint(0, 4, (m,), device="cuda", generator=g, dtype=torch.int64)]
    return T


@pytest.mark.parametrize("waves,bits", [("1", 32), ("3", 32), ("3", 64)])
def test_host_path_256mi(L, monkeypatch, waves, bits):
    """256 Mi random DNA through the host path (caps_sa_hip_build_bwt_u32 and _u64), the BWT leaving the device in 1 / 3 slices;
    checked against the build's own SA (itself checked by the device verifier) with a torch gather."""
    import torch
    monkeypatch.setenv("CAPS_SA_HOST_WAVES", waves)
    n = 256 << 20
    Td = _random_dna(torch, n, 17)
    T = Td.cpu().numpy()
    SA, LCP, BWT, primary, st = L.build_bwt(T, p=8000, idx_bits=bits, pinned=True)
    assert st["idx_bytes"] == bits // 8
    assert (st["result_waves"] == 1) if waves == "1" else (st["result_waves"] >= 2), st["result_waves"]
    view = np.int32 if bits == 32 else np.int64
    SAd = torch.from_numpy(SA.view(view)).cuda()
    LCPd = torch.from_numpy(LCP.view(view)).cuda()
    assert L.verify_device(Td.data_ptr(), n, SAd.data_ptr(), LCPd.data_ptr(), idx_bits=bits) == 0
    exp = _torch_gather(torch, Td, SAd, n)
    assert torch.equal(torch.from_numpy(BWT).cuda(), exp)
    assert primary == _rank_of_zero(torch, SAd)


def test_c3_device_resident(L):
    """C3-size: build_device -> verify_device -> bwt_device over the whole SA, against a chunked torch gather from the raw text."""
    import torch
    n = 3_000_000_001
    T = _random_dna(torch, n, 42)
    T[n - 1] = ord("C")
    SA = torch.empty(n, dtype=torch.int32, device="cuda")
    LCP = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
    assert L.verify_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr()) == 0
    del LCP
    torch.cuda.empty_cache()
    BWT = torch.empty(n, dtype=torch.uint8, device="cuda")
    primary = L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, BWT.data_ptr())
    assert primary == _rank_of_zero(torch, SA)
    assert torch.equal(BWT, _torch_gather(torch, T, SA, n))
    # a slice that ends mid-word, from an odd rank (unaligned SA and output pointers)
    first, cnt = 1_000_000_007, 123_456_789
    out = torch.empty(cnt + 1, dtype=torch.uint8, device="cuda")
    pr = L.bwt_device(T.data_ptr(), n, SA.data_ptr() + 4 * first, first, cnt, out.data_ptr() + 1)
    assert torch.equal(out[1:], BWT[first:first + cnt])
    assert pr == (primary if first <= primary < first + cnt else NONE)


def test_u64_positions_beyond_2_pow_32(L, oracle):
    """64-bit indices with n > 2^32.  A whole build of that size does not fit one MI355X (test_gpu_u64_large.py), so: a 64-bit
    build of the suffixes around and beyond 2^32 (sort_suffixes: a sorted list of them, checked against the oracle), then
    bwt_device_u64 over that list as a slice at ranks beyond 2^32, against a torch gather; plus a slice that holds position 0."""
    import torch
    TWO32 = 1 << 32
    n = TWO32 + 200_000_001
    T = _random_dna(torch, n, 64)
    Th = T.cpu().numpy()
    idx = np.concatenate([np.arange(TWO32 - 2_000_000, TWO32 + 2_000_000, dtype=np.uint64),
                          np.arange(n - 1_000_000, n, dtype=np.uint64), np.arange(0, 1000, dtype=np.uint64)])
    np.random.RandomState(3).shuffle(idx)
    sa, _ = L.sort_suffixes(Th, idx, idx_bits=64)
    assert np.array_equal(sa[:20_000], oracle.merge_sort(Th, sa[:20_000].copy(), idx_bits=64)[0])
    SAd = torch.from_numpy(sa.view(np.int64)).cuda()
    out = torch.empty(sa.size, dtype=torch.uint8, device="cuda")
    first = TWO32 + 12_345                                             # the ranks of the slice: beyond 2^32
    pr = L.bwt_device(T.data_ptr(), n, SAd.data_ptr(), first, sa.size, out.data_ptr(), idx_bits=64)
    assert torch.equal(out, _torch_gather(torch, T, SAd, n))
    assert pr == first + int(np.where(sa == 0)[0][0])
    assert int((SAd >= TWO32).sum()) > 1_000_000 and out[int(np.where(sa == 0)[0][0])].item() == Th[n - 1]


def test_cli_bwt_file(L, oracle, tmp_path):
    """caps_sa --bwt PATH on a small FASTA: u64 n, u64 primary, n bytes -- the BWT of the remapped text by the dump's SA."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    exe = os.path.join(ROOT, "caps-sa_amd", "caps_sa")
    rs = np.random.RandomState(4)
    lines = [b">chr1 test"] + [bytes(rs.choice(list(b"ACGTNacgt"), size=60).tolist()) for _ in range(800)]
    raw = b"\n".join(lines) + b"\n"
    inp, out, bwt = tmp_path / "in.fa", tmp_path / "out.bin", tmp_path / "out.bwt"
    inp.write_bytes(raw)
    subprocess.check_call([exe, str(inp), str(out), "64", "--bwt", str(bwt)])
    n = len(raw)
    d = out.read_bytes()
    assert int(np.frombuffer(d[:8], dtype=np.uint64)[0]) == n
    SA = np.frombuffer(d[8:8 + 4 * n], dtype=np.uint32)
    b = bwt.read_bytes()
    hdr = np.frombuffer(b[:16], dtype=np.uint64)
    assert int(hdr[0]) == n and len(b) == 16 + n
    T = oracle.remap(raw)
    exp, pr = _expect(T, SA)
    assert np.array_equal(np.frombuffer(b[16:], dtype=np.uint8), exp) and int(hdr[1]) == pr
