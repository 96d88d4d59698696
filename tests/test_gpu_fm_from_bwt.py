"""GPU (-m gpu): the FM-index with its SA samples from (BWT, primary) alone on the MI355X (caps_sa_hip_fm_build_from_bwt_*).

What the emulation cannot see is here: the global atomic OR on the mark words while other waves read the same lines, the LDS walk
counter, partly filled last workgroups.  The device form writes into an index preset to 0xA5 with a 64-byte guard behind it, on a
workspace preset to 0xA5; every blob is compared byte for byte with fm_reference.encode or with fm_build_device given the SA.
One process; every input is one the contract defines."""
import os
import subprocess

import numpy as np
import pytest

import fm_reference as R
from test_emul_fm_from_bwt import LEVEL_SIZES, SPLITTER_SIZES, blobs_from_bwt, walk_edges
from test_emul_fm_index import check_answers, check_locate, make_patterns
from test_emul_geometry import LARGE, MILLION, SAMPLES, SMALL

pytestmark = pytest.mark.gpu
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
GUARD = 64
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(a).cuda()


class DeviceForm:
    """fm_build_from_bwt through the *_device entry point: index and workspace preset to 0xA5, a guard behind each."""

    def __init__(self, L):
        import torch
        self.L, self.torch = L, torch
        self.build_bwt = L.build_bwt
        self.fm_index_bytes = L.fm_index_bytes

    def _filled(self, nbytes):
        return self.torch.full((nbytes + GUARD,), FILL, dtype=self.torch.uint8, device="cuda")

    def fm_build_from_bwt(self, B, primary, s=32, bits=32):
        torch = self.torch
        n = int(B.size)
        dB = _dev(torch, B if n else np.zeros(1, dtype=np.uint8))
        nbytes = self.L.fm_index_bytes(n, s, bits)
        ws_bytes = self.L.fm_from_bwt_workspace_bytes(n, s, bits)
        index, ws = self._filled(nbytes), self._filled(ws_bytes)
        torch.cuda.synchronize()
        self.L.fm_build_from_bwt_device(dB.data_ptr(), n, primary, s, index.data_ptr(), nbytes, ws.data_ptr(), ws_bytes, idx_bits=bits)
        assert bool((ws[ws_bytes:] == FILL).all()), "bytes behind the workspace were written"
        out = index.cpu().numpy()
        assert (out[nbytes:] == FILL).all(), "bytes behind the index were written"
        return out[:nbytes].copy()


def test_blob_bytes_device_form(L):
    """The sweep of test_emul_fm_from_bwt.test_blob_bytes (against the encoder; the build with the SA is compared in the 8 Mi test)."""
    D = DeviceForm(L)
    assert blobs_from_bwt(D, SMALL, with_fm_build=False) + blobs_from_bwt(D, LARGE, with_fm_build=False) >= 400


def test_blob_bytes_host_form_against_the_build_with_the_sa(L):
    assert blobs_from_bwt(L, SMALL, samples=(1, 32, 1024)) >= 100


def test_walk_edges_device_form(L):
    D = DeviceForm(L)
    assert walk_edges(D, SPLITTER_SIZES, SAMPLES) == 240
    assert walk_edges(D, LEVEL_SIZES, (1, 32, 1024)) == len(LEVEL_SIZES) * 5 * 3 * 2


@pytest.mark.parametrize("n", MILLION)
def test_third_ranking_level(L, n):
    """Every sample distance and both widths around 2^20 rows."""
    D = DeviceForm(L)
    T = np.random.RandomState(n).choice(DNA, size=n)
    SA, _, B, primary, _ = L.build_bwt(T)
    for s in SAMPLES:
        for bits in (32, 64):
            blob = D.fm_build_from_bwt(B, primary, s, bits)
            want = R.encode(B, primary, SA, s, bits // 8)
            assert blob.size == want.size and np.array_equal(blob, want), (n, s, bits, np.flatnonzero(blob != want)[:8])


@pytest.mark.parametrize("n", [(8 << 20) - 1, 8 << 20, (8 << 20) + 1])
def test_blob_over_512_tiles(L, n):
    """8 Mi +- 1 rows: 512 tiles, 131 k splitters, three list levels.  The SA from the build on the GPU; the blob from the BWT alone
    must be torch.equal to fm_build_device with that SA, at s = 1 and 32 in u32 and s = 32 in u64."""
    import torch
    T = np.random.RandomState(n % 1000).choice(DNA, size=n)
    dT = _dev(torch, T)
    dSA = torch.empty(n, dtype=torch.int32, device="cuda")
    dLCP = torch.empty(n, dtype=torch.int32, device="cuda")
    dB = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.build_device(dT.data_ptr(), n, dSA.data_ptr(), dLCP.data_ptr())
    primary = L.bwt_device(dT.data_ptr(), n, dSA.data_ptr(), 0, n, dB.data_ptr())
    del dLCP, dT
    dSA64 = dSA.to(torch.int64) & 0xFFFFFFFF
    for s, bits in ((1, 32), (32, 32), (32, 64)):
        nbytes = L.fm_index_bytes(n, s, bits)
        ws_bytes = L.fm_from_bwt_workspace_bytes(n, s, bits)
        assert ws_bytes <= ((n - 1) // s + 1) * (bits // 8) + 32 * (n // 64 + 1) + 2**20
        want = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        got = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        ws = torch.full((ws_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        L.fm_build_device(dB.data_ptr(), n, primary, (dSA if bits == 32 else dSA64).data_ptr(), s, want.data_ptr(), nbytes, idx_bits=bits)
        L.fm_build_from_bwt_device(dB.data_ptr(), n, primary, s, got.data_ptr(), nbytes, ws.data_ptr(), ws_bytes, idx_bits=bits)
        assert bool((got[nbytes:] == FILL).all()) and bool((ws[ws_bytes:] == FILL).all())
        assert torch.equal(got, want), (n, s, bits, torch.nonzero(got != want)[:8].flatten().tolist())


def test_host_form_and_the_resident_index(L):
    """The host form gives the device form's bytes on three sizes, and leaves the index resident: count and locate through the
    host forms right after it (no upload in between) answer from the SA."""
    import caps_sa_amd
    D = DeviceForm(L)
    for n in (1000, 16_385, 300_001):
        rs = np.random.RandomState(n)
        T = rs.choice(DNA, size=n)
        SA, _, B, primary, _ = L.build_bwt(T)
        for s, bits in ((32, 32), (2, 64)):
            fm = caps_sa_amd.FMIndex.from_bwt_only(B, primary, s, bits)
            pats = make_patterns(T, rs)
            first, count = fm.count(pats)
            hits = fm.locate(pats, max_hits=50)
            check_answers(T, SA, pats, first, count)
            check_locate(SA, first, np.minimum(count, np.uint64(50)), hits)
            assert np.array_equal(fm.blob, D.fm_build_from_bwt(B, primary, s, bits)), (n, s, bits)
            assert np.array_equal(fm.blob, R.encode(B, primary, SA, s, bits // 8)), (n, s, bits)


# a swap of two bytes of different letters in the BWT of RandomState(100_000).choice(DNA, 100_000) that breaks the LF cycle: found
# on the CPU with the emulated inverse BWT, which refuses the swapped pair
NOT_A_BWT_SWAP = (77_708, 98_539)


def test_not_a_bwt_returns(L):
    """An input the contract defines: EINVAL with the inverse's message, the call returns, and the next valid call on the same
    workspace succeeds."""
    import caps_sa_amd
    import torch
    n = 100_000
    T = np.random.RandomState(n).choice(DNA, size=n)
    SA, _, B, primary, _ = L.build_bwt(T)
    assert primary == 42_397
    i, j = NOT_A_BWT_SWAP
    bad = B.copy()
    assert bad[i] != bad[j]
    bad[i], bad[j] = B[j], B[i]
    for bits in (32, 64):
        nbytes = L.fm_index_bytes(n, 32, bits)
        ws_bytes = L.fm_from_bwt_workspace_bytes(n, 32, bits)
        index = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        ws = torch.full((ws_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        d_bad, d_good = _dev(torch, bad), _dev(torch, B)
        torch.cuda.synchronize()
        with pytest.raises(caps_sa_amd.CapsSaError) as e:
            L.fm_build_from_bwt_device(d_bad.data_ptr(), n, primary, 32, index.data_ptr(), nbytes, ws.data_ptr(), ws_bytes, idx_bits=bits)
        assert e.value.code == EINVAL and "LF mapping is not one cycle" in str(e.value)
        L.fm_build_from_bwt_device(d_good.data_ptr(), n, primary, 32, index.data_ptr(), nbytes, ws.data_ptr(), ws_bytes, idx_bits=bits)
        out = index.cpu().numpy()
        assert (out[nbytes:] == FILL).all() and bool((ws[ws_bytes:] == FILL).all())
        assert np.array_equal(out[:nbytes], R.encode(B, primary, SA, 32, bits // 8)), bits
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        L.fm_build_from_bwt(bad, primary, 32)
    assert e.value.code == EINVAL and "LF mapping is not one cycle" in str(e.value)


def test_cli_round_trip(L, tmp_path):
    """caps_sa in out --bwt x.bwt --fm-index a.fm, then caps_sa --fm-from-bwt x.bwt b.fm: the same bytes."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    exe = os.path.join(ROOT, "caps-sa_amd", "caps_sa")
    rs = np.random.RandomState(9)
    raw = b"\n".join([b">chr1 test"] + [bytes(rs.choice(list(b"ACGTNacgt"), size=60).tolist()) for _ in range(2000)]) + b"\n"
    inp, out, bwt, a, b = (tmp_path / x for x in ("in.fa", "out.bin", "x.bwt", "a.fm", "b.fm"))
    inp.write_bytes(raw)
    for sample in (None, "4"):
        extra = [] if sample is None else ["--fm-sample", sample]
        subprocess.check_call([exe, str(inp), str(out), "--bwt", str(bwt), "--fm-index", str(a)] + extra)
        subprocess.check_call([exe, "--fm-from-bwt", str(bwt), str(b)] + extra)
        blob = a.read_bytes()
        assert len(blob) == L.fm_index_bytes(len(raw), int(sample or 32), 32) and b.read_bytes() == blob
