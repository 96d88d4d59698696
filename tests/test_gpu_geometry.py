"""GPU (-m gpu): the sweeps of test_emul_geometry.py on the MI355X -- sizes and `primary` on the edges of the kernels' geometry.

What the emulation cannot see is here: barriers, LDS atomics, the unaligned 16-byte loads of fm_code_word and partially filled last
workgroups.  Every FM blob is byte-equal to fm_reference.encode; the device entry points write into buffers preset to 0xA5, so that
a byte the build leaves unwritten shows; queries go through the host and the device forms; the inverse BWT runs on a workspace
preset to 0xA5; bwt_device reads and writes through pointers of every alignment.  8 Mi +- 1 rows (512 tiles) cover the tile-prefix
scan.  One process; every input is valid."""
import numpy as np
import pytest

import fm_reference as R
from test_emul_geometry import (LARGE, MILLION, NOT_FOUND, SMALL, blobs_with_samples, blobs_without_samples, bwt_round_trip, bwt_sweep,
                                chosen_primaries, family_case, queries, slice_list)

pytestmark = pytest.mark.gpu
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
FILL = 0xA5
GUARD = 64


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


def _dev(torch, a):
    """numpy array (unsigned included) -> device tensor of the same bytes"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(a).cuda()


class DeviceForm:
    """The calls the sweeps make on a CapsLib, through the *_device entry points: every output buffer preset to 0xA5 with a guard
    behind it that must keep that value."""

    def __init__(self, L):
        import torch
        self.L, self.torch = L, torch
        self._kept = (None, None)
        self.build_bwt = L.build_bwt
        self.fm_index_bytes = L.fm_index_bytes

    def _filled(self, nbytes):
        return self.torch.full((nbytes + GUARD,), FILL, dtype=self.torch.uint8, device="cuda")

    def _back(self, buf, nbytes):
        out = buf.cpu().numpy()
        assert (out[nbytes:] == FILL).all(), "bytes behind the output were written"
        return out[:nbytes].copy()

    def fm_build(self, B, primary, SA=None, s=32, bits=32):
        torch = self.torch
        n = int(B.size)
        dB = _dev(torch, B)
        dSA = None if SA is None else _dev(torch, np.asarray(SA).astype(np.uint32 if bits == 32 else np.uint64))
        nbytes = self.L.fm_index_bytes(n, s if SA is not None else 0, bits)
        index = self._filled(nbytes)
        torch.cuda.synchronize()
        self.L.fm_build_device(dB.data_ptr(), n, primary, 0 if dSA is None else dSA.data_ptr(), s, index.data_ptr(), nbytes, idx_bits=bits)
        blob = self._back(index, nbytes)
        self._kept = (blob, index)
        return blob

    def _index(self, blob):
        if self._kept[0] is blob:
            return self._kept[1]
        index = self.torch.from_numpy(blob).cuda()
        self._kept = (blob, index)
        return index

    def fm_count(self, blob, patterns):
        torch = self.torch
        cat, off = self.L._patterns(patterns)
        q = off.size - 1
        d_cat = _dev(torch, cat if cat.size else np.zeros(1, dtype=np.uint8))
        d_off = _dev(torch, off)
        out = self._filled(16 * q)
        index = self._index(blob)
        torch.cuda.synchronize()
        self.L.fm_count_device(index.data_ptr(), blob.size, d_cat.data_ptr(), d_off.data_ptr(), q, out.data_ptr(), out.data_ptr() + 8 * q)
        both = self._back(out, 16 * q).view(np.uint64)
        return both[:q].copy(), both[q:].copy()

    def fm_locate(self, blob, first, count, out_off=None):
        torch = self.torch
        first = np.ascontiguousarray(first, dtype=np.uint64)
        count = np.ascontiguousarray(count, dtype=np.uint64)
        q = first.size
        if out_off is None:
            out_off = np.zeros(q + 1, dtype=np.uint64)
            out_off[1:] = np.cumsum(count, dtype=np.uint64)
        total = int(out_off[-1])
        # every slot is written when count[j] >= its share of the offsets, as in every call of the sweeps
        assert (np.diff(out_off.astype(np.int64)) <= count.astype(np.int64)).all()
        pos = self._filled(8 * total)
        index = self._index(blob)
        d_first, d_count, d_off = _dev(torch, first), _dev(torch, count), _dev(torch, out_off)
        torch.cuda.synchronize()
        self.L.fm_locate_device(index.data_ptr(), blob.size, d_first.data_ptr(), d_count.data_ptr(), d_off.data_ptr(), q, pos.data_ptr())
        return self._back(pos, 8 * total).view(np.uint64), out_off

    def inverse_bwt(self, B, primary, idx_bits=32):
        torch = self.torch
        n = int(B.size)
        ws_bytes = self.L.inverse_bwt_workspace_bytes(n, idx_bits)
        dB = _dev(torch, B)
        ws = self._filled(ws_bytes)
        out = self._filled(n)
        torch.cuda.synchronize()
        self.L.inverse_bwt_device(dB.data_ptr(), n, primary, out.data_ptr(), ws.data_ptr(), ws_bytes, idx_bits=idx_bits)
        assert bool((ws[ws_bytes:] == FILL).all()), "bytes behind the workspace were written"
        return self._back(out, n)


# ---- FM blobs ------------------------------------------------------------------------------------------------------------------

def test_blob_bytes_without_samples_host_form(L):
    assert blobs_without_samples(L) >= 5000


def test_blob_bytes_with_samples_host_form(L):
    assert blobs_with_samples(L, SMALL) + blobs_with_samples(L, LARGE) >= 400


def test_blob_bytes_device_form(L):
    """fm_build_device over EDGE_SIZES x the chosen primaries x {no samples, s = 32} x both widths, into 0xA5-filled buffers."""
    D = DeviceForm(L)
    done = 0
    for n in R.EDGE_SIZES:
        for j in chosen_primaries(n):
            T, SA, B, primary = family_case(L, n, j)
            for sa, s in ((None, 0), (SA, 32)):
                for bits in (32, 64):
                    blob = D.fm_build(B, primary, sa, s, bits)
                    want = R.encode(B, primary, sa, s, bits // 8)
                    assert blob.size == want.size, (n, j, s, bits)
                    assert np.array_equal(blob, want), (n, j, s, bits, np.flatnonzero(blob != want)[:8])
                    done += 1
    assert done >= 4 * len(R.EDGE_SIZES) * 2


def test_queries_host_form(L):
    ranks, fitted = queries(L, SMALL)
    assert ranks >= 400 and fitted >= 300, (ranks, fitted)
    ranks, fitted = queries(L, LARGE)
    assert ranks >= 10_000 and fitted >= 9000, (ranks, fitted)


def test_queries_device_form(L):
    D = DeviceForm(L)
    ranks, fitted = queries(D, SMALL, samples=(1, 32, 1024))
    assert ranks >= 400 and fitted >= 300, (ranks, fitted)
    ranks, fitted = queries(D, LARGE, samples=(1, 32, 1024))
    assert ranks >= 10_000 and fitted >= 9000, (ranks, fitted)


@pytest.mark.parametrize("n", [(8 << 20) - 1, 8 << 20, (8 << 20) + 1])
def test_blob_over_512_tiles(L, n):
    """Random DNA around 8 Mi rows: the SA from build_device, accepted by verify_device; bwt_device; fm_build_device with s = 32 at
    both widths against the encoder -- many workgroups, the scan over the tile counts, a last tile of 1 or 2 rows or a full one."""
    import torch
    rs = np.random.RandomState(n % 1000)
    T = rs.choice(DNA, size=n)
    dT = _dev(torch, T)
    dSA = torch.empty(n, dtype=torch.int32, device="cuda")
    dLCP = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.build_device(dT.data_ptr(), n, dSA.data_ptr(), dLCP.data_ptr())
    assert L.verify_device(dT.data_ptr(), n, dSA.data_ptr(), dLCP.data_ptr()) == 0
    dB = torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    primary = L.bwt_device(dT.data_ptr(), n, dSA.data_ptr(), 0, n, dB.data_ptr())
    SA = dSA.cpu().numpy().view(np.uint32)
    B = dB.cpu().numpy()
    assert (B[n:] == FILL).all()
    B = B[:n].copy()
    B2, p2 = R.bwt_of(T, SA)
    assert np.array_equal(B, B2) and primary == p2
    for bits in (32, 64):
        d_sa = dSA if bits == 32 else _dev(torch, SA.astype(np.uint64))
        nbytes = L.fm_index_bytes(n, 32, bits)
        index = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        L.fm_build_device(dB.data_ptr(), n, primary, d_sa.data_ptr(), 32, index.data_ptr(), nbytes, idx_bits=bits)
        blob = index.cpu().numpy()
        assert (blob[nbytes:] == FILL).all()
        want = R.encode(B, primary, SA, 32, bits // 8)
        assert want.size == nbytes and np.array_equal(blob[:nbytes], want), (n, bits, np.flatnonzero(blob[:nbytes] != want)[:8])


# ---- BWT and inverse BWT -------------------------------------------------------------------------------------------------------

def test_bwt_and_inverse_host_form(L):
    assert bwt_sweep(L, SMALL) >= 4 * len(SMALL) + 100
    assert bwt_sweep(L, LARGE) >= 4 * len(LARGE) + 50


def test_bwt_and_inverse_device_form(L):
    D = DeviceForm(L)
    assert bwt_sweep(D, SMALL) >= 4 * len(SMALL) + 100
    assert bwt_sweep(D, LARGE) >= 4 * len(LARGE) + 50


@pytest.mark.parametrize("n", MILLION)
def test_bwt_and_inverse_at_the_second_ranking_level(L, n):
    T = np.random.RandomState(n).choice(DNA, size=n)
    bwt_round_trip(L, T)
    bwt_round_trip(DeviceForm(L), T)


def test_bwt_device_with_unaligned_pointers(L):
    """The SA pointer `first` entries into the array (first = 0 .. 16), the output pointer 0 .. 3 bytes off a 16-byte boundary,
    cnt = 0 .. 33 and three lengths around 4,096, plus the slices around primary: the numpy gather, and the bytes before and
    behind the output slice keep their preset value."""
    import torch
    rs = np.random.RandomState(51)
    T = rs.choice(DNA, size=20_000)
    n = T.size
    dT = _dev(torch, T)
    lead = 16
    for bits in (32, 64):
        SA = L.build(T, idx_bits=bits)[0]
        S = SA.astype(np.int64)
        want = T[(S + n - 1) % n]
        primary = int(np.flatnonzero(S == 0)[0])
        assert 17 < primary < n - 2
        dSA = _dev(torch, SA)
        cases = [(f, c, o) for f in range(17) for c in list(range(34)) + [4095, 4096, 4097] for o in range(4)]
        cases += [(f, c, o) for f, c in slice_list(primary, n)[17 * 34:] for o in range(4)]
        assert len(cases) == 17 * 37 * 4 + 9 * 4
        buf = torch.empty(lead + 4 + 4097 + GUARD, dtype=torch.uint8, device="cuda")
        for first, cnt, o in cases:
            buf.fill_(FILL)
            torch.cuda.synchronize()
            p = L.bwt_device(dT.data_ptr(), n, dSA.data_ptr() + first * (bits // 8), first, cnt, buf.data_ptr() + lead + o, idx_bits=bits)
            out = buf.cpu().numpy()
            a = lead + o
            assert np.array_equal(out[a:a + cnt], want[first:first + cnt]), (bits, first, cnt, o)
            assert (out[:a] == FILL).all() and (out[a + cnt:] == FILL).all(), (bits, first, cnt, o)
            assert p == (primary if first <= primary < first + cnt else NOT_FOUND), (bits, first, cnt, o, p)
