"""GPU (-m gpu): format version 2 of the FM-index and extract on the MI355X (caps_sa_hip_fm_add_text_samples_*,
caps_sa_hip_fm_extract_*).

The sweeps of test_emul_fm_extract.py through the *_device entry points.  What the emulation cannot see is here: neighbouring lanes,
waves and workgroups own neighbouring bytes of dText, so the output always starts at an odd offset of a buffer preset to 0xA5 with a
64-byte guard behind it, neighbouring queries share 4-byte words and 64-byte lines, and every byte outside the ranges must still be
0xA5 afterwards; index and workspace are preset and guarded in the same way.  Every comparison is exact; the truth is the text.
One process; every input is one the contract defines or refuses on the host."""
import os
import subprocess

import numpy as np
import pytest

import fm_extract_reference as X
import fm_reference as R
from test_emul_fm_extract import few_primaries, odd_ranges, sweep

pytestmark = pytest.mark.gpu
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
GUARD = 64
BASE = 3                       # the odd offset at which every device-form output starts
EINVAL, EUNSUPPORTED = -1, -2


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
    """The upgrade and extract through the *_device entry points on preset, guarded buffers; everything else is the library's."""

    def __init__(self, L):
        import torch
        self.L, self.torch = L, torch
        for name in ("build_bwt", "fm_build", "fm_build_from_bwt", "fm_index_bytes_ex", "fm_count", "fm_locate", "inverse_bwt",
                     "fm_extract_workspace_bytes"):
            setattr(self, name, getattr(L, name))

    def _filled(self, nbytes):
        return self.torch.full((nbytes + GUARD,), FILL, dtype=self.torch.uint8, device="cuda")

    def fm_add_text_samples(self, blob, t):
        torch = self.torch
        h = blob[:256].view(np.uint64)
        need = self.L.fm_index_bytes_ex(int(h[2]), int(h[12]), t, 8 * int(h[4]))
        cap = max(need, blob.size)
        index = self._filled(cap)
        index[:blob.size] = torch.from_numpy(blob).cuda()
        torch.cuda.synchronize()
        self.L.fm_add_text_samples_device(index.data_ptr(), cap, t)
        out = index.cpu().numpy()
        assert (out[cap:] == FILL).all(), "bytes behind the index were written"
        if cap > need and cap > blob.size:
            assert (out[max(need, blob.size):cap] == FILL).all()
        return out[:need].copy()

    def extract_raw(self, blob, starts, off, workspace=True):
        """-> the whole text buffer (np.uint8, off[-1] + GUARD bytes) after fm_extract_device."""
        torch = self.torch
        q = starts.size
        total = int(off[-1])
        index = self._filled(blob.size)
        index[:blob.size] = torch.from_numpy(blob).cuda()
        text = self._filled(total)
        ws_bytes = self.L.fm_extract_workspace_bytes(q)
        ws = self._filled(ws_bytes)
        d_s, d_o = _dev(torch, starts), _dev(torch, off)
        torch.cuda.synchronize()
        self.L.fm_extract_device(index.data_ptr(), blob.size, d_s.data_ptr(), d_o.data_ptr(), q, text.data_ptr(),
                                 ws.data_ptr() if workspace else 0, ws_bytes if workspace else 0)
        assert bool((ws[ws_bytes:] == FILL).all()), "bytes behind the workspace were written"
        assert bool((index[blob.size:] == FILL).all()) and np.array_equal(index[:blob.size].cpu().numpy(), blob), "the index was written"
        return text.cpu().numpy()

    def fm_extract(self, blob, starts, lengths):
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        off = np.full(starts.size + 1, BASE, dtype=np.uint64)
        off[1:] += np.cumsum(np.asarray(lengths, dtype=np.uint64), dtype=np.uint64)
        out = self.extract_raw(blob, starts, off)
        total = int(off[-1])
        assert (out[:BASE] == FILL).all() and (out[total:] == FILL).all(), "bytes outside every range were written"
        return out[BASE:total].copy(), off - np.uint64(BASE)


@pytest.fixture(scope="module")
def D(L):
    return DeviceForm(L)


def device_sizes(t):
    return sorted(set(X.chunk_edge_sizes(t)) | {1, 2, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097})


@pytest.mark.parametrize("s,t", X.DISTANCES)
def test_blob_bytes_and_extract_device_form(D, s, t):
    """The sweep of test_emul_fm_extract.py on the kernels' and the chunks' edge sizes, three primaries each, both widths."""
    assert sweep(D, device_sizes, distances=((s, t),), primaries=few_primaries) >= 60


def test_blob_bytes_and_extract_device_form_large(D):
    assert sweep(D, lambda t: [16_383, 16_384, 16_385, 32_768], distances=((1, 1), (32, 64)), queries=False) == 4 * 3 * 2 * 2


def test_host_forms(L):
    """The same sweep through the host forms on a subset of the shapes: the upgrade rewrites the caller's blob and leaves the device
    copy equal to it (extract right after it, without an upload in between, answers from the new section)."""
    assert sweep(L, lambda t: [129, 4097, 16_385], distances=((32, 64), (1, 1024)), primaries=few_primaries) == 3 * 3 * 2 * 2
    T = np.random.RandomState(4).choice(DNA, size=300_001)
    SA, _, B, primary, _ = L.build_bwt(T)
    for bits in (32, 64):
        v1 = L.fm_build(B, primary, SA, 32, bits)
        buf = np.zeros(L.fm_index_bytes_ex(T.size, 32, 64, bits), dtype=np.uint8)
        buf[:v1.size] = v1
        f1, c1 = L.fm_count(buf[:v1.size], [T[5:25].tobytes()])                      # (the version-1 blob is resident now)
        assert L._f("fm_add_text_samples")(buf.ctypes.data, buf.size, 64, 0) == 0
        text, _ = L.fm_extract(buf, [0, 299_000, 150_000], [300, 1001, 5000])
        assert np.array_equal(text, np.concatenate([T[:300], T[299_000:], T[150_000:155_000]])), bits
        f2, c2 = L.fm_count(buf, [T[5:25].tobytes()])
        assert (f1, c1) == (f2, c2) and np.array_equal(buf, X.add_text_samples(R.encode(B, primary, SA, 32, bits // 8), SA, 64))


def test_neighbouring_queries_share_words_and_lines(D):
    """Ranges of 0 .. 11 bytes back to back from an odd offset: every 4-byte word and 64-byte line of the output is shared by several
    lanes.  A word store over a neighbour's bytes shows as a wrong byte or as a byte outside the ranges that is no longer 0xA5."""
    T = np.random.RandomState(3).choice(DNA, size=100_003)
    SA, _, B, primary, _ = D.build_bwt(T)
    for s, t, bits in ((1, 1, 32), (32, 32, 32), (32, 64, 32), (32, 64, 64), (32, 1024, 64)):
        v2 = D.L.fm_add_text_samples(D.L.fm_build(B, primary, SA, s, bits), t)
        for base, count, longest in ((1, 5000, 11), (3, 5000, 3), (61, 3000, 200), (2, 300, 3000)):
            rg = odd_ranges(T.size, np.random.RandomState(base + t), count, longest)
            starts, off = X.pack(rg)
            off = off + np.uint64(base)
            for ws in (True, False):
                out = D.extract_raw(v2, starts, off, ws)
                total = int(off[-1])
                assert (out[:base] == FILL).all() and (out[total:] == FILL).all(), (s, t, bits, base)
                want = X.expected(T, rg)
                assert np.array_equal(out[base:total], want), (s, t, bits, base, np.flatnonzero(out[base:total] != want)[:8])


@pytest.mark.parametrize("n", [(8 << 20) - 1, 8 << 20, (8 << 20) + 1])
def test_8_mi_rows(L, n):
    """8 Mi +- 1 rows, both widths, s = 32, t = 32, 64, 1024: 2^16 + 1 random ranges of 1 .. 300 bytes and extract(0, n), compared on
    the device with the text; the last workgroup of every kernel is partly filled."""
    import torch
    dev = torch.device("cuda")
    T = np.random.RandomState(n % 1000).choice(DNA, size=n)
    dT = _dev(torch, T)
    dSA = torch.empty(n, dtype=torch.int32, device=dev)
    dLCP = torch.empty(n, dtype=torch.int32, device=dev)
    dB = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    L.build_device(dT.data_ptr(), n, dSA.data_ptr(), dLCP.data_ptr())
    primary = L.bwt_device(dT.data_ptr(), n, dSA.data_ptr(), 0, n, dB.data_ptr())
    del dLCP
    dSA64 = dSA.to(torch.int64) & 0xFFFFFFFF
    q = (1 << 16) + 1
    g = torch.Generator(device="cuda")
    g.manual_seed(n)
    lengths = torch.randint(1, 301, (q,), device=dev, generator=g)
    starts = (torch.rand(q, device=dev, generator=g, dtype=torch.float64) * (n - lengths + 1).to(torch.float64)).to(torch.int64)
    starts[0], lengths[0] = n - 300, 300                     # (a range that ends at the text's end: its last chunk starts at row 0)
    off = torch.full((q + 1,), BASE, dtype=torch.int64, device=dev)
    off[1:] += torch.cumsum(lengths, 0)
    total = int(off[-1])
    where = torch.repeat_interleave(starts - off[:-1], lengths) + torch.arange(BASE, total, device=dev)
    want = dT[where]
    ws_bytes = L.fm_extract_workspace_bytes(q)
    one_s = torch.zeros(1, dtype=torch.int64, device=dev)
    one_o = torch.tensor([BASE, BASE + n], dtype=torch.int64, device=dev)
    for bits in (32, 64):
        for t in (32, 64, 1024):
            cap = L.fm_index_bytes_ex(n, 32, t, bits)
            index = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device=dev)
            ws = torch.full((ws_bytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
            text = torch.full((total + GUARD,), FILL, dtype=torch.uint8, device=dev)
            whole = torch.full((BASE + n + GUARD,), FILL, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            L.fm_build_device(dB.data_ptr(), n, primary, (dSA if bits == 32 else dSA64).data_ptr(), 32, index.data_ptr(), cap, idx_bits=bits)
            L.fm_add_text_samples_device(index.data_ptr(), cap, t)
            L.fm_extract_device(index.data_ptr(), cap, starts.data_ptr(), off.data_ptr(), q, text.data_ptr(), ws.data_ptr(), ws_bytes)
            L.fm_extract_device(index.data_ptr(), cap, one_s.data_ptr(), one_o.data_ptr(), 1, whole.data_ptr(), ws.data_ptr(), ws_bytes)
            what = (n, bits, t)
            assert bool((index[cap:] == FILL).all()) and bool((ws[ws_bytes:] == FILL).all()), what
            assert bool((text[:BASE] == FILL).all()) and bool((text[total:] == FILL).all()), what
            assert bool((whole[:BASE] == FILL).all()) and bool((whole[BASE + n:] == FILL).all()), what
            assert torch.equal(text[BASE:total], want), (what, torch.nonzero(text[BASE:total] != want)[:8].flatten().tolist())
            assert torch.equal(whole[BASE:BASE + n], dT), what
            m = (n - 1) // t + 1                                        # rowof against the SA's inverse, on the device
            rowof = index[cap - ((m * (bits // 8) + 63) // 64 * 64):cap].view(torch.int32 if bits == 32 else torch.int64)[:m]
            inverse = torch.empty(n, dtype=torch.int64, device=dev)
            inverse[dSA64] = torch.arange(1, n + 1, dtype=torch.int64, device=dev)
            assert torch.equal(rowof.to(torch.int64) & 0xFFFFFFFF, inverse[::t]), what
            del index, ws, text, whole, inverse


def test_header_refusals_on_the_device_entry_points(L, D):
    """Host-side checks only (the body stays a valid index): an unknown version, the section's header words off by one, a short
    index_bytes, a version-1 blob; a valid call afterwards on the same buffers."""
    import caps_sa_amd
    import torch
    T = np.random.RandomState(6).choice(DNA, size=200_000)
    SA, _, B, primary, _ = L.build_bwt(T)
    v1 = L.fm_build(B, primary, SA, 32)
    v2 = L.fm_add_text_samples(v1, 64)
    starts, off = X.pack([(0, 10), (199_990, 10), (77, 0), (1234, 567)])
    off = off + np.uint64(BASE)
    d_s, d_o = _dev(torch, starts), _dev(torch, off)
    text = torch.full((int(off[-1]) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    index = torch.full((v2.size + GUARD,), FILL, dtype=torch.uint8, device="cuda")

    def call(blob, nbytes=None):
        index[:blob.size] = torch.from_numpy(blob).cuda()
        torch.cuda.synchronize()
        L.fm_extract_device(index.data_ptr(), blob.size if nbytes is None else nbytes, d_s.data_ptr(), d_o.data_ptr(), 4, text.data_ptr())

    def refused(blob, code, word, nbytes=None):
        with pytest.raises(caps_sa_amd.CapsSaError) as e:
            call(blob, nbytes)
        assert e.value.code == code and word in str(e.value), str(e.value)
        assert bool((text == FILL).all())

    for version in (0, 3, 9):
        bad = v2.copy()
        bad[:256].view(np.uint64)[1] = version
        refused(bad, EINVAL, "format version")
    for word in (19, 20, 21, 22):
        for d in (1, -1):
            bad = v2.copy()
            bad[:256].view(np.uint64)[word] = int(v2[:256].view(np.uint64)[word]) + d
            refused(bad, EINVAL, "FM-index header")
            with pytest.raises(caps_sa_amd.CapsSaError):
                L.fm_add_text_samples_device(index.data_ptr(), v2.size, 64)
    refused(v2, EINVAL, "truncated", v2.size - 1)
    refused(v2, EINVAL, "smaller than an FM-index header", 255)
    refused(v1, EUNSUPPORTED, "format version 1")
    for t in (16, 48, 2048):
        with pytest.raises(caps_sa_amd.CapsSaError) as e:
            L.fm_add_text_samples_device(index.data_ptr(), v2.size, t)
        assert e.value.code == EINVAL
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        L.fm_add_text_samples_device(index.data_ptr(), v2.size - 1, 64)           # (the version-1 blob is in the buffer: one byte short)
    assert e.value.code == EINVAL and "index_bytes too small" in str(e.value)
    assert np.array_equal(index[:v1.size].cpu().numpy(), v1)
    L.fm_add_text_samples_device(index.data_ptr(), v2.size, 64)
    assert np.array_equal(index.cpu().numpy()[:v2.size], v2) and bool((index[v2.size:] == FILL).all())
    call(v2)
    out = text.cpu().numpy()
    total = int(off[-1])
    assert (out[:BASE] == FILL).all() and (out[total:] == FILL).all()
    assert np.array_equal(out[BASE:total], np.concatenate([T[0:10], T[199_990:200_000], T[1234:1801]]))


def test_python_surface(L):
    """caps_sa_amd.FMIndex: with_text_samples, text_sample, extract, save / load of a version-2 blob."""
    import caps_sa_amd
    T = np.random.RandomState(8).choice(DNA, size=50_001)
    SA, _, B, primary, _ = L.build_bwt(T)
    fm1 = caps_sa_amd.FMIndex.from_bwt(B, primary, SA, 32)
    assert fm1.text_sample == 0
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        fm1.extract([0], [1])
    assert e.value.code == EUNSUPPORTED
    fm = fm1.with_text_samples()
    assert fm.text_sample == 32 and fm.nbytes == L.fm_index_bytes_ex(T.size, 32, 32, 32) > fm1.nbytes and fm1.text_sample == 0
    tb = T.tobytes()
    assert fm.extract([0, 50_000, 123, 7], [5, 1, 1000, 0]) == [tb[0:5], tb[50_000:], tb[123:1123], b""]
    assert fm.extract([], []) == []
    assert fm.locate([tb[100:140]])[0].tolist() == fm1.locate([tb[100:140]])[0].tolist()
    assert fm.with_text_samples(256).extract([0], [T.size]) == [tb]


def test_cli_round_trip(L, tmp_path):
    """caps_sa in.fa out.bin --fm-index x.fm --fm-text-sample 64, then --fm-extract x.fm ranges.txt against the remapped text;
    --fm-from-bwt x.bwt y.fm --fm-text-sample 64 gives the same file."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    exe = os.path.join(ROOT, "caps-sa_amd", "caps_sa")
    rs = np.random.RandomState(9)
    raw = b"\n".join([b">chr1 test"] + [bytes(rs.choice(list(b"ACGTNacgt"), size=60).tolist()) for _ in range(2000)]) + b"\n"
    inp, out, bwt, a, b, rg = (tmp_path / x for x in ("in.fa", "out.bin", "x.bwt", "x.fm", "y.fm", "ranges.txt"))
    inp.write_bytes(raw)
    subprocess.check_call([exe, str(inp), str(out), "--bwt", str(bwt), "--fm-index", str(a), "--fm-text-sample", "64"])
    subprocess.check_call([exe, "--fm-from-bwt", str(bwt), str(b), "--fm-text-sample", "64"])
    blob = a.read_bytes()
    n = len(raw)
    assert len(blob) == L.fm_index_bytes_ex(n, 32, 64, 32) and b.read_bytes() == blob
    assert int(np.frombuffer(blob[:256], dtype=np.uint64)[1]) == 2 and int(np.frombuffer(blob[:256], dtype=np.uint64)[19]) == 64
    remapped = np.frombuffer(b"ACTG", dtype=np.uint8)[(np.frombuffer(raw, dtype=np.uint8) & 0x6) >> 1].tobytes().decode()
    ranges = [(0, 10), (n - 1, 1), (n, 0), (63, 130), (5000, 0), (0, n)] + [(int(rs.randint(0, n - 200)), int(rs.randint(0, 200))) for _ in range(50)]
    rg.write_text("".join(f"{x} {ln}\n" for x, ln in ranges))
    r = subprocess.run([exe, "--fm-extract", str(a), str(rg)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "".join(remapped[x:x + ln] + "\n" for x, ln in ranges)
    # a version-1 file is refused, with the way out
    subprocess.check_call([exe, "--fm-from-bwt", str(bwt), str(b)])
    r = subprocess.run([exe, "--fm-extract", str(b), str(rg)], capture_output=True, text=True)
    assert r.returncode != 0 and "--fm-text-sample" in r.stderr and r.stdout == ""
