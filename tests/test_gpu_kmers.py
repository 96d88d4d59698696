"""GPU (-m gpu): k-mer tables, spectra and the census from SA and LCP on the MI355X (caps_sa_hip_kmers_*, caps_sa_hip_kmer_spectrum_*,
caps_sa_hip_kmer_census_*).

The sweeps of test_emul_kmers.py through the host AND the device entry points, both widths: the device form always works on
buffers preset to 0xA5 with guards before and behind the records and behind the workspace.  The truth of the small cases is
kmer_reference; the text of 2^20 + 1 bases is built with build_device and checked on the device against torch.unique over the
packed k-mer codes.  Every comparison is exact.  One process; every input is one the contract defines or refuses on the host.  The
_u64 forms run at these sizes only: ranks beyond 2^32 are untested."""
import numpy as np
import pytest

import kmer_reference as R
from test_emul_kmers import (SIZES, DeviceForm, HostForm, capacity_sweep, census_sweep, check_table, filter_sweep, forms_of, refusal_sweep,
                             short_text_sweep, size_sweep)

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


class TorchMem:
    """Device memory for the sweeps' *_device calls."""

    def __init__(self):
        import torch
        self.torch = torch

    def filled(self, nbytes):
        return self.torch.full((nbytes,), FILL, dtype=self.torch.uint8, device="cuda")

    def put(self, a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return self.torch.from_numpy(a.copy() if a.size else np.zeros(8, dtype=np.uint8)).cuda()

    def ptr(self, buf):
        self.torch.cuda.synchronize()
        return buf.data_ptr()

    def get(self, buf):
        return buf.cpu().numpy()


@pytest.fixture(scope="module")
def mem(L):
    return TorchMem()


@pytest.mark.parametrize("sizes", [tuple(SIZES[:6]), (16383, 16384, 16385), (32767, 32768, 32769), (49153,)])
def test_sizes_texts_and_ks(L, mem, sizes):
    assert size_sweep(forms_of(L, mem), sizes) == len(sizes) * 3 * 4


def test_short_texts(L, mem):
    assert short_text_sweep(forms_of(L, mem), max_len=4, widths=(32,)) == 2 * sum(3 ** n for n in range(1, 5))


def test_census_and_bins(L, mem):
    census_sweep(forms_of(L, mem))


def test_count_filters(L, mem):
    filter_sweep(forms_of(L, mem), n=6000)


def test_counting_call_writing_call_and_capacity(L, mem):
    capacity_sweep(L, mem)


def test_refusals_and_the_empty_text(L, mem):
    refusal_sweep(L, mem)


def test_a_built_text_against_torch_unique(L):
    """2^20 + 1 random bases, build_device, everything stays on the device: the table at k = 8 and 12 against torch.unique over the
    packed codes (for ACGT integer order is the table's order), the spectrum against the counts' bincount, the census against the
    table's sizes."""
    import torch
    import caps_sa_amd
    n = (1 << 20) + 1
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    code = torch.randint(0, 4, (n,), device="cuda", generator=g)
    T = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[code]
    SA = torch.empty(n, dtype=torch.int32, device="cuda")
    LCP = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr())
    distinct, unique = L.kmer_census_device(SA.data_ptr(), LCP.data_ptr(), n, 16)
    for k in (8, 12):
        packed = torch.zeros(n - k + 1, dtype=torch.int64, device="cuda")
        for j in range(k):
            packed = packed * 4 + code[j:n - k + 1 + j]
        vals, counts = torch.unique(packed, return_counts=True)
        found = L.kmers_device(SA.data_ptr(), LCP.data_ptr(), n, k)
        assert found == vals.numel() == int(distinct[k])
        rec = torch.full((found + 1, 3), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert L.kmers_device(SA.data_ptr(), LCP.data_ptr(), n, k, dRecords_ptr=rec.data_ptr(), capacity=found) == found
        assert bool((rec[found] == -1).all())
        first, count, pos = rec[:found, 0], rec[:found, 1], rec[:found, 2]
        assert torch.equal(packed[pos], vals) and torch.equal(count, counts)
        assert torch.equal(SA[first].to(torch.int64), pos)
        assert bool((first[1:] >= first[:-1] + count[:-1]).all()) and int(first[-1] + count[-1]) <= n
        hist = L.kmer_spectrum_device(SA.data_ptr(), LCP.data_ptr(), n, k, 1024)
        want = torch.bincount(counts.clamp(max=1024), minlength=1025).cpu().numpy().astype(np.uint64)
        assert np.array_equal(hist, want) and int(unique[k]) == int(want[1])
        two = L.kmers_device(SA.data_ptr(), LCP.data_ptr(), n, k, 2, 0)
        assert two == int((counts >= 2).sum())
    assert rec.numel() and caps_sa_amd.KMER_DTYPE.itemsize == 24


def test_python_methods_on_a_constructed_suffix_array(L):
    import caps_sa_amd
    rs = np.random.RandomState(8)
    T = rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=20011).astype(np.uint8)
    T[5000:9000] = T[100:4100]
    s = caps_sa_amd.SuffixArray(T)
    with pytest.raises(RuntimeError):
        s.kmers(5)                                            # construct() has not been called
    s.construct()
    SA = s.SA().astype(np.int64)
    for k in (5, 31):
        check_table(T, SA, s.kmers(k), R.table(T, k), k)
        assert np.array_equal(s.kmer_spectrum(k, 16), R.spectrum(T, k, 16))
    check_table(T, SA, s.kmers(11, min_count=2, max_count=2), R.table(T, 11, 2, 2), 11)
    d, u = s.kmer_census(12)
    want = R.census_by_counter(T, 12)
    assert np.array_equal(d, want[0]) and np.array_equal(u, want[1])
    assert np.array_equal(caps_sa_amd.kmer_spectrum(s.SA(), s.LCP(), 5), s.kmer_spectrum(5))
    assert np.array_equal(caps_sa_amd.kmers(s.SA(), s.LCP(), 5, min_count=3), s.kmers(5, min_count=3))
    assert np.array_equal(caps_sa_amd.kmer_census(s.SA(), s.LCP(), 9)[0], d[:10])
    b = caps_sa_amd.SuffixArray(T, max_context=16)
    b.construct()
    for call in (lambda: b.kmers(5), lambda: b.kmer_spectrum(5), lambda: b.kmer_census(5)):
        with pytest.raises(ValueError):
            call()
