"""GPU (-m gpu): the inverse suffix array, range minima over LCP and longest common extensions on the MI355X (caps_sa_hip_isa_*,
caps_sa_hip_lce_*).

The sweeps of test_emul_lce.py through the host AND the device entry points, both widths: the device form always works on buffers
preset to 0xA5 with guards before and behind them, the index 80 bytes into its buffer.  The truth is lce_reference (brute force on the
text, the array rules, a numpy sparse table, the encoder of the blob).  The text of 2^20 + 1 bases is built with build_device and
indexed on the device.  One process; every input is one the contract defines or refuses on the host.  The _u64 forms run at these
sizes only: ranks beyond 2^32 are untested."""
import numpy as np
import pytest

import lce_reference as R
from test_emul_lce import (SIZES, DeviceForm, HostForm, arbitrary_sweep, forms_of, garbage_lcp_sweep, header_sweep, isa_sweep, planted_sweep, refusal_sweep,
                           short_text_sweep, size_sweep)
from test_gpu_kmers import TorchMem

pytestmark = pytest.mark.gpu
N = (1 << 20) + 1
Q = 1 << 16


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


@pytest.fixture(scope="module")
def mem(L):
    return TorchMem()


@pytest.mark.parametrize("sizes", [tuple(SIZES[:11]), tuple(SIZES[11:17]), tuple(SIZES[17:21]), tuple(SIZES[21:])])
def test_sizes_and_texts(L, mem, sizes):
    assert size_sweep(forms_of(L, mem), sizes) == len(sizes) * 4 * 4


def test_short_texts(L, mem):
    assert short_text_sweep(forms_of(L, mem), max_len=4) == sum(3 ** n for n in range(1, 5))


def test_range_min_of_every_block_pair_and_tier(L, mem):
    assert arbitrary_sweep(forms_of(L, mem)) > 290000


def test_a_planted_minimum_is_seen_inside_and_not_outside(L, mem):
    assert planted_sweep(forms_of(L, mem)) > 60


def test_isa_of_six_permutations(L, mem):
    assert isa_sweep(forms_of(L, mem))


def test_garbage_lcp_terminates_in_range(L, mem):
    garbage_lcp_sweep(forms_of(L, mem))


def test_refusals_the_empty_text_and_values_that_are_no_positions(L, mem):
    refusal_sweep(L, mem)


def test_every_damaged_header_word_is_refused(L, mem):
    header_sweep(L, mem)


def _index_on_device(torch, L, SA, LCP):
    """The index of two resident int32 arrays -> the blob on the device; a guard behind it must stay."""
    n = SA.numel()
    need = L.lce_index_bytes(n, 32)
    blob = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.lce_build_device(SA.data_ptr(), LCP.data_ptr(), n, blob.data_ptr(), need)
    assert bool((blob[need:] == 0xA5).all())
    return blob[:need]


def _ask(torch, call, blob, a, b, *extra):
    da, db = torch.from_numpy(a.astype(np.int64)).cuda(), torch.from_numpy(b.astype(np.int64)).cuda()
    out = torch.full((a.size + 1,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    call(blob.data_ptr(), blob.numel(), da.data_ptr(), db.data_ptr(), a.size, *extra, out.data_ptr())
    assert int(out[a.size]) == -7
    return out[:a.size].cpu().numpy().view(np.uint64)


def test_a_built_text_against_brute_force_and_a_sparse_table(L):
    """2^20 + 1 random bases (257 superblocks, 9 top levels), build_device and lce_build_device: the blob is the encoder's, 2^16
    random pairs at k = 0 and k = 3 are the text's by brute force, 2^16 random rank pairs of range_min are a numpy sparse table's."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    T = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[torch.randint(0, 4, (N,), device="cuda", generator=g)]
    SA = torch.empty(N, dtype=torch.int32, device="cuda")
    LCP = torch.empty(N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.build_device(T.data_ptr(), N, SA.data_ptr(), LCP.data_ptr())
    blob = _index_on_device(torch, L, SA, LCP)
    sa, lcp = SA.cpu().numpy().view(np.uint32), LCP.cpu().numpy().view(np.uint32)
    assert R.layout(N, 4)["ns"] == 257 and R.layout(N, 4)["tl"] == 9
    assert np.array_equal(blob.cpu().numpy(), R.encode(sa, lcp, 4))
    rs = np.random.RandomState(5)
    t = T.cpu().numpy()
    I, J = rs.randint(0, N, size=Q), rs.randint(0, N, size=Q)
    I[:4], J[:4] = [0, N - 1, 5, N - 2], [0, N - 1, 5, N - 1]
    for k in (0, 3):
        got = _ask(torch, L.lce_device, blob, I, J, k)
        same = I == J
        assert np.array_equal(got[~same], R.lce_brute_np(t, I[~same], J[~same], k, cap=128)), k
        assert np.array_equal(got[same], (N - I[same]).astype(np.uint64))
    a, b = rs.randint(0, N, size=Q), rs.randint(0, N, size=Q)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    hi[:Q // 4] = np.minimum(lo[:Q // 4] + rs.randint(0, 9000, size=Q // 4), N - 1)      # short spans too: inside a block, a few blocks
    want = R.SparseTable(R.lcp0(lcp)).query(lo, hi)
    assert np.array_equal(_ask(torch, L.lce_range_min_device, blob, lo, hi), want)
    ISA = torch.full((N + 1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.isa_device(SA.data_ptr(), N, ISA.data_ptr())
    assert int(ISA[N]) == -7 and np.array_equal(ISA[:N].cpu().numpy()[sa.astype(np.int64)], np.arange(N, dtype=np.int32))


def test_one_letter_against_its_closed_form(L):
    """'A' * (2^20 + 1), whose arrays are SA[r] = n - 1 - r and LCP[r] = r: lce(i, j, k) = n - max(i, j) for every k."""
    import torch
    LCP = torch.arange(N, device="cuda", dtype=torch.int32)
    SA = LCP.flip(0).contiguous()
    blob = _index_on_device(torch, L, SA, LCP)
    rs = np.random.RandomState(6)
    I, J = rs.randint(0, N, size=Q), rs.randint(0, N, size=Q)
    I[:3], J[:3] = [0, N - 1, 0], [0, N - 1, N - 1]
    for k in (0, 3, 1024):
        assert np.array_equal(_ask(torch, L.lce_device, blob, I, J, k), (N - np.maximum(I, J)).astype(np.uint64))
    lo, hi = np.minimum(I, J), np.maximum(I, J)
    assert np.array_equal(_ask(torch, L.lce_range_min_device, blob, lo, hi), lo.astype(np.uint64))      # LCP[r] = r


def test_python_class_on_a_constructed_suffix_array(L, tmp_path):
    import caps_sa_amd
    rs = np.random.RandomState(8)
    T = rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=20011).astype(np.uint8)
    T[5000:9000] = T[100:4100]
    s = caps_sa_amd.SuffixArray(T)
    with pytest.raises(RuntimeError):
        s.ISA()                                               # construct() has not been called
    s.construct()
    isa = s.ISA()
    assert isa.dtype == s.SA().dtype and np.array_equal(isa[s.SA().astype(np.int64)], np.arange(T.size))
    assert np.array_equal(caps_sa_amd.isa(s.SA()), isa)
    x = caps_sa_amd.LCEIndex.from_suffix_array(s)
    assert np.array_equal(x.blob, R.encode(s.SA(), s.LCP(), 4)) and np.array_equal(x.isa(), isa) and x.n == T.size
    I, J = rs.randint(0, T.size, size=500), rs.randint(0, T.size, size=500)
    I[:2], J[:2] = [5000, 100], [100, 5001]
    far = I != J
    for k in (0, 2):
        got = x.lce(I, J, mismatches=k)
        assert np.array_equal(got[far], R.lce_brute_np(T, I[far], J[far], k, cap=256))
    assert int(x.lce([5000], [100])[0]) >= 4000
    first, count = 17, 40                                     # the string depth of an SA interval: one range minimum
    depth = int(x.range_min([first + 1], [first + count - 1])[0])
    t, sa = T.tobytes(), s.SA()
    assert depth == min(R.lce_brute(t, int(sa[r - 1]), int(sa[r])) for r in range(first + 1, first + count))
    x.save(str(tmp_path / "x.lce"))
    assert np.array_equal(caps_sa_amd.LCEIndex.load(str(tmp_path / "x.lce")).lce(I, J), x.lce(I, J))
    assert np.array_equal(caps_sa_amd.LCEIndex.from_arrays(s.SA(), s.LCP()).blob, x.blob)
    b = caps_sa_amd.SuffixArray(T, max_context=16)
    b.construct()
    with pytest.raises(ValueError):
        b.ISA()
    with pytest.raises(ValueError):
        caps_sa_amd.LCEIndex.from_suffix_array(b)
