"""GPU (-m gpu): LPF, Prev and the LZ77 factorization from SA and LCP on the MI355X (caps_sa_hip_lpf_*, caps_sa_hip_lz77_*).

The sweeps of test_emul_lz.py through the host AND the device entry points, both widths: the device form always works on buffers
preset to 0xA5 with guards before and behind the outputs and behind the workspace.  The truth is lz_reference (the array rule by
stacks, the clamped chain); the text of 2^20 + 1 bases is built with build_device, LPF, Prev and the parse are made on the device and
compared exactly with the stack reference on the host.  One process; every input is one the contract defines or refuses on the host.
The _u64 forms run at these sizes only: ranks beyond 2^32 are untested."""
import numpy as np
import pytest

import lz_reference as R
from test_emul_lz import (LPF_TILE, LZ_GROUP, LZ_TILE, SIZES, DeviceForm, HostForm, arbitrary_sweep, capacity_sweep, forms_of, group_sweep, monotone_sweep, parse_sweep,
                          refusal_sweep, short_text_sweep, size_sweep, small_buffer_sweep)
from test_gpu_kmers import TorchMem

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("sizes", [tuple(SIZES[:9]), (16383, 16384, 16385), (32767, 32768, 32769), (49153,)])
def test_sizes_and_texts(L, mem, sizes):
    assert size_sweep(forms_of(L, mem), sizes) == len(sizes) * 4 * 4


def test_short_texts(L, mem):
    assert short_text_sweep(forms_of(L, mem), max_len=4) == sum(3 ** n for n in range(1, 5))


def test_arbitrary_arrays_of_twelve_tiles(L, mem):
    assert arbitrary_sweep(forms_of(L, mem), 49153, LPF_TILE) == 24


def test_monotone_permutations_finish_because_the_search_skips(L, mem):
    """2^20 + 1 ranks: 257 tiles under two more levels; a search that walked rank by rank would make 2^39 steps."""
    monotone_sweep(DeviceForm(L, mem), (1 << 20) + 1)
    monotone_sweep(HostForm(L), 65537)


def test_parse_edges_literals_and_garbage(L, mem):
    parse_sweep(DeviceForm(L, mem), LZ_TILE)


def test_parse_over_groups_of_tiles(L, mem):
    group_sweep(DeviceForm(L, mem), LZ_GROUP, LZ_TILE)


def test_counting_call_writing_call_and_capacity(L, mem):
    capacity_sweep(L, mem)


def test_refusals_the_empty_text_and_values_that_are_no_positions(L, mem):
    refusal_sweep(L, mem)


def test_python_lz77_when_the_first_buffer_is_too_small(L):
    small_buffer_sweep(L)


def test_a_built_text_against_the_stack_reference(L):
    """2^20 + 1 bases with a planted repeat, build_device, lpf and lz77 on the device; LPF, Prev and the records against the stack
    reference over the downloaded SA and LCP, and the parse decodes to the text."""
    import torch
    import caps_sa_amd
    n = (1 << 20) + 1
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    code = torch.randint(0, 4, (n,), device="cuda", generator=g)
    code[600000:700000] = code[1000:101000]
    T = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[code]
    SA = torch.empty(n, dtype=torch.int32, device="cuda")
    LCP = torch.empty(n, dtype=torch.int32, device="cuda")
    LPF = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    Prev = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr())
    L.lpf_device(SA.data_ptr(), LCP.data_ptr(), n, LPF.data_ptr(), Prev.data_ptr())
    assert int(LPF[n]) == -7 and int(Prev[n]) == -7
    z = L.lz77_device(LPF.data_ptr(), Prev.data_ptr(), n)
    rec = torch.full((z + 1, 3), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L.lz77_device(LPF.data_ptr(), Prev.data_ptr(), n, dRecords_ptr=rec.data_ptr(), capacity=z) == z
    assert bool((rec[z] == -1).all())
    sa, lcp = SA.cpu().numpy().astype(np.uint32), LCP.cpu().numpy().astype(np.uint32)
    want_l, want_p = R.lpf_stack(sa, lcp)
    lpf, prev = LPF[:n].cpu().numpy().view(np.uint32), Prev[:n].cpu().numpy().view(np.uint32)
    assert np.array_equal(lpf, np.array(want_l, dtype=np.uint32)) and np.array_equal(prev, np.array(want_p, dtype=np.uint32))
    assert int(lpf.max()) >= 100000
    parse = R.lz_parse(want_l, want_p, n)
    assert len(parse) == z
    assert np.array_equal(rec[:z].cpu().numpy().view(np.uint64), np.array(parse, dtype=np.uint64))
    assert R.lz_decode(parse, T.cpu().numpy().tobytes()) == T.cpu().numpy().tobytes()
    assert caps_sa_amd.LZ_DTYPE.itemsize == 24


def test_python_methods_on_a_constructed_suffix_array(L):
    import caps_sa_amd
    rs = np.random.RandomState(8)
    T = rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=20011).astype(np.uint8)
    T[5000:9000] = T[100:4100]
    s = caps_sa_amd.SuffixArray(T)
    with pytest.raises(RuntimeError):
        s.lpf()                                               # construct() has not been called
    s.construct()
    want_l, want_p = R.lpf_stack(s.SA(), s.LCP())
    lpf, prev = s.lpf()
    assert lpf.tolist() == want_l and prev.tolist() == want_p
    rec = s.lz77()
    assert rec.dtype == caps_sa_amd.LZ_DTYPE and rec.tolist() == R.lz_parse(want_l, want_p, T.size)
    assert R.lz_decode(rec.tolist(), T.tobytes()) == T.tobytes()
    assert np.array_equal(caps_sa_amd.lz77(s.SA(), s.LCP()), rec)
    assert np.array_equal(caps_sa_amd.lpf(s.SA(), s.LCP())[0], lpf)
    b = caps_sa_amd.SuffixArray(T, max_context=16)
    b.construct()
    for call in (b.lpf, b.lz77):
        with pytest.raises(ValueError):
            call()
