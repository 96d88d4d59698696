"""GPU (-m gpu): the device verifier itself on the MI355X (kernels.h verify_kernel through libcaps_sa_hip.so), on device tensors.
About thirty tests of this suite end in verify_device(...) == 0 at sizes no oracle reaches; this file shows that the kernel the GPU
runs says no to every kind of wrong SA / LCP, with the count of tests/verify_model.py (written from the counting rule of
include/caps_sa_hip.h).  The cases are those of tests/test_emul_verifier.py (tests/verifier_cases.py): every single fault, the
refusals and the whole fuzz; of the slice windows a part, since a call costs an allocation, two memsets, a launch and a
synchronisation and the file keeps to MAX_CALLS of them.  Then the grid-stride loop at 4,194,304 + 513 entries on arrays the
oracle has confirmed, and one call on a stream of its own."""
import time

import numpy as np
import pytest

import verifier_cases as VC
import verify_model as M
from conftest import text_bytes

pytestmark = pytest.mark.gpu
MAX_CALLS = 3000
calls = [0]


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


def _dev(values, bits):
    """A list of unsigned values as a device tensor of the signed type of the same width."""
    import torch
    dt = np.uint32 if bits == 32 else np.uint64
    a = np.array(values, dtype=np.uint64).astype(dt)
    assert a.tolist() == [int(x) for x in values], "a value does not fit the index type"
    return torch.from_numpy(a.view(np.int32 if bits == 32 else np.int64)).cuda()


def verifier(L):
    def verify(bits, T, SA, LCP, cnt, is_head):
        """One call: whole arrays with is_head through verify_device_*, everything else through the slice call."""
        import torch
        dT = torch.from_numpy(np.array(T, dtype=np.uint8)).cuda()
        dSA, dLCP = _dev(SA, bits), _dev(LCP, bits)
        calls[0] += 1
        if cnt == T.size and is_head:
            return L.verify_device(dT.data_ptr(), T.size, dSA.data_ptr(), dLCP.data_ptr(), idx_bits=bits)
        return L.verify_slice_device(dT.data_ptr(), T.size, dSA.data_ptr(), dLCP.data_ptr(), cnt, bool(is_head), idx_bits=bits)
    return verify


def test_accepts_the_golden_and_the_random_true_arrays(L, golden_cases):
    for k, c in enumerate(golden_cases):
        T = text_bytes(c["text"])
        assert VC.check(verifier(L), (32, 64)[k % 2], "golden", (c["name"], T, c["sa"], c["lcp"], T.size, 1, 0)) == 0
    for k, case in enumerate(VC.cases("accepted", VC.accepted_cases)):
        VC.check(verifier(L), (32, 64)[k % 2], "accepted", case)


@pytest.mark.parametrize("bits", [32, 64])
def test_single_faults_count_what_they_isolate(L, bits):
    """Every single fault of the CPU file, both index widths: LCP off by one at wave and workgroup edges (lanes 0 and 1 of a wave are
    the shape of DESIGN section 9) and at a pair that runs into the end of the text; the head LCP; one entry out of range (n, n + 1,
    the top of the type, + 2^32); a value twice; unsigned byte order; prefix order; two neighbours swapped."""
    all_cases = VC.cases(f"single{bits}", lambda: VC.single_faults(bits))
    got = {case[0]: VC.check(verifier(L), bits, f"single{bits}", case) for case in all_cases}
    assert len(got) == len(all_cases)
    assert got["prefix order"] == 299
    assert got["unsigned order"] > 300
    assert all(v > 0 for k, v in got.items() if k.startswith("repeat"))


def test_fuzz_of_small_edits(L):
    """The 2,000 cases of the CPU file, index widths in turn."""
    all_cases = VC.cases("fuzz", VC.fuzz_cases)
    assert len(all_cases) >= 2000
    t0 = time.perf_counter()
    rejected = sum(VC.check(verifier(L), (32, 64)[k % 2], "fuzz", case) > 0 for k, case in enumerate(all_cases))
    print(f"fuzz: {len(all_cases)} verifier calls with their uploads and the model in {time.perf_counter() - t0:.2f} s")
    assert 500 < rejected < len(all_cases) - 500


def test_slices(L):
    """Windows of the 70-character text (each first with one entry and with all that follow, both is_head), the edge windows of the
    600-character one, and the windows around a repeat whose first copy they may leave out."""
    all_cases = VC.cases("some slices", lambda: VC.slice_cases(every_window=False))
    VC.check_slice_counts({case[0]: VC.check(verifier(L), (32, 64)[k % 2], "slices", case) for k, case in enumerate(all_cases)})


@pytest.mark.parametrize("bits", [32, 64])
def test_refusals(L, bits):
    T = VC.slice_text()
    SA, LCP = (x.tolist() for x in M.true_arrays(T))
    import torch
    dT, dSA, dLCP = torch.from_numpy(T).cuda(), _dev(SA, bits), _dev(LCP, bits)
    VC.check_refusals(L, bits, T.size, dT.data_ptr(), dSA.data_ptr(), dLCP.data_ptr())
    calls[0] += 2                                          # the refused and the empty calls launch nothing


@pytest.fixture(scope="module")
def grid_arrays(L, oracle):
    """Random DNA one grid of 16,384 x 256 threads and 513 entries long, built on the device and confirmed by the oracle."""
    import torch
    Th = VC.grid_text()
    n = Th.size
    T = torch.from_numpy(Th).cuda()
    SA = torch.empty(n, dtype=torch.int32, device="cuda")
    LCP = torch.empty(n, dtype=torch.int32, device="cuda")
    L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr())
    SAo, LCPo = oracle.build_sa_lcp(Th)
    assert np.array_equal(SA.cpu().numpy().view(np.uint32), SAo) and np.array_equal(LCP.cpu().numpy().view(np.uint32), LCPo)
    return T, SA, LCP


def test_grid_stride_loop(L, grid_arrays):
    """n = 4,194,304 + 513: the launch is capped at 16,384 workgroups, so the entries from 4,194,304 on are a thread's second trip
    through the loop.  One bump on either side of that edge and at the end counts 1; 1,000 bumps count 1,000 -- no atomic addition
    to the error word lost or made twice."""
    import torch
    T, SA, LCP = grid_arrays
    n = T.numel()

    def errs():
        calls[0] += 1
        return L.verify_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr())
    assert errs() == 0
    for i in VC.GRID_SINGLE:
        LCP[i] += 1
        got = errs()
        LCP[i] -= 1
        assert got == 1, i
    many = torch.from_numpy(VC.grid_many()).cuda()
    LCP[many] += 1
    got = errs()
    LCP[many] -= 1
    assert got == 1000
    assert errs() == 0


def test_on_a_stream_of_its_own(L):
    """The arrays are written on a non-default stream and verified on it straight away: the call's memsets, kernel and copy are in
    order behind the writes."""
    import torch
    T = VC.base_text()
    SA, LCP = (x.tolist() for x in M.true_arrays(T))
    LCP[64] += 1
    pinned = [torch.from_numpy(a).pin_memory() for a in (T, np.array(SA, dtype=np.int32), np.array(LCP, dtype=np.int32))]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dT, dSA, dLCP = (a.to("cuda", non_blocking=True) for a in pinned)
        calls[0] += 1
        got = L.verify_device(dT.data_ptr(), T.size, dSA.data_ptr(), dLCP.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert got == 1 == M.count(T, T.size, SA, LCP, T.size, 1)


def test_the_file_keeps_to_its_budget_of_calls():
    assert calls[0] <= MAX_CALLS, calls[0]
    print(f"{calls[0]} verifier calls")
