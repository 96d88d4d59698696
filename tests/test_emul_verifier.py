"""CPU: the device verifier (kernels.h verify_kernel behind caps_sa_hip_verify_device_* / caps_sa_hip_verify_slice_device_*) through
the host emulation of the kernels, on host pointers.  Every "== 0" of the -m gpu suite at sizes no oracle reaches rests on this one
kernel, so every kind of wrong SA / LCP it must reject is pinned here: *n_errors equals the count of tests/verify_model.py (written
from the counting rule of include/caps_sa_hip.h) in every case, the count a construction isolates where there is one, and for whole
arrays zero exactly when the arrays are the naive ones.  The cases are tests/verifier_cases.py; the same run on the MI355X in
tests/test_gpu_verifier.py."""
import numpy as np
import pytest

import verifier_cases as VC
import verify_model as M
from conftest import text_bytes

LIBS = ("emul", "small", "rev")


@pytest.fixture(scope="module", params=LIBS)
def E(request):
    import emul_util
    return {"emul": emul_util.emul, "small": emul_util.emul_small, "rev": emul_util.emul_rev}[request.param]()


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def verifier(E):
    def verify(bits, T, SA, LCP, cnt, is_head):
        """*n_errors of the first cnt entries; whole arrays with is_head go through verify_device_* and the slice call both."""
        T = np.ascontiguousarray(T, dtype=np.uint8)
        sa = np.array(SA, dtype=np.uint64).astype(_dt(bits))
        lcp = np.array(LCP, dtype=np.uint64).astype(_dt(bits))
        assert sa.tolist() == [int(x) for x in SA] and lcp.tolist() == [int(x) for x in LCP], "a value does not fit the index type"
        errs = E.verify_slice_device(T.ctypes.data, T.size, sa.ctypes.data, lcp.ctypes.data, cnt, bool(is_head), idx_bits=bits)
        if cnt == T.size and is_head:
            assert E.verify_device(T.ctypes.data, T.size, sa.ctypes.data, lcp.ctypes.data, idx_bits=bits) == errs
        return errs
    return verify


@pytest.mark.parametrize("bits", [32, 64])
def test_accepts_the_golden_arrays(E, bits, golden_cases):
    for c in golden_cases:
        T = text_bytes(c["text"])
        assert VC.check(verifier(E), bits, "golden", (c["name"], T, c["sa"], c["lcp"], T.size, 1, 0)) == 0


@pytest.mark.parametrize("bits", [32, 64])
def test_accepts_the_true_arrays_of_random_texts(E, bits):
    """n on both sides of a wave and a workgroup, over one, two and four letters, bytes on both sides of 0x80, and all 256."""
    for case in VC.cases("accepted", VC.accepted_cases):
        VC.check(verifier(E), bits, "accepted", case)


@pytest.mark.parametrize("bits", [32, 64])
def test_single_faults_count_what_they_isolate(E, bits):
    """LCP off by one at wave and workgroup edges and at a pair that runs into the end of the text; the head LCP; one entry out of
    range (n, n + 1, the top of the type, + 2^32); a value twice; unsigned byte order; prefix order; two neighbours swapped."""
    all_cases = VC.cases(f"single{bits}", lambda: VC.single_faults(bits))
    got = {case[0]: VC.check(verifier(E), bits, f"single{bits}", case) for case in all_cases}
    assert len(got) == len(all_cases)
    assert got["prefix order"] == 299
    assert got["unsigned order"] > 300
    assert all(v > 0 for k, v in got.items() if k.startswith("repeat"))


@pytest.mark.parametrize("bits", [32, 64])
def test_fuzz_of_small_edits(E, bits):
    """2,000 texts of n <= 48 with 0, 1 or 2 edits of the true arrays; none left out."""
    all_cases = VC.cases("fuzz", VC.fuzz_cases)
    assert len(all_cases) >= 2000
    rejected = sum(VC.check(verifier(E), bits, "fuzz", case) > 0 for case in all_cases)
    assert 500 < rejected < len(all_cases) - 500          # the seeds give both kinds in number


@pytest.mark.parametrize("bits", [32, 64])
def test_slices(E, bits):
    """Every window of a 70-character text and the edge windows of a 600-character one, both is_head: the true arrays (is_head on a
    window whose first LCP is not 0 counts 1), and arrays with one repeat, whose first copy may lie outside the window."""
    all_cases = VC.cases("slices", VC.slice_cases)
    assert len(all_cases) > 4 * 2556
    VC.check_slice_counts({case[0]: VC.check(verifier(E), bits, "slices", case) for case in all_cases})


@pytest.mark.parametrize("bits", [32, 64])
def test_refusals(E, bits):
    """cnt > n, a null n_errors, a null array with something to check: CAPS_SA_EINVAL; nothing to check: CAPS_SA_OK and 0."""
    T = VC.slice_text()
    SA, LCP = (np.ascontiguousarray(x.astype(_dt(bits))) for x in M.true_arrays(T))
    VC.check_refusals(E, bits, T.size, T.ctypes.data, SA.ctypes.data, LCP.ctypes.data)


@pytest.fixture(scope="module")
def grid_arrays():
    """Random DNA one grid of 16,384 x 256 threads and 513 entries long, built by the emulation."""
    import emul_util
    T = VC.grid_text()
    SA, LCP, _ = emul_util.emul().build(T)
    return T, SA, LCP


def test_grid_stride_loop(E, grid_arrays):
    """n = 4,194,304 + 513: the launch is capped at 16,384 workgroups, so the entries from 4,194,304 on are a thread's second trip
    through the loop.  One bump on either side of that edge and at the end counts 1; 1,000 bumps count 1,000 -- no addition to the
    error word lost or made twice."""
    T, SA, LCP = grid_arrays
    n = T.size

    def errs(lcp):
        return E.verify_device(T.ctypes.data, n, SA.ctypes.data, lcp.ctypes.data)
    assert errs(LCP) == 0
    for i in VC.GRID_SINGLE:
        bad = LCP.copy()
        bad[i] += 1
        assert errs(bad) == 1, i
    bad = LCP.copy()
    bad[VC.grid_many()] += 1
    assert errs(bad) == 1000
    SA64, bad64 = SA.astype(np.uint64), bad.astype(np.uint64)
    assert E.verify_device(T.ctypes.data, n, SA64.ctypes.data, bad64.ctypes.data, idx_bits=64) == 1000
