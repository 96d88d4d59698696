"""A plain model of the device verifier's count, written from the counting rule of include/caps_sa_hip.h
(caps_sa_hip_verify_device_* / caps_sa_hip_verify_slice_device_*): Python loops over bytes, no code shared with the kernels,
the emulation or the oracle.  tests/test_emul_verifier.py and tests/test_gpu_verifier.py assert *n_errors == count(...).

For whole arrays there is a second statement that needs no rule at all: the SA and LCP of a text are unique, so
*n_errors == 0 exactly when the arrays equal the naive ones (is_true_arrays)."""
import numpy as np

from fm_reference import naive_lcp, naive_sa


def _signed(x):
    return x - 256 if x >= 128 else x


def common_prefix(tb, a, b):
    """Bytes the suffixes at a and b share, by walking them."""
    n = len(tb)
    l = 0
    while a + l < n and b + l < n and tb[a + l] == tb[b + l]:
        l += 1
    return l


def in_order(tb, a, b):
    """Is suffix a strictly before suffix b?  Signed bytes, a proper prefix first."""
    n = len(tb)
    l = common_prefix(tb, a, b)
    if a + l == n or b + l == n:          # one ran out: it is a prefix of the other (or a == b)
        return a > b                      # the shorter one starts later
    return _signed(tb[a + l]) < _signed(tb[b + l])


def count(T, n, SA, LCP, cnt, is_head):
    """*n_errors of the verifier on the first cnt entries of SA / LCP (sequences of non-negative Python ints or unsigned numpy
    values) over the text T (n bytes)."""
    tb = np.ascontiguousarray(T, dtype=np.uint8).tobytes()
    assert len(tb) == n and cnt <= n
    SA = [int(x) for x in SA[:cnt]]
    LCP = [int(x) for x in LCP[:cnt]]
    met = set()
    bad = 0
    for i in range(cnt):
        b = SA[i]
        if b >= n:
            bad += 1
            continue
        if b in met:
            bad += 1
        met.add(b)
        if i == 0:
            if is_head and LCP[0] != 0:
                bad += 1
            continue
        a = SA[i - 1]
        if a >= n:
            continue
        if LCP[i] != common_prefix(tb, a, b):
            bad += 1
        if a != b and not in_order(tb, a, b):
            bad += 1
    return bad


def true_arrays(T):
    """(SA, LCP) of T as int64 arrays: fm_reference's sort of the suffixes themselves."""
    T = np.ascontiguousarray(T, dtype=np.uint8)
    SA = naive_sa(T)
    return SA, naive_lcp(T, SA)


def is_true_arrays(T, SA, LCP):
    SAo, LCPo = true_arrays(T)
    return [int(x) for x in SA] == SAo.tolist() and [int(x) for x in LCP] == LCPo.tolist()
