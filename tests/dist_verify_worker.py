"""Worker of tests/test_dist_gloo.py::test_verify_sharded_across_slice_boundaries: caps_sa_dist.verify_sharded over gloo with the host
emulation of the slice verifier.  Nothing is built: every rank cuts its slice out of the naive SA / LCP (tests/fm_reference.py) of one
1,500-character text and edits it, so that each case is seen by ONE of the checks verify_sharded adds to the slice verifier -- the
slices join, the pair across a boundary (order, repeat and the LCP at the slice head), the lengths sum to n -- or by none."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

N = 1500


def cases(T):
    """(name, global SA, global LCP, cuts, offs or None, expect or None): rank r verifies entries cuts[r] .. cuts[r+1] of the arrays
    and says they start at offs[r] (None: at cuts[r]).  expect None: any count above 0."""
    from fm_reference import naive_sa
    from verify_model import common_prefix
    tb = T.tobytes()

    def lcps(sa):                                          # of any list of positions, n entries or not
        return np.array([0] + [common_prefix(tb, int(a), int(b)) for a, b in zip(sa[:-1], sa[1:])], dtype=np.int64)
    n = T.size
    SA = naive_sa(T)
    LCP = lcps(SA)
    even = [0, 500, 1000, n]
    yield "even split", SA, LCP, even, None, 0
    yield "empty middle slice", SA, LCP, [0, 750, 750, n], None, 0
    yield "empty first slice", SA, LCP, [0, 0, 700, n], None, 0
    yield "empty last slice", SA, LCP, [0, 700, n, n], None, 0
    yield "slice of one entry", SA, LCP, [0, 500, 501, n], None, 0
    for k in (500, 1000):                                  # the first entry of rank 1's and of rank 2's slice
        assert LCP[k] > 0
        for d in (1, -1):                                  # the slice verifier does not look at the LCP of a slice head that is not the
            bad = LCP.copy()                               # head of the array: only the pair across the boundary does
            bad[k] += d
            yield f"head lcp {d:+d} at {k}", SA, bad, even, None, 1
        sw = SA.copy()                                     # the rank below ends .., SA[k-2], SA[k]; this one starts SA[k-1], SA[k+1], ..
        sw[k - 1], sw[k] = SA[k], SA[k - 1]
        yield f"order across {k}", sw, lcps(sw), even, None, 1
        rep = SA.copy()                                    # this rank's first entry repeats the last of the rank below; every LCP
        rep[k] = SA[k - 1]                                 # exact (the whole suffix between the copies)
        yield f"repeat across {k}", rep, lcps(rep), even, None, 1
        gone = np.delete(SA, k)                            # one suffix missing: sorted, joined, exact LCPs -- but n - 1 entries
        yield f"suffix {k} missing", gone, lcps(gone), [0, 500, 1000, n - 1], None, 1
    yield "one off shifted", SA, LCP, even, [0, 501, 1000], None          # ranks 1 and 2 both see a gap
    yield "every off shifted", SA, LCP, even, [1, 501, 1001], 1           # joined, but the first slice does not start at 0


def main():
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    import caps_sa_dist
    from emul_util import emul
    E = emul()
    T_np = np.random.RandomState(17).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=N).astype(np.uint8)
    T = torch.from_numpy(T_np)
    ok = True
    for name, SA, LCP, cuts, offs, expect in cases(T_np):
        for bits in (32, 64):
            dt = torch.int32 if bits == 32 else torch.int64
            lo, hi = cuts[rank], cuts[rank + 1]
            sa = torch.tensor(SA[lo:hi].tolist(), dtype=dt)
            lcp = torch.tensor(LCP[lo:hi].tolist(), dtype=dt)
            errs = caps_sa_dist.verify_sharded(E, T, sa, lcp, offs[rank] if offs else lo, bits)
            good = errs == expect if expect is not None else errs > 0
            if rank == 0:
                print(f"verify case '{name}' bits={bits} errs={errs} expect={'>0' if expect is None else expect} "
                      f"{'OK' if good else 'MISMATCH'}", flush=True)
            ok = ok and good
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
