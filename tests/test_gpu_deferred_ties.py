"""GPU (-m gpu): the deferred-tie refinement (kernels.h "Deferred ties, resolved", pipeline.h msd_refine) at every route, size and
window edge, through the compiled kernels at tiles of 4,096 elements: finish <= 32 members, msd_quick_kernel's classes <= 256 /
1,024 / 4,096 (8 / 32 / 128 KB of LDS), the level loop above.  The texts and the witnesses are tests/deferred_tie_cases.py's (FULL):
every case proves from the library's own output -- the sentinels a build with CAPS_SA_DEBUG_NO_MSD leaves, the "[msd]" lines of
CAPS_SA_DEBUG -- that a group of exactly the intended size existed at the intended level, and compares SA and LCP entry by entry
with the oracle; the build that compares every tie (CAPS_SA_NO_DEFER) must be bit-identical.

    text          n          level 0                                  level 1
    edges         3,000,000  1025, 4096 (rank 0), 4097 (rank n - 1)
    around        3,200,000  4095, 8193
    nested_small  2,400,000  2, 31, 32, 33, 256, 257, 1024, 1025, 4097  the same nine sizes, from one group of 6,757
    nested_big    3,600,000  16384                                    4095, 4096, 8193
    long          4,500,000  4100, jumps from 64 to 224 chars; long_runs: every kernel in its <LONG = true> build.  The run
                             of 1,030 chars stands BESIDE the groups, not in them (a family of such runs leaves the direct path at
                             these tiles): the run-table branch of the comparators inside a group runs in the CPU file only
    edges_wide    2,000,000  as edges, 8 bits per char
    nested_wide   2,000,000  as nested_small, 8 bits per char"""
import numpy as np
import pytest

import deferred_tie_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", sorted(C.FULL))
def test_every_route_size_and_edge_on_the_device(L, oracle, monkeypatch, capfd, name, bits):
    """Host entry point, both index widths: full_case() asserts the witnessed sizes per level (FULL_LEVEL0 / FULL_LEVEL1), both
    ends of the rank range ("edges"), the jump and long_runs ("long")."""
    groups, gens, st = C.full_case(L, monkeypatch, capfd, oracle, name, bits=bits)
    if name == "edges":           # the 128 KB class holds groups of 1,025 and of exactly 4,096 members, the loop one of 4,097
        sizes = C.size_counts(groups)
        assert sizes[1025] >= 8 and sizes[4096] >= 8
        assert gens[0]["quick"][2] >= sizes[1025] + sizes[4096] and gens[0]["above_tile"] >= sizes[4097] >= 8
    if name == "nested_small":
        assert gens[0]["sizes"].get(32, 0) >= 1 and gens[1]["sizes"].get(32, 0) >= 1       # finish: exactly MSD_FIN_MAX members


@pytest.mark.parametrize("name", ["nested_small", "long"])
def test_the_device_entry_point(L, oracle, name):
    """Text, SA and LCP in device memory (caps_sa_hip_build_device): entry by entry against the oracle, and the device verifier."""
    import torch
    Th, want = C.full_text(name, oracle)
    n = Th.size
    T = torch.from_numpy(np.array(Th)).cuda()
    SA = torch.empty(n, dtype=torch.int32, device="cuda")
    LCP = torch.empty(n, dtype=torch.int32, device="cuda")
    st = L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr())
    assert st["path_direct"] == 1 and st["tie_groups_deferred"] > 0 and st["tie_levels"] >= 2, st
    assert np.array_equal(SA.cpu().numpy().view(np.uint32), want[32][0])
    assert np.array_equal(LCP.cpu().numpy().view(np.uint32), want[32][1])
    assert L.verify_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr()) == 0
