"""GPU (-m gpu): the five kernel-level entry points of libcaps_sa_hip.so (lcp, sort_suffixes, merge, upper_bound, sort_segments) on
texts whose keys tie -- the COMPILED segmented_sort, merge_partition_kernel / merge_pass_kernel, locate_kernel, finalize_kernel and
lcp_pairs_kernel behind an equal key, where test_gpu_parity.py's random DNA never takes them.  The same texts and position lists as
test_emul_kernel_entry.py (kernel_entry_cases.py), the same truth (suffix_order_reference.py), every comparison exact; and the same
classic-path builds that take the galloping locate.  A compiled kernel has differed from its source logic before:
the emulation half alone does not pin this.

Sizes: at most 5E + 1 positions on texts of at most 6E chars, E the tile size of the sources (kernel_entry_cases.TILE_E: 20,481 and
24,576) -- the tie structure is what matters, not n.  The texts of a period the run table does not know come at their full 5 tiles + 1
here (cases(E, full=True)): the emulation keeps them at one tile + 1 for its own speed."""
import pytest

import kernel_entry_cases as K

pytestmark = pytest.mark.gpu
TILE_E = K.TILE_E


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


@pytest.mark.parametrize("name", K.NAMES)
def test_entry_points_on_ties(L, name):
    K.check_case(L, TILE_E, name, full=True)


@pytest.mark.parametrize("name", K.CLASSIC_NAMES)
def test_classic_builds_with_the_galloping_locate(L, name, monkeypatch):
    monkeypatch.setenv("CAPS_SA_PATH", "classic")
    K.check_classic_builds(L, TILE_E, name)
