"""CPU: the caller's workspace of every *_device entry point (tests/workspace_cases.py) through the host emulation of the kernels.

What the other emulation tests leave open: a caller's pointer that is NOT 256-byte aligned -- the case the 256 bytes on top of every
layout exist for -- and the exact size at which each entry point starts to refuse.  test_gpu_workspace.py runs the same cases on
device memory."""
import pytest

import workspace_cases as W
from emul_util import emul


@pytest.fixture(scope="module", params=(32, 64))
def cases(request):
    return {c.name: c for c in W.cases(emul(), W.HostMem(), request.param)}


def test_the_sizes_the_cases_stand_for():
    """n = 16385 is one rank past a tile of the k-mer, collection and cross kernels and has a second level of inverse-BWT splitters;
    the larger MEM batch is scanned in two columns."""
    assert W.N_BIG == W.KMER_TILE + 1 and W.N_BIG // W.IBWT_S0 + 1 > W.IBWT_TOP >= (W.N_BIG // W.IBWT_S0) // 64 + 1
    assert (W.FM_MEM_COL_MIN + 1 + 1 + W.FM_MEM_COL_MIN - 1) // W.FM_MEM_COL_MIN == 2


ENTRIES = ("inverse_bwt", "fm_from_bwt", "fm_wide", "fm_extract", "fm_mems", "kmers", "kmer_spectrum", "kmer_census", "coll_kmers",
           "coll_sharing", "cross_mums", "cross_mems", "lpf", "lz77")
STRICT = ("inverse_bwt", "fm_from_bwt", "fm_wide", "fm_extract")


@pytest.mark.parametrize("entry", ENTRIES)
def test_workspace_at_any_alignment_and_the_refusal_boundary(cases, entry):
    mine = [c for name, c in cases.items() if name.split("-")[0] == entry]
    assert len(mine) == 2 and all(c.strict == (entry in STRICT) for c in mine)
    for c in mine:
        assert W.check(W.HostMem(), c) == (6 if c.strict else 8)


def test_every_entry_point_has_its_cases(cases):
    assert sorted({name.split("-")[0] for name in cases}) == sorted(ENTRIES)
