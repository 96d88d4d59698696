"""GPU (-m gpu): the caller's workspace of every *_device entry point on the MI355X -- the cases of tests/workspace_cases.py (see
test_emul_workspace.py) on device memory: a workspace of exactly the reported size at 0, 8 and 248 bytes behind a 256-byte aligned
address gives the outputs of a NULL workspace and nothing outside it is written; too small a workspace is refused on the host before
anything is launched.  One process, one small call per case."""
import numpy as np
import pytest

import workspace_cases as W
from test_emul_workspace import ENTRIES, STRICT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


class TorchMem:
    """Device memory for the *_device calls."""

    def __init__(self):
        import torch
        self.torch = torch

    def filled(self, nbytes):
        return self.torch.full((nbytes,), W.FILL, dtype=self.torch.uint8, device="cuda")

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


@pytest.fixture(scope="module", params=(32, 64))
def cases(request, L, mem):
    return {c.name: c for c in W.cases(L, mem, request.param)}


@pytest.mark.parametrize("entry", ENTRIES)
def test_workspace_at_any_alignment_and_the_refusal_boundary(cases, mem, entry):
    mine = [c for name, c in cases.items() if name.split("-")[0] == entry]
    assert len(mine) == 2 and all(c.strict == (entry in STRICT) for c in mine)
    for c in mine:
        assert W.check(mem, c) == (6 if c.strict else 8)
