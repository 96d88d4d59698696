"""GPU (-m gpu): the inverse Burrows-Wheeler transform on the MI355X (include/caps_sa_hip.h caps_sa_hip_inverse_bwt_*).

The fixtures through SuffixArray(bwt=True) and back; 256 Mi random DNA through the host path at both index widths; C3 on the device
(build_device -> bwt_device -> inverse_bwt_device, compared with the text itself); 64-bit rows beyond 2^32 from a BWT built in
closed form; inputs that are not a BWT (refused, no hang, the next call still works); the CLI's --bwt file back to the text."""
import os
import subprocess

import numpy as np
import pytest

from conftest import LARGE_GOLDEN, large_golden, text_bytes

pytestmark = pytest.mark.gpu
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


def _random_dna(torch, n, seed, letters=b"ACGT"):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    lut = torch.tensor(list(letters), dtype=torch.uint8, device="cuda")
    T = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for o in range(0, n, step):
        m = min(step, n - o)
        T[o:o + m] = lut[torch.randint(0, len(letters), (m,), device="cuda", generator=g, dtype=torch.int64)]
    return T


def _device_inverse(L, torch, B, n, primary, bits):
    ws_bytes = L.inverse_bwt_workspace_bytes(n, bits)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.inverse_bwt_device(B.data_ptr(), n, primary, out.data_ptr(), ws.data_ptr(), ws_bytes, idx_bits=bits)
    del ws
    return out


def test_golden_and_large_fixtures(L, golden_cases):
    import caps_sa_amd
    texts = [text_bytes(c["text"]) for c in golden_cases] + [large_golden(name)[0] for name in LARGE_GOLDEN]
    for T in texts:
        if T.size == 0:
            continue
        s = caps_sa_amd.SuffixArray(T, bwt=True)
        s.construct()
        assert np.array_equal(caps_sa_amd.inverse_bwt(s.BWT(), s.primary()), T)


@pytest.mark.parametrize("bits", [32, 64])
def test_host_path_256mi(L, bits):
    import caps_sa_amd
    import torch
    n = 256 << 20
    T = _random_dna(torch, n, 19).cpu().numpy()
    _, _, B, primary, _ = L.build_bwt(T, p=8000, idx_bits=32)
    assert np.array_equal(L.inverse_bwt(B, primary, idx_bits=bits), T)
    if bits == 32:
        assert np.array_equal(caps_sa_amd.inverse_bwt(B, primary), T)


def test_c3_device_resident(L):
    """C3: build_device -> bwt_device -> inverse_bwt_device, byte-exact against the text (neither the SA nor its verifier)."""
    import torch
    n = 3_000_000_001
    T = _random_dna(torch, n, 42)
    SA = torch.empty(n, dtype=torch.int32, device="cuda")
    LCP = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
    del LCP
    torch.cuda.empty_cache()
    B = torch.empty(n, dtype=torch.uint8, device="cuda")
    primary = L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, B.data_ptr())
    del SA
    torch.cuda.empty_cache()
    out = _device_inverse(L, torch, B, n, primary, 32)
    assert torch.equal(out, T)


def test_u64_rows_beyond_2_pow_32(L):
    """T = 'A' * m + R, m = 2^32 + 1000, R = 1e7 letters over {C, G, T}: its BWT in closed form from the library's SA of R --
    primary = 0, BWT = R[-1], 'A' * (m - 1), then R[s - 1] (or 'A' for s = 0) for s in SA_R.  R's rows lie beyond 2^32."""
    import torch
    m = (1 << 32) + 1000
    Rd = _random_dna(torch, 10_000_000, 7, b"CGT")
    R = Rd.cpu().numpy()
    SA_R, _, _ = L.build(R, p=256)
    SA_R = SA_R.astype(np.int64)
    tail = np.where(SA_R > 0, R[SA_R - 1], ord("A")).astype(np.uint8)
    n = m + R.size
    B = torch.empty(n, dtype=torch.uint8, device="cuda")
    B[0] = int(R[-1])
    B[1:m] = ord("A")
    B[m:] = torch.from_numpy(tail).cuda()
    out = _device_inverse(L, torch, B, n, 0, 64)
    del B
    step = 1 << 30
    for o in range(0, m, step):
        assert bool((out[o:min(m, o + step)] == ord("A")).all()), o
    assert torch.equal(out[m:], Rd)


def test_not_a_bwt_is_refused_without_a_hang(L):
    import caps_sa_amd
    import torch
    with pytest.raises(caps_sa_amd.CapsSaError) as e:
        caps_sa_amd.inverse_bwt(b"aa", 0)
    assert e.value.code == EINVAL and "not the BWT" in str(e.value)
    rs = np.random.RandomState(2024)
    B = rs.randint(0, 256, size=1 << 20).astype(np.uint8)
    primary = int(rs.randint(0, B.size))
    for dev in (False, True):
        try:
            if dev:
                Bd = torch.from_numpy(B).cuda()
                T = _device_inverse(L, torch, Bd, B.size, primary, 32).cpu().numpy()
            else:
                T = caps_sa_amd.inverse_bwt(B, primary)
        except caps_sa_amd.CapsSaError as e:
            assert e.code == EINVAL and "not the BWT" in str(e)
        else:                                                          # (1 pair in n is a BWT)
            _, _, B2, p2, _ = L.build_bwt(T)
            assert np.array_equal(B2, B) and p2 == primary
    T = np.random.RandomState(5).choice(DNA, size=100_000)             # a valid call in the same process still works
    _, _, B, primary, _ = L.build_bwt(T)
    assert np.array_equal(caps_sa_amd.inverse_bwt(B, primary), T)


def test_cli_round_trip(L, tmp_path):
    """caps_sa in.fa out.bin --bwt x.bwt, then caps_sa --inverse-bwt x.bwt back: back is the remapped input."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    exe = os.path.join(ROOT, "caps-sa_amd", "caps_sa")
    rs = np.random.RandomState(8)
    lines = [b">chr1 test"] + [bytes(rs.choice(list(b"ACGTNacgt"), size=60).tolist()) for _ in range(2000)]
    raw = b"\n".join(lines) + b"\n"
    inp, out, bwt, back = tmp_path / "in.fa", tmp_path / "out.bin", tmp_path / "x.bwt", tmp_path / "back"
    inp.write_bytes(raw)
    subprocess.check_call([exe, str(inp), str(out), "--bwt", str(bwt)])
    subprocess.check_call([exe, "--inverse-bwt", str(bwt), str(back)])
    remapped = np.frombuffer(b"ACTG", dtype=np.uint8)[(np.frombuffer(raw, dtype=np.uint8) & 0x6) >> 1]
    assert back.read_bytes() == remapped.tobytes()
