"""GPU (-m gpu): MUMs and rare MEMs between two texts from SA, LCP and BWT on the MI355X (caps_sa_hip_cross_mums_*,
caps_sa_hip_cross_mems_*).

The tile-size and tile-edge sweeps of test_emul_cross.py through the host AND the device entry points, both widths: the device form
always works on buffers preset to 0xA5 with guards before and behind the records and behind the workspace.  One text of 2^20 + 1 bytes
(A of 2^19 bytes, a separator, B = A with a substitution every 97 bytes) is built on the device with its BWT and both modes are
checked against the numpy rank rule, the MUM count also against the rule written in tensor ops; then the Python methods and the CLI
round trip on the same text.  Every comparison is exact.  One process; every input is one the contract defines or refuses on the host.
The _u64 forms run at these sizes only: ranks beyond 2^32 are untested."""
import os
import subprocess

import numpy as np
import pytest

import cross_reference as R
from test_emul_cross import (SIZES, Form, capacity_sweep, corner_sweep, forms_of, mem_edge_sweep, mum_edge_sweep, n_short_texts, refusal_sweep,
                             short_text_sweep, size_sweep)

pytestmark = pytest.mark.gpu
FILL = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's)
    import caps_sa_amd
    lib = caps_sa_amd.lib()
    if lib.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests need a GPU (there is no CPU fallback)")
    return lib


class TorchMem:
    """Device memory for the sweeps' *_device calls."""

    def __init__(self):
        import torch
        self.torch = torch

    def filled(self, nbytes):
        return self.torch.full((nbytes,), FILL, dtype=self.torch.uint8, device="cuda")

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


@pytest.mark.parametrize("sizes", [tuple(SIZES[:3]), tuple(SIZES[3:6]), tuple(SIZES[6:])])
def test_sizes_and_text_shapes(L, mem, sizes):
    assert size_sweep(forms_of(L, mem), sizes) == len(sizes) * 4 * 4


def test_short_texts(L, mem):
    assert short_text_sweep(forms_of(L, mem), max_len=3, widths=(32,), seps=(0x80,)) == n_short_texts(3)


def test_mum_ranks_on_the_tile_edges(L, mem):
    assert mum_edge_sweep(forms_of(L, mem)) == 3 * 4


@pytest.mark.parametrize("c, widths", [(2, (32, 64)), (3, (32, 64)), (64, (32,)), (64, (64,))])
def test_mem_runs_across_the_tile_edges_and_skipped_runs_counted_once(L, mem, c, widths):
    assert mem_edge_sweep(forms_of(L, mem), occs=(c,), widths=widths) == (c + 2) * 2 * len(widths)


def test_split_at_the_ends_sa_zero_in_a_pair_and_no_separator(L, mem):
    assert corner_sweep(forms_of(L, mem)) > 100


def test_counting_call_writing_call_and_capacity(L, mem):
    capacity_sweep(L, mem)


def test_refusals_and_the_empty_text(L, mem):
    refusal_sweep(L, mem)


# ---- one text of 2^20 + 1 bytes, built on the device ---------------------------------------------------------------------------------------

HALF = 1 << 19
MIN_LEN = 16


def two_sides():
    rs = np.random.RandomState(6)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    A = rs.choice(dna, size=HALF).astype(np.uint8)
    B = A.copy()
    B[40::97] = dna[(np.searchsorted(dna, B[40::97]) + 1) % 4]
    return np.concatenate([A, np.array([0xFF], dtype=np.uint8), B]), HALF + 1


@pytest.fixture(scope="module")
def built(L):
    """The text, the constructed SuffixArray (bwt=True), and both modes' truth by the numpy rank rule."""
    import caps_sa_amd
    T, split = two_sides()
    s = caps_sa_amd.SuffixArray(T, bwt=True)
    s.construct()
    SA, LCP, BWT = s.SA(), s.LCP(), s.BWT()
    assert np.array_equal(BWT, T[(SA.astype(np.int64) - 1) % T.size])
    truth = {"mums": R.rank_rule(SA, LCP, BWT, split, MIN_LEN, None), "mems": R.rank_rule(SA, LCP, BWT, split, MIN_LEN, 4)}
    return T, split, s, truth


def test_a_built_text_both_modes_on_the_device(L, built):
    """build_device and bwt_device, everything stays on the device: both modes against the numpy rule (records with torch.equal), the
    MUM count against torch.count_nonzero of the rule written in tensor ops, every record against the text."""
    import torch
    T, split, s, truth = built
    n = T.size
    dT = torch.from_numpy(T).cuda()
    SA = torch.empty(n, dtype=torch.int32, device="cuda")
    LCP = torch.empty(n, dtype=torch.int32, device="cuda")
    BWT = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L.build_device(dT.data_ptr(), n, SA.data_ptr(), LCP.data_ptr())
    L.bwt_device(dT.data_ptr(), n, SA.data_ptr(), 0, n, BWT.data_ptr())
    assert np.array_equal(SA.cpu().numpy().view(np.uint32), s.SA()) and np.array_equal(BWT.cpu().numpy(), s.BWT())
    l, sa, b = LCP.to(torch.int64), SA.to(torch.int64), BWT
    ok = (l[1:] >= MIN_LEN) & (torch.cat([l[:1] * 0, l[1:-1]]) < l[1:]) & (torch.cat([l[2:], l[:1] * 0]) < l[1:])
    ok &= (sa[:-1] >= split) != (sa[1:] >= split)
    ok &= (sa[:-1] == 0) | (sa[1:] == 0) | (b[:-1] != b[1:])
    n_mums = int(torch.count_nonzero(ok))
    assert n_mums == len(truth["mums"][0]) > HALF // 200
    for which, occ in (("mums", 64), ("mems", 4)):
        want_rec, want_summary = truth[which]
        args = (which, SA.data_ptr(), LCP.data_ptr(), BWT.data_ptr(), n, split, MIN_LEN, occ)
        summary = L.cross_device(*args)
        assert summary.tolist() == want_summary
        found = int(summary[0])
        rec = torch.full((found + 1, 3), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert L.cross_device(*args, dRecords_ptr=rec.data_ptr(), capacity=found).tolist() == want_summary
        assert bool((rec[found] == -1).all())
        assert torch.equal(rec[:found].cpu(), torch.tensor(want_rec, dtype=torch.int64).reshape(-1, 3))
        a_, b_, ln = rec[:found, 0], rec[:found, 1], rec[:found, 2]
        assert bool(((a_ < split) & (b_ >= split)).all())
        assert bool((dT[a_] == dT[b_]).all()) and bool((dT[a_ + ln - 1] == dT[b_ + ln - 1]).all())
        assert bool(((b_ + ln == n) | (dT[a_ + ln] != dT[(b_ + ln).clamp(max=n - 1)])).all())        # (a + len <= split - 1 < n)
        assert bool(((a_ == 0) | (dT[(a_ - 1).clamp(min=0)] != dT[b_ - 1])).all())
    assert n_mums == int(L.cross_device("mums", SA.data_ptr(), LCP.data_ptr(), BWT.data_ptr(), n, split, MIN_LEN)[0])


def test_python_methods_on_a_constructed_suffix_array(L, built):
    import caps_sa_amd
    T, split, s, truth = built
    fresh = caps_sa_amd.SuffixArray(T, bwt=True)
    with pytest.raises(RuntimeError):
        fresh.cross_mums(split)                               # construct() has not been called
    rec, summary = s.cross_mums(split, MIN_LEN, return_summary=True)
    assert [tuple(r) for r in rec.tolist()] == truth["mums"][0]
    assert [summary[k] for k in ("records", "skipped_runs", "lcs_len", "lcs_a", "lcs_b")] == truth["mums"][1][:5]
    by_a = s.cross_mums(split, MIN_LEN, sort=True)
    assert by_a["a"].tolist() == sorted(rec["a"].tolist()) and sorted(map(tuple, by_a.tolist())) == sorted(truth["mums"][0])
    rec, summary = s.cross_mems(split, MIN_LEN, max_occ=4, return_summary=True)
    assert [tuple(r) for r in rec.tolist()] == truth["mems"][0] and summary["skipped_runs"] == truth["mems"][1][1]
    ln, a, b = s.longest_common_substring(split)
    assert [ln, a, b] == truth["mums"][1][2:5] and ln >= 96 and bytes(T[a:a + ln]) == bytes(T[b:b + ln])
    # the module-level functions on the arrays alone
    assert np.array_equal(caps_sa_amd.cross_mums(s.SA(), s.LCP(), s.BWT(), split, MIN_LEN), s.cross_mums(split, MIN_LEN))
    assert np.array_equal(caps_sa_amd.cross_mems(s.SA(), s.LCP(), s.BWT(), split, MIN_LEN, max_occ=4), rec)
    # a build without bwt=True makes the BWT with the existing call
    plain = caps_sa_amd.SuffixArray(np.concatenate([T[:3000], T[HALF:HALF + 1], T[split:split + 3000]]))
    plain.construct()
    SA, LCP = plain.SA(), plain.LCP()
    BWT = plain.T()[(SA.astype(np.int64) - 1) % plain.n()]
    want = R.rank_rule(SA, LCP, BWT, 3001, 12, None)
    assert len(want[0]) > 10 and [tuple(r) for r in plain.cross_mums(3001, 12).tolist()] == want[0]
    assert plain.longest_common_substring(3001) == tuple(want[1][2:5])
    # a bounded-context build is refused
    bounded = caps_sa_amd.SuffixArray(T[:5000], max_context=16)
    bounded.construct()
    for call in (lambda: bounded.cross_mums(2500), lambda: bounded.cross_mems(2500), lambda: bounded.longest_common_substring(2500)):
        with pytest.raises(ValueError):
            call()


def test_cli_round_trip(L, built, tmp_path):
    T, split, _, truth = built
    exe = os.path.join(ROOT, "caps-sa_amd", "caps_sa")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    (tmp_path / "two.bin").write_bytes(T.tobytes())
    r = subprocess.run([exe, str(tmp_path / "two.bin"), str(tmp_path / "two.sa"), "--raw", "--cross-mums", str(split), str(tmp_path / "mums.tsv"),
                        "--cross-mems", str(split), str(tmp_path / "mems.tsv"), "--min-len", str(MIN_LEN), "--max-occ", "4"],
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for name, which in (("mums.tsv", "mums"), ("mems.tsv", "mems")):
        rec, summary = truth[which]
        assert (tmp_path / name).read_bytes() == "".join(f"{a}\t{b}\t{l}\n" for a, b, l in rec).encode()
        line = f"cross-{which}: {summary[0]} records, {summary[1]} skipped runs, longest common substring {summary[2]} at {summary[3]} and {summary[4]}."
        assert line.encode() in r.stderr
