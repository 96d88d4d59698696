"""GPU (-m gpu): matching statistics and maximal exact matches on the MI355X (caps_sa_hip_fm_match_*, caps_sa_hip_fm_mems_*).

The sweeps of test_emul_fm_match.py through the host AND the device entry points: the device form always works on buffers preset to
0xA5 with a 64-byte guard behind each.  The truth of the small cases is fm_match_reference; the text of 2^20 + 1 bytes is checked on
the device, with fm_count as the independent witness of every reported piece.  Every comparison is exact.  One process; every input
is one the contract defines or refuses on the host."""
import os
import subprocess

import numpy as np
import pytest

import fm_match_reference as M
import fm_reference as R
from test_emul_fm_match import (FILL, GUARD, DeviceForm, buffer_sweep, cap_sweep, columns_sweep, geometry_sweep, mapping_sweep, mems_sweep, reads_of,
                                self_consistency)

pytestmark = pytest.mark.gpu
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
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
        return self.torch.full((nbytes + GUARD,), FILL, dtype=self.torch.uint8, device="cuda")

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


def edge_primaries_few(n):
    return sorted(p for p in {0, 127, 255, n - 1} if 0 <= p <= n - 1)


@pytest.mark.parametrize("sizes", [(127, 128, 129), (255, 256, 257), (4095,), (4096,), (4097,)])
def test_geometry_host_and_device_forms(L, mem, sizes):
    """Intervals at the '$' row and beside the block edges of both widths, T itself, T + one byte, one byte, the empty pattern."""
    want = 2 * sum(len(edge_primaries_few(n)) for n in sizes)
    assert geometry_sweep(L, sizes, primaries=edge_primaries_few, forms=(L, DeviceForm(L, mem))) == want


def test_lane_to_pattern_mapping(L, mem):
    mapping_sweep(L)
    mapping_sweep(DeviceForm(L, mem))


def test_cap(L, mem):
    cap_sweep(L)
    cap_sweep(DeviceForm(L, mem))


def test_output_buffers(L, mem):
    buffer_sweep(L, mem)


def test_mems(L, mem):
    mems_sweep(L, mem)


def test_mems_across_scan_columns(L, mem):
    columns_sweep(L, 2 * 65536 + 100)
    columns_sweep(DeviceForm(L, mem), 2 * 65536 + 100)


def test_count_is_the_witness_small(L, mem):
    T = np.random.RandomState(12).choice(DNA, size=50_001)
    SA, _, B, primary, _ = L.build_bwt(T)
    pats = reads_of(T, np.random.RandomState(13), 40, 20, 120) + [b"", b"ACGTNNACGT"]
    for bits in (32, 64):
        blob = L.fm_build(B, primary, None, 0, bits)
        for form in (L, DeviceForm(L, mem)):
            assert self_consistency(form, blob, pats) == sum(len(p) for p in pats)
            self_consistency(form, blob, pats, max_len=19)


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return torch.from_numpy(a).cuda()


def test_a_million_rows(L):
    """n = 2^20 + 1, both widths: 4,096 reads of 64 .. 200 bytes cut from T, every second one with one substituted base.  On the
    device: fm_count of every reported piece gives the reported interval, and the piece one byte longer to the left counts 0 -- so
    L is right; the MEM records are then the rule L[e + 1] <= L[e] applied to that L in numpy."""
    import torch
    dev = torch.device("cuda")
    n, q = (1 << 20) + 1, 4096
    rs = np.random.RandomState(20)
    T = rs.choice(DNA, size=n)
    SA, _, B, primary, _ = L.build_bwt(T)
    del SA
    lens = rs.randint(64, 201, size=q).astype(np.int64)
    starts = (rs.random_sample(q) * (n - lens + 1)).astype(np.int64)
    off = np.zeros(q + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    cat = T[np.repeat(starts - off[:-1], lens) + np.arange(total)].copy()
    odd = np.arange(1, q, 2)
    at = off[odd] + (rs.random_sample(odd.size) * lens[odd]).astype(np.int64)
    cat[at] = DNA[(np.searchsorted(DNA, cat[at]) + 1 + rs.randint(0, 3, size=odd.size)) % 4]
    d_cat, d_off = _dev(torch, cat), torch.from_numpy(off).cuda()
    slot = torch.arange(total, device=dev)
    e = slot - torch.repeat_interleave(d_off[:-1], torch.from_numpy(lens).cuda()) + 1

    def count_pieces(index, nbytes, start, length):
        """fm_count on the device of the pieces cat[start : start + length) -> (first, count)"""
        poff = torch.zeros(length.numel() + 1, dtype=torch.int64, device=dev)
        poff[1:] = torch.cumsum(length, 0)
        pieces = d_cat[torch.repeat_interleave(start - poff[:-1], length) + torch.arange(int(poff[-1]), device=dev)]
        f = torch.empty(length.numel(), dtype=torch.int64, device=dev)
        c = torch.empty_like(f)
        torch.cuda.synchronize()
        L.fm_count_device(index.data_ptr(), nbytes, pieces.data_ptr(), poff.data_ptr(), length.numel(), f.data_ptr(), c.data_ptr())
        return f, c

    for bits in (32, 64):
        blob = L.fm_build(B, primary, None, 0, bits)
        index = torch.full((blob.size + GUARD,), FILL, dtype=torch.uint8, device=dev)
        index[:blob.size] = torch.from_numpy(blob).cuda()
        d_len = torch.full((total + 16,), -1, dtype=torch.int32, device=dev)
        d_first = torch.full((total + 8,), -1, dtype=torch.int64, device=dev)
        d_count = torch.full((total + 8,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        L.fm_match_device(index.data_ptr(), blob.size, d_cat.data_ptr(), d_off.data_ptr(), q, 0, d_len.data_ptr(), d_first.data_ptr(), d_count.data_ptr())
        assert bool((d_len[total:] == -1).all()) and bool((d_first[total:] == -1).all()) and bool((d_count[total:] == -1).all()), bits
        assert bool((index[blob.size:] == FILL).all()), bits
        Ld, first, count = d_len[:total].to(torch.int64), d_first[:total], d_count[:total]
        assert bool((Ld >= 1).all()) and bool((Ld <= e).all()), bits                  # (every byte is a letter of T)
        f, c = count_pieces(index, blob.size, slot - Ld + 1, Ld)
        assert torch.equal(f, first) and torch.equal(c, count) and bool((c >= 1).all()), bits
        short = Ld < e
        _, c = count_pieces(index, blob.size, (slot - Ld)[short], (Ld + 1)[short])
        assert not bool(c.any()), bits
        Lh = Ld.cpu().numpy()
        exact = np.arange(0, q, 2)
        assert (Lh[off[exact + 1] - 1] == lens[exact]).all() and (Lh[off[odd + 1] - 1] < lens[odd]).sum() >= odd.size * 9 // 10
        # the MEMs of at least 20 bytes: the rule on the checked L
        min_len = 20
        nxt = np.append(Lh[1:], 0)
        nxt[off[1:] - 1] = 0                                                          # e = m
        ends = np.flatnonzero((Lh >= min_len) & (nxt <= Lh))
        want = np.zeros(ends.size, dtype=M.MEM_DTYPE)
        pat = np.searchsorted(off, ends, side="right") - 1
        want["pattern"], want["length"] = pat, Lh[ends]
        want["start"] = ends - off[pat] + 1 - Lh[ends]
        want["first"], want["count"] = first.cpu().numpy()[ends], count.cpu().numpy()[ends]
        woff = np.searchsorted(ends, off).astype(np.uint64)
        d_moff = torch.full((q + 1 + 8,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        L.fm_mems_device(index.data_ptr(), blob.size, d_cat.data_ptr(), d_off.data_ptr(), q, min_len, d_moff.data_ptr())
        assert np.array_equal(d_moff.cpu().numpy()[:q + 1].view(np.uint64), woff) and bool((d_moff[q + 1:] == -1).all()), bits
        d_mems = torch.full((32 * ends.size + GUARD,), FILL, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        L.fm_mems_device(index.data_ptr(), blob.size, d_cat.data_ptr(), d_off.data_ptr(), q, min_len, d_moff.data_ptr(), d_mems.data_ptr(), ends.size)
        got = d_mems.cpu().numpy()
        assert got[:32 * ends.size].tobytes() == want.tobytes() and (got[32 * ends.size:] == FILL).all(), bits
        assert ends.size >= q + odd.size // 3


def test_python_surface(L):
    """caps_sa_amd.FMIndex.matching_statistics and .mems against the reference, on an index without samples."""
    import caps_sa_amd
    T = np.random.RandomState(8).choice(DNA, size=3001)
    SA = R.naive_sa(T)
    B, primary = R.bwt_of(T, SA)
    ref = M.Text(T, SA)
    fm = caps_sa_amd.FMIndex.from_bwt(B, primary)
    assert fm.sa_sample == 0
    pats = reads_of(T, np.random.RandomState(9), 6, 30, 60) + [b"", b"GATTNACA"]
    Ls, firsts, counts = fm.matching_statistics(pats, intervals=True)
    for P, Lp, f, c in zip(pats, Ls, firsts, counts):
        want = ref.lengths(P)
        wf, wc = ref.intervals(P, want)
        assert np.array_equal(Lp, want) and np.array_equal(f, wf) and np.array_equal(c, wc), P
    for P, Lp in zip(pats, fm.matching_statistics(pats, max_len=9)):
        assert np.array_equal(Lp, ref.lengths(P, 9)), P
    for P, ms in zip(pats, fm.mems(pats, min_len=4)):
        assert [tuple(int(x) for x in m) for m in ms] == ref.mems(P, 4), P


def test_cli_round_trip(L, tmp_path):
    """caps_sa in.fa out.bin --fm-index x.fm, then --fm-mems x.fm reads.txt [--min-len 8] against the reference on the remapped text."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    exe = os.path.join(ROOT, "caps-sa_amd", "caps_sa")
    rs = np.random.RandomState(9)
    raw = b"\n".join([b">chr1 test"] + [bytes(rs.choice(list(b"ACGTacgt"), size=60).tolist()) for _ in range(50)]) + b"\n"
    inp, out, fm, reads = (tmp_path / x for x in ("in.fa", "out.bin", "x.fm", "reads.txt"))
    inp.write_bytes(raw)
    subprocess.check_call([exe, str(inp), str(out), "--fm-index", str(fm)])
    remap = np.frombuffer(b"ACTG", dtype=np.uint8)
    text = remap[(np.frombuffer(raw.upper(), dtype=np.uint8) & 0x6) >> 1]
    ref = M.Text(text, R.naive_sa(text))
    lines = [raw[a:a + ln] for a, ln in ((12, 40), (100, 25), (500, 57), (11, 1))] + [b"", b"acgtacgtacgtacgtacgtacgtacgt"]
    lines[1] = lines[1][:10] + (b"A" if lines[1][10:11] != b"A" else b"C") + lines[1][11:]
    reads.write_bytes(b"".join(ln.replace(b"\n", b"N") + b"\n" for ln in lines))
    for min_len in (1, 8):
        r = subprocess.run([exe, "--fm-mems", str(fm), str(reads)] + (["--min-len", "8"] if min_len == 8 else []), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        want = ""
        for ln in lines:
            P = remap[(np.frombuffer(ln.replace(b"\n", b"N").upper(), dtype=np.uint8) & 0x6) >> 1].tobytes()
            ms = ref.mems(P, min_len)
            want += str(len(ms)) + "".join(f" {s}:{l}:{c}" for s, l, f, c in ms) + "\n"
        assert r.stdout == want, (min_len, r.stdout, want)
