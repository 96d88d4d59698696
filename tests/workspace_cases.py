"""The caller's workspace of every *_device entry point that takes one (include/caps_sa_hip.h): what caps_sa_hip_*_workspace_bytes
reports is enough at ANY alignment of the caller's pointer, nothing outside [workspace, workspace + reported) is written, a workspace
that is too small is refused with nothing written, and every entry point keeps its refusal boundary.

Shared by test_emul_workspace.py (the host emulation: "device" memory is host memory) and test_gpu_workspace.py (device memory).  A
case is one small call of one entry point; check() runs it with a NULL workspace (the call's own: the reference), then with a workspace
of exactly the reported size at 0, 8 and 248 bytes behind a 256-byte aligned address inside a block preset to 0xA5.

Two refusal boundaries exist (csrc/capi_impl.h; the list below was read from the code before the carve was shared):
  STRICT   anything below the reported size is refused, whatever its alignment:
           inverse_bwt_device (the header promises it; it also refuses a NULL workspace), fm_build_from_bwt_device,
           fm_build_wide_device, fm_extract_device
  SLACK    the bytes lost to aligning the pointer up are subtracted first, so an aligned pointer may be 256 bytes short:
           fm_mems_device, kmers / kmer_spectrum / kmer_census_device, coll_kmers / coll_sharing_device, cross_mums / cross_mems_device,
           lpf_device, lz77_device"""
import ctypes
import os
import re

import numpy as np

from sa_check import sa_lcp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FILL = 0xA5
SENTINEL = 0x5A5A
ALIGN = 256
OFFSETS = (0, 8, 248)
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)
_U64P = ctypes.POINTER(ctypes.c_uint64)


def _const(header, pattern):
    with open(os.path.join(ROOT, "caps-sa_amd", "csrc", header)) as f:
        return re.search(pattern, f.read())


KMER_TILE = 16384                                            # kernels.h KMER_TILE = FM_TILE (also XM_TILE; LPF / LZ tiles are smaller)
_m = _const("kernels.h", r"IBWT_S0_LOG = (\d+), IBWT_S1_LOG = (\d+);")
IBWT_S0 = 1 << int(_m.group(1))
IBWT_TOP = int(_const("kernels.h", r"constexpr uint32_t IBWT_TOP = (\d+);").group(1))
IBWT_TWO_LEVELS = IBWT_S0 * IBWT_TOP                         # n / IBWT_S0 + 1 nodes > IBWT_TOP: a second level of splitters
FM_MEM_COL_MIN = 1 << int(_const("capi_impl.h", r"FM_MEM_COL_MIN = 1u << (\d+)").group(1))
assert KMER_TILE + 1 >= IBWT_TWO_LEVELS                      # one text serves both families
N_BIG = KMER_TILE + 1


class HostMem:
    """Memory of the *_device entry points of the emulation: host memory."""

    def filled(self, nbytes):
        return np.full(nbytes, FILL, dtype=np.uint8)

    def put(self, a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return a.copy() if a.size else np.zeros(8, dtype=np.uint8)

    def ptr(self, buf):
        return buf.ctypes.data

    def get(self, buf):
        return buf


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


_texts = {}


def text(n):
    """(T, SA, LCP, BWT, primary) of a random DNA text of n bytes; SA and LCP 64-bit."""
    if n not in _texts:
        T = np.random.RandomState(7 + n).choice(DNA, size=n).astype(np.uint8)
        SA, LCP = sa_lcp(T, 64)
        BWT = T[(SA.astype(np.int64) - 1) % n]
        _texts[n] = (T, SA, LCP, BWT, int(np.flatnonzero(SA == 0)[0]))
    return _texts[n]


class Case:
    """One call: `call(out pointers, host outputs, workspace pointer or None, workspace bytes)` -> the return code."""

    def __init__(self, name, strict, reported, out_bytes, host_words, call, expected=None, null_ok=True):
        self.name, self.strict, self.reported = name, strict, int(reported)
        self.out_bytes, self.host_words, self.call = out_bytes, host_words, call
        self.expected, self.null_ok = expected, null_ok

    def run(self, mem, ws, wsb):
        """(return code, the device outputs as host arrays, the host outputs)."""
        outs = [mem.filled(b) for b in self.out_bytes]
        host = [np.full(w, SENTINEL, dtype=np.uint64) for w in self.host_words]
        rc = self.call([mem.ptr(o) for o in outs], host, ws, wsb)
        return rc, [np.array(mem.get(o)) for o in outs], [h.tolist() for h in host]

    def untouched(self, got):
        return all((o == FILL).all() for o in got[1]) and all(set(h) <= {SENTINEL} for h in got[2])


def _u64p(h):
    return h.ctypes.data_as(_U64P)


def cases(lib, mem, bits):
    """Every entry point at n = 1 and at the smallest size with a second tile / splitter level / scan column, in one index width."""
    sfx, w = ("u32", 4) if bits == 32 else ("u64", 8)
    f = lib._f
    out = []
    for n in (1, N_BIG):
        T, SA, LCP, BWT, primary = text(n)
        sa, lcp = SA.astype(_dt(bits)), LCP.astype(_dt(bits))
        dSA, dLCP, dB = mem.put(sa), mem.put(lcp), mem.put(BWT)
        S, Lp, B = mem.ptr(dSA), mem.ptr(dLCP), mem.ptr(dB)
        keep = (dSA, dLCP, dB)                               # (the closures keep the device arrays alive)
        tag = f"{sfx}-n{n}"

        # ---- the strict entries -------------------------------------------------------------------------------------------------
        out.append(Case(f"inverse_bwt-{tag}", True, lib.inverse_bwt_workspace_bytes(n, bits), [n], [],
                        lambda o, h, ws, wsb, n=n, B=B, primary=primary, keep=keep:
                        f(f"inverse_bwt_device_{sfx}")(B, n, primary, o[0], ws, wsb, None), expected=[T], null_ok=False))
        ib = lib.fm_index_bytes(n, 32, bits)
        out.append(Case(f"fm_from_bwt-{tag}", True, lib.fm_from_bwt_workspace_bytes(n, 32, bits), [ib], [],
                        lambda o, h, ws, wsb, n=n, B=B, primary=primary, ib=ib, keep=keep:
                        f(f"fm_build_from_bwt_device_{sfx}")(B, n, primary, 32, o[0], ib, ws, wsb, None)))
        wb = lib.fm_wide_index_bytes(n, 0, 32, bits)
        out.append(Case(f"fm_wide-{tag}", True, lib.fm_wide_workspace_bytes(n, bits), [wb], [],
                        lambda o, h, ws, wsb, n=n, B=B, S=S, primary=primary, wb=wb, keep=keep:
                        f(f"fm_build_wide_device_{sfx}")(B, n, primary, S, 32, o[0], wb, ws, wsb, None)))

        # ---- the entries that subtract the alignment slack ------------------------------------------------------------------------
        k, cap = (1, 4) if n == 1 else (3, 128)
        kw = lib.kmer_workspace_bytes(n, bits)
        out.append(Case(f"kmers-{tag}", False, kw, [24 * cap], [1],
                        lambda o, h, ws, wsb, n=n, S=S, Lp=Lp, k=k, cap=cap, keep=keep:
                        f(f"kmers_device_{sfx}")(S, Lp, n, k, 0, 0, o[0], cap, _u64p(h[0]), ws, wsb, None)))
        out.append(Case(f"kmer_spectrum-{tag}", False, kw, [], [17],
                        lambda o, h, ws, wsb, n=n, S=S, Lp=Lp, k=k, keep=keep:
                        f(f"kmer_spectrum_device_{sfx}")(S, Lp, n, k, 16, h[0].ctypes.data, ws, wsb, None)))
        out.append(Case(f"kmer_census-{tag}", False, kw, [], [9, 9],
                        lambda o, h, ws, wsb, n=n, S=S, Lp=Lp, keep=keep:
                        f(f"kmer_census_device_{sfx}")(S, Lp, n, 8, h[0].ctypes.data, h[1].ctypes.data, ws, wsb, None)))
        m = 1 if n == 1 else 2
        start = np.array([0, n // 2][:m], dtype=np.uint64)
        length = np.array([n if m == 1 else n // 2, n - n // 2][:m], dtype=np.uint64)
        docs = (start.ctypes.data, length.ctypes.data, m)
        cw = lib.coll_workspace_bytes(n, bits)
        out.append(Case(f"coll_kmers-{tag}", False, cw, [32 * cap], [1],
                        lambda o, h, ws, wsb, n=n, S=S, Lp=Lp, k=k, cap=cap, docs=docs, keep=(keep, start, length):
                        f(f"coll_kmers_device_{sfx}")(S, Lp, n, k, *docs, 0, 0, 0, 0, o[0], cap, _u64p(h[0]), ws, wsb, None)))
        out.append(Case(f"coll_sharing-{tag}", False, cw, [], [65, m * m],
                        lambda o, h, ws, wsb, n=n, S=S, Lp=Lp, k=k, docs=docs, keep=(keep, start, length):
                        f(f"coll_sharing_device_{sfx}")(S, Lp, n, k, *docs, h[0].ctypes.data, h[1].ctypes.data, ws, wsb, None)))
        split, min_len = (n // 2, 1) if n == 1 else (n // 2, 6)
        xw = lib.cross_workspace_bytes(n, bits)
        out.append(Case(f"cross_mums-{tag}", False, xw, [24 * n], [8],
                        lambda o, h, ws, wsb, n=n, S=S, Lp=Lp, B=B, split=split, min_len=min_len, keep=keep:
                        f(f"cross_mums_device_{sfx}")(S, Lp, B, n, split, min_len, o[0], n, h[0].ctypes.data, ws, wsb, None)))
        out.append(Case(f"cross_mems-{tag}", False, xw, [24 * n], [8],
                        lambda o, h, ws, wsb, n=n, S=S, Lp=Lp, B=B, split=split, min_len=min_len, keep=keep:
                        f(f"cross_mems_device_{sfx}")(S, Lp, B, n, split, min_len + 2, 4, o[0], n, h[0].ctypes.data, ws, wsb, None)))
        out.append(Case(f"lpf-{tag}", False, lib.lpf_workspace_bytes(n, bits), [n * w, n * w], [],
                        lambda o, h, ws, wsb, n=n, S=S, Lp=Lp, keep=keep:
                        f(f"lpf_device_{sfx}")(S, Lp, n, o[0], o[1], ws, wsb, None)))
        lpf, prev = np.zeros(n, dtype=_dt(bits)), np.zeros(n, dtype=_dt(bits))
        assert f(f"lpf_{sfx}")(sa.ctypes.data, lcp.ctypes.data, n, lpf.ctypes.data, prev.ctypes.data, 0) == 0
        dF, dP = mem.put(lpf), mem.put(prev)
        out.append(Case(f"lz77-{tag}", False, lib.lz77_workspace_bytes(n, bits), [24 * n], [1],
                        lambda o, h, ws, wsb, n=n, F=mem.ptr(dF), P=mem.ptr(dP), keep=(dF, dP):
                        f(f"lz77_device_{sfx}")(F, P, n, o[0], n, _u64p(h[0]), ws, wsb, None)))

    # ---- the FM queries: an index of the larger text; the workspace follows the batch ------------------------------------------------
    T, SA, LCP, BWT, primary = text(N_BIG)
    blob = lib.fm_add_text_samples(lib.fm_build(BWT, primary, SA.astype(_dt(bits)), 32, bits), 32)
    d_index = mem.put(blob)
    I = mem.ptr(d_index)
    for q in (1, 40):                                        # u64[q + 1]: one 256-byte unit, two
        starts = (np.arange(q, dtype=np.uint64) * 397) % np.uint64(N_BIG - 64)
        off = np.arange(q + 1, dtype=np.uint64) * 50
        dS, dO = mem.put(starts), mem.put(off)
        out.append(Case(f"fm_extract-{sfx}-q{q}", True, lib.fm_extract_workspace_bytes(q), [50 * q], [],
                        lambda o, h, ws, wsb, q=q, s=mem.ptr(dS), oo=mem.ptr(dO), keep=(d_index, dS, dO):
                        f("fm_extract_device")(I, blob.size, s, oo, q, o[0], ws, wsb, None),
                        expected=[np.concatenate([T[int(s):int(s) + 50] for s in starts])]))
    rs = np.random.RandomState(11)
    for total, q in ((1, 1), (FM_MEM_COL_MIN + 1, 16)):      # one scan column, two
        cat = rs.choice(DNA, size=total).astype(np.uint8)
        off = (np.arange(q + 1, dtype=np.uint64) * total) // q
        dC, dO = mem.put(cat), mem.put(off)
        out.append(Case(f"fm_mems-{sfx}-total{total}", False, lib.fm_mems_workspace_bytes(total, q), [8 * (q + 1), 32 * total], [],
                        lambda o, h, ws, wsb, q=q, total=total, c=mem.ptr(dC), oo=mem.ptr(dO), keep=(d_index, dC, dO):
                        f("fm_mems_device")(I, blob.size, c, oo, q, 4, o[0], o[1], total, ws, wsb, None)))
    return out


def _block(mem, case, off, size):
    """A block preset to 0xA5 with `size` bytes at `off` behind a 256-byte aligned address -> (block, pointer, offset in the block)."""
    blk = mem.filled(2 * ALIGN + max(OFFSETS) + case.reported + 2 * ALIGN)
    p = mem.ptr(blk)
    at = (-p) % ALIGN + ALIGN + off
    assert (p + at - off) % ALIGN == 0
    return blk, p + at, at


def check(mem, case):
    """Every assertion of one case; -> the number of calls made."""
    err = case.name
    ref = case.run(mem, None, 0)
    if case.null_ok:
        assert ref[0] == 0, err
        want = ref[1:]
    else:                                                    # (a NULL workspace is refused: the reference is the known answer)
        assert ref[0] == EINVAL and case.untouched(ref), err
        want = ([np.asarray(e).view(np.uint8) for e in case.expected], [])
    if case.expected is not None:
        for e, o in zip(case.expected, want[0]):
            assert np.array_equal(np.asarray(e).view(np.uint8), o[:np.asarray(e).nbytes]), err
    calls = 1

    def same(got):
        return got[0] == 0 and all(np.array_equal(a, b) for a, b in zip(got[1], want[0])) and got[2] == want[1]

    def clean(blk, at, size):
        b = mem.get(blk)
        return (b[:at] == FILL).all() and (b[at + size:] == FILL).all()

    # a buffer of exactly the reported size at any alignment: accepted, the same outputs, nothing written outside it
    for off in OFFSETS:
        blk, ws, at = _block(mem, case, off, case.reported)
        got = case.run(mem, ws, case.reported)
        assert same(got), (err, off, got[0])
        assert clean(blk, at, case.reported), (err, off, "written outside the workspace")
        calls += 1
    # too small: refused, nothing written
    refused = [max(case.reported - 512, 0)]
    if case.strict:
        refused.append(case.reported - 1)
    else:
        # the slack of an aligned pointer is 0: the layout alone is enough, one byte less is not
        blk, ws, at = _block(mem, case, 0, case.reported - ALIGN)
        got = case.run(mem, ws, case.reported - ALIGN)
        assert same(got), (err, "aligned, 256 short", got[0])
        assert clean(blk, at, case.reported - ALIGN), (err, "written outside the workspace")
        refused.append(case.reported - ALIGN - 1)
        # ... and at 8 bytes behind an aligned address 248 are lost
        refused_at_8 = case.reported - ALIGN + 247
        blk, ws, at = _block(mem, case, 8, refused_at_8)
        got = case.run(mem, ws, refused_at_8)
        assert got[0] == EINVAL and case.untouched(got) and (mem.get(blk) == FILL).all(), (err, "8 behind, 9 short", got[0])
        calls += 2
    for size in refused:
        blk, ws, at = _block(mem, case, 0, size)
        got = case.run(mem, ws, size)
        assert got[0] == EINVAL, (err, size, got[0])
        assert case.untouched(got) and (mem.get(blk) == FILL).all(), (err, size, "a refused call wrote")
        calls += 1
    return calls
