"""GPU (-m gpu): k-mers across a collection of sequences from SA and LCP on the MI355X (caps_sa_hip_coll_kmers_*,
caps_sa_hip_coll_sharing_*).

The size, edge, document, protocol and refusal sweeps of test_emul_coll.py through the host AND the device entry points, both widths:
the device form always works on buffers preset to 0xA5 with guards before and behind the records and behind the workspace.  One text
of 2^20 + 1 bytes (8 documents: a random base of 2^17 - 1 bytes and 7 copies with a substitution every 97 bytes, each followed by one
0xFF byte) is built on the device and freq, shared and the records for min_docs = 8 and for max_docs = 1 are checked against numpy:
every document's 16-byte windows packed into 64-bit words, np.unique per document, the bits ORed over the union.  Then the Python
methods on the same text.  Every comparison is exact.  One process; every input is one the contract defines or refuses on the host.
The _u64 forms run at these sizes only: ranks beyond 2^32 are untested."""
import numpy as np
import pytest

import coll_reference as R
from test_emul_coll import (EDGE_N, LANE, SIZES, TILE, capacity_sweep, document_sweep, edge_cases, edge_sweep, forms_of, n_short_cases,
                            refusal_sweep, short_text_sweep, size_sweep)

pytestmark = pytest.mark.gpu
FILL = 0xA5


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


@pytest.mark.parametrize("sizes", [tuple(SIZES[:5])] + [(n,) for n in SIZES[5:]])
def test_sizes_and_text_shapes(L, mem, sizes):
    assert size_sweep(forms_of(L, mem), sizes) == len(sizes) * 4 * 4 * 2


def test_short_texts(L, mem):
    assert short_text_sweep(forms_of(L, mem), max_len=3, tie_rank_rule=False) == n_short_cases(3)


@pytest.mark.parametrize("part", range(4))
def test_one_run_across_the_lane_and_tile_edges(L, mem, part):
    cases = edge_cases()[part::4]
    assert edge_sweep(forms_of(L, mem), cases) == len(cases) > 40


def test_the_long_runs_in_both_widths_and_forms(L, mem):
    """The runs over whole tiles once more, so that each meets both forms and both widths."""
    cases = [(TILE - 3, 3 * TILE + 2), (0, EDGE_N), (LANE - 1, 2 * TILE + 1), (5, 3 * TILE)]
    for shift in range(4):
        assert edge_sweep(forms_of(L, mem), cases[shift:] + cases[:shift]) == 4


def test_documents_and_filters(L, mem):
    assert document_sweep(forms_of(L, mem)) > 30


def test_counting_call_writing_call_and_capacity(L, mem):
    capacity_sweep(L, mem)


def test_refusals_and_the_empty_text(L, mem):
    refusal_sweep(L, mem)


# ---- one text of 2^20 + 1 bytes, built on the device ---------------------------------------------------------------------------------------

PART = (1 << 17) - 1
K = 16
M = 8


def eight_documents():
    rs = np.random.RandomState(11)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = rs.choice(dna, size=PART).astype(np.uint8)
    parts, docs = [], []
    for c in range(M):
        d = base.copy()
        if c:
            # a substitution every 97 bytes; copies 4 .. 7 repeat every other one of copies 0 .. 3 (copy 4: of its own)
            at = np.arange(7 + 13 * (c % 4), PART, 97 if c < 4 else 194)
            d[at] = dna[(np.searchsorted(dna, d[at]) + 1 + c % 3) % 4]
        docs.append((c * (PART + 1), PART))
        parts += [d, np.array([0xFF], dtype=np.uint8)]
    parts.append(np.array([0xFF], dtype=np.uint8))
    T = np.concatenate(parts)
    assert T.size == (1 << 20) + 1
    return T, docs


def packed_windows(codes: np.ndarray) -> np.ndarray:
    """Every K-byte window of a document as a 64-bit word, 3 bits per byte, the first byte highest: their order is the byte order."""
    w = np.zeros(codes.size - K + 1, dtype=np.uint64)
    for j in range(K):
        w = (w << np.uint64(3)) | codes[j:codes.size - K + 1 + j].astype(np.uint64)
    return w


@pytest.fixture(scope="module")
def built(L):
    """The text, its documents, the constructed SuffixArray and the truth by numpy: (the distinct windows in order, their masks, their
    numbers of occurrences)."""
    import caps_sa_amd
    T, docs = eight_documents()
    s = caps_sa_amd.SuffixArray(T)
    s.construct()
    code = np.zeros(256, dtype=np.uint8)
    code[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    per_doc = [np.unique(packed_windows(code[T[st:st + ln]]), return_counts=True) for st, ln in docs]
    every = np.unique(np.concatenate([u for u, _ in per_doc]))
    mask = np.zeros(every.size, dtype=np.uint64)
    occ = np.zeros(every.size, dtype=np.uint64)
    for d, (u, c) in enumerate(per_doc):
        at = np.searchsorted(every, u)
        mask[at] |= np.uint64(1 << d)
        occ[at] += c.astype(np.uint64)
    return T, docs, s, (every, mask, occ, code)


def test_a_built_text_on_the_device(L, built):
    """build_device, everything stays on the device: freq and shared against numpy, the records for min_docs = 8 and for max_docs = 1
    with every field: docs and occ from the packed windows, count = occ (the separators keep every run inside the documents), and the
    text at SA[first] is the window the record stands for, in order."""
    import torch
    T, docs, s, (every, mask, occ, code) = built
    n = T.size
    dT = torch.from_numpy(T).cuda()
    SA = torch.empty(n, dtype=torch.int32, device="cuda")
    LCP = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.build_device(dT.data_ptr(), n, SA.data_ptr(), LCP.data_ptr())
    sa_host = SA.cpu().numpy().view(np.uint32)
    assert np.array_equal(sa_host, s.SA())
    pop = np.array([R.popcount(x) for x in np.unique(mask)], dtype=np.int64)
    pop_of = dict(zip(np.unique(mask).tolist(), pop.tolist()))
    c = np.array([pop_of[x] for x in mask.tolist()], dtype=np.int64)
    want_freq = np.bincount(c, minlength=65).astype(np.uint64)
    bits = ((mask[:, None] >> np.arange(M, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)
    want_shared = (bits.T @ bits).astype(np.uint64)
    assert want_freq[M] > 1000 and want_freq[1] > 1000 and np.count_nonzero(want_freq[2:M]) >= 2 and want_freq[0] == 0
    freq, shared = L.coll_sharing_device(SA.data_ptr(), LCP.data_ptr(), n, K, docs)
    assert np.array_equal(freq, want_freq) and np.array_equal(shared, want_shared)
    ws_bytes = L.coll_workspace_bytes(n, 32)
    ws = torch.full((ws_bytes + 64,), FILL, dtype=torch.uint8, device="cuda")
    for filt, keep in ((dict(min_docs=M), c == M), (dict(max_docs=1), c == 1)):
        torch.cuda.synchronize()
        found = L.coll_kmers_device(SA.data_ptr(), LCP.data_ptr(), n, K, docs, dWS_ptr=ws.data_ptr(), ws_bytes=ws_bytes, **filt)
        assert found == int(keep.sum())
        rec = torch.full((found + 1, 4), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert L.coll_kmers_device(SA.data_ptr(), LCP.data_ptr(), n, K, docs, dRecords_ptr=rec.data_ptr(), capacity=found,
                                   dWS_ptr=ws.data_ptr(), ws_bytes=ws_bytes, **filt) == found
        assert bool((rec[found] == -1).all()) and bool((ws[ws_bytes:] == FILL).all())
        r = rec[:found].cpu().numpy().view(np.uint64)
        assert np.array_equal(r[:, 3], mask[keep]) and np.array_equal(r[:, 2], occ[keep]) and np.array_equal(r[:, 1], occ[keep])
        assert (np.diff(r[:, 0].astype(np.int64)) > 0).all()
        pos = sa_host[r[:, 0].astype(np.int64)].astype(np.int64)
        got = np.zeros(found, dtype=np.uint64)
        for j in range(K):
            got = (got << np.uint64(3)) | code[T[pos + j]].astype(np.uint64)
        assert (T[pos[:, None] + np.arange(K)[None, :]] != 0xFF).all() and np.array_equal(got, every[keep])
    # the unfiltered count is the sum of freq
    assert L.coll_kmers_device(SA.data_ptr(), LCP.data_ptr(), n, K, docs) == int(want_freq.sum()) == every.size


def test_python_methods_on_a_constructed_suffix_array(L, built):
    import caps_sa_amd
    T, docs, s, (every, mask, occ, code) = built
    fresh = caps_sa_amd.SuffixArray(T)
    with pytest.raises(RuntimeError):
        fresh.kmer_sharing(K, docs)                             # construct() has not been called
    core = s.collection_kmers(K, docs, min_docs=M)
    assert core.dtype == caps_sa_amd.COLL_DTYPE and np.array_equal(core["docs"], mask[mask == np.uint64(255)])
    only3 = s.collection_kmers(K, docs, all_of=1 << 3, none_of=255 ^ (1 << 3))
    assert np.array_equal(only3["occ"], occ[mask == np.uint64(8)]) and len(only3) > 100
    freq, shared = s.kmer_sharing(K, docs)
    assert int(freq[M]) == len(core) and int(freq.sum()) == every.size and int(shared[3, 3]) == int(((mask >> np.uint64(3)) & np.uint64(1)).sum())
    J = s.kmer_jaccard(K, docs)
    sh = shared.astype(np.float64)
    assert J.shape == (M, M) and np.allclose(np.diag(J), 1.0) and J[0, 1] == sh[0, 1] / (sh[0, 0] + sh[1, 1] - sh[0, 1]) and 0.2 < J[0, 1] < 1.0
    assert np.array_equal(J, J.T)
    # a document without a k-mer: 0, not a division by zero
    J2 = s.kmer_jaccard(K, [(0, 5), (10, 3), docs[1]])
    assert J2[0, 1] == 0.0 and J2[0, 0] == 0.0 and J2[2, 2] == 1.0
    # the module-level functions on the arrays alone
    assert np.array_equal(caps_sa_amd.collection_kmers(s.SA(), s.LCP(), K, docs, min_docs=M), core)
    f2, s2 = caps_sa_amd.kmer_sharing(s.SA(), s.LCP(), K, docs)
    assert np.array_equal(f2, freq) and np.array_equal(s2, shared)
    # a bounded-context build is refused
    bounded = caps_sa_amd.SuffixArray(T[:5000], max_context=16)
    bounded.construct()
    for call in (lambda: bounded.collection_kmers(4, [(0, 100)]), lambda: bounded.kmer_sharing(4, [(0, 100)]),
                 lambda: bounded.kmer_jaccard(4, [(0, 100)])):
        with pytest.raises(ValueError):
            call()


def test_cli_round_trip(L, built, tmp_path):
    """The CLI on the same text with --raw --kmer-sharing (all of the file against numpy), and --coll-kmers on its remapped twin -- the
    separators become 'G' there, so the documents are given with one-byte gaps -- against the Python method on the same bytes."""
    import os
    import subprocess
    import caps_sa_amd
    T, docs, s, (every, mask, occ, code) = built
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "caps-sa_amd", "caps_sa")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "caps-sa_amd"), "caps_sa"])
    (tmp_path / "eight.bin").write_bytes(T.tobytes())
    (tmp_path / "eight.docs").write_text("".join(f"{st} {ln}\n" for st, ln in docs))
    r = subprocess.run([exe, str(tmp_path / "eight.bin"), str(tmp_path / "eight.sa"), "--raw", "--docs", str(tmp_path / "eight.docs"),
                        "--kmer-sharing", str(K), str(tmp_path / "eight.sharing")], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    freq, shared = s.kmer_sharing(K, docs)
    want = "".join(f"S\t{a}\t{b}\t{int(shared[a, b])}\n" for a in range(M) for b in range(a, M))
    want += "".join(f"F\t{c}\t{int(freq[c])}\n" for c in range(1, M + 1))
    assert (tmp_path / "eight.sharing").read_bytes() == want.encode() and int(freq.sum()) == every.size
    r = subprocess.run([exe, str(tmp_path / "eight.bin"), str(tmp_path / "mapped.sa"), "--docs", str(tmp_path / "eight.docs"),
                        "--coll-kmers", str(K), str(tmp_path / "core.tsv"), "--min-docs", str(M)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mapped = np.frombuffer(b"ACTG", dtype=np.uint8)[(T & 6) >> 1]          # the CLI's remap of upper-case bytes
    m = caps_sa_amd.SuffixArray(mapped)
    m.construct()
    core = m.collection_kmers(K, docs, min_docs=M)
    sa = m.SA().astype(np.int64)
    lines = (tmp_path / "core.tsv").read_bytes().split(b"\n")
    assert lines[-1] == b"" and len(lines) - 1 == len(core) > 1000
    for j in (0, 1, len(core) // 2, len(core) - 1):
        p = int(sa[int(core["first"][j])])
        assert lines[j] == mapped[p:p + K].tobytes() + f"\t{int(core['occ'][j])}\t{int(core['docs'][j]):016x}".encode()
    assert all(ln.endswith(b"\t00000000000000ff") for ln in lines[:-1])
