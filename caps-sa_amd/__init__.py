"""caps-sa_amd: MI355X-native suffix-array / LCP-array construction (SA+LCP of a text).

Host-side mirror of the reference's class surface ``CaPS_SA::Suffix_Array<idx>``
(reference include/Suffix_Array.hpp:148-181) for Python callers; the C++ mirror is
caps-sa_amd/csrc/Suffix_Array.hpp.  All work happens in libcaps_sa_hip.so (HIP kernels for
gfx950) through the C ABI of include/caps_sa_hip.h.  There is no CPU fallback: importing
works without a GPU (so that the build can be checked), but any computation without the
HIP library or without a device raises.
"""
from __future__ import annotations

import os
import subprocess

import numpy as np

from ._binding import CapsLib, CapsSaError, Stats, Shard, ShardInfo, EXPORTS, MEM_DTYPE, KMER_DTYPE, LZ_DTYPE, LZ_LITERAL, CROSS_DTYPE, CROSS_MAX_OCC, COLL_DTYPE, COLL_MAX_DOCS  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# CAPS_SA_LIB selects a tuning variant built by `make variant` (benchmarking only).
LIB_PATH = os.environ.get("CAPS_SA_LIB") or os.path.join(_HERE, "libcaps_sa_hip.so")
_lib: CapsLib | None = None


def build_library(force: bool = False) -> str:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "caps_sa_hip.h"))
    stale = (not os.path.exists(LIB_PATH)
             or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs))
    if force or stale:
        subprocess.check_call(["make", "-s", "-C", _HERE, "libcaps_sa_hip.so"])
    return LIB_PATH


def lib() -> CapsLib:
    """The bound product library.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)")
        _lib = CapsLib(LIB_PATH, "caps_sa_hip_")
    return _lib


def inverse_bwt(BWT, primary: int, device: int = 0) -> np.ndarray:
    """The text back from its Burrows-Wheeler transform (include/caps_sa_hip.h caps_sa_hip_inverse_bwt_*): the inverse of
    ``SuffixArray(T, bwt=True)``'s ``BWT()`` and ``primary()`` -> np.uint8 array.  The index width follows n.  An input that is
    not the BWT of any text raises CapsSaError (code -1)."""
    return lib().inverse_bwt(BWT, primary, device=device)


def kmers(SA, LCP, k: int, min_count: int = 1, max_count: int = 0, device: int = 0, _lib: CapsLib | None = None) -> np.ndarray:
    """The k-mer table of the text whose full-context SA and LCP these are (include/caps_sa_hip.h "k-mers from SA and LCP"), e.g.
    arrays read from a dump: a structured array (KMER_DTYPE: first, count, pos) of the distinct k-mers with min_count <= count
    (<= max_count unless that is 0), in the library's byte order.  K-mer j is T[pos : pos + k] and occurs at
    SA[first : first + count].  The index width is SA's dtype."""
    return (_lib or lib()).kmers(SA, LCP, k, min_count, max_count, device=device)


def kmer_spectrum(SA, LCP, k: int, bins: int = 1024, device: int = 0, _lib: CapsLib | None = None) -> np.ndarray:
    """np.uint64[bins + 1]: hist[c] = the distinct k-mers that occur c times, hist[bins] = bins times or more, hist[0] = 0."""
    return (_lib or lib()).kmer_spectrum(SA, LCP, k, bins, device=device)


def kmer_census(SA, LCP, max_k: int, device: int = 0, _lib: CapsLib | None = None):
    """(distinct, unique), np.uint64[max_k + 1] each: for every k in 1 .. max_k the number of distinct k-mers and of those that
    occur once, from one pass."""
    return (_lib or lib()).kmer_census(SA, LCP, max_k, device=device)


def collection_kmers(SA, LCP, k: int, docs, min_docs: int = 1, max_docs: int = 0, all_of: int = 0, none_of: int = 0, device: int = 0,
                     _lib: CapsLib | None = None) -> np.ndarray:
    """The k-mers of a collection of sequences inside one text (include/caps_sa_hip.h "k-mers across a collection"): ``docs`` is a
    sequence of up to 64 ascending, disjoint ``(start, length)``.  A structured array (COLL_DTYPE: first, count, occ, docs) in the
    library's byte order of the k-mers that occur inside a document and whose set of documents -- the bit mask ``docs`` -- has
    min_docs .. max_docs members (max_docs = 0: no upper bound), all of ``all_of`` and none of ``none_of``.  ``min_docs=m`` gives the
    core k-mers, ``max_docs=1`` the private ones."""
    return (_lib or lib()).coll_kmers(SA, LCP, k, docs, min_docs, max_docs, all_of, none_of, device=device)


def kmer_sharing(SA, LCP, k: int, docs, device: int = 0, _lib: CapsLib | None = None):
    """(freq, shared) over every k-mer of the collection: freq (np.uint64[65]) counts the k-mers by the number of documents that hold
    them, shared (np.uint64[m, m]) those that documents a and b both hold; the diagonal is a document's number of distinct k-mers."""
    return (_lib or lib()).coll_sharing(SA, LCP, k, docs, device=device)


def jaccard_from_shared(shared) -> np.ndarray:
    """Jaccard(a, b) = S_ab / (S_aa + S_bb - S_ab) as a float matrix, 0 where both documents have no k-mer."""
    s = np.asarray(shared, dtype=np.float64)
    d = np.diag(s)
    union = d[:, None] + d[None, :] - s
    return np.divide(s, union, out=np.zeros_like(s), where=union > 0)


def lpf(SA, LCP, device: int = 0, _lib: CapsLib | None = None):
    """(LPF, Prev) of the text whose full-context SA and LCP these are (include/caps_sa_hip.h "LPF and LZ77 from SA and LCP"), e.g.
    arrays read from a dump, in text order and SA's dtype: LPF[i] = the longest prefix of T[i:] that also starts at some j < i,
    Prev[i] = such a j (all ones where LPF[i] = 0)."""
    return (_lib or lib()).lpf(SA, LCP, device=device)


def isa(SA, device: int = 0, _lib: CapsLib | None = None) -> np.ndarray:
    """The inverse suffix array of SA, in SA's dtype: ISA[SA[r]] = r.  Anything but a permutation of 0 .. n - 1: CapsSaError (-1)."""
    return (_lib or lib()).isa(SA, device=device)


def lz77(SA, LCP, device: int = 0, _lib: CapsLib | None = None) -> np.ndarray:
    """The LZ77 factorization of that text: a structured array (LZ_DTYPE: pos, len, src) in text order; phrase j is
    T[src : src + len] (the two may overlap), or the one byte T[pos] where src = LZ_LITERAL."""
    return (_lib or lib()).lz77(SA, LCP, device=device)


def _cross_result(rec, summary, sort: bool, return_summary: bool):
    if sort:
        rec = rec[np.argsort(rec["a"], kind="stable")]
    return (rec, CapsLib.cross_summary(summary)) if return_summary else rec


def cross_mums(SA, LCP, BWT, split: int, min_len: int = 1, sort: bool = False, return_summary: bool = False, device: int = 0,
               _lib: CapsLib | None = None):
    """The maximal unique matches between A = T[:split] (with its separator at split - 1) and B = T[split:], from the full-context
    SA and LCP of T = A . sep . B and its BWT in rank order (include/caps_sa_hip.h "MUMs and MEMs between two texts"), e.g. arrays
    read from a dump: a structured array (CROSS_DTYPE: a, b, len) -- T[a : a + len] == T[b : b + len], a on side A, b on side B, both
    absolute in T -- in rank order, or ordered by ``a`` with sort=True.  return_summary=True: (records, dict with records,
    skipped_runs, lcs_len, lcs_a, lcs_b -- the longest common substring of A and B).  The index width is SA's dtype."""
    rec, summary = (_lib or lib()).cross_mums(SA, LCP, BWT, split, min_len, device=device)
    return _cross_result(rec, summary, sort, return_summary)


def cross_mems(SA, LCP, BWT, split: int, min_len: int = 1, max_occ: int = CROSS_MAX_OCC, sort: bool = False, return_summary: bool = False,
               device: int = 0, _lib: CapsLib | None = None):
    """Every maximal exact match of at least min_len bytes between A and B whose first min_len bytes occur at most max_occ (2 .. 64)
    times in T, each once; the summary's skipped_runs counts the more frequent seeds that were left out."""
    rec, summary = (_lib or lib()).cross_mems(SA, LCP, BWT, split, min_len, max_occ, device=device)
    return _cross_result(rec, summary, sort, return_summary)


class SuffixArray:
    """Python mirror of ``CaPS_SA::Suffix_Array<T_idx_>`` (include/Suffix_Array.hpp:22-181).

    ``SuffixArray(T, subproblem_count=0, max_context=0)``; ``construct()``; ``SA()``;
    ``LCP()``; ``T()``; ``n()``; ``dump(path)``.  Index width follows src/main.cpp:76-87
    unless ``idx_bits`` is given.  ``bwt=True``: ``construct()`` also returns the Burrows-Wheeler
    transform, ``BWT()`` (np.uint8) and ``primary()`` (include/caps_sa_hip.h; one device only).
    """

    def __init__(self, T, subproblem_count: int = 0, max_context: int = 0, idx_bits: int | None = None, device: int = 0,
                 devices: list[int] | None = None, pinned: bool = False, bwt: bool = False):
        if bwt and devices:
            raise ValueError("bwt=True is built on one device: the sharded build (devices=[...]) has no BWT output")
        self._T = CapsLib._text(T)
        self._n = int(self._T.size)
        self._p = int(subproblem_count)
        self._ctx = int(max_context)
        self._bits = idx_bits or (32 if self._n <= 0xFFFFFFFF else 64)
        self._device = device
        self._devices = list(devices) if devices else None      # several GPUs from this process (caps_sa_hip_build_multi_*)
        self._pinned = pinned                                    # page-locked result arrays (what the C++ mirror allocates)
        self._bwt = bool(bwt)
        self._SA = None
        self._LCP = None
        self._BWT = None
        self._primary: int | None = None
        self._cross_bwt = None                                   # the BWT made for cross_* by a build without bwt=True
        self.stats: dict | None = None

    def T(self) -> np.ndarray:
        return self._T

    def n(self) -> int:
        return self._n

    def construct(self) -> None:
        if self._bwt:
            self._SA, self._LCP, self._BWT, self._primary, self.stats = lib().build_bwt(self._T, self._p, self._ctx, self._bits,
                                                                                       self._device, self._pinned)
        elif self._devices:
            self._SA, self._LCP, self.stats = lib().build_multi(self._T, self._devices, self._p, self._ctx, self._bits, self._pinned)
        else:
            self._SA, self._LCP, self.stats = lib().build(self._T, self._p, self._ctx, self._bits, self._device, self._pinned)

    def SA(self) -> np.ndarray:
        if self._SA is None:
            raise RuntimeError("construct() has not been called")
        return self._SA

    def LCP(self) -> np.ndarray:
        if self._LCP is None:
            raise RuntimeError("construct() has not been called")
        return self._LCP

    def BWT(self) -> np.ndarray:
        """BWT[k] = T[(SA[k] + n - 1) mod n] (needs bwt=True)."""
        if not self._bwt:
            raise RuntimeError("the BWT was not asked for: SuffixArray(..., bwt=True)")
        if self._BWT is None:
            raise RuntimeError("construct() has not been called")
        return self._BWT

    def primary(self) -> int:
        """The k with SA[k] == 0 (needs bwt=True)."""
        if not self._bwt:
            raise RuntimeError("the BWT was not asked for: SuffixArray(..., bwt=True)")
        if self._primary is None:
            raise RuntimeError("construct() has not been called")
        return self._primary

    def _kmer_arrays(self, what: str = "k-mers"):
        if self._ctx:
            raise ValueError(f"{what} need a full-context suffix array: this one was built with max_context set")
        return self.SA(), self.LCP()

    def kmers(self, k: int, min_count: int = 1, max_count: int = 0) -> np.ndarray:
        """The distinct k-mers with min_count <= count (<= max_count unless that is 0) as a structured array (KMER_DTYPE: first, count,
        pos) in the library's byte order: k-mer j is T()[pos : pos + k] and occurs at SA()[first : first + count]."""
        SA, LCP = self._kmer_arrays()
        return lib().kmers(SA, LCP, k, min_count, max_count, self._bits, self._device)

    def kmer_spectrum(self, k: int, bins: int = 1024) -> np.ndarray:
        """np.uint64[bins + 1]: hist[c] = the distinct k-mers that occur c times, hist[bins] = bins times or more."""
        SA, LCP = self._kmer_arrays()
        return lib().kmer_spectrum(SA, LCP, k, bins, self._bits, self._device)

    def kmer_census(self, max_k: int):
        """(distinct, unique), np.uint64[max_k + 1] each: the number of distinct k-mers and of those that occur once, k = 1 .. max_k."""
        SA, LCP = self._kmer_arrays()
        return lib().kmer_census(SA, LCP, max_k, self._bits, self._device)

    def collection_kmers(self, k: int, docs, min_docs: int = 1, max_docs: int = 0, all_of: int = 0, none_of: int = 0) -> np.ndarray:
        """The k-mers of the documents ``docs`` (up to 64 ascending, disjoint ``(start, length)`` in T()) as a structured array
        (COLL_DTYPE: first, count, occ, docs), filtered by the number of documents and the masks: see ``collection_kmers``."""
        SA, LCP = self._kmer_arrays("collection k-mers")
        return lib().coll_kmers(SA, LCP, k, docs, min_docs, max_docs, all_of, none_of, self._bits, self._device)

    def kmer_sharing(self, k: int, docs):
        """(freq, shared): see ``kmer_sharing``."""
        SA, LCP = self._kmer_arrays("collection k-mers")
        return lib().coll_sharing(SA, LCP, k, docs, self._bits, self._device)

    def kmer_jaccard(self, k: int, docs) -> np.ndarray:
        """The exact k-mer Jaccard index of every pair of documents as a float matrix (0 where both have no k-mer)."""
        return jaccard_from_shared(self.kmer_sharing(k, docs)[1])

    def lpf(self):
        """(LPF, Prev) in text order: LPF[i] = the longest prefix of T()[i:] that also starts at some j < i, Prev[i] = such a j (all
        ones where LPF[i] = 0)."""
        SA, LCP = self._kmer_arrays("LPF and LZ77")
        return lib().lpf(SA, LCP, self._bits, self._device)

    def lz77(self) -> np.ndarray:
        """The LZ77 factorization as a structured array (LZ_DTYPE: pos, len, src): phrase j is T()[src : src + len], or the one byte
        T()[pos] where src = LZ_LITERAL."""
        SA, LCP = self._kmer_arrays("LPF and LZ77")
        return lib().lz77(SA, LCP, self._bits, self._device)

    def ISA(self) -> np.ndarray:
        """The inverse suffix array: ISA()[SA()[r]] = r (the rank of every text position)."""
        SA, _ = self._kmer_arrays("ISA and the LCE index")
        return lib().isa(SA, self._bits, self._device)

    def _cross_arrays(self):
        """(SA, LCP, BWT in rank order): the BWT of a bwt=True build, otherwise made once from T and SA on the device
        (caps_sa_hip_bwt_device_*; torch carries the arrays there and back)."""
        SA, LCP = self._kmer_arrays("MUMs and MEMs")
        if self._bwt:
            return SA, LCP, self.BWT()
        if self._cross_bwt is None:
            import torch
            dev = torch.device("cuda", self._device)
            signed = np.int32 if self._bits == 32 else np.int64
            dT = torch.from_numpy(self._T).to(dev)
            dSA = torch.from_numpy(np.ascontiguousarray(SA).view(signed)).to(dev)
            dB = torch.empty(self._n, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            with torch.cuda.device(dev):
                lib().bwt_device(dT.data_ptr(), self._n, dSA.data_ptr(), 0, self._n, dB.data_ptr(), self._bits)
            self._cross_bwt = dB.cpu().numpy()
        return SA, LCP, self._cross_bwt

    def cross_mums(self, split: int, min_len: int = 1, sort: bool = False, return_summary: bool = False):
        """The maximal unique matches between T()[:split] and T()[split:] (``caps_sa_amd.cross_mums``); the byte at split - 1 is
        the separator and occurs nowhere else."""
        SA, LCP, BWT = self._cross_arrays()
        rec, summary = lib().cross_mums(SA, LCP, BWT, split, min_len, self._bits, self._device)
        return _cross_result(rec, summary, sort, return_summary)

    def cross_mems(self, split: int, min_len: int = 1, max_occ: int = CROSS_MAX_OCC, sort: bool = False, return_summary: bool = False):
        """The maximal exact matches between the two sides whose first min_len bytes occur at most max_occ times
        (``caps_sa_amd.cross_mems``)."""
        SA, LCP, BWT = self._cross_arrays()
        rec, summary = lib().cross_mems(SA, LCP, BWT, split, min_len, max_occ, self._bits, self._device)
        return _cross_result(rec, summary, sort, return_summary)

    def longest_common_substring(self, split: int):
        """(len, a, b): the longest common substring of T()[:split] and T()[split:], T()[a : a + len] == T()[b : b + len] with a on
        the first side; (0, 0, 0) when the sides share no byte."""
        SA, LCP, BWT = self._cross_arrays()
        _, summary = lib().cross_mums(SA, LCP, BWT, split, max(self._n, 1), self._bits, self._device)
        return int(summary[2]), int(summary[3]), int(summary[4])

    def dump(self, path: str) -> None:
        """Suffix_Array::dump format (src/Suffix_Array.cpp:497-509): u64 n, SA, LCP."""
        with open(path, "wb") as f:
            f.write(np.uint64(self._n).tobytes())
            f.write(self.SA().tobytes())
            f.write(self.LCP().tobytes())


class FMIndex:
    """FM-index over (BWT, primary) (include/caps_sa_hip.h "FM-index"): batched ``count``, ``locate``, ``matching_statistics``, ``mems`` and (after
    ``with_text_samples``) ``extract`` on the GPU for texts of at most 4 distinct bytes; ``wide=True`` builds the wide format for 1 .. 256 distinct bytes (everything but ``extract``).  The index is one blob (``blob``, np.uint8; ``nbytes``); ``save`` / ``load`` write and read exactly it."""

    def __init__(self, blob: np.ndarray, device: int = 0, _lib: CapsLib | None = None):
        self.blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._device = device
        self._lib = _lib
        if self.blob.size < 256 or bytes(self.blob[:8]) not in (b"CAPSFMI1", b"CAPSFMW1"):
            raise ValueError("not an FM-index blob")
        hdr = self.blob[:256].view(np.uint64)
        self._wide = bytes(self.blob[:8]) == b"CAPSFMW1"
        self._n, self._sample, self._sigma = int(hdr[2]), int(hdr[12]), int(hdr[5])
        self._text_sample = int(hdr[19]) if int(hdr[1]) == 2 and not self._wide else 0

    def _l(self) -> CapsLib:
        return self._lib or lib()

    @classmethod
    def from_bwt(cls, BWT, primary: int, SA=None, sa_sample: int = 32, idx_bits: int | None = None, device: int = 0,
                 _lib: CapsLib | None = None, wide: bool = False) -> "FMIndex":
        """SA = None: an index that counts; with the suffix array it also locates (every sa_sample-th text position is kept).
        wide=True: the wide format, 1 .. 256 distinct bytes."""
        if wide:
            return cls((_lib or lib()).fm_build_wide(BWT, primary, SA, sa_sample, idx_bits, device), device, _lib)
        return cls((_lib or lib()).fm_build(BWT, primary, SA, sa_sample, idx_bits, device), device, _lib)

    @classmethod
    def from_bwt_only(cls, BWT, primary: int, sa_sample: int = 32, idx_bits: int | None = None, device: int = 0,
                      _lib: CapsLib | None = None, wide: bool = False) -> "FMIndex":
        """An index that locates from (BWT, primary) ALONE: the SA samples come from an LF walk over the index itself, the blob is
        the one ``from_bwt`` builds with the suffix array.  Not the BWT of any text: CapsSaError with code -1.  wide=True: not
        built for the wide format, CapsSaError with code -2."""
        if wide:
            raise CapsSaError(-2, "the build from the BWT alone is not built for the wide format (build with the suffix array: from_bwt(..., wide=True))")
        return cls((_lib or lib()).fm_build_from_bwt(BWT, primary, sa_sample, idx_bits, device), device, _lib)

    @classmethod
    def from_suffix_array(cls, sa_obj: "SuffixArray", sa_sample: int = 32, wide: bool = False) -> "FMIndex":
        """From a constructed ``SuffixArray(..., bwt=True)``."""
        return cls.from_bwt(sa_obj.BWT(), sa_obj.primary(), sa_obj.SA(), sa_sample, sa_obj._bits, sa_obj._device, wide=wide)

    @property
    def n(self) -> int:
        return self._n

    @property
    def wide(self) -> bool:
        """The wide format ("CAPSFMW1"): 1 .. 256 distinct bytes, no extract."""
        return self._wide

    @property
    def sigma(self) -> int:
        """The number of distinct bytes of the indexed text."""
        return self._sigma

    @property
    def nbytes(self) -> int:
        return int(self.blob.size)

    @property
    def sa_sample(self) -> int:
        """0: built without an SA (count only)."""
        return self._sample

    def count(self, patterns):
        """(first, count), np.uint64 arrays: pattern j occurs at SA[first[j] : first[j] + count[j]] (count 0: first 0)."""
        return self._l().fm_count(self.blob, patterns, self._device)

    def locate(self, patterns, max_hits: int | None = None) -> list:
        """Per pattern its text positions in SA order (np.uint64), at most max_hits of them."""
        first, count = self.count(patterns)
        take = count if max_hits is None else np.minimum(count, np.uint64(max_hits))
        off = np.zeros(take.size + 1, dtype=np.uint64)
        off[1:] = np.cumsum(take, dtype=np.uint64)
        pos, _ = self._l().fm_locate(self.blob, first, count, off, self._device)
        return [pos[int(off[j]):int(off[j + 1])] for j in range(take.size)]

    def matching_statistics(self, patterns, max_len: int = 0, intervals: bool = False):
        """Per pattern P an np.uint32 array L of len(P) entries: L[e - 1] = the length of the longest piece of P ending at e that
        occurs in the text (at most max_len when max_len > 0; 0 when P[e - 1] is no letter of the index).  intervals=True:
        (L, first, count) lists -- the piece's occurrences are SA[first : first + count].  Needs no SA samples."""
        ln, first, count, off = self._l().fm_match(self.blob, patterns, max_len, intervals, self._device)
        cut = [(int(off[j] - off[0]), int(off[j + 1] - off[0])) for j in range(off.size - 1)]
        lens = [ln[a:b] for a, b in cut]
        if not intervals:
            return lens
        return lens, [first[a:b] for a, b in cut], [count[a:b] for a, b in cut]

    def mems(self, patterns, min_len: int = 1) -> list:
        """Per pattern its maximal exact matches of at least min_len bytes, by increasing end: a structured array with the fields
        ``start`` (within the pattern), ``length``, ``first`` and ``count`` (occurrences SA[first : first + count])."""
        rec, off = self._l().fm_mems(self.blob, patterns, min_len, self._device)
        rec = rec[["start", "length", "first", "count"]]
        return [rec[int(off[j]):int(off[j + 1])] for j in range(off.size - 1)]

    @property
    def text_sample(self) -> int:
        """The distance of the text-position samples that ``extract`` walks from; 0: a version-1 blob (no extract)."""
        return self._text_sample

    def with_text_samples(self, text_sample: int = 32) -> "FMIndex":
        """A new FMIndex (format version 2, a larger blob) that also extracts: one row per text_sample text positions, derived from
        the SA samples of this one.  An index without SA samples: CapsSaError with code -2."""
        return FMIndex(self._l().fm_add_text_samples(self.blob, text_sample, self._device), self._device, self._lib)

    def extract(self, starts, lengths) -> list:
        """T[starts[j] : starts[j] + lengths[j]] for every j, as a list of ``bytes`` (needs ``with_text_samples``)."""
        text, off = self._l().fm_extract(self.blob, starts, lengths, self._device)
        raw = text.tobytes()
        return [raw[int(off[j]):int(off[j + 1])] for j in range(off.size - 1)]

    def save(self, path: str) -> None:
        with open(path, "wb") as f:
            f.write(self.blob.tobytes())

    @classmethod
    def load(cls, path: str, device: int = 0, _lib: CapsLib | None = None) -> "FMIndex":
        return cls(np.fromfile(path, dtype=np.uint8), device, _lib)


class LCEIndex:
    """ISA, LCP and range-minimum tables over a suffix array as one blob (include/caps_sa_hip.h "ISA and longest common extensions"):
    batched ``lce(i, j, mismatches)`` of text positions and ``range_min(lo, hi)`` of ranks on the GPU.  The blob alone answers
    (``blob``, np.uint8; ``nbytes``); ``save`` / ``load`` write and read exactly it."""

    def __init__(self, blob: np.ndarray, device: int = 0, _lib: CapsLib | None = None):
        self.blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._device = device
        self._lib = _lib
        if self.blob.size < 256 or bytes(self.blob[:8]) != b"CAPSLCE1":
            raise ValueError("not an LCE index blob")
        hdr = self.blob[:256].view(np.uint64)
        self._n, self._w = int(hdr[2]), int(hdr[3])
        if self._w not in (4, 8) or int(hdr[15]) > self.blob.size or int(hdr[9]) != 256 or int(hdr[10]) < 256 + self._n * self._w:
            raise ValueError("not an LCE index blob")

    def _l(self) -> CapsLib:
        return self._lib or lib()

    @classmethod
    def from_arrays(cls, SA, LCP, idx_bits: int | None = None, device: int = 0, _lib: CapsLib | None = None) -> "LCEIndex":
        """From the full-context SA and LCP of a text, e.g. arrays read from a dump."""
        return cls((_lib or lib()).lce_build(SA, LCP, idx_bits, device), device, _lib)

    @classmethod
    def from_suffix_array(cls, sa_obj: "SuffixArray") -> "LCEIndex":
        """From a constructed full-context ``SuffixArray``; a bounded-context one raises ValueError."""
        SA, LCP = sa_obj._kmer_arrays("ISA and the LCE index")
        return cls.from_arrays(SA, LCP, sa_obj._bits, sa_obj._device)

    @property
    def n(self) -> int:
        return self._n

    @property
    def nbytes(self) -> int:
        return int(self.blob.size)

    def lce(self, i, j, mismatches: int = 0) -> np.ndarray:
        """np.uint64: the largest l such that T[i : i + l] and T[j : j + l] differ in at most ``mismatches`` (0 .. 1024) places."""
        return self._l().lce(self.blob, i, j, mismatches, self._device)

    def range_min(self, lo, hi) -> np.ndarray:
        """np.uint64: min LCP[lo .. hi] over ranks, both ends inclusive (LCP[0] read as 0): the string depth of the SA interval
        [lo - 1, hi], e.g. ``range_min(first + 1, first + count - 1)`` for the (first, count) of ``FMIndex.count``."""
        return self._l().lce_range_min(self.blob, lo, hi, self._device)

    def isa(self) -> np.ndarray:
        """The inverse suffix array the blob holds (a copy), in the index dtype."""
        return self.blob[256:256 + self._n * self._w].view(np.uint32 if self._w == 4 else np.uint64).copy()

    def save(self, path: str) -> None:
        with open(path, "wb") as f:
            f.write(self.blob.tobytes())

    @classmethod
    def load(cls, path: str, device: int = 0, _lib: CapsLib | None = None) -> "LCEIndex":
        return cls(np.fromfile(path, dtype=np.uint8), device, _lib)
