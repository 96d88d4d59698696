"""Reference for ISA, range minima over LCP and longest common extensions (include/caps_sa_hip.h "ISA and longest common extensions").

numpy and plain Python, no product code: lce by brute force on the text, the array rules of the header as naive slices, and an
encoder of the blob written from the header's format table."""
import numpy as np

BLOCK, SUPER = 64, 4096
MAGIC = int.from_bytes(b"CAPSLCE1", "little")
HDR_WORDS = 32


# ---- on the text ----------------------------------------------------------------------------------------------------------------------

def lce_brute(t: bytes, i: int, j: int, k: int = 0) -> int:
    """The largest l <= n - max(i, j) such that t[i : i + l] and t[j : j + l] differ in at most k places."""
    n = len(t)
    l, used = 0, 0
    while max(i, j) + l < n:
        if t[i + l] != t[j + l]:
            if used == k:
                break
            used += 1
        l += 1
    return l


def lce_brute_np(T: np.ndarray, I, J, k: int, cap: int = 4096) -> np.ndarray:
    """lce_brute for many pairs at once: a cumulative count of mismatches over a window of `cap` bytes; the few extensions that fill
    the window are done again one by one."""
    n = T.size
    I, J = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64)
    room = n - np.maximum(I, J)
    w = np.arange(cap, dtype=np.int64)[None, :]
    ok = w < room[:, None]
    a = T[np.minimum(I[:, None] + w, n - 1)]
    b = T[np.minimum(J[:, None] + w, n - 1)]
    mism = np.cumsum((a != b) & ok, axis=1)
    good = ok & (mism <= k)                                   # a prefix of every row
    out = good.sum(axis=1)
    t = T.tobytes()
    for x in np.flatnonzero((out >= cap) & (room > cap)).tolist():
        out[x] = lce_brute(t, int(I[x]), int(J[x]), k)
    return out.astype(np.uint64)


# ---- on the arrays ----------------------------------------------------------------------------------------------------------------------

def isa_of(SA) -> list:
    out = [0] * len(SA)
    for r, i in enumerate(SA):
        out[int(i)] = r
    return out


def lcp0(LCP) -> np.ndarray:
    """LCP with entry 0 read as 0."""
    L = np.array(LCP, dtype=np.uint64)
    if L.size:
        L[0] = 0
    return L


def range_min(L0, lo: int, hi: int) -> int:
    return int(np.min(L0[lo:hi + 1]))


def lce0(ISA, L0, n: int, i: int, j: int) -> int:
    if i == j:
        return n - i
    a, b = int(ISA[i]), int(ISA[j])
    return min(range_min(L0, min(a, b) + 1, max(a, b)), n - max(i, j))


def lce_arrays(ISA, L0, n: int, i: int, j: int, k: int = 0) -> int:
    """Kangaroo jumps, as the header words them."""
    l, used = 0, 0
    while True:
        l += lce0(ISA, L0, n, i + l, j + l)
        if max(i, j) + l == n or used == k:
            return l
        l += 1
        used += 1
        if max(i, j) + l == n:                                # (lce0 at position n would be the clamp, 0: stop here)
            return l


class SparseTable:
    """min over any [lo, hi] of an array, numpy: the truth for batches of range minima."""

    def __init__(self, A):
        self.lv = [np.asarray(A, dtype=np.uint64)]
        j = 1
        while 2 * j <= self.lv[0].size:
            p = self.lv[-1]
            self.lv.append(np.minimum(p[:-j], p[j:]))
            j *= 2

    def query(self, lo, hi) -> np.ndarray:
        lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        ln = hi - lo + 1
        lev = np.floor(np.log2(ln)).astype(np.int64)
        lev = np.where((np.int64(1) << lev) > ln, lev - 1, lev)
        out = np.empty(lo.size, dtype=np.uint64)
        for j in np.unique(lev).tolist():
            m = lev == j
            t = self.lv[j]
            out[m] = np.minimum(t[lo[m]], t[hi[m] - (1 << j) + 1])
        return out


# ---- the blob ---------------------------------------------------------------------------------------------------------------------------

def _up(b: int) -> int:
    return (b + 255) // 256 * 256


def layout(n: int, w: int) -> dict:
    nb, ns = (n + BLOCK - 1) // BLOCK, (n + SUPER - 1) // SUPER
    tl = ns.bit_length()                                      # floor(log2 ns) + 1, 0 for ns = 0
    off_isa = 8 * HDR_WORDS
    off_lcp = off_isa + _up(n * w)
    off_m = off_lcp + _up(n * w)
    m_stride, t_stride = _up(nb * w), _up(ns * w)
    off_t = off_m + 7 * m_stride
    return dict(nb=nb, ns=ns, tl=tl, off_isa=off_isa, off_lcp=off_lcp, off_m=off_m, m_stride=m_stride, off_t=off_t, t_stride=t_stride,
                total=off_t + tl * t_stride)


def index_bytes(n: int, w: int) -> int:
    return layout(n, w)["total"]


def header(n: int, w: int) -> np.ndarray:
    l = layout(n, w)
    h = np.zeros(HDR_WORDS, dtype=np.uint64)
    h[:16] = [MAGIC, 1, n, w, BLOCK, SUPER, l["nb"], l["ns"], l["tl"], l["off_isa"], l["off_lcp"], l["off_m"], l["m_stride"], l["off_t"],
              l["t_stride"], l["total"]]
    return h


def _windows(base: np.ndarray, j: int) -> np.ndarray:
    """out[x] = min base[x .. min(x + 2^j, size) - 1]"""
    out = base.copy()
    for d in range(1, min(1 << j, base.size)):
        out[:-d] = np.minimum(out[:-d], base[d:])
    return out


def encode(SA, LCP, w: int) -> np.ndarray:
    """The blob of (SA, LCP), from the format table."""
    dt = np.uint32 if w == 4 else np.uint64
    n = len(SA)
    l = layout(n, w)
    blob = np.zeros(l["total"], dtype=np.uint8)
    blob[:8 * HDR_WORDS] = header(n, w).view(np.uint8)
    if n == 0:
        return blob

    def put(off, a):
        a = np.ascontiguousarray(a, dtype=dt)
        blob[off:off + a.size * w] = a.view(np.uint8)

    isa = np.zeros(n, dtype=np.uint64)
    isa[np.asarray(SA, dtype=np.int64)] = np.arange(n, dtype=np.uint64)
    L0 = lcp0(LCP)
    put(l["off_isa"], isa)
    put(l["off_lcp"], L0)
    top = np.uint64(np.iinfo(np.uint64).max)
    pad = np.concatenate([L0, np.full(l["nb"] * BLOCK - n, top, dtype=np.uint64)])
    m0 = pad.reshape(l["nb"], BLOCK).min(axis=1)
    for j in range(7):
        put(l["off_m"] + j * l["m_stride"], _windows(m0, j))
    pad = np.concatenate([m0, np.full(l["ns"] * (SUPER // BLOCK) - l["nb"], top, dtype=np.uint64)])
    t0 = pad.reshape(l["ns"], SUPER // BLOCK).min(axis=1)
    cur = t0
    for j in range(l["tl"]):
        if j:
            d = 1 << (j - 1)
            nxt = cur.copy()
            nxt[:-d] = np.minimum(cur[:-d], cur[d:])
            cur = nxt
        put(l["off_t"] + j * l["t_stride"], cur)
    return blob
