"""An independent encoder of the FM-index blob (numpy only), written from the format table of include/caps_sa_hip.h ("FM-index",
"The blob, byte by byte"), plus what the geometry tests need beside it: a naive suffix array, texts with a chosen `primary`, and
the sizes and primaries on the edges of the kernels' geometry.

It shares no code with the library, the emulation or the oracle: test_emul_geometry.py and test_gpu_geometry.py compare the
library's blobs with encode() byte for byte."""
import numpy as np

MAGIC = int.from_bytes(b"CAPSFMI1", "little")
VERSION = 1
HEADER_WORDS = 32


def _up64(b):
    return (b + 63) // 64 * 64


def signed_order(letters):
    """Byte values in signed-char order: 0x80 .. 0xFF, then 0x00 .. 0x7F."""
    return sorted((int(b) for b in letters), key=lambda b: b ^ 0x80)


def encode(BWT, primary, SA=None, s=0, idx_bytes=4):
    """The blob of (BWT, primary) as np.uint8: without samples when SA is None (s ignored), else with every SA value that is a
    multiple of s."""
    B = np.ascontiguousarray(BWT, dtype=np.uint8)
    n = int(B.size)
    assert idx_bytes in (4, 8) and (n == 0 or 0 <= primary < n)
    if SA is None:
        s = 0
    else:
        assert s >= 1 and s & (s - 1) == 0 and s <= 1024 and len(SA) == n
    idx = np.dtype("<u4") if idx_bytes == 4 else np.dtype("<u8")
    rows = 128 if idx_bytes == 4 else 256
    n_blocks = (n + 1) // rows + 1
    total_rows = n_blocks * rows
    n_samples = (n - 1) // s + 1 if s and n else 0

    # the alphabet and the stored code of every row: L[0] = BWT[primary], L[r] = BWT[r - 1], '$' and the rows behind n are 0
    letters = signed_order(np.unique(B))
    sigma = len(letters)
    assert sigma <= 4
    lut = np.zeros(256, dtype=np.uint8)
    for c, b in enumerate(letters):
        lut[b] = c
    code = np.zeros(total_rows, dtype=np.uint8)
    C = [1, n + 1, n + 1, n + 1, n + 1]
    if n:
        code[1:n + 1] = lut[B]
        code[0] = lut[B[primary]]
        code[primary + 1] = 0
        hist = np.bincount(lut[B], minlength=4)
        for c in range(4):
            C[c + 1] = C[c] + int(hist[c])
        assert C[4] == n + 1

    # Occ blocks: 4 counts of the stored codes before the block | code words of 16 rows | mark words of 32 rows
    per_block = (code.reshape(n_blocks, rows)[:, :, None] == np.arange(4, dtype=np.uint8)).sum(axis=1, dtype=np.uint64)
    before = np.cumsum(per_block, axis=0) - per_block
    shifts = (2 * np.arange(16, dtype=np.uint32))
    words = (code.reshape(-1, 16).astype(np.uint32) << shifts).sum(axis=1, dtype=np.uint32).reshape(n_blocks, rows // 16)
    mark = np.zeros(total_rows, dtype=np.uint8)
    if s and n:
        mark[1:n + 1] = (np.asarray(SA).astype(np.uint64) & np.uint64(s - 1)) == 0
    mwords = (mark.reshape(-1, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)
    mwords = mwords.reshape(n_blocks, rows // 32)
    occ = np.concatenate([before.astype(idx).view(np.uint8).reshape(n_blocks, 4 * idx_bytes),
                          words.astype("<u4").view(np.uint8).reshape(n_blocks, rows // 4),
                          mwords.astype("<u4").view(np.uint8).reshape(n_blocks, rows // 8)], axis=1)
    assert occ.shape == (n_blocks, rows // 2)

    off_occ = HEADER_WORDS * 8
    off_mrank = off_occ + n_blocks * (rows // 2)
    off_samples = off_mrank + (_up64(n_blocks * idx_bytes) if s else 0)
    total = off_samples + (_up64(n_samples * idx_bytes) if s else 0)
    blob = np.zeros(total, dtype=np.uint8)
    blob[off_occ:off_mrank] = occ.reshape(-1)
    if s:
        per = mark.reshape(n_blocks, rows).sum(axis=1, dtype=np.uint64)
        mrank = np.cumsum(per) - per
        blob[off_mrank:off_mrank + n_blocks * idx_bytes] = mrank.astype(idx).view(np.uint8)
        if n:
            SA = np.asarray(SA).astype(np.uint64)
            samples = SA[(SA & np.uint64(s - 1)) == 0]
            assert samples.size == n_samples, "SA is not a permutation of 0 .. n - 1"
            blob[off_samples:off_samples + n_samples * idx_bytes] = samples.astype(idx).view(np.uint8)

    h = np.zeros(HEADER_WORDS, dtype="<u8")
    h[0], h[1], h[2], h[3], h[4], h[5] = MAGIC, VERSION, n, primary if n else 0, idx_bytes, sigma
    h[6] = sum(b << (8 * c) for c, b in enumerate(letters))
    h[7:12] = C
    h[12], h[13], h[14], h[15], h[16], h[17], h[18] = s, n_samples, n_blocks, off_occ, off_mrank, off_samples, total
    blob[:off_occ] = h.view(np.uint8)
    return blob


# ---- suffix arrays and texts ---------------------------------------------------------------------------------------------------

def naive_sa(T):
    """The suffix array in the library's order (signed-char bytes, a proper prefix before the longer suffix) by sorting the
    suffixes themselves: for n up to a few thousand."""
    T = np.ascontiguousarray(T, dtype=np.uint8)
    key = (T ^ 0x80).tobytes()
    return np.array(sorted(range(T.size), key=lambda i: key[i:]), dtype=np.int64)


def naive_lcp(T, SA):
    """LCP[k] = the common prefix of the suffixes at ranks k - 1 and k (LCP[0] = 0), byte by byte."""
    tb = np.ascontiguousarray(T, dtype=np.uint8).tobytes()
    n = len(tb)
    out = np.zeros(n, dtype=np.int64)
    for k in range(1, n):
        a, b = int(SA[k - 1]), int(SA[k])
        m = 0
        while a + m < n and b + m < n and tb[a + m] == tb[b + m]:
            m += 1
        out[k] = m
    return out


def bwt_of(T, SA):
    """(BWT, primary) from the suffix array: BWT[k] = T[(SA[k] + n - 1) mod n], primary = the k with SA[k] == 0."""
    T = np.ascontiguousarray(T, dtype=np.uint8)
    SA = np.asarray(SA).astype(np.int64)
    return T[(SA + T.size - 1) % T.size], int(np.flatnonzero(SA == 0)[0])


DNA_LETTERS = b"ACGT"
SIGNED_LETTERS = bytes([0x80, 0xFE, 0x05, 0x7F])      # ascending in signed-char order, two on each side of 0x80


def text_with_primary(n, j, seed=0, letters=DNA_LETTERS):
    """T = c . a^j . R with R random over {g, t}, for letters a < c < g < t in signed-char order.  The suffixes below T itself are
    exactly the j that start with a, so primary = j for any 0 <= j <= n - 1."""
    a, c, g, t = letters
    assert signed_order(letters) == [a, c, g, t] and 0 <= j <= n - 1
    rs = np.random.RandomState(seed)
    T = np.empty(n, dtype=np.uint8)
    T[0] = c
    T[1:1 + j] = a
    T[1 + j:] = rs.choice(np.array([g, t], dtype=np.uint8), size=n - 1 - j)
    return T


def _around(m):
    return (m - 2, m - 1, m)          # x with x + 1 = -1, 0, 1 (mod m), nearest m


EDGE_MODULI = (16, 32, 64, 128, 256, 4096, 16_384)
EDGE_SIZES = tuple(sorted({n for m in EDGE_MODULI for n in _around(m)} | {1, 2, 3, 32_767, 32_768}))
PRIMARY_MODULI = (16, 128, 256, 16_384)


def edge_primaries(n):
    """0, n - 1 and every p with p + 1 = -1, 0, 1 modulo 16, 128, 256 and 16,384 nearest each modulus, inside 0 .. n - 1."""
    ps = {0, n - 1} | {p for m in PRIMARY_MODULI for p in _around(m)}
    return sorted(p for p in ps if 0 <= p <= n - 1)
