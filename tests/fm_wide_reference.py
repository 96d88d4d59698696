"""An independent encoder of the WIDE FM-index blob (numpy only), written from the format table of include/caps_sa_hip.h ("FM-index:
the wide format", "The blob, byte by byte"): the levels come from numpy's stable sort of the actual code sequence, zone[] from the
descent itself with counted ranks.  It shares no code with the library, the emulation or the oracle; the naive suffix array and the
edge sizes come from fm_reference."""
import numpy as np

from fm_reference import bwt_of, edge_primaries, naive_sa, signed_order  # noqa: F401  (re-exported for the tests)

MAGIC = int.from_bytes(b"CAPSFMW1", "little")
VERSION = 1
HEADER_WORDS = 32
TABLE_BYTES = 4800
OFF_LETTERS, OFF_CODE_OF, OFF_C, OFF_ZONE, OFF_Z = 0, 256, 512, 2568, 4616


def _up64(b):
    return (b + 63) // 64 * 64


def levels_of(sigma):
    lv = 1
    while 4 ** lv < sigma:
        lv += 1
    return lv


def _occ_section(digit, n_rows_real, n_blocks, rows, idx, mark=None):
    """One level: 4 counts | 2-bit digit words | mark words per block.  digit: the digits of positions 0 .. n; the rest is 0."""
    total_rows = n_blocks * rows
    d = np.zeros(total_rows, dtype=np.uint8)
    d[:n_rows_real] = digit
    real = np.zeros(total_rows, dtype=bool)
    real[:n_rows_real] = True
    per_block = ((d.reshape(n_blocks, rows)[:, :, None] == np.arange(4, dtype=np.uint8)) & real.reshape(n_blocks, rows)[:, :, None]).sum(axis=1, dtype=np.uint64)
    before = np.cumsum(per_block, axis=0) - per_block
    words = (d.reshape(-1, 16).astype(np.uint32) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint32).reshape(n_blocks, rows // 16)
    m = np.zeros(total_rows, dtype=np.uint8) if mark is None else mark
    mwords = (m.reshape(-1, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint32).reshape(n_blocks, rows // 32)
    sec = np.concatenate([before.astype(idx).view(np.uint8).reshape(n_blocks, -1),
                          words.astype("<u4").view(np.uint8).reshape(n_blocks, rows // 4),
                          mwords.astype("<u4").view(np.uint8).reshape(n_blocks, rows // 8)], axis=1)
    assert sec.shape == (n_blocks, rows // 2)
    return sec.reshape(-1)


def encode(BWT, primary, SA=None, s=0, idx_bytes=4):
    """The wide blob of (BWT, primary) as np.uint8: without samples when SA is None (s ignored)."""
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
    n_samples = (n - 1) // s + 1 if s and n else 0
    letters = signed_order(np.unique(B))
    sigma = len(letters)
    Lv = levels_of(sigma)

    tab = np.zeros(TABLE_BYTES, dtype=np.uint8)
    C = np.full(257, n + 1, dtype="<u8")
    C[0] = 1
    zone = np.zeros(256, dtype="<u8")
    Z = np.zeros((4, 4), dtype="<u8")
    level_bytes = n_blocks * (rows // 2)
    sections = []
    mark = np.zeros(n_blocks * rows, dtype=np.uint8)
    if n:
        tab[OFF_LETTERS:OFF_LETTERS + sigma] = letters
        skey = sorted(b ^ 0x80 for b in letters)
        for b in range(256):
            tab[OFF_CODE_OF + b] = sum(1 for k in skey if k < (b ^ 0x80))
        lut = np.zeros(256, dtype=np.uint8)
        lut[letters] = np.arange(sigma, dtype=np.uint8)
        hist = np.bincount(lut[B], minlength=256)
        C[1:] = 1 + np.cumsum(hist)
        code = np.zeros(n + 1, dtype=np.uint8)
        code[1:] = lut[B]
        code[0] = lut[B[primary]]
        code[primary + 1] = 0
        if s:
            mark[1:n + 1] = (np.asarray(SA).astype(np.uint64) & np.uint64(s - 1)) == 0
        seqs = []
        cur = code
        for lv in range(Lv):
            digit = (cur >> (2 * (Lv - 1 - lv))) & 3
            seqs.append(digit)
            for d in range(4):
                Z[lv, d] = int((digit < d).sum())
            sections.append(_occ_section(digit, n + 1, n_blocks, rows, idx, mark if lv == 0 else None))
            cur = cur[np.argsort(digit, kind="stable")]
        for c in range(sigma):                           # zone[c]: the descent of code c from position 0
            p = 0
            for lv in range(Lv):
                d = (c >> (2 * (Lv - 1 - lv))) & 3
                p = int(Z[lv, d]) + int((seqs[lv][:p] == d).sum())
            zone[c] = p
    else:
        C[:] = 1
        sections = [np.zeros(level_bytes, dtype=np.uint8)] * Lv
    tab[OFF_C:OFF_C + 257 * 8] = C.view(np.uint8)
    tab[OFF_ZONE:OFF_ZONE + 256 * 8] = zone.view(np.uint8)
    tab[OFF_Z:OFF_Z + 128] = Z.reshape(-1).view(np.uint8)

    off_tab = HEADER_WORDS * 8
    off_lev0 = off_tab + TABLE_BYTES
    off_mrank = off_lev0 + Lv * level_bytes
    off_samples = off_mrank + (_up64(n_blocks * idx_bytes) if s else 0)
    total = off_samples + (_up64(n_samples * idx_bytes) if s else 0)
    blob = np.zeros(total, dtype=np.uint8)
    blob[off_tab:off_lev0] = tab
    for lv in range(Lv):
        blob[off_lev0 + lv * level_bytes:off_lev0 + (lv + 1) * level_bytes] = sections[lv]
    if s:
        per = mark.reshape(n_blocks, rows).sum(axis=1, dtype=np.uint64)
        blob[off_mrank:off_mrank + n_blocks * idx_bytes] = (np.cumsum(per) - per).astype(idx).view(np.uint8)
        if n:
            SA = np.asarray(SA).astype(np.uint64)
            samples = SA[(SA & np.uint64(s - 1)) == 0]
            assert samples.size == n_samples, "SA is not a permutation of 0 .. n - 1"
            blob[off_samples:off_samples + n_samples * idx_bytes] = samples.astype(idx).view(np.uint8)
    h = np.zeros(HEADER_WORDS, dtype="<u8")
    h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8] = MAGIC, VERSION, n, primary if n else 0, idx_bytes, sigma, Lv, off_tab, level_bytes
    h[12], h[13], h[14], h[15], h[16], h[17], h[18] = s, n_samples, n_blocks, off_lev0, off_mrank, off_samples, total
    blob[:off_tab] = h.view(np.uint8)
    return blob


def text_with_sigma(n, sigma, seed=0):
    """A random text of n >= sigma bytes with exactly sigma distinct ones, bytes >= 0x80 among them (every second letter)."""
    assert 1 <= sigma <= 256 and n >= sigma
    rs = np.random.RandomState(seed * 1000 + sigma)
    pool = np.array([(0x80 + k // 2) if k % 2 else k // 2 for k in range(256)], dtype=np.uint8)
    assert np.unique(pool).size == 256
    letters = pool[:sigma]
    T = letters[rs.randint(0, sigma, size=n)]
    T[rs.permutation(n)[:sigma]] = letters                  # every letter at least once
    return T
