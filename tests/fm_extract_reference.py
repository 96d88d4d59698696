"""An independent encoder of format version 2 of the FM-index blob (numpy only), written from the format table of
include/caps_sa_hip.h ("FM-index: extract"): a version-1 blob with samples plus rowof[], the row of the suffix at every t-th text
position.  rowof comes from the naive inverse of the suffix array (fm_reference.naive_sa or any SA the caller trusts), never from the
library.  It also holds what the extract tests share: the ranges on the edges of the chunks and the packing of a batch."""
import numpy as np

import fm_reference as R

VERSION2 = 2


def _up64(b):
    return (b + 63) // 64 * 64


def add_text_samples(blob_v1, SA, t):
    """The version-2 bytes of the version-1 blob `blob_v1` (np.uint8, with samples) of the text whose suffix array is SA."""
    blob_v1 = np.ascontiguousarray(blob_v1, dtype=np.uint8)
    h = blob_v1[:256].view("<u8").copy()
    assert int(h[0]) == R.MAGIC and int(h[1]) == R.VERSION
    n, W, s, end_v1 = int(h[2]), int(h[4]), int(h[12]), int(h[18])
    assert s >= 1 and t >= s and t <= 1024 and t & (t - 1) == 0 and blob_v1.size == end_v1 and len(SA) == n
    m = (n - 1) // t + 1 if n else 0
    total = end_v1 + _up64(m * W)
    out = np.zeros(total, dtype=np.uint8)
    out[:end_v1] = blob_v1
    if n:
        SA = np.asarray(SA).astype(np.int64)
        rank = np.empty(n, dtype=np.int64)           # the naive inverse: rank[SA[k]] = k
        rank[SA] = np.arange(n, dtype=np.int64)
        rowof = rank[np.arange(m, dtype=np.int64) * t] + 1
        assert rowof[0] == int(h[3]) + 1
        out[end_v1:end_v1 + m * W] = rowof.astype("<u4" if W == 4 else "<u8").view(np.uint8)
    h[1], h[19], h[20], h[21], h[22] = VERSION2, t, m, end_v1, total
    assert not h[23:].any()
    out[:256] = h.view(np.uint8)
    return out


# the (s, t) pairs of the sweeps
DISTANCES = ((1, 1), (1, 1024), (32, 32), (32, 64), (32, 1024), (1024, 1024))


def chunk_edge_sizes(t, ks=(1, 2)):
    """n = k t - 1, k t, k t + 1."""
    return sorted({n for k in ks for n in (k * t - 1, k * t, k * t + 1) if n >= 1})


def edge_ranges(n, t):
    """(start, length) pairs on the edges of the chunks of t positions: starts at 0, k t - 1, k t, k t + 1 and n - 1; lengths 0, 1,
    t - 1, t, t + 1, 2 t + 1 and up to n - start (the last chunk then starts at row 0)."""
    starts = {0, n - 1}
    for k in (1, 2, (n - 1) // t):
        starts |= {k * t - 1, k * t, k * t + 1}
    out = []
    for a in sorted(x for x in starts if 0 <= x < n):
        for ln in sorted({0, 1, t - 1, t, t + 1, 2 * t + 1, n - a}):
            if 0 <= ln <= n - a:
                out.append((a, ln))
    out.append((n, 0))                                # the empty range at the text's end
    return out


def pack(ranges):
    """(starts u64[q], out_off u64[q + 1]) of a batch, the ranges back to back."""
    starts = np.array([a for a, _ in ranges], dtype=np.uint64)
    off = np.zeros(len(ranges) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([ln for _, ln in ranges], dtype=np.uint64)
    return starts, off


def expected(T, ranges):
    """The bytes of the batch: the text itself."""
    T = np.ascontiguousarray(T, dtype=np.uint8)
    parts = [T[a:a + ln] for a, ln in ranges]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
