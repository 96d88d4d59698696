"""CPU, no library: the arithmetic of the slot keys (csrc/kernels.h "slot keys": slot_key_shift, slot_key_base, slot_key_restore)
on the plain-Python copy of the maps they ride on (slot_keys_model.py: make_bucket_params / bucket_of, the linear map of a group onto
its buckets, and the double-precision nominal lower end of a bucket that bucket_ranges_kernel hands to the tile sort).

Level B stores r = (uint32_t)(key >> s) per element, one shift s per group; the tile sort takes x = r - (uint32_t)(base >> s) in
32-bit wrap-around arithmetic, base = max(0, l - 2^(30 + s)), l the bucket's nominal lower end.  Checked per bucket, over the keys
that bucket_of really sends there:
  * the keys span less than 2^(31 + s), and every key has 0 <= (k >> s) - (base >> s) < 2^32;
  * x is non-decreasing over the sorted keys (whichever multiple of 2^(32 + s) the bucket straddles);
  * equal x  =>  the top 64 - s bits of the keys are equal (the tie-break may start at (64 - s) / 2 chars);
  * different x  =>  the LCP read off the keys put together again, clz64(ka' ^ kb') / 2, is the one of the 64-bit keys.
Bit-exact: integers only, but for the one double computation the kernel makes."""
import random

import pytest

from slot_keys_model import (M64, bucket_of, clz64, make_bucket_params, nominal_lower_end, slot_key_base, slot_key_restore,
                             slot_key_shift)

BS = (2, 3, 7, 64, 257, 800, 2048)
RANGE_BITS = (20, 21, 27, 31, 32, 33, 40, 44, 45, 52, 53, 59, 63, 64)


def groups(B):
    """(kmin, kmax) of the groups a case checks: ranges of 20 to 64 bits at several places of the key space, the full range
    (kmin = 0 and kmax = 2^64 - 1: what the first and the last group of a text can reach) among them."""
    rs = random.Random(1000 + B)
    out = [(0, M64)]
    for bits in RANGE_BITS:
        rng = (1 << bits) - 1 if bits == 64 else rs.randrange(1 << (bits - 1), 1 << bits)
        out.append((0, rng))                                    # a first group
        out.append((M64 - rng, M64))                            # a last group
        if rng < M64:
            kmin = rs.randrange(0, M64 - rng)                   # ... and one somewhere in between
            out.append((kmin, kmin + rng))
    return out


def keys_of(kmin, kmax, B, s, rs):
    ks = {kmin, min(kmin + 1, kmax), kmax, max(kmax - 1, kmin)}
    rng = kmax - kmin
    for _ in range(1500):
        k = kmin + rs.randrange(0, rng + 1)
        ks.add(k)
        ks.add(min(kmax, k + 1))                                # a neighbour in the low bits (equal x when s > 0)
        ks.add(min(kmax, k + (1 << s)))                         # ... and one that differs in the lowest kept bit
    # one below, on and one above multiples of the window 2^(32 + s), all over the group
    w = 32 + s
    if w < 64:
        first, last = (kmin >> w) + 1, kmax >> w
        cnt = last - first + 1
        picks = range(first, last + 1) if cnt <= 48 else [first + rs.randrange(0, cnt) for _ in range(48)] + [first, last]
        for q in picks:
            for k in ((q << w) - 1, q << w, (q << w) + 1):
                if kmin <= k <= kmax:
                    ks.add(k)
    # the edges of every bucket (B small) or of some (B large): nominal ends, one below and one above
    for bk in (range(B) if B <= 64 else [rs.randrange(0, B) for _ in range(64)] + [0, B - 1]):
        l = nominal_lower_end(kmin, kmax, B, bk)
        for k in (l - 1, l, l + 1):
            if kmin <= k <= kmax:
                ks.add(k)
    return sorted(ks)


@pytest.mark.parametrize("B", BS)
def test_slot_keys_keep_order_and_lcp_in_every_bucket(B):
    rs = random.Random(B)
    wrapped = tied = 0
    for kmin, kmax in groups(B):
        bp = make_bucket_params(kmin, kmax, B)
        s = slot_key_shift(bp["range"], B)
        assert 0 <= s <= 34 and (64 - s) // 2 >= 15, (kmin, kmax, B, s)
        W = bp["range"] // B + 1
        assert (1 << (30 + s)) > W or s == 0 and W <= (1 << 30), (W, s)
        by_bucket = {}
        for k in keys_of(kmin, kmax, B, s, rs):
            by_bucket.setdefault(bucket_of(bp, k), []).append(k)
        assert all(0 <= b < B for b in by_bucket)
        prev_max = -1
        for b in sorted(by_bucket):
            keys = by_bucket[b]                                 # ascending
            assert keys[0] > prev_max, "bucket_of is monotone"
            prev_max = keys[-1]
            l = nominal_lower_end(kmin, kmax, B, b)
            base = slot_key_base(l, s)
            where = (kmin, kmax, B, b, s, l)
            assert keys[-1] - keys[0] < (1 << (31 + s)), where  # (a bucket is about W < 2^(30 + s) wide: the map rounds)
            d = [(k >> s) - (base >> s) for k in keys]
            assert d[0] >= 0 and d[-1] < (1 << 32), (where, d[0], d[-1])
            x = [((k >> s) & 0xFFFFFFFF) - ((base >> s) & 0xFFFFFFFF) & 0xFFFFFFFF for k in keys]     # what the kernel computes
            assert x == d, where
            if 32 + s < 64 and (keys[0] >> (32 + s)) != (keys[-1] >> (32 + s)):
                wrapped += 1
            for i in range(1, len(keys)):
                ka, kb = keys[i - 1], keys[i]
                assert x[i - 1] <= x[i], (where, ka, kb)
                if x[i - 1] == x[i]:
                    tied += 1
                    assert ka >> s == kb >> s, (where, ka, kb)
                else:
                    ra, rb = slot_key_restore(base, s, (ka >> s) & 0xFFFFFFFF), slot_key_restore(base, s, (kb >> s) & 0xFFFFFFFF)
                    assert ra == (ka >> s) << s and rb == (kb >> s) << s, (where, ka, kb)
                    assert clz64(ra ^ rb) // 2 == clz64(ka ^ kb) // 2, (where, ka, kb)
    assert wrapped > 0 and tied > 0, (B, wrapped, tied)        # the corners existed


def test_shift_rule_at_the_sizes_the_documents_quote():
    """C3 (3e9 bases, ~915 groups of ~800 buckets): s = 15, 24 chars kept; a million bases in 20 groups of ~15 buckets: s = 26."""
    assert slot_key_shift(M64 // 915, 800) == 15
    assert slot_key_shift(M64 // 20, 15) in (26, 27)
    assert slot_key_shift(0, 1) == 0 and slot_key_shift(M64, 2) == 34
