"""The arithmetic of the slot keys (csrc/kernels.h "slot keys") in plain Python, shared by test_slot_keys_model.py and slot_keys_cases.py:
copies of make_bucket_params / bucket_of (the linear map of a group onto its buckets) and of the double-precision nominal lower end
of a bucket that bucket_ranges_kernel hands to the tile sort, and -- written once, from the comment above slot_key_shift in
kernels.h -- the shift rule, the base rule and the reconstruction of a key."""

M64 = (1 << 64) - 1


def clz64(x):
    return 64 - x.bit_length()


def make_bucket_params(kmin, kmax, B):
    """kernels.h make_bucket_params."""
    rng = kmax - kmin if kmax > kmin else 0
    shift = clz64(rng) if rng else 0
    r32 = ((rng << shift) & M64) >> 32
    bits = 1
    while (2 * B) >> bits:
        bits += 1
    post = 32 - bits if bits < 32 else 0
    m = ((B << (32 + post)) // (r32 + 1)) & 0xFFFFFFFF if rng else 0
    return dict(kmin=kmin, range=rng, shift=shift, B=B, post=post, m=m)


def bucket_of(bp, key):
    """kernels.h bucket_of."""
    if bp["B"] <= 1 or key <= bp["kmin"]:
        return 0
    d = key - bp["kmin"]
    if d >= bp["range"]:
        return bp["B"] - 1
    d32 = ((d << bp["shift"]) & M64) >> 32
    b = ((d32 * bp["m"]) >> 32) >> bp["post"]
    return b if b < bp["B"] else bp["B"] - 1


def nominal_lower_end(kmin, kmax, B, bk):
    """kernels.h bucket_ranges_kernel (the plain split): l of bucket bk, in double precision as there."""
    range1 = float(kmax - kmin) + 1.0
    return kmin + int(float(bk) / float(B) * range1) if bk > 0 else kmin


# ---- the two rules, written once from the comment above slot_key_shift in kernels.h ----
def slot_key_shift(rng, B):
    """s = max(0, bitlength(W) - 30), W = range / B + 1."""
    W = rng // B + 1
    return max(0, W.bit_length() - 30)


def slot_key_base(l, s):
    """base = max(0, l - 2^(30 + s)); 0 when 30 + s >= 64."""
    if 30 + s >= 64:
        return 0
    return max(0, l - (1 << (30 + s)))


def slot_key_restore(base, s, r):
    bs = base >> s
    return (bs + ((r - (bs & 0xFFFFFFFF)) & 0xFFFFFFFF)) << s
