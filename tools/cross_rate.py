"""Rates of the MUM / MEM calls between two texts (include/caps_sa_hip.h "MUMs and MEMs between two texts", caps_sa_hip_cross_*_device_u32).

    python tools/cross_rate.py [--warm 2] [--runs 7] [--n-bases 1500000000] [--out profiles/cross_rate_c3.json]

T = A . 0xFF . B: A = --n-bases bases of the bench's generator stream (bench.make_text "uniform"), B = A with one substitution per 100
bases (block i of 100 bases: the base at offset (i * 6364136223846793005 + 1442695040888963407 mod 2^64) >> 33 mod 100 becomes the next
letter of ACGT).  One build_device (u32) and one bwt_device; SA, LCP and BWT stay resident.  Then, HIP-event timed, --warm warm-up runs
+ --runs timed ones, median / min / max ms:
1. cross_mums at min_len = 20: the counting call, and the writing call into a buffer of exactly that many records;
2. cross_mems at min_len = 20, max_occ = 8: the same two calls (reported beside the MUM mode's, with records and skipped runs; no gate);
3. the yardstick, NOT the code under test: R = torch.count_nonzero(dLCP < 20) on the same tensor in the same process.
GATE: the MUM counting call takes at most (2 W + 1) / W = 2.25 x R at W = 4 -- the bytes the rule may touch (SA, LCP, BWT) over the
bytes the yardstick reads (LCP); no margin on top.
Checked exactly in the same run, on the device: the MUM records equal torch.nonzero of the rank rule written in tensor ops (in chunks
of 2^30 ranks), and every record of both modes passes the text test -- bytes equal over len, different or at an end just beyond, left
bytes different or at a start, a on side A and b on side B.  Prints one JSON object (and writes it to --out).  Needs no network and no
file but this repository's.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHUNK = 1 << 30                                        # ranks per torch call of the checks (index arithmetic below 2^31 elements)
MIN_LEN, MAX_OCC = 20, 8


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs_ms": [round(x, 3) for x in ms]}


def _timed(torch, fn, warm, runs):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def two_texts(torch, n_bases, dev):
    """(T, split): A . 0xFF . B on the device."""
    from bench import make_text
    A = make_text(torch, n_bases, 42, dev, "uniform")[:n_bases]
    T = torch.empty(2 * n_bases + 1, dtype=torch.uint8, device=dev)
    T[:n_bases] = A
    T[n_bases] = 0xFF
    B = T[n_bases + 1:]
    B.copy_(A)
    del A
    nxt = torch.arange(256, dtype=torch.uint8, device=dev)
    for a, b in zip(b"ACGT", b"CGTA"):
        nxt[a] = b
    blocks = n_bases // 100
    step = 1 << 26
    for o in range(0, blocks, step):
        i = torch.arange(o, min(o + step, blocks), dtype=torch.int64, device=dev)
        x = ((i * 6364136223846793005 + 1442695040888963407) >> 33) & 0x7FFFFFFF       # (int64 arithmetic wraps: mod 2^64)
        at = i * 100 + x % 100
        B[at] = nxt[B[at].long()]
    return T, n_bases + 1


def mum_rule(torch, SA, LCP, BWT, n, split, min_len):
    """The ranks the MUM rule accepts, by the header's four conditions in tensor ops, in chunks -> int64 tensor of ranks, ascending."""
    out = []
    for a in range(0, n, CHUNK):
        b = min(a + CHUNK, n)
        m = b - a

        def padded(X, wide):
            """X[a - 1 : b + 1] with a zero where the array ends: index i is rank a - 1 + i."""
            mid = X[max(a - 1, 0):min(b + 1, n)]
            mid = (mid.to(torch.int64) & 0xFFFFFFFF) if wide else mid
            zero = torch.zeros(1, dtype=mid.dtype, device=mid.device)
            return torch.cat(([zero] if a == 0 else []) + [mid] + ([zero] if b == n else []))

        L = padded(LCP, True)
        if a == 0:
            L[1] = 0                                    # LCP[0] counts as 0
        cur, prev, nxt = L[1:1 + m], L[0:m], L[2:2 + m]
        ok = (cur >= min_len) & (prev < cur) & (nxt < cur)
        del L, cur, prev, nxt
        S = padded(SA, True)
        sp, sq = S[0:m], S[1:1 + m]
        ok &= (sp >= split) != (sq >= split)
        Bw = padded(BWT, False)
        ok &= (sp == 0) | (sq == 0) | (Bw[0:m] != Bw[1:1 + m])
        if a == 0:
            ok[0] = False                               # rank 0 has no rank before it
        out.append(torch.nonzero(ok).view(-1) + a)
        del S, sp, sq, Bw, ok
        torch.cuda.empty_cache()
    return torch.cat(out)


def text_test(torch, T, rec, n, split):
    """Every record (a, b, len): a < split <= b, T[a : a + len] == T[b : b + len], maximal to the right and to the left."""
    if rec.shape[0] == 0:
        return True
    a, b, ln = rec[:, 0], rec[:, 1], rec[:, 2]
    ok = bool(((a < split) & (b >= split) & (ln >= 1) & (b + ln <= n) & (a + ln <= n)).all())
    if not ok:
        return False
    idx = torch.arange(rec.shape[0], device=rec.device)
    j = 0
    while idx.numel():                                  # position j of every match that is longer than j
        if not bool((T[a[idx] + j] == T[b[idx] + j]).all()):
            return False
        j += 1
        idx = idx[ln[idx] > j]
    end = (b + ln == n) | (a + ln == n)
    right = end | (T[(a + ln).clamp(max=n - 1)] != T[(b + ln).clamp(max=n - 1)])
    left = (a == 0) | (T[(a - 1).clamp(min=0)] != T[b - 1])
    return bool(right.all()) and bool(left.all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--n-bases", type=int, default=1_500_000_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import caps_sa_amd
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    T, split = two_texts(torch, a.n_bases, dev)
    n = T.numel()
    SA = torch.empty(n, dtype=torch.int32, device=dev)
    LCP = torch.empty(n, dtype=torch.int32, device=dev)
    BWT = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
    L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, BWT.data_ptr())
    print(f"built, n = {n}, split = {split}", file=sys.stderr, flush=True)
    wsb = L.cross_workspace_bytes(n, 32)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    S, Lp, Bp, W = SA.data_ptr(), LCP.data_ptr(), BWT.data_ptr(), ws.data_ptr()
    res = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": a.runs, "measured_on": "MI355X (this run)", "n": n, "split": split,
           "min_len": MIN_LEN, "max_occ": MAX_OCC, "workspace_bytes": wsb, "gate_factor": 2.25}
    got = {}
    res["yardstick_count_nonzero"] = _summary(_timed(torch, lambda: got.__setitem__("R", torch.count_nonzero(LCP < MIN_LEN)), a.warm, a.runs))
    recs = {}
    for which, occ in (("mums", MAX_OCC), ("mems", MAX_OCC)):
        count = lambda: got.__setitem__(which, L.cross_device(which, S, Lp, Bp, n, split, MIN_LEN, occ, 0, 0, W, wsb))
        res[f"{which}_count"] = _summary(_timed(torch, count, a.warm, a.runs))
        summary = got[which]
        found = int(summary[0])
        rec = torch.empty((max(found, 1), 3), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        write = lambda: L.cross_device(which, S, Lp, Bp, n, split, MIN_LEN, occ, rec.data_ptr(), found, W, wsb)
        res[f"{which}_write"] = _summary(_timed(torch, write, a.warm, a.runs))
        res[f"{which}_write"].update(records=found, skipped_runs=int(summary[1]), lcs=[int(x) for x in summary[2:5]])
        recs[which] = rec[:found]
    print("timed, checking", file=sys.stderr, flush=True)
    R = res["yardstick_count_nonzero"]["median_ms"]
    res["mums_count_over_yardstick"] = round(res["mums_count"]["median_ms"] / R, 3)
    res["mems_count_over_yardstick"] = round(res["mems_count"]["median_ms"] / R, 3)
    res["gate_mums_count"] = res["mums_count"]["median_ms"] <= 2.25 * R
    # exact checks
    ranks = mum_rule(torch, SA, LCP, BWT, n, split, MIN_LEN)
    rec = recs["mums"]
    same = ranks.numel() == rec.shape[0]
    if same and rec.shape[0]:
        sp = SA[ranks - 1].to(torch.int64) & 0xFFFFFFFF
        sq = SA[ranks].to(torch.int64) & 0xFFFFFFFF
        want = torch.stack([torch.minimum(sp, sq), torch.maximum(sp, sq), LCP[ranks].to(torch.int64) & 0xFFFFFFFF], dim=1)
        same = bool(torch.equal(rec, want))
    res["all_exact"] = {"mums_equal_torch_nonzero_of_the_rule": bool(same),
                        "mums_pass_the_text_test": text_test(torch, T, recs["mums"], n, split),
                        "mems_pass_the_text_test": text_test(torch, T, recs["mems"], n, split)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
