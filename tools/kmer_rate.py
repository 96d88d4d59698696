"""Rates of the k-mer calls at C3 and g3r (include/caps_sa_hip.h "k-mers from SA and LCP", caps_sa_hip_kmer*_device_u32).

    python tools/kmer_rate.py [--warm 3] [--runs 10] [--kinds uniform,genome+r] [--out profiles/kmer_rate_c3.json]

For each text kind (bench.make_text: "uniform" is C3, "genome+r" is g3r's repeat-rich genome; 3e9 bases + the trailing 'C'): one
build_device (u32), SA and LCP stay resident; then, HIP-event timed, --warm warm-up runs + --runs timed ones, median / min / max ms:
1. kmer_spectrum at k = 31 (1024 bins);
2. kmers at k = 31 with min_count = 2: the counting call, and the writing call into a buffer of exactly that many records;
3. kmer_census with max_k = 64;
4. the yardstick, NOT the code under test: R = torch.count_nonzero(dLCP < k) on the same tensor.
GATES (derived from bytes moved): spectrum <= 2.5 x R and census <= 2.5 x R.
Every answer is checked exactly in the run against torch on the device: the heads are nonzero(LCP < k) with rank 0, the counts their
differences, the valid ones those with SA <= n - k; the spectrum is their bincount, the table the ones with count >= 2 (first, count,
pos compared with torch.equal), distinct / unique of the census at k = 1, 31 and 64 their numbers (in chunks of 2^30 ranks).  Prints one JSON object (and
writes it to --out).  Needs no network and no file but this repository's.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


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


CHUNK = 1 << 30                                        # ranks per torch call of the checks (index arithmetic below 2^31 elements)


def truth(torch, SA, LCP, n, k, bins, rec=None, min_count=2):
    """By the definitions, with torch on the device, in chunks from the last rank down (a chunk's last run ends at the first head of
    the chunk behind it): -> (hist np.uint64[bins + 1], the k-mers with count >= min_count, rec holds exactly them)."""
    import numpy as np
    hist = torch.zeros(bins + 1, dtype=torch.int64, device=SA.device)
    nxt, taken, same = n, 0, True
    for a in reversed(range(0, n, CHUNK)):
        head = LCP[a:a + CHUNK] < k
        if a == 0:
            head[0] = True
        first = torch.nonzero(head).view(-1) + a
        del head
        if first.numel() == 0:
            continue
        count = torch.diff(first, append=torch.tensor([nxt], dtype=first.dtype, device=first.device))
        nxt = int(first[0])
        pos = SA[first].to(torch.int64) & 0xFFFFFFFF
        ok = pos <= n - k
        first, count, pos = first[ok], count[ok], pos[ok]
        hist += torch.bincount(count.clamp(max=bins), minlength=bins + 1)
        sel = count >= min_count
        m = int(sel.sum())
        if rec is not None and m:
            lo = rec.shape[0] - taken - m
            same = same and lo >= 0 and bool(torch.equal(rec[lo:lo + m], torch.stack([first[sel], count[sel], pos[sel]], dim=1)))
        taken += m
        del first, count, pos, ok, sel
        torch.cuda.empty_cache()
    return hist.cpu().numpy().astype(np.uint64), taken, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kinds", default="uniform,genome+r")
    ap.add_argument("--n-bases", type=int, default=3_000_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--max-k", type=int, default=64)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import caps_sa_amd
    from bench import make_text
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": a.runs, "measured_on": "MI355X (this run)", "k": a.k,
           "max_k": a.max_k, "gate_factor": 2.5}
    k, bins = a.k, 1024
    for kind in a.kinds.split(","):
        T = make_text(torch, a.n_bases, 42, dev, kind)
        n = T.numel()
        SA = torch.empty(n, dtype=torch.int32, device=dev)
        LCP = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
        del T
        torch.cuda.empty_cache()
        print(f"{kind}: built, n = {n}", file=sys.stderr, flush=True)
        wsb = L.kmer_workspace_bytes(n, 32)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        S, Lp, W = SA.data_ptr(), LCP.data_ptr(), ws.data_ptr()
        r = {"n": n, "workspace_bytes": wsb}
        got = {}
        r["yardstick_count_nonzero"] = _summary(_timed(torch, lambda: got.__setitem__("R", torch.count_nonzero(LCP < k)), a.warm, a.runs))
        r["kmer_spectrum"] = _summary(_timed(torch, lambda: got.__setitem__("hist", L.kmer_spectrum_device(S, Lp, n, k, bins, W, wsb)), a.warm, a.runs))
        r["kmers_count_min2"] = _summary(_timed(torch, lambda: got.__setitem__("found", L.kmers_device(S, Lp, n, k, 2, 0, 0, 0, W, wsb)), a.warm, a.runs))
        found = got["found"]
        rec = torch.empty((max(found, 1), 3), dtype=torch.int64, device=dev)
        r["kmers_write_min2"] = _summary(_timed(torch, lambda: L.kmers_device(S, Lp, n, k, 2, 0, rec.data_ptr(), found, W, wsb), a.warm, a.runs))
        r["kmers_write_min2"]["records"] = found
        r["kmer_census"] = _summary(_timed(torch, lambda: got.__setitem__("census", L.kmer_census_device(S, Lp, n, a.max_k, W, wsb)), a.warm, a.runs))
        print(f"{kind}: timed, checking", file=sys.stderr, flush=True)
        R = r["yardstick_count_nonzero"]["median_ms"]
        r["spectrum_over_yardstick"] = round(r["kmer_spectrum"]["median_ms"] / R, 3)
        r["census_over_yardstick"] = round(r["kmer_census"]["median_ms"] / R, 3)
        r["gate_spectrum"] = r["kmer_spectrum"]["median_ms"] <= 2.5 * R
        r["gate_census"] = r["kmer_census"]["median_ms"] <= 2.5 * R
        # exact checks
        hist = got["hist"]
        r["distinct"], r["unique"] = int(hist.sum()), int(hist[1])
        want_hist, want_found, same = truth(torch, SA, LCP, n, k, bins, rec[:found], 2)
        ok_spec = bool(np.array_equal(hist, want_hist))
        ok_table = found == want_found and same
        distinct, unique = got["census"]
        ok_census = int(distinct[k]) == int(want_hist.sum()) and int(unique[k]) == int(want_hist[1])
        for kk in (1, a.max_k):
            h2, _, _ = truth(torch, SA, LCP, n, kk, 2)
            ok_census = ok_census and int(distinct[kk]) == int(h2.sum()) and int(unique[kk]) == int(h2[1])
        r["all_exact"] = {"spectrum": ok_spec, "table": bool(ok_table), "census": bool(ok_census)}
        del SA, LCP, ws, rec
        torch.cuda.empty_cache()
        res["c3" if kind == "uniform" else ("g3r" if kind == "genome+r" else kind)] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
