"""Rate of the inverse Burrows-Wheeler transform at C3 (include/caps_sa_hip.h caps_sa_hip_inverse_bwt_device_* / _inverse_bwt_*).

    python tools/inverse_bwt_rate.py [--runs 5] [--kinds uniform,genome+r] [--out profiles/inverse_bwt_rate_c3.json]

For each text kind (bench.make_text: "uniform" is C3, "genome+r" is g3r's repeat-rich genome; 3e9 bases + the trailing 'C'):
1. build_device (u32) and bwt_device over the whole SA: the input of the inverse;
2. bwt_device timed: warm-up + --runs runs (HIP events), median / min / max ms -- one independent random text load per symbol;
3. inverse_bwt_device_u32 timed the same way: two walks of n + 1 dependent LF loads, plus the LF table;
   every timed output is compared with the text (torch.equal);
4. C3 only: the host path, inverse_bwt_u32 from a pageable BWT into page-locked T (host wall clock): warm-up + --runs runs.
Prints one JSON object (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs_ms": [round(x, 3) for x in ms]}


def _timed(torch, fn, runs):
    fn()                                                   # warm-up
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kinds", default="uniform,genome+r")
    ap.add_argument("--n-bases", type=int, default=3_000_000_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import caps_sa_amd
    from bench import make_text
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "runs": a.runs}
    for kind in a.kinds.split(","):
        T = make_text(torch, a.n_bases, 42, dev, kind)
        n = T.numel()
        SA = torch.empty(n, dtype=torch.int32, device=dev)
        LCP = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
        del LCP
        torch.cuda.empty_cache()
        B = torch.empty(n, dtype=torch.uint8, device=dev)
        primary = []
        r = {"n": n}
        r["bwt_device"] = _summary(_timed(torch, lambda: primary.append(L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, B.data_ptr())),
                                          a.runs))
        del SA
        torch.cuda.empty_cache()
        p = primary[-1]
        ws_bytes = L.inverse_bwt_workspace_bytes(n, 32)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        exact = []

        def inv():
            out.fill_(0)
            a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record()
            L.inverse_bwt_device(B.data_ptr(), n, p, out.data_ptr(), ws.data_ptr(), ws_bytes, idx_bits=32)
            b0.record()
            b0.synchronize()
            exact.append(bool(torch.equal(out, T)))
            return a0.elapsed_time(b0)
        inv()                                              # warm-up
        r["inverse_bwt_device"] = _summary([inv() for _ in range(a.runs)])
        r["inverse_bwt_device"]["exact_runs"] = sum(exact)
        r["inverse_bwt_device"]["all_exact"] = all(exact)
        r["workspace_bytes"] = ws_bytes
        r["inverse_over_bwt_device"] = round(r["inverse_bwt_device"]["median_ms"] / r["bwt_device"]["median_ms"], 2)
        r["ns_per_symbol"] = round(r["inverse_bwt_device"]["median_ms"] * 1e6 / n, 3)
        del ws, out
        torch.cuda.empty_cache()
        if kind == "uniform":
            Bh = B.cpu().numpy()
            Th = T.cpu().numpy()
            del B, T
            torch.cuda.empty_cache()
            hT = L.pinned_empty(n, "uint8")
            f = L._f("inverse_bwt_u32")
            ms = []
            for i in range(a.runs + 1):
                t0 = time.perf_counter()
                L._check(f(Bh.ctypes.data, n, p, hT.ctypes.data, 0))
                if i:
                    ms.append((time.perf_counter() - t0) * 1e3)
            r["host_inverse_bwt_pinned_T"] = _summary(ms)
            r["host_inverse_bwt_pinned_T"]["exact"] = bool((hT == Th).all())
            L.release_cache()
            del Bh, Th, hT
        else:
            del B, T
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
