"""Rate of the Burrows-Wheeler transform output at C3 (include/caps_sa_hip.h caps_sa_hip_bwt_device_* / caps_sa_hip_build_bwt_*).

    python tools/bwt_rate.py [--runs 5] [--host-runs 7] [--other-lib PATH] [--out profiles/bwt_rate_c3.json]

1. C3 = gen_rand_seq 42 3e9 + the remapped trailing newline (n = 3,000,000,001, as bench.py builds it), built with build_device
   (a warm-up build first: the time quoted is the second);
2. bwt_device over the whole SA: warm-up + --runs timed runs (HIP events), median / min / max ms and GB/s of bytes moved
   (4n SA read + n BWT written + n text bytes gathered);
3. the baseline in the same process: a chunked torch gather T[(SA + n - 1) % n], timed the same way;
4. the host path: build() against build_bwt() (page-locked result arrays, host wall clock): one warm-up of each, then --host-runs
   rounds of (build, build_bwt) interleaved; every run is listed with its device time and its copy tail (ms_d2h).
   --other-lib: the same block again with another build of the library (a measurement variant, e.g. the host path gathering from
   the raw text: docs/r06_bwt_host_path_from_raw_text.patch), after the first library's device memory is released.
Prints one JSON object (and writes it to --out).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _summary(ms, bytes_moved):
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs_ms": [round(x, 3) for x in ms],
            "GBps_median": round(bytes_moved / (med * 1e-3) / 1e9, 1)}


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
    ap.add_argument("--host-runs", type=int, default=7)
    ap.add_argument("--other-lib", default="", help="another build of the library, timed the same way (measurement only)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import caps_sa_amd
    from bench import make_text
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    T = make_text(torch, 3_000_000_000, 42, dev, "uniform")
    n = T.numel()
    SA = torch.empty(n, dtype=torch.int32, device=dev)
    LCP = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)          # warm-up
    st = L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
    del LCP
    torch.cuda.empty_cache()
    BWT = torch.empty(n, dtype=torch.uint8, device=dev)
    res = {"n": n, "device": torch.cuda.get_device_name(0), "build_device_ms": round(st["ms_total"], 3)}
    moved = 4 * n + n + n
    primary = []
    bwt_ms = _timed(torch, lambda: primary.append(L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, BWT.data_ptr())), a.runs)
    res["bwt_device"] = _summary(bwt_ms, moved)
    res["bwt_device"]["gather_source"] = "raw text (n bytes; the host path's slices gather from the packed text)"
    res["primary"] = primary[-1]

    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    step = 1 << 28

    def torch_gather():
        for o in range(0, n, step):
            s = SA[o:o + step].to(torch.int64) & 0xFFFFFFFF          # (u32 entries held in int32)
            ref[o:o + step] = T[(s + (n - 1)) % n]
    tg_ms = _timed(torch, torch_gather, a.runs)
    res["torch_gather"] = _summary(tg_ms, moved)
    res["speedup_vs_torch_gather"] = round(statistics.median(tg_ms) / statistics.median(bwt_ms), 2)
    res["bwt_equals_torch_gather"] = bool(torch.equal(BWT, ref))
    zero = [o + int(z[0, 0]) for o in range(0, n, step) for z in [torch.nonzero(SA[o:o + step] == 0)] if z.numel()]
    res["primary_check"] = zero == [res["primary"]]
    Th = T.cpu().numpy()
    bwt_ref = BWT.cpu().numpy()
    del SA, BWT, ref, T
    torch.cuda.empty_cache()

    # ---- the host path: build() vs build_bwt(), page-locked results re-used between the calls
    hSA = L.pinned_empty(n, "uint32")
    hLCP = L.pinned_empty(n, "uint32")
    hBWT = L.pinned_empty(n, "uint8")
    pr = ctypes.c_uint64(0)

    def host(lib, bwt):
        s = caps_sa_amd.Stats()
        t0 = time.perf_counter()
        if bwt:
            rc = lib._f("build_bwt_u32")(Th.ctypes.data, n, 8000, 0, hSA.ctypes.data, hLCP.ctypes.data, hBWT.ctypes.data, ctypes.byref(pr),
                                         0, ctypes.byref(s))
        else:
            rc = lib._f("build_u32")(Th.ctypes.data, n, 8000, 0, hSA.ctypes.data, hLCP.ctypes.data, 0, ctypes.byref(s))
        ms = (time.perf_counter() - t0) * 1e3
        lib._check(rc)
        return {"wall_ms": round(ms, 1), "ms_total": round(s.ms_total, 2), "ms_d2h": round(s.ms_d2h, 1), "result_waves": s.result_waves,
                "lcp_bytes_on_link": s.lcp_bytes_on_link}

    def host_block(lib):
        host(lib, True)                                    # warm-ups: the device block grows to build_bwt's size once
        host(lib, False)
        runs = {"build": [], "build_bwt": []}
        for _ in range(a.host_runs):                       # interleaved: both kinds see the same state of the box
            runs["build"].append(host(lib, False))
            runs["build_bwt"].append(host(lib, True))
        blk = {}
        for k, v in runs.items():
            ms = [r["wall_ms"] for r in v]
            blk[k] = {"median_ms": round(statistics.median(ms), 1), "min_ms": min(ms), "max_ms": max(ms), "runs": v}
        blk["build_bwt_minus_build_ms"] = round(blk["build_bwt"]["median_ms"] - blk["build"]["median_ms"], 1)
        blk["primary_matches"] = pr.value == res["primary"]
        blk["bwt_matches_device_gather"] = bool(np.array_equal(hBWT, bwt_ref))
        lib.release_cache()
        return blk
    res["host"] = host_block(L)
    if a.other_lib:
        res["host_other_lib"] = host_block(caps_sa_amd.CapsLib(a.other_lib, "caps_sa_hip_"))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
