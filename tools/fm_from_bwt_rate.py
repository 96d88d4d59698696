"""Time of the FM-index built from the BWT alone at C3 and g3r (include/caps_sa_hip.h caps_sa_hip_fm_build_from_bwt_device_*).

    python tools/fm_from_bwt_rate.py [--warm 3] [--runs 10] [--kinds uniform,genome+r] [--out profiles/fm_from_bwt_rate_c3.json]

For each text kind (bench.make_text: "uniform" is C3, "genome+r" is g3r's repeat-rich genome; 3e9 bases + the trailing 'C'), in ONE
process, HIP events around the calls, --warm warm-up runs + --runs timed ones of each route, the two routes alternating:
1. build_device (u32) and bwt_device: the input (BWT, primary), and the reference blob fm_build_device(BWT, primary, SA, s = 32);
2. the NEW route: fm_build_from_bwt_device_u32 on a caller's workspace -- two walks of n + 1 dependent LF steps, one 64-byte Occ
   block each; after every run the blob is compared with the reference (torch.equal);
3. the YARDSTICK, the only route to the same blob from the same input without the new call: inverse_bwt_device, then build_device,
   then fm_build_device with the SA, on caller's workspaces -- timed as one window and call by call; its blob is compared too;
4. the device bytes each route needs beside its input (summed buffer sizes: outputs and workspaces alive at the route's peak) and
   torch.cuda.max_memory_allocated over the timed runs of each (the workspaces are torch tensors).
Prints one JSON object (and writes it to --out).  --only new|yardstick: one route alone, for a kernel trace of its own.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kinds", default="uniform,genome+r")
    ap.add_argument("--n-bases", type=int, default=3_000_000_000)
    ap.add_argument("--sa-sample", type=int, default=32)
    ap.add_argument("--only", default="", choices=["", "new", "yardstick"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import caps_sa_amd
    from bench import make_text
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    s, P = a.sa_sample, 8000
    res = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": a.runs, "sa_sample": s, "measured_on": "MI355X (this run)"}

    def u8(nbytes):
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for kind in a.kinds.split(","):
        T = make_text(torch, a.n_bases, 42, dev, kind)
        n = T.numel()
        SA = torch.empty(n, dtype=torch.int32, device=dev)
        LCP = torch.empty(n, dtype=torch.int32, device=dev)
        B = u8(n)
        torch.cuda.synchronize()
        L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=P)
        p = L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, B.data_ptr())
        nb = L.fm_index_bytes(n, s, 32)
        ref = u8(nb)
        L.fm_build_device(B.data_ptr(), n, p, SA.data_ptr(), s, ref.data_ptr(), nb)
        del T, SA, LCP
        torch.cuda.empty_cache()
        r = {"n": n, "index_bytes": nb, "bwt_bytes": n}

        # the new route: index + workspace
        ws_new_bytes = L.fm_from_bwt_workspace_bytes(n, s, 32)
        r["new_workspace_bytes"] = ws_new_bytes
        r["new_workspace_bound_bytes"] = ((n - 1) // s + 1) * 4 + 32 * (n // 64 + 1) + 2**20
        r["new_route_device_bytes"] = nb + ws_new_bytes
        # the yardstick: the text, the inverse's workspace (freed before the build), SA + LCP + the build's workspace, the index
        ws_inv_bytes = L.inverse_bwt_workspace_bytes(n, 32)
        ws_build_bytes = L.workspace_bytes(n, P, 32)
        r["yardstick_buffers_bytes"] = {"T": n, "inverse_workspace": ws_inv_bytes, "SA": 4 * n, "LCP": 4 * n, "build_workspace": ws_build_bytes,
                                        "index": nb}
        r["yardstick_route_device_bytes"] = max(n + ws_inv_bytes, n + 8 * n + ws_build_bytes, 4 * n + nb)
        base_alloc = torch.cuda.memory_allocated()
        new_ms, yard_ms, parts = [], [], {"inverse_bwt_device": [], "build_device": [], "fm_build_device": []}
        equal = {"new": [], "yardstick": []}
        peak = {"new": 0, "yardstick": 0}

        def run_new(timed):
            torch.cuda.reset_peak_memory_stats()
            index, ws = u8(nb), u8(ws_new_bytes)
            index.fill_(0xA5)
            torch.cuda.synchronize()
            ms = window(lambda: L.fm_build_from_bwt_device(B.data_ptr(), n, p, s, index.data_ptr(), nb, ws.data_ptr(), ws_new_bytes))
            equal["new"].append(bool(torch.equal(index, ref)))
            if timed:
                new_ms.append(ms)
                peak["new"] = max(peak["new"], torch.cuda.max_memory_allocated() - base_alloc)

        def run_yardstick(timed):
            torch.cuda.reset_peak_memory_stats()
            T2, ws_inv = u8(n), u8(ws_inv_bytes)
            torch.cuda.synchronize()
            t_inv = window(lambda: L.inverse_bwt_device(B.data_ptr(), n, p, T2.data_ptr(), ws_inv.data_ptr(), ws_inv_bytes, idx_bits=32))
            del ws_inv
            SA2 = torch.empty(n, dtype=torch.int32, device=dev)
            LCP2 = torch.empty(n, dtype=torch.int32, device=dev)
            ws_b = u8(ws_build_bytes)
            torch.cuda.synchronize()
            t_build = window(lambda: L.build_device(T2.data_ptr(), n, SA2.data_ptr(), LCP2.data_ptr(), p=P, workspace_ptr=ws_b.data_ptr(),
                                                    workspace_bytes=ws_build_bytes))
            del ws_b, LCP2, T2
            index = u8(nb)
            index.fill_(0xA5)
            torch.cuda.synchronize()
            t_fm = window(lambda: L.fm_build_device(B.data_ptr(), n, p, SA2.data_ptr(), s, index.data_ptr(), nb))
            equal["yardstick"].append(bool(torch.equal(index, ref)))
            if timed:
                yard_ms.append(t_inv + t_build + t_fm)
                for k, v in zip(parts, (t_inv, t_build, t_fm)):
                    parts[k].append(v)
                peak["yardstick"] = max(peak["yardstick"], torch.cuda.max_memory_allocated() - base_alloc)
            del SA2, index
            torch.cuda.empty_cache()

        for i in range(a.warm + a.runs):                     # the two routes alternate
            if a.only != "yardstick":
                run_new(i >= a.warm)
            if a.only != "new":
                run_yardstick(i >= a.warm)
        if new_ms:
            r["fm_build_from_bwt_device"] = _summary(new_ms)
            r["fm_build_from_bwt_device"]["all_equal_to_fm_build_device"] = all(equal["new"])
            r["fm_build_from_bwt_device"]["ns_per_row"] = round(r["fm_build_from_bwt_device"]["median_ms"] * 1e6 / (n + 1), 4)
            r["new_route_peak_allocated_bytes"] = peak["new"]
        if yard_ms:
            r["yardstick_inverse_build_fm_build"] = _summary(yard_ms)
            r["yardstick_inverse_build_fm_build"]["all_equal_to_fm_build_device"] = all(equal["yardstick"])
            for k, v in parts.items():
                r["yardstick_" + k] = _summary(v)
            r["yardstick_route_peak_allocated_bytes"] = peak["yardstick"]
        if new_ms and yard_ms:
            r["new_over_yardstick"] = round(r["fm_build_from_bwt_device"]["median_ms"] / r["yardstick_inverse_build_fm_build"]["median_ms"], 3)
        del B, ref
        torch.cuda.empty_cache()
        res["c3" if kind == "uniform" else ("g3r" if kind == "genome+r" else kind)] = r
        print(f"{kind}: done", file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
