"""Rates of lpf and lz77 at C3 and g3r (include/caps_sa_hip.h "LPF and LZ77 from SA and LCP", caps_sa_hip_lpf_device_u32,
caps_sa_hip_lz77_device_u32).

    python tools/lz_rate.py [--warm 3] [--runs 10] [--kinds uniform,genome+r] [--out profiles/lz_rate_c3.json]

For each text kind (bench.make_text: "uniform" is C3, "genome+r" is g3r's repeat-rich genome; 3e9 bases + the trailing 'C'): one
build_device (u32), SA and LCP stay resident; then, HIP-event timed, --warm warm-up runs + --runs timed ones, median / min / max ms:
1. the yardstick, NOT the code under test: B = caps_sa_hip_bwt_device_u32 on the same SA;
2. lpf (LPF and Prev);
3. lz77: the counting call, and the writing call into a buffer of exactly z records.
GATE: lpf <= 3 x B on both texts.  lz77 has no gate: its times, z and the length of the single-lane chain (lz_hop_kernel makes one dependent step per group of 64
tiles that the parse enters) are reported; --kernel-times adds the device time of every lpf_* / lz_* kernel of one more lpf and
one more counting call (torch.profiler), and the hop's share of the counting call.
Exactness inside the run: Prev < i wherever LPF > 0 (every entry); at 2^22 sampled positions the bytes agree for all LPF bytes and differ behind
them, or the text ends; 64 windows of 2^16 ranks across tile edges recomputed with the stack
reference on the host -- every rank whose two neighbours lie inside its window must match exactly; the whole parse by torch gathers.
Prints one JSON object (and writes it to --out).  Needs no network and no file but this repository's.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from kmer_rate import _summary, _timed  # noqa: E402

CHUNK = 1 << 29
LZ_TILE = 16384
LZ_GROUP = 64 * LZ_TILE


def u32(t):
    return t.to(__import__("torch").int64) & 0xFFFFFFFF


def check_prev(torch, LPF, Prev, n):
    ok = True
    for a in range(0, n, CHUNK):
        l, p = u32(LPF[a:a + CHUNK]), u32(Prev[a:a + CHUNK])
        i = torch.arange(a, a + l.numel(), device=l.device)
        ok = ok and bool(torch.where(l > 0, (p < i) & (l <= n - i), p == 0xFFFFFFFF).all())
        del l, p, i
    return ok


def check_samples(torch, T, LPF, Prev, n, count=1 << 22, cap=4096):
    """The bytes agree for LPF bytes and differ behind them (or the text ends): offset by offset for the first `cap` bytes of every
    sample, and for the few samples longer than that in blocks of `cap` offsets -> (all agree, samples longer than cap, longest)."""
    g = torch.Generator(device=T.device)
    g.manual_seed(11)
    i = torch.randint(0, n, (count,), device=T.device, generator=g)
    l, p = u32(LPF[i]), u32(Prev[i])
    p = torch.where(l > 0, p, torch.zeros_like(p))
    ok = torch.ones_like(i, dtype=torch.bool)
    for k in range(min(int(l.max()), cap)):
        live = l > k
        ok &= ~live | (T[(i + k).clamp(max=n - 1)] == T[(p + k).clamp(max=n - 1)])
    end = (i + l >= n)
    ok &= (l == 0) | end | (T[(i + l).clamp(max=n - 1)] != T[(p + l).clamp(max=n - 1)])
    all_ok = bool(ok.all())
    big = l > cap
    bi, bp, bl = i[big], p[big], l[big]
    off = torch.arange(cap, device=T.device)
    for a in range(cap, int(l.max()) if bl.numel() else 0, cap):
        k = (a + off)[None, :]
        live = k < bl[:, None]
        same = T[(bi[:, None] + k).clamp(max=n - 1)] == T[(bp[:, None] + k).clamp(max=n - 1)]
        all_ok = all_ok and bool((~live | same).all())
    return all_ok, int(big.sum()), int(l.max())


def check_windows(torch, SA, LCP, LPF, Prev, n, windows=64, size=1 << 16, tile=4096):
    import numpy as np
    import lz_reference as R
    checked, bad = 0, 0
    for w in range(windows):
        edge = ((w + 1) * (n // tile) // (windows + 1)) * tile
        a = max(0, min(edge - size // 2, n - size))
        sa = u32(SA[a:a + size]).cpu().numpy()
        lcp = u32(LCP[a:a + size]).cpu().numpy()
        left, right = R.stack_sides(sa, lcp)
        pos = torch.from_numpy(sa.astype(np.int64)).to(SA.device)
        gl, gp = u32(LPF[pos]).cpu().tolist(), u32(Prev[pos]).cpu().tolist()
        for r in range(size):
            if left[r] is None or right[r] is None:
                continue
            # (a span that ends at a neighbour inside the window never reads the window's LCP[0], which stack_sides counts as 0)
            want = R._pick(left[r], right[r], 0xFFFFFFFF)
            checked += 1
            bad += (gl[r], gp[r]) != want
    return checked, bad


def check_parse(torch, rec, LPF, Prev, n):
    pos, ln, src = rec[:, 0], rec[:, 1], rec[:, 2]
    ok = int(pos[0]) == 0 and bool((pos[1:] == pos[:-1] + ln[:-1]).all()) and int(pos[-1] + ln[-1]) == n
    l = u32(LPF[pos])
    ok = ok and bool((ln == torch.minimum(l.clamp(min=1), n - pos)).all())
    ok = ok and bool(torch.where(l > 0, src == u32(Prev[pos]), src == -1).all())
    return ok


def kernel_times(torch, fn):
    """fn() once under torch.profiler (device activities only) -> {kernel: ms} for the lpf_* / lz_* kernels and fm_scan_kernel."""
    import re
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        m = re.search(r"(lpf_\w+?_kernel|lz_\w+?_kernel|fm_scan_kernel)(<[^>]*>)?", e.key)
        if m:
            us = getattr(e, "device_time_total", None)
            if us is None:
                us = getattr(e, "cuda_time_total", 0.0)
            out[m.group(0)] = round(out.get(m.group(0), 0.0) + us / 1e3, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kinds", default="uniform,genome+r")
    ap.add_argument("--n-bases", type=int, default=3_000_000_000)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-times", action="store_true",
                    help="one more lpf and one more counting lz77 under torch.profiler: device time per lpf_* / lz_* kernel into the JSON")
    a = ap.parse_args()
    import torch
    import caps_sa_amd
    from bench import make_text
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": a.runs, "measured_on": "MI355X (this run)", "gate_factor": 3.0}
    for kind in a.kinds.split(","):
        T = make_text(torch, a.n_bases, 42, dev, kind)
        n = T.numel()
        SA = torch.empty(n, dtype=torch.int32, device=dev)
        LCP = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
        print(f"{kind}: built, n = {n}", file=sys.stderr, flush=True)
        BWT = torch.empty(n, dtype=torch.uint8, device=dev)
        LPF = torch.empty(n, dtype=torch.int32, device=dev)
        Prev = torch.empty(n, dtype=torch.int32, device=dev)
        wl, wz = L.lpf_workspace_bytes(n, 32), L.lz77_workspace_bytes(n, 32)
        ws = torch.empty(max(wl, wz), dtype=torch.uint8, device=dev)
        S, Lp, W, F, P = SA.data_ptr(), LCP.data_ptr(), ws.data_ptr(), LPF.data_ptr(), Prev.data_ptr()
        r = {"n": n, "lpf_workspace_bytes": wl, "lz77_workspace_bytes": wz}
        got = {}
        torch.cuda.synchronize()
        r["yardstick_bwt_device"] = _summary(_timed(torch, lambda: L.bwt_device(T.data_ptr(), n, S, 0, n, BWT.data_ptr()), a.warm, a.runs))
        del BWT
        r["lpf"] = _summary(_timed(torch, lambda: L.lpf_device(S, Lp, n, F, P, W, wl), a.warm, a.runs))
        print(f"{kind}: lpf {r['lpf']['median_ms']} ms, yardstick {r['yardstick_bwt_device']['median_ms']} ms", file=sys.stderr, flush=True)
        r["lz77_count"] = _summary(_timed(torch, lambda: got.__setitem__("z", L.lz77_device(F, P, n, 0, 0, W, wz)), a.warm, a.runs))
        z = got["z"]
        rec = torch.empty((z, 3), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        r["lz77_write"] = _summary(_timed(torch, lambda: L.lz77_device(F, P, n, rec.data_ptr(), z, W, wz), a.warm, a.runs))
        B = r["yardstick_bwt_device"]["median_ms"]
        r["z"] = z
        r["lpf_over_yardstick"] = round(r["lpf"]["median_ms"] / B, 3)
        r["gate_lpf"] = r["lpf"]["median_ms"] <= 3.0 * B
        if a.kernel_times:
            try:
                r["lpf_kernel_ms"] = kernel_times(torch, lambda: L.lpf_device(S, Lp, n, F, P, W, wl))
                r["lz77_count_kernel_ms"] = kernel_times(torch, lambda: L.lz77_device(F, P, n, 0, 0, W, wz))
                hop = r["lz77_count_kernel_ms"].get("lz_hop_kernel<unsigned int>")
                if hop is None:
                    hop = sum(v for k, v in r["lz77_count_kernel_ms"].items() if k.startswith("lz_hop_kernel"))
                r["hop_share_of_counting_call"] = round(hop / r["lz77_count"]["median_ms"], 4)
            except Exception as e:                                                   # the timings above stand without it
                r["kernel_times_error"] = repr(e)
        print(f"{kind}: timed, z = {z}, checking", file=sys.stderr, flush=True)
        first = torch.ones(z, dtype=torch.bool, device=dev)                  # the first phrase that starts in its tile / group
        first[1:] = rec[1:, 0] // LZ_TILE != rec[:-1, 0] // LZ_TILE
        gfirst = first.clone()
        gfirst[1:] = rec[1:, 0] // LZ_GROUP != rec[:-1, 0] // LZ_GROUP
        r["tiles_entered"], r["tiles"] = int(first.sum()), (n + LZ_TILE - 1) // LZ_TILE
        r["groups_entered"], r["groups"] = int(gfirst.sum()), (n + LZ_GROUP - 1) // LZ_GROUP
        # lz_hop_kernel: one dependent step per group entered; an entry at 64 or more positions into its group costs up to 64 loads more
        r["hop_chain_steps"] = r["groups_entered"]
        r["hop_entries_beyond_the_composed_exits"] = int((gfirst & (rec[:, 0] % LZ_GROUP >= 64)).sum())
        r["longest_phrase"] = int(rec[:, 1].max())
        r["literals"] = int((rec[:, 2] == -1).sum())
        ok_s, partial, longest = check_samples(torch, T, LPF, Prev, n)
        checked, bad = check_windows(torch, SA, LCP, LPF, Prev, n)
        r["all_exact"] = {"prev_below_i": check_prev(torch, LPF, Prev, n), "samples": ok_s, "samples_longer_than_4096_bytes": partial,
                          "longest_sampled_lpf": longest, "window_ranks_checked": checked, "window_ranks_wrong": bad,
                          "parse": check_parse(torch, rec, LPF, Prev, n)}
        del T, SA, LCP, LPF, Prev, ws, rec
        torch.cuda.empty_cache()
        res["c3" if kind == "uniform" else ("g3r" if kind == "genome+r" else kind)] = r
        print(json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
