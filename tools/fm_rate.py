"""Rates of the FM-index at C3 and g3r (include/caps_sa_hip.h caps_sa_hip_fm_*).

    python tools/fm_rate.py [--warm 3] [--runs 10] [--kinds uniform,genome+r] [--out profiles/fm_rate_c3.json]

For each text kind (bench.make_text: "uniform" is C3, "genome+r" is g3r's repeat-rich genome; 3e9 bases + the trailing 'C'), HIP-event
timed, --warm warm-up runs + --runs timed ones, median / min / max ms:
1. build_device (u32) and bwt_device over the whole SA; bwt_device timed: the gate's other side, in the same process;
2. fm_build_device without SA samples and with them (s = 32).  GATE: the build without samples takes no longer than bwt_device;
3. fm_count_device: 2^22 patterns of length 32 cut from T -> patterns/s and Occ lookups/s (every pattern occurs, so each takes
   2 x 32 lookups); every answer is checked to hold the position the pattern was cut from (through locate, below);
4. fm_locate_device: 2^22 random ranks, one position each -> positions/s and LF steps/s (a walk from text position p takes
   p mod s steps); compared with the SA (torch.equal);
5. the yardstick of both query kernels, NOT the code under test: torch.index_select of 2^26 random rows of a [blocks, 16] int32
   tensor as large as the Occ section (one random 64-byte line per row) -> lines/s; count_lookups_over_yardstick = 3. / 5.
Prints one JSON object (and writes it to --out).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kinds", default="uniform,genome+r")
    ap.add_argument("--n-bases", type=int, default=3_000_000_000)
    ap.add_argument("--queries", type=int, default=1 << 22)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import caps_sa_amd
    from bench import make_text
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": a.runs, "measured_on": "MI355X (this run)"}
    q, m, s = a.queries, 32, 32
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
        r = {"n": n, "sa_sample": s}
        r["bwt_device"] = _summary(_timed(torch, lambda: primary.append(L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, B.data_ptr())),
                                          a.warm, a.runs))
        p = primary[-1]
        nb0, nb = L.fm_index_bytes(n, 0, 32), L.fm_index_bytes(n, s, 32)
        index = torch.empty(nb, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        r["fm_build_no_samples"] = _summary(_timed(torch, lambda: L.fm_build_device(B.data_ptr(), n, p, 0, 0, index.data_ptr(), nb0), a.warm, a.runs))
        r["fm_build_with_samples"] = _summary(_timed(torch, lambda: L.fm_build_device(B.data_ptr(), n, p, SA.data_ptr(), s, index.data_ptr(), nb),
                                                     a.warm, a.runs))
        r["index_bytes_no_samples"], r["index_bytes"] = nb0, nb
        r["bytes_per_base"] = round(nb / n, 4)
        r["build_no_samples_over_bwt_device"] = round(r["fm_build_no_samples"]["median_ms"] / r["bwt_device"]["median_ms"], 3)
        r["gate_build_no_slower_than_bwt_device"] = r["fm_build_no_samples"]["median_ms"] <= r["bwt_device"]["median_ms"]
        del B
        torch.cuda.empty_cache()
        # count: patterns of length m cut from T
        g = torch.Generator(device="cuda")
        g.manual_seed(11)
        starts = torch.randint(0, n - m, (q,), device=dev, generator=g)
        pat = T[starts[:, None] + torch.arange(m, device=dev)].contiguous().view(-1)
        off = torch.arange(q + 1, dtype=torch.int64, device=dev) * m
        first = torch.zeros(q, dtype=torch.int64, device=dev)
        count = torch.zeros(q, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ms = _timed(torch, lambda: L.fm_count_device(index.data_ptr(), nb, pat.data_ptr(), off.data_ptr(), q, first.data_ptr(), count.data_ptr()),
                    a.warm, a.runs)
        r["fm_count"] = _summary(ms)
        r["fm_count"]["patterns"] = q
        r["fm_count"]["pattern_length"] = m
        r["fm_count"]["patterns_per_s"] = round(q / (r["fm_count"]["median_ms"] * 1e-3))
        r["fm_count"]["occ_lookups_per_s"] = round(2 * m * q / (r["fm_count"]["median_ms"] * 1e-3))
        # exact: every count >= 1 and the interval's first and last suffix start with the pattern
        def starts_with(rank):
            sa = SA[rank].to(torch.int64) & 0xFFFFFFFF
            ok = sa + m <= n
            return ok & (T[(sa[:, None] + torch.arange(m, device=dev)).clamp(max=n - 1)] == pat.view(q, m)).all(1)
        r["fm_count"]["all_exact"] = bool((count >= 1).all()) and bool(starts_with(first).all()) and bool(starts_with(first + count - 1).all())
        # locate: one position for each of q random ranks
        ranks = torch.randint(0, n, (q,), device=dev, generator=g)
        ones = torch.ones(q, dtype=torch.int64, device=dev)
        out_off = torch.arange(q + 1, dtype=torch.int64, device=dev)
        pos = torch.zeros(q, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ms = _timed(torch, lambda: L.fm_locate_device(index.data_ptr(), nb, ranks.data_ptr(), ones.data_ptr(), out_off.data_ptr(), q, pos.data_ptr()),
                    a.warm, a.runs)
        r["fm_locate"] = _summary(ms)
        steps = int((pos & (s - 1)).sum())
        r["fm_locate"]["positions"] = q
        r["fm_locate"]["lf_steps"] = steps
        r["fm_locate"]["positions_per_s"] = round(q / (r["fm_locate"]["median_ms"] * 1e-3))
        r["fm_locate"]["lf_steps_per_s"] = round(steps / (r["fm_locate"]["median_ms"] * 1e-3))
        r["fm_locate"]["all_exact"] = bool(torch.equal(pos, SA[ranks].to(torch.int64) & 0xFFFFFFFF))
        del SA, pat, first, count, pos
        torch.cuda.empty_cache()
        if not a.no_yardstick:
            blocks = (nb0 - 256) // 64
            table = torch.empty((blocks, 16), dtype=torch.int32, device=dev)
            table.view(-1)[::16] = 1
            rows = torch.randint(0, blocks, (1 << 26,), device=dev, generator=g)
            torch.cuda.synchronize()
            ms = _timed(torch, lambda: torch.index_select(table, 0, rows), a.warm, a.runs)
            r["yardstick_index_select"] = _summary(ms)
            r["yardstick_index_select"]["rows"] = rows.numel()
            r["yardstick_index_select"]["lines_per_s"] = round(rows.numel() / (r["yardstick_index_select"]["median_ms"] * 1e-3))
            r["count_lookups_over_yardstick"] = round(r["fm_count"]["occ_lookups_per_s"] / r["yardstick_index_select"]["lines_per_s"], 3)
            r["locate_steps_over_yardstick"] = round(r["fm_locate"]["lf_steps_per_s"] / r["yardstick_index_select"]["lines_per_s"], 3)
            del table, rows
        del T, index
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
