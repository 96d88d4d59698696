"""Rates of the wide FM-index at C3 (include/caps_sa_hip.h "FM-index: the wide format"), fm_rate.py's protocol: HIP events, --warm
warm-up runs + --runs timed ones, everything in one process, median / min / max ms.

    python tools/fm_wide_rate.py [--warm 3] [--runs 10] [--n-bases 3000000000] [--out profiles/fm_wide_rate_c3.json]

1. "acgtn": bench.make_text with every 1,000th base set to 'N' (5 letters, 2 levels).  fm_build_wide_device without samples
   against bwt_device in the same run.  GATE (DESIGN 4.9's own): the build takes no longer than the gather.  Then count and locate
   times on that text and the line reads per second (2 * Lv per count step, Lv per LF step): recorded, no gate.
2. "c3": the C3 text itself (4 letters, 1 level), wide against narrow in the same process: 2^22 32-mers for count, 2^22 ranks for
   locate.  A step touches the same lines in both formats; the wide kernels add the LDS table reads and the zone subtraction.
   GATE: wide time <= 1.25 x narrow time, for count and for locate.
Every answer is checked (count: the interval's ends start with the pattern; locate: torch.equal with the SA).
Prints one JSON object (and writes it to --out).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fm_rate import _summary, _timed  # noqa: E402


def queries(torch, L, T, SA, index, nb, q, m, s, warm, runs, lv):
    """count of q m-mers cut from T and locate of q random ranks on the blob at `index`: times, rates, exactness."""
    dev, n = T.device, T.numel()
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    starts = torch.randint(0, n - m, (q,), device=dev, generator=g)
    ar = torch.arange(m, device=dev)
    pat = T[starts[:, None] + ar].contiguous().view(-1)
    off = torch.arange(q + 1, dtype=torch.int64, device=dev) * m
    first = torch.zeros(q, dtype=torch.int64, device=dev)
    count = torch.zeros(q, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    r = {}
    r["fm_count"] = _summary(_timed(torch, lambda: L.fm_count_device(index.data_ptr(), nb, pat.data_ptr(), off.data_ptr(), q, first.data_ptr(),
                                                                     count.data_ptr()), warm, runs))
    sec = r["fm_count"]["median_ms"] * 1e-3
    r["fm_count"].update(patterns=q, pattern_length=m, patterns_per_s=round(q / sec), steps_per_s=round(m * q / sec), lookups_per_s=round(2 * m * q / sec),
                         line_reads_per_s=round(2 * lv * m * q / sec))

    def starts_with(rank):
        sa = SA[rank].to(torch.int64) & 0xFFFFFFFF
        return (sa + m <= n) & (T[(sa[:, None] + ar).clamp(max=n - 1)] == pat.view(q, m)).all(1)
    r["fm_count"]["all_exact"] = bool((count >= 1).all()) and bool(starts_with(first).all()) and bool(starts_with(first + count - 1).all())
    ranks = torch.randint(0, n, (q,), device=dev, generator=g)
    ones = torch.ones(q, dtype=torch.int64, device=dev)
    out_off = torch.arange(q + 1, dtype=torch.int64, device=dev)
    pos = torch.zeros(q, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    r["fm_locate"] = _summary(_timed(torch, lambda: L.fm_locate_device(index.data_ptr(), nb, ranks.data_ptr(), ones.data_ptr(), out_off.data_ptr(), q,
                                                                       pos.data_ptr()), warm, runs))
    sec = r["fm_locate"]["median_ms"] * 1e-3
    steps = int((pos & (s - 1)).sum())
    r["fm_locate"].update(positions=q, lf_steps=steps, positions_per_s=round(q / sec), lf_steps_per_s=round(steps / sec),
                          line_reads_per_s=round(lv * steps / sec), all_exact=bool(torch.equal(pos, SA[ranks].to(torch.int64) & 0xFFFFFFFF)))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--n-bases", type=int, default=3_000_000_000)
    ap.add_argument("--queries", type=int, default=1 << 22)
    ap.add_argument("--texts", default="acgtn,c3")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import caps_sa_amd
    from bench import make_text
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": a.runs}
    q, m, s = a.queries, 32, 32
    for text in a.texts.split(","):
        T = make_text(torch, a.n_bases, 42, dev, "uniform")
        if text == "acgtn":
            T[999:a.n_bases:1000] = ord("N")
        n = T.numel()
        SA = torch.empty(n, dtype=torch.int32, device=dev)
        LCP = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
        del LCP
        torch.cuda.empty_cache()
        B = torch.empty(n, dtype=torch.uint8, device=dev)
        primary = []
        sigma, lv = (5, 2) if text == "acgtn" else (4, 1)
        r = {"n": n, "sa_sample": s, "sigma": sigma, "levels": lv}
        r["bwt_device"] = _summary(_timed(torch, lambda: primary.append(L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, B.data_ptr())), a.warm, a.runs))
        p = primary[-1]
        nb0, nb = L.fm_wide_index_bytes(n, sigma, 0, 32), L.fm_wide_index_bytes(n, sigma, s, 32)
        ws_bytes = L.fm_wide_workspace_bytes(n, 32)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        index = torch.empty(nb, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        r["build_wide_no_samples"] = _summary(_timed(torch, lambda: L.fm_build_wide_device(B.data_ptr(), n, p, 0, 0, index.data_ptr(), nb0, ws.data_ptr(),
                                                                                          ws_bytes), a.warm, a.runs))
        r["build_wide_with_samples"] = _summary(_timed(torch, lambda: L.fm_build_wide_device(B.data_ptr(), n, p, SA.data_ptr(), s, index.data_ptr(), nb,
                                                                                            ws.data_ptr(), ws_bytes), a.warm, a.runs))
        del ws
        r["index_bytes"], r["bytes_per_base"], r["workspace_bytes"] = nb, round(nb / n, 4), ws_bytes
        r["build_no_samples_over_bwt_device"] = round(r["build_wide_no_samples"]["median_ms"] / r["bwt_device"]["median_ms"], 3)
        if text == "acgtn":
            r["gate_build_no_slower_than_bwt_device"] = r["build_wide_no_samples"]["median_ms"] <= r["bwt_device"]["median_ms"]
        r["wide"] = queries(torch, L, T, SA, index, nb, q, m, s, a.warm, a.runs, lv)
        if text == "c3":
            nn = L.fm_index_bytes(n, s, 32)
            narrow = torch.empty(nn, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            L.fm_build_device(B.data_ptr(), n, p, SA.data_ptr(), s, narrow.data_ptr(), nn)
            r["narrow"] = queries(torch, L, T, SA, narrow, nn, q, m, s, a.warm, a.runs, 1)
            for k in ("fm_count", "fm_locate"):
                ratio = r["wide"][k]["median_ms"] / r["narrow"][k]["median_ms"]
                r[f"{k}_wide_over_narrow"] = round(ratio, 3)
                r[f"gate_{k}_wide_within_1.25x_narrow"] = ratio <= 1.25
            del narrow
        del T, SA, B, index
        torch.cuda.empty_cache()
        res[text] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
