"""Rates of the FM-index's text-position samples and extract at C3 and g3r (include/caps_sa_hip.h "FM-index: extract").

    python tools/fm_extract_rate.py [--warm 3] [--runs 10] [--kinds uniform,genome+r] [--ts 32,64,128,256]
                                    [--out profiles/fm_extract_rate_c3.json] [--u64-large]

For each text kind (bench.make_text: "uniform" is C3, "genome+r" is g3r; 3e9 bases + the trailing 'C'), W = 4, s = 32, HIP-event
timed, --warm warm-up runs + --runs timed ones, median / min / max ms, one process:
1. fm_build_device with samples: the upgrade's yardstick, in the same run;
2. per t: fm_add_text_samples_device.  GATE: no slower than 1. (it reads the mark words and the samples once);
3. fm_locate_device on 2^22 random ranks -> LF steps/s: extract's yardstick, in the same run;
4. per t: fm_extract_device on 2^22 random ranges of length 100 -> ms, ranges/s, LF steps/s (steps as the kernel's plan counts them:
   from the end of the last chunk of a range down to its start), compared with the resident text (torch.equal).
   GATE at --default-t: extract's steps/s >= 0.8 x locate's of this run;
   cost[t] = bytes per base of the version-2 index x the median ms: the default t is the sweep's smallest;
5. extract(0, n) and 3,000 ranges of 10^6 at --default-t next to inverse_bwt_device: recorded, no gate.
--u64-large: one more leg, T = 'A' * (2^32 + 1000) + R (the closed form of test_u64_rows_beyond_2_pow_32), W = 8: ranges around
position 2^32 and inside R compared exactly; its pass or fail goes into the JSON.
Prints one JSON object (and writes it to --out); progress goes to stderr.
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


def _say(*a):
    print(*a, file=sys.stderr, flush=True)


def _extract(L, torch, index, nb, starts, lengths):
    """(fn, text, off): fn runs fm_extract_device of the ranges into text, on a workspace of the caller."""
    q = starts.numel()
    off = torch.zeros(q + 1, dtype=torch.int64, device=starts.device)
    off[1:] = torch.cumsum(lengths, 0)
    text = torch.zeros(int(off[-1]), dtype=torch.uint8, device=starts.device)
    ws_bytes = L.fm_extract_workspace_bytes(q)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=starts.device)
    return (lambda: L.fm_extract_device(index.data_ptr(), nb, starts.data_ptr(), off.data_ptr(), q, text.data_ptr(), ws.data_ptr(), ws_bytes),
            text, off)


def _gathered(torch, T, starts, length):
    """T[starts[j] : starts[j] + length] for every j, in pieces (the index tensor of 2^22 x 100 positions is 3 GB)."""
    out = torch.empty((starts.numel(), length), dtype=torch.uint8, device=T.device)
    ar = torch.arange(length, device=T.device)
    for a in range(0, starts.numel(), 1 << 20):
        out[a:a + (1 << 20)] = T[starts[a:a + (1 << 20), None] + ar]
    return out.view(-1)


def measure_kind(L, torch, a, kind, dev):
    from bench import make_text
    s, q = 32, a.queries
    T = make_text(torch, a.n_bases, 42, dev, kind)
    n = T.numel()
    SA = torch.empty(n, dtype=torch.int32, device=dev)
    LCP = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
    del LCP
    torch.cuda.empty_cache()
    B = torch.empty(n, dtype=torch.uint8, device=dev)
    primary = L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, B.data_ptr())
    ts = [int(x) for x in a.ts.split(",")]
    nb1 = L.fm_index_bytes(n, s, 32)
    cap = max(L.fm_index_bytes_ex(n, s, t, 32) for t in ts)
    index = torch.empty(cap, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    r = {"n": n, "sa_sample": s, "index_bytes_v1": nb1}
    r["fm_build_with_samples"] = _summary(_timed(torch, lambda: L.fm_build_device(B.data_ptr(), n, primary, SA.data_ptr(), s, index.data_ptr(), nb1),
                                                 a.warm, a.runs))
    _say(kind, "build", r["fm_build_with_samples"]["median_ms"])
    # locate: the yardstick of the walk
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    ranks = torch.randint(0, n, (q,), device=dev, generator=g)
    ones = torch.ones(q, dtype=torch.int64, device=dev)
    out_off = torch.arange(q + 1, dtype=torch.int64, device=dev)
    pos = torch.zeros(q, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ms = _timed(torch, lambda: L.fm_locate_device(index.data_ptr(), nb1, ranks.data_ptr(), ones.data_ptr(), out_off.data_ptr(), q, pos.data_ptr()),
                a.warm, a.runs)
    r["fm_locate"] = _summary(ms)
    steps = int((pos & (s - 1)).sum())
    r["fm_locate"].update(positions=q, lf_steps=steps, lf_steps_per_s=round(steps / (r["fm_locate"]["median_ms"] * 1e-3)),
                          all_exact=bool(torch.equal(pos, SA[ranks].to(torch.int64) & 0xFFFFFFFF)))
    _say(kind, "locate", r["fm_locate"]["median_ms"], r["fm_locate"]["lf_steps_per_s"])
    del SA, ranks, ones, out_off, pos
    torch.cuda.empty_cache()
    ln = a.length
    starts = torch.randint(0, n - ln, (q,), device=dev, generator=g)
    lengths = torch.full((q,), ln, dtype=torch.int64, device=dev)
    want = _gathered(torch, T, starts, ln)
    r["upgrade"], r["extract_short"] = {}, {}
    for t in ts:
        nb = L.fm_index_bytes_ex(n, s, t, 32)
        u = _summary(_timed(torch, lambda: L.fm_add_text_samples_device(index.data_ptr(), cap, t), a.warm, a.runs))
        u["index_bytes"], u["bytes_per_base"] = nb, round(nb / n, 4)
        u["over_fm_build_with_samples"] = round(u["median_ms"] / r["fm_build_with_samples"]["median_ms"], 3)
        u["gate_no_slower_than_fm_build"] = u["median_ms"] <= r["fm_build_with_samples"]["median_ms"]
        r["upgrade"][str(t)] = u
        fn, text, _ = _extract(L, torch, index, nb, starts, lengths)
        e = _summary(_timed(torch, fn, a.warm, a.runs))
        plan_steps = int((torch.clamp(((starts + ln - 1) // t + 1) * t, max=n) - starts).sum())
        e.update(ranges=q, length=ln, lf_steps=plan_steps, ranges_per_s=round(q / (e["median_ms"] * 1e-3)),
                 lf_steps_per_s=round(plan_steps / (e["median_ms"] * 1e-3)), all_exact=bool(torch.equal(text, want)))
        e["steps_per_s_over_locate"] = round(e["lf_steps_per_s"] / r["fm_locate"]["lf_steps_per_s"], 3)
        e["cost_bytes_per_base_x_ms"] = round(u["bytes_per_base"] * e["median_ms"], 3)
        r["extract_short"][str(t)] = e
        _say(kind, "t", t, "upgrade", u["median_ms"], "extract", e["median_ms"], e["lf_steps_per_s"], e["all_exact"])
        del text
    del want, starts, lengths
    torch.cuda.empty_cache()
    t = a.default_t
    r["default_t"] = t
    r["best_t_by_cost"] = int(min(ts, key=lambda x: r["extract_short"][str(x)]["cost_bytes_per_base_x_ms"]))
    if str(t) in r["extract_short"]:
        r["gate_extract_steps_at_least_0p8_of_locate"] = r["extract_short"][str(t)]["steps_per_s_over_locate"] >= 0.8
    nb = L.fm_index_bytes_ex(n, s, t, 32)
    L.fm_add_text_samples_device(index.data_ptr(), cap, t)
    # the whole text, next to the inverse BWT
    ws_bytes = L.inverse_bwt_workspace_bytes(n, 32)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    back = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    r["inverse_bwt_device"] = _summary(_timed(torch, lambda: L.inverse_bwt_device(B.data_ptr(), n, primary, back.data_ptr(), ws.data_ptr(), ws_bytes),
                                              a.warm, a.runs))
    r["inverse_bwt_device"]["all_exact"] = bool(torch.equal(back, T))
    del ws, back, B
    torch.cuda.empty_cache()
    fn, text, _ = _extract(L, torch, index, nb, torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), n, dtype=torch.int64, device=dev))
    r["extract_whole_text"] = _summary(_timed(torch, fn, a.warm, a.runs))
    r["extract_whole_text"].update(text_sample=t, all_exact=bool(torch.equal(text, T)),
                                   over_inverse_bwt_device=round(statistics.median(r["extract_whole_text"]["runs_ms"]) / r["inverse_bwt_device"]["median_ms"], 3))
    del text
    big = 1_000_000
    if n > 2 * big:
        starts = torch.randint(0, n - big, (3000,), device=dev, generator=g)
        fn, text, off = _extract(L, torch, index, nb, starts, torch.full((3000,), big, dtype=torch.int64, device=dev))
        r["extract_3000_x_1e6"] = _summary(_timed(torch, fn, a.warm, a.runs))
        ok = all(bool(torch.equal(text[j * big:(j + 1) * big], T[int(starts[j]):int(starts[j]) + big])) for j in range(0, 3000, 97))
        r["extract_3000_x_1e6"].update(text_sample=t, sampled_ranges_exact=ok)
        del text
    _say(kind, "whole", r["extract_whole_text"]["median_ms"], "inverse", r["inverse_bwt_device"]["median_ms"])
    del T, index
    torch.cuda.empty_cache()
    return r


def u64_large(L, torch, t):
    """'A' * (2^32 + 1000) + R: BWT and SA in closed form from the library's SA of R; W = 8, s = 32."""
    import numpy as np
    dev = torch.device("cuda")
    m = (1 << 32) + 1000
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    Rd = torch.tensor(list(b"CGT"), dtype=torch.uint8, device=dev)[torch.randint(0, 3, (10_000_000,), device=dev, generator=g)]
    R = Rd.cpu().numpy()
    SA_R, _, _ = L.build(R, p=256)
    tail = np.where(SA_R > 0, R[SA_R.astype(np.int64) - 1], ord("A")).astype(np.uint8)
    n = m + R.size
    B = torch.empty(n, dtype=torch.uint8, device=dev)
    B[0] = int(R[-1])
    B[1:m] = ord("A")
    B[m:] = torch.from_numpy(tail).cuda()
    SA = torch.empty(n, dtype=torch.int64, device=dev)
    step = 1 << 30
    for o in range(0, m, step):
        SA[o:min(m, o + step)] = torch.arange(o, min(m, o + step), dtype=torch.int64, device=dev)
    SA[m:] = torch.from_numpy(SA_R.astype(np.int64)).cuda() + m
    cap = L.fm_index_bytes_ex(n, 32, t, 64)
    index = torch.empty(cap, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    L.fm_build_device(B.data_ptr(), n, 0, SA.data_ptr(), 32, index.data_ptr(), cap, idx_bits=64)
    del B, SA
    torch.cuda.empty_cache()
    L.fm_add_text_samples_device(index.data_ptr(), cap, t)
    two32 = 1 << 32
    ranges = [(two32 - 150, 300), (two32 - 1, 1), (two32, 1), (two32, 2000), (m - 70, 140), (m, 1), (m - 1, 2), (n - 300, 300), (n - 1, 1),
              (m + 5_000_000, 300), (0, 3), (two32 - 3 * t, 6 * t + 1)]
    starts = torch.tensor([x for x, _ in ranges], dtype=torch.int64, device=dev)
    lengths = torch.tensor([x for _, x in ranges], dtype=torch.int64, device=dev)
    fn, text, off = _extract(L, torch, index, cap, starts, lengths)
    fn()
    torch.cuda.synchronize()
    ok = True
    for j, (x, ln) in enumerate(ranges):
        got = text[int(off[j]):int(off[j + 1])]
        na = max(0, min(m, x + ln) - x)                     # the letters of the range inside 'A' * m
        ok = ok and bool((got[:na] == ord("A")).all()) and bool(torch.equal(got[na:], Rd[max(x, m) - m:x + ln - m]))
    return {"n": n, "text_sample": t, "ranges": len(ranges), "all_exact": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kinds", default="uniform,genome+r")
    ap.add_argument("--n-bases", type=int, default=3_000_000_000)
    ap.add_argument("--queries", type=int, default=1 << 22)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--ts", default="32,64,128,256")
    ap.add_argument("--default-t", type=int, default=32)
    ap.add_argument("--u64-large", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import caps_sa_amd
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": a.runs, "measured_on": "MI355X (this run)",
           "byte_stores_only": bool(os.environ.get("CAPS_SA_FM_EXTRACT_BYTES"))}
    for kind in [k for k in a.kinds.split(",") if k]:
        res["c3" if kind == "uniform" else ("g3r" if kind == "genome+r" else kind)] = measure_kind(L, torch, a, kind, dev)
    if a.u64_large:
        try:
            res["u64_large"] = u64_large(L, torch, a.default_t)
        except Exception as e:                               # (recorded: the leg's pass or fail belongs in the JSON)
            res["u64_large"] = {"all_exact": False, "error": str(e)[:300]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
