"""Rates of the FM-index's matching statistics and MEMs at C3 and g3r (include/caps_sa_hip.h "FM-index: matching statistics").

    python tools/fm_match_rate.py [--warm 3] [--runs 10] [--kinds uniform,genome+r] [--reads 1048576] [--length 100]
                                  [--out profiles/fm_match_rate_c3.json]

For each text kind (bench.make_text: "uniform" is C3, "genome+r" is g3r; 3e9 bases + the trailing 'C'), W = 4, an index without
samples, HIP-event timed, --warm warm-up runs + --runs timed ones, median / min / max ms, one process:
1. fm_count_device of 2^22 32-mers cut from T -> Occ lookups/s (2 per pattern byte): the yardstick, in the same run;
2. fm_match_device on --reads reads of --length bases cut from T, and on the same reads with one substituted base each, with and
   without intervals -> ms and Occ lookups/s.  The lookups come from the returned lengths: a lane that reports L took L + 1 steps
   (the last one found the empty interval) unless it stopped at its pattern's first byte (L = e), 2 lookups per step;
   ratio = match's lookups/s over count's of this run;
3. fm_mems_device for min_len 20 on both read sets (the counting call and the writing call), with the number of MEMs.
The exact reads are checked: L[e] = e for every lane.  Prints one JSON object (and writes it to --out); progress goes to stderr.
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


def _cut(torch, T, starts, length):
    """T[starts[j] : starts[j] + length] for every j, concatenated, in pieces."""
    out = torch.empty((starts.numel(), length), dtype=torch.uint8, device=T.device)
    ar = torch.arange(length, device=T.device)
    for a in range(0, starts.numel(), 1 << 20):
        out[a:a + (1 << 20)] = T[starts[a:a + (1 << 20), None] + ar]
    return out.view(-1)


def measure_kind(L, torch, a, kind, dev):
    from bench import make_text
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
    del SA
    torch.cuda.empty_cache()
    nb = L.fm_index_bytes(n, 0, 32)
    index = torch.empty(nb, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    L.fm_build_device(B.data_ptr(), n, primary, 0, 0, index.data_ptr(), nb)
    del B
    torch.cuda.empty_cache()
    r = {"n": n, "index_bytes": nb}
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    # 1. the yardstick: count of 2^22 32-mers
    qc, k = a.count_patterns, 32
    pats = _cut(torch, T, torch.randint(0, n - k, (qc,), device=dev, generator=g), k)
    poff = torch.arange(qc + 1, dtype=torch.int64, device=dev) * k
    first = torch.empty(qc, dtype=torch.int64, device=dev)
    count = torch.empty(qc, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    c = _summary(_timed(torch, lambda: L.fm_count_device(index.data_ptr(), nb, pats.data_ptr(), poff.data_ptr(), qc, first.data_ptr(), count.data_ptr()),
                        a.warm, a.runs))
    c.update(patterns=qc, length=k, occ_lookups=2 * qc * k, occ_lookups_per_s=round(2 * qc * k / (c["median_ms"] * 1e-3)),
             all_found=bool((count >= 1).all()))
    r["fm_count"] = c
    _say(kind, "count", c["median_ms"], c["occ_lookups_per_s"])
    del pats, poff, first, count
    # 2. and 3. the two read sets
    q, ln = a.reads, a.length
    starts = torch.randint(0, n - ln, (q,), device=dev, generator=g)
    exact = _cut(torch, T, starts, ln)
    hdr = index[:256].cpu().numpy().view("<u8")                              # the letters of the index: header words 5 and 6
    sigma = int(hdr[5])
    letters = torch.tensor([(int(hdr[6]) >> (8 * c)) & 0xFF for c in range(sigma)], dtype=torch.uint8, device=dev)
    at = torch.arange(q, device=dev) * ln + torch.randint(0, ln, (q,), device=dev, generator=g)
    code = (letters[None, :] == exact[at][:, None]).to(torch.int64).argmax(1)
    one_off = exact.clone()
    one_off[at] = letters[(code + torch.randint(1, sigma, (q,), device=dev, generator=g)) % sigma]
    off = torch.arange(q + 1, dtype=torch.int64, device=dev) * ln
    total = q * ln
    e = (torch.arange(total, device=dev) % ln + 1).to(torch.int32)
    d_len = torch.empty(total, dtype=torch.int32, device=dev)
    d_first = torch.empty(total, dtype=torch.int64, device=dev)
    d_count = torch.empty(total, dtype=torch.int64, device=dev)
    ws_bytes = L.fm_mems_workspace_bytes(total, q)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    moff = torch.empty(q + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for name, reads in (("exact_reads", exact), ("one_substitution", one_off)):
        leg = {"reads": q, "length": ln, "lanes": total}
        for what, fp, cp in (("match_lengths_only", 0, 0), ("match_with_intervals", d_first.data_ptr(), d_count.data_ptr())):
            m = _summary(_timed(torch, lambda: L.fm_match_device(index.data_ptr(), nb, reads.data_ptr(), off.data_ptr(), q, 0, d_len.data_ptr(), fp, cp),
                                a.warm, a.runs))
            steps = int((d_len + (d_len < e).to(torch.int32)).to(torch.int64).sum())
            m.update(occ_lookups=2 * steps, occ_lookups_per_s=round(2 * steps / (m["median_ms"] * 1e-3)), mean_length=round(float(d_len.float().mean()), 2))
            m["lookups_per_s_over_count"] = round(m["occ_lookups_per_s"] / c["occ_lookups_per_s"], 3)
            leg[what] = m
            _say(kind, name, what, m["median_ms"], m["occ_lookups_per_s"], m["lookups_per_s_over_count"])
        if name == "exact_reads":
            leg["all_exact"] = bool(torch.equal(d_len, e)) and bool((d_count >= 1).all())
        mc = _summary(_timed(torch, lambda: L.fm_mems_device(index.data_ptr(), nb, reads.data_ptr(), off.data_ptr(), q, a.min_len, moff.data_ptr(), 0, 0,
                                                            ws.data_ptr(), ws_bytes), a.warm, a.runs))
        found = int(moff[-1])
        mems = torch.empty(max(found, 1) * 32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        mw = _summary(_timed(torch, lambda: L.fm_mems_device(index.data_ptr(), nb, reads.data_ptr(), off.data_ptr(), q, a.min_len, moff.data_ptr(),
                                                            mems.data_ptr(), found, ws.data_ptr(), ws_bytes), a.warm, a.runs))
        leg["mems_counting_call"], leg["mems_writing_call"] = mc, mw
        leg["mems"] = {"min_len": a.min_len, "found": found, "per_read": round(found / q, 3)}
        _say(kind, name, "mems", mc["median_ms"], mw["median_ms"], found)
        del mems
        r[name] = leg
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kinds", default="uniform,genome+r")
    ap.add_argument("--n-bases", type=int, default=3_000_000_000)
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--count-patterns", type=int, default=1 << 22)
    ap.add_argument("--min-len", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import caps_sa_amd
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": a.runs, "measured_on": "MI355X (this run)"}
    for kind in [k for k in a.kinds.split(",") if k]:
        res["c3" if kind == "uniform" else ("g3r" if kind == "genome+r" else kind)] = measure_kind(L, torch, a, kind, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
