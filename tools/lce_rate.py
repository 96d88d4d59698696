"""Rates of isa, the LCE index build, range_min and lce at C3 and g3r (include/caps_sa_hip.h "ISA and longest common extensions",
caps_sa_hip_isa_device_u32, caps_sa_hip_lce_build_device_u32, caps_sa_hip_lce_range_min_device, caps_sa_hip_lce_device).

    python tools/lce_rate.py [--warm 3] [--runs 10] [--kinds uniform,genome+r] [--queries 4194304] [--out profiles/lce_rate_c3.json]

For each text kind (bench.make_text: "uniform" is C3, "genome+r" is g3r's repeat-rich genome; 3e9 bases + the trailing 'C'): one
build_device (u32), SA and LCP stay resident; then, HIP-event timed, --warm warm-up runs + --runs timed ones, median / min / max ms.
One process.  The yardsticks are NOT the code under test:
1. isa against the only route a user had before it: torch ISA[SA_chunk.long() & 0xFFFFFFFF] = arange_chunk in chunks of 2^28.
   GATE: isa <= that route.  bwt_device on the same SA is recorded beside it, no gate.
2. build minus isa against LCP.clone().  Allowed ratio = (the bytes the passes read and write, counted here from the shapes) /
   (2 n W), times 1.25.  Recorded beside it, no gate: the same difference with isa writing into the blob's own ISA section (the
   destination the build scatters to), and with --kernel-times the device time of every kernel of one more build.
3. range_min and lce(k = 0) on --queries random queries against the torch dependent double gather LCP[ISA[x]] over 2 q indices
   (the ranks widened and masked likewise),
   which touches 4 lines per query.  Allowed ratio = (the mean number of distinct 128-byte lines a query touches, counted here from
   the query geometry on the same pairs) / 4, times 1.25.  lce at k = 8 is recorded, no gate.
A gate that is missed is reported as missed ("gate_*": false).
Exactness inside the run: ISA[SA[r]] = r for every r; the blob's LCP copy, M_0 .. M_6 and every T_j against torch reductions of LCP;
every range_min against a torch sparse table over torch's own block minima plus the partial blocks by gathers; every lce at k = 0 and
k = 8 against the text (mismatch counts over a window of 192 bytes; the few longer extensions one by one on the host).
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

B, S, LINE = 64, 4096, 128
CHUNK = 1 << 28
TOP = 0xFFFFFFFF


def u32(t):
    return t.to(__import__("torch").int64) & 0xFFFFFFFF


def layout(n, w=4):
    up = lambda b: (b + 255) // 256 * 256
    nb, ns = (n + B - 1) // B, (n + S - 1) // S
    tl = ns.bit_length()
    off_isa = 256
    off_lcp = off_isa + up(n * w)
    off_m = off_lcp + up(n * w)
    ms, ts = up(nb * w), up(ns * w)
    off_t = off_m + 7 * ms
    return dict(nb=nb, ns=ns, tl=tl, off_isa=off_isa, off_lcp=off_lcp, off_m=off_m, m_stride=ms, off_t=off_t, t_stride=ts, total=off_t + tl * ts)


def section(torch, blob, off, count):
    return blob[off:off + 4 * count].view(torch.int32)


def torch_isa(torch, SA, ISA, n):
    """The route a user had: torch has no unsigned 32-bit indices, so the chunk is widened and masked (beyond 2^31 a plain .long() is
    negative and indexes from the end), and the ranks are narrowed back to the 32-bit pattern."""
    for a in range(0, n, CHUNK):
        b = min(a + CHUNK, n)
        ISA[u32(SA[a:b])] = torch.arange(a, b, device=SA.device).to(torch.int32)


def kernel_times(torch, fn):
    """fn() once under torch.profiler (device activities only) -> {kernel: ms} for the isa_* / lce_* kernels."""
    import re
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        m = re.search(r"(isa_\w+?_kernel|lce_\w+?_kernel)", e.key)
        if m:
            us = getattr(e, "device_time_total", None)
            if us is None:
                us = getattr(e, "cuda_time_total", 0.0)
            out[m.group(0)] = round(out.get(m.group(0), 0.0) + us / 1e3, 3)
    return out


def block_minima(torch, LCP, n, nb):
    """torch's own M_0 (int64 of the unsigned values), LCP[0] read as 0."""
    out = torch.empty(nb, dtype=torch.int64, device=LCP.device)
    step = CHUNK
    for a in range(0, n, step):
        b = min(a + step, n)
        x = u32(LCP[a:b])
        if a == 0:
            x[0] = 0
        pad = (-x.numel()) % B
        if pad:
            x = torch.cat([x, torch.full((pad,), TOP, dtype=torch.int64, device=x.device)])
        out[a // B:a // B + x.numel() // B] = x.view(-1, B).min(dim=1).values
        del x
    return out


def check_tables(torch, blob, LCP, n, lay, m0):
    ok = {}
    copy = section(torch, blob, lay["off_lcp"], n)
    same = True
    for a in range(0, n, CHUNK):
        b = min(a + CHUNK, n)
        x = LCP[a:b].clone()
        if a == 0:
            x[0] = 0
        same = same and bool((copy[a:b] == x).all())
        del x
    ok["lcp_copy"] = same
    nb, ns = lay["nb"], lay["ns"]
    cur, good = m0, True
    for j in range(7):
        if j:
            d = 1 << (j - 1)
            nxt = cur.clone()
            if d < nb:
                nxt[:nb - d] = torch.minimum(cur[:nb - d], cur[d:])
            cur = nxt
        good = good and bool((u32(section(torch, blob, lay["off_m"] + j * lay["m_stride"], nb)) == cur).all())
    ok["block_tables"] = good
    pad = (-nb) % (S // B)
    t0 = torch.cat([m0, torch.full((pad,), TOP, dtype=torch.int64, device=m0.device)]).view(-1, S // B).min(dim=1).values
    cur, good = t0, True
    for j in range(lay["tl"]):
        if j:
            d = 1 << (j - 1)
            nxt = cur.clone()
            nxt[:ns - d] = torch.minimum(cur[:ns - d], cur[d:])
            cur = nxt
        good = good and bool((u32(section(torch, blob, lay["off_t"] + j * lay["t_stride"], ns)) == cur).all())
    ok["top_tables"] = good
    return ok


class BlockTable:
    """A torch sparse table over torch's own block minima: min over whole blocks [fb, le)."""

    def __init__(self, torch, m0):
        self.torch, self.lv = torch, [m0]
        j = 1
        while 2 * j <= m0.numel():
            p = self.lv[-1]
            self.lv.append(torch.minimum(p[:-j], p[j:]))
            j *= 2

    def query(self, fb, le):
        torch = self.torch
        cnt = le - fb
        out = torch.full_like(fb, TOP)
        live = cnt > 0
        lev = torch.zeros_like(fb)
        lev[live] = torch.floor(torch.log2(cnt[live].double() + 0.5)).long()
        for j in torch.unique(lev[live]).tolist():
            m = live & (lev == j)
            t = self.lv[j]
            out[m] = torch.minimum(t[fb[m]], t[le[m] - (1 << j)])
        return out


def truth_range_min(torch, LCP, table, lo, hi, n):
    """By the definition, with torch: whole blocks from the table, the ranks before and behind them by gathers."""
    fb, le = (lo + B - 1) // B, (hi + 1) // B                  # whole blocks fb .. le - 1 (none: fb >= le)
    none = fb >= le
    out = table.query(torch.where(none, torch.zeros_like(fb), fb), torch.where(none, torch.zeros_like(le), le))
    off = torch.arange(B, device=lo.device)[None, :]
    for a in range(0, lo.numel(), 1 << 20):
        sl = slice(a, a + (1 << 20))
        l, h, f, e, nn = lo[sl, None], hi[sl, None], fb[sl, None], le[sl, None], none[sl, None]
        head_end = torch.where(nn, h + 1, f * B)                 # ranks l .. head_end - 1
        idx = l + off
        v = u32(LCP[idx.clamp(max=n - 1)])
        v = torch.where(idx == 0, torch.zeros_like(v), v)
        m = torch.where(idx < head_end, v, torch.full_like(v, TOP)).min(dim=1).values
        if int(((head_end - l) > B).sum()):                      # no whole block but a span of up to 2 B - 2 ranks: its second half
            idx2 = idx + B
            v2 = u32(LCP[idx2.clamp(max=n - 1)])
            m = torch.minimum(m, torch.where(idx2 < head_end, v2, torch.full_like(v2, TOP)).min(dim=1).values)
        idx = e * B + off                                       # ranks le * B .. h
        v = u32(LCP[idx.clamp(max=n - 1)])
        m = torch.minimum(m, torch.where(~nn & (idx <= h), v, torch.full_like(v, TOP)).min(dim=1).values)
        out[sl] = torch.minimum(out[sl], m)
    return out


def lines_touched(torch, lay, lo, hi, n, w=4):
    """The distinct 128-byte lines of the blob one range_min(lo, hi) reads, from the header's decomposition -> int64 per query."""
    per = LINE // w
    bl, bh = lo // B, hi // B
    head_whole, tail_whole = lo % B == 0, (hi % B == B - 1) | (hi == n - 1)
    single = (bl == bh) & ~(head_whole & tail_whole)
    span = lambda a, b: (b // per) - (a // per) + 1
    lines = torch.where(single, span(lo, hi), torch.zeros_like(lo))
    lines += torch.where(~single & ~head_whole, span(lo, (bl + 1) * B - 1), torch.zeros_like(lo))
    lines += torch.where(~single & ~tail_whole, span(bh * B, hi), torch.zeros_like(lo))
    fb, le = torch.where(head_whole, bl, bl + 1), torch.where(tail_whole, bh + 1, bh)
    cnt = torch.where(single, torch.zeros_like(lo), (le - fb).clamp(min=0))
    ids = []                                                    # table reads as global line numbers, -1: none

    def cover(tier_off, stride, levels, size, first, c):
        live = c > 0
        j = torch.floor(torch.log2(c.clamp(min=1).double() + 0.5)).long().clamp(max=levels - 1)
        wdt = torch.ones_like(c) << j
        x, y = first.clamp(max=size - 1), (first + c - wdt).clamp(min=0, max=size - 1)
        for z in (x, y):
            ids.append(torch.where(live, (tier_off + j * stride) // LINE + z // per, torch.full_like(z, -1)))

    small = cnt <= S // B
    e1, e2 = (fb + S // B - 1) // (S // B) * (S // B), le // (S // B) * (S // B)
    zero = torch.zeros_like(cnt)
    cover(lay["off_m"], lay["m_stride"], 7, lay["nb"], fb, torch.where(small, cnt, zero))
    cover(lay["off_m"], lay["m_stride"], 7, lay["nb"], fb, torch.where(small, zero, e1 - fb))
    cover(lay["off_m"], lay["m_stride"], 7, lay["nb"], e2, torch.where(small, zero, le - e2))
    cover(lay["off_t"], lay["t_stride"], max(lay["tl"], 1), max(lay["ns"], 1), e1 // (S // B), torch.where(small, zero, (e2 - e1) // (S // B)))
    t = torch.stack(ids, dim=1).sort(dim=1).values
    distinct = (t[:, 1:] != t[:, :-1]).sum(dim=1) + 1 - (t[:, 0] == -1).long()
    return lines + distinct


def truth_lce(torch, T, I, J, k, n, cap=192):
    """lce(i, j, k) by the definition over a window of cap bytes -> (lengths, the queries whose extension fills the window)."""
    out = torch.empty_like(I)
    room = n - torch.maximum(I, J)
    off = torch.arange(cap, device=I.device)[None, :]
    for a in range(0, I.numel(), 1 << 19):
        sl = slice(a, a + (1 << 19))
        i, j, r = I[sl, None], J[sl, None], room[sl, None]
        ok = off < r
        mism = ((T[(i + off).clamp(max=n - 1)] != T[(j + off).clamp(max=n - 1)]) & ok).cumsum(dim=1)
        out[sl] = (ok & (mism <= k)).sum(dim=1)
    return out, (out >= cap) & (room > cap)


def brute(t, i, j, k, n):
    l = used = 0
    while max(i, j) + l < n:
        if t[i + l] != t[j + l]:
            if used == k:
                break
            used += 1
        l += 1
    return l


def check_lce(torch, T, I, J, k, n, got):
    want, long_ = truth_lce(torch, T, I, J, k, n)
    same = I == J
    want = torch.where(same, n - I, want)
    long_ &= ~same
    bad = int(((got != want) & ~long_).sum())
    idx = long_.nonzero().flatten().tolist()
    for x in idx[:4096]:                                         # the few long ones: the bytes themselves, on the host
        i, j, g = int(I[x]), int(J[x]), int(got[x])
        m = max(i, j)
        a, b = T[i:i + g + 1].cpu().numpy(), T[j:j + g + 1].cpu().numpy()
        mm = int((a[:g] != b[:g]).sum())
        end = m + g == n
        bad += not (mm <= k and (end or (mm == k and a[g] != b[g])))
    return {"wrong": bad, "longer_than_the_window": len(idx), "longest": int(got.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--kinds", default="uniform,genome+r")
    ap.add_argument("--n-bases", type=int, default=3_000_000_000)
    ap.add_argument("--queries", type=int, default=1 << 22)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-times", action="store_true",
                    help="one more build and one more isa under torch.profiler: device time per isa_* / lce_* kernel into the JSON")
    a = ap.parse_args()
    import torch
    import caps_sa_amd
    from bench import make_text
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    q = a.queries
    res = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": a.runs, "queries": q, "measured_on": "MI355X (this run)", "margin": 1.25}
    for kind in a.kinds.split(","):
        T = make_text(torch, a.n_bases, 42, dev, kind)
        n = T.numel()
        SA = torch.empty(n, dtype=torch.int32, device=dev)
        LCP = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
        print(f"{kind}: built, n = {n}", file=sys.stderr, flush=True)
        lay = layout(n)
        need = L.lce_index_bytes(n, 32)
        assert need == lay["total"]
        r = {"n": n, "index_bytes": need, "index_bytes_per_base": round(need / n, 4)}
        # 1. isa
        ISA = torch.empty(n, dtype=torch.int32, device=dev)
        BWT = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        r["yardstick_torch_scatter"] = _summary(_timed(torch, lambda: torch_isa(torch, SA, ISA, n), a.warm, a.runs))
        r["bwt_device"] = _summary(_timed(torch, lambda: L.bwt_device(T.data_ptr(), n, SA.data_ptr(), 0, n, BWT.data_ptr()), a.warm, a.runs))
        del BWT
        mine = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        r["isa"] = _summary(_timed(torch, lambda: L.isa_device(SA.data_ptr(), n, mine.data_ptr()), a.warm, a.runs))
        r["isa_over_yardstick"] = round(r["isa"]["median_ms"] / r["yardstick_torch_scatter"]["median_ms"], 3)
        r["gate_isa"] = r["isa"]["median_ms"] <= r["yardstick_torch_scatter"]["median_ms"]
        ok_isa = bool((mine == ISA).all())
        for c in range(0, n, CHUNK):
            e = min(c + CHUNK, n)
            ok_isa = ok_isa and bool((mine[u32(SA[c:e])] == torch.arange(c, e, device=dev).to(torch.int32)).all())
        ISA2 = mine
        print(f"{kind}: isa {r['isa']['median_ms']} ms, torch {r['yardstick_torch_scatter']['median_ms']} ms", file=sys.stderr, flush=True)
        # 2. the build
        blob = torch.empty(need, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        r["yardstick_lcp_clone"] = _summary(_timed(torch, lambda: LCP.clone(), a.warm, a.runs))
        r["build"] = _summary(_timed(torch, lambda: L.lce_build_device(SA.data_ptr(), LCP.data_ptr(), n, blob.data_ptr(), need), a.warm, a.runs))
        w, nb, ns = 4, lay["nb"], lay["ns"]
        # lce_block_kernel reads LCP and writes the copy and M_0; every level of lce_table_kernel reads two entries and writes one
        moved = 2 * n * w + nb * w + 6 * 3 * nb * w + 2 * ns * w + (lay["tl"] - 1) * 3 * ns * w
        r["build_minus_isa_ms"] = round(r["build"]["median_ms"] - r["isa"]["median_ms"], 3)
        r["build_bytes_over_clone_bytes"] = round(moved / (2 * n * w), 4)
        r["build_allowed_ratio"] = round(moved / (2 * n * w) * 1.25, 4)
        r["build_minus_isa_over_clone"] = round(r["build_minus_isa_ms"] / r["yardstick_lcp_clone"]["median_ms"], 3)
        r["gate_build"] = r["build_minus_isa_over_clone"] <= r["build_allowed_ratio"]
        # beside the gate, no gate of its own: isa into the blob's own ISA section, the destination the build scatters to (the time of
        # 3e9 scattered stores depends on where the destination lies, so the subtraction above mixes two destinations)
        r["isa_into_the_blob"] = _summary(_timed(torch, lambda: L.isa_device(SA.data_ptr(), n, blob.data_ptr() + lay["off_isa"]), a.warm, a.runs))
        r["build_minus_isa_into_the_blob_ms"] = round(r["build"]["median_ms"] - r["isa_into_the_blob"]["median_ms"], 3)
        r["build_minus_isa_into_the_blob_over_clone"] = round(r["build_minus_isa_into_the_blob_ms"] / r["yardstick_lcp_clone"]["median_ms"], 3)
        if a.kernel_times:
            try:
                r["build_kernel_ms"] = kernel_times(torch, lambda: L.lce_build_device(SA.data_ptr(), LCP.data_ptr(), n, blob.data_ptr(), need))
                r["isa_kernel_ms"] = kernel_times(torch, lambda: L.isa_device(SA.data_ptr(), n, ISA2.data_ptr()))
            except Exception as e:                                                   # the timings above stand without it
                r["kernel_times_error"] = repr(e)
        m0 = block_minima(torch, LCP, n, nb)
        exact = {"isa": ok_isa, "isa_section": bool((section(torch, blob, lay["off_isa"], n) == ISA).all())}
        exact.update(check_tables(torch, blob, LCP, n, lay, m0))
        print(f"{kind}: build {r['build']['median_ms']} ms, clone {r['yardstick_lcp_clone']['median_ms']} ms", file=sys.stderr, flush=True)
        # 3. the queries
        g = torch.Generator(device=dev)
        g.manual_seed(17)
        x, y = torch.randint(0, n, (q,), device=dev, generator=g), torch.randint(0, n, (q,), device=dev, generator=g)
        lo, hi = torch.minimum(x, y), torch.maximum(x, y)
        out = torch.empty(q, dtype=torch.int64, device=dev)
        both = torch.cat([x, y])
        torch.cuda.synchronize()
        r["yardstick_double_gather"] = _summary(_timed(torch, lambda: LCP[u32(ISA[both])], a.warm, a.runs))
        Y = r["yardstick_double_gather"]["median_ms"]
        bp, nbytes = blob.data_ptr(), need
        r["range_min"] = _summary(_timed(torch, lambda: L.lce_range_min_device(bp, nbytes, lo.data_ptr(), hi.data_ptr(), q, out.data_ptr()), a.warm, a.runs))
        got_min = out.clone()
        r["lce_k0"] = _summary(_timed(torch, lambda: L.lce_device(bp, nbytes, x.data_ptr(), y.data_ptr(), q, 0, out.data_ptr()), a.warm, a.runs))
        got0 = out.clone()
        r["lce_k8"] = _summary(_timed(torch, lambda: L.lce_device(bp, nbytes, x.data_ptr(), y.data_ptr(), q, 8, out.data_ptr()), a.warm, a.runs))
        got8 = out.clone()
        ln_min = lines_touched(torch, lay, lo, hi, n).double().mean().item()
        ra, rb = u32(ISA[x]), u32(ISA[y])
        l2, h2 = torch.minimum(ra, rb) + 1, torch.maximum(ra, rb)
        valid = l2 <= h2
        isa_lines = 1 + (x // (LINE // 4) != y // (LINE // 4)).long()
        ln_lce = (torch.where(valid, lines_touched(torch, lay, torch.where(valid, l2, h2), h2, n), torch.zeros_like(l2)) + isa_lines).double().mean().item()
        for name, lines in (("range_min", ln_min), ("lce_k0", ln_lce)):
            r[name + "_mean_lines"] = round(lines, 3)
            r[name + "_allowed_ratio"] = round(lines / 4 * 1.25, 3)
            r[name + "_over_yardstick"] = round(r[name]["median_ms"] / Y, 3)
            r["gate_" + name] = r[name + "_over_yardstick"] <= r[name + "_allowed_ratio"]
        r["lce_k8_over_yardstick"] = round(r["lce_k8"]["median_ms"] / Y, 3)
        print(f"{kind}: timed, checking", file=sys.stderr, flush=True)
        table = BlockTable(torch, m0)
        exact["range_min_wrong"] = int((got_min != truth_range_min(torch, LCP, table, lo, hi, n)).sum())
        del table, m0
        exact["lce_k0"] = check_lce(torch, T, x, y, 0, n, got0)
        exact["lce_k8"] = check_lce(torch, T, x, y, 8, n, got8)
        r["all_exact"] = exact
        del T, SA, LCP, ISA, ISA2, mine, blob, out, x, y, lo, hi, both
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
