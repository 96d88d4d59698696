"""Rates of the collection k-mer calls (include/caps_sa_hip.h "k-mers across a collection", caps_sa_hip_coll_*_device_u32).

    python tools/coll_rate.py [--warm 2] [--runs 7] [--n-bases 3000000000] [--out profiles/coll_rate_c3.json]

One process, HIP events, --warm warm-up runs + --runs timed ones, median / min / max ms, u32, k = 31.  SA and LCP stay resident.

Workload 1, the streaming cost: the bench's C3 text (bench.make_text "uniform", --n-bases bases + the trailing 'C') cut into 24 equal
documents.  Nearly every 31-mer is unique, so the matrix path is idle.  The yardstick, NOT the code under test: R =
torch.count_nonzero(dLCP < 31) on the same tensor in the same process.
GATE, for the coll_sharing call and for the coll_kmers counting call: at most 2.5 x R.

Workload 2, no gate: 8 documents -- a stream of --n-bases / 8 bases and 7 copies with one substitution per 100 bases (block i of 100
bases of copy c: the base at offset ((i + c * 1000003) * 6364136223846793005 + 1442695040888963407 mod 2^64) >> 33 mod 100 becomes the
next letter of ACGT), each followed by one 0xFF byte.  Most k-mers carry several bits.  Both calls, and counting + writing at
min_docs = 8.  Checked exactly in the same run: every freq and shared value against tensor ops on the device (documents by
torch.bucketize, runs by a cumulative sum over the heads, in chunks that end at a head), and the record count against freq.
Prints one JSON object (and writes it to --out).  Needs no network and no file but this repository's.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHUNK = 1 << 28                                        # ranks per chunk of the check
K = 31


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


def eight_documents(torch, part, dev):
    """(T, docs): the stream and 7 mutated copies, a 0xFF byte behind each."""
    from bench import make_text
    A = make_text(torch, part, 42, dev, "uniform")[:part]
    T = torch.empty(8 * (part + 1), dtype=torch.uint8, device=dev)
    nxt = torch.arange(256, dtype=torch.uint8, device=dev)
    for a, b in zip(b"ACGT", b"CGTA"):
        nxt[a] = b
    docs = []
    blocks = part // 100
    step = 1 << 26
    for c in range(8):
        s = c * (part + 1)
        B = T[s:s + part]
        B.copy_(A)
        T[s + part] = 0xFF
        docs.append((s, part))
        if c == 0:
            continue
        for o in range(0, blocks, step):
            i = torch.arange(o, min(o + step, blocks), dtype=torch.int64, device=dev)
            x = (((i + c * 1000003) * 6364136223846793005 + 1442695040888963407) >> 33) & 0x7FFFFFFF    # (int64 arithmetic wraps)
            at = i * 100 + x % 100
            B[at] = nxt[B[at].long()]
    return T, docs


def truth(torch, SA, LCP, n, k, docs):
    """(freq[65], shared[m, m]) by the header's rules in tensor ops."""
    dev = SA.device
    m = len(docs)
    starts = torch.tensor([s for s, _ in docs], dtype=torch.int64, device=dev)
    ends = torch.tensor([s + l for s, l in docs], dtype=torch.int64, device=dev)
    freq = torch.zeros(65, dtype=torch.int64, device=dev)
    shared = torch.zeros((m, m), dtype=torch.int64, device=dev)
    a = 0
    while a < n:
        b = min(a + CHUNK, n)
        while b < n:                                    # the chunk ends at the next head
            w = min(b + (1 << 20), n)
            nz = torch.nonzero((LCP[b:w].to(torch.int64) & 0xFFFFFFFF) < k).view(-1)
            if nz.numel():
                b += int(nz[0])
                break
            b = w
        head = (LCP[a:b].to(torch.int64) & 0xFFFFFFFF) < k
        head[0] = True
        rid = torch.cumsum(head, 0) - 1
        runs = int(rid[-1]) + 1
        del head
        sa = SA[a:b].to(torch.int64) & 0xFFFFFFFF
        d = torch.bucketize(sa, starts, right=True) - 1
        dd = d.clamp(min=0)
        inn = (d >= 0) & (sa + k <= ends[dd])
        del sa, d
        mask = torch.zeros(runs, dtype=torch.int64, device=dev)
        for bit in range(m):
            present = torch.zeros(runs, dtype=torch.bool, device=dev)
            present[rid[inn & (dd == bit)]] = True
            mask |= present.to(torch.int64) << bit
            del present
        del rid, dd, inn
        mask = mask[mask != 0]
        bits = [((mask >> x) & 1) for x in range(m)]
        freq += torch.bincount(sum(bits), minlength=65)
        for x in range(m):
            for y in range(x, m):
                c = torch.count_nonzero(bits[x] & bits[y])
                shared[x, y] += c
                if y != x:
                    shared[y, x] += c
        del mask, bits
        torch.cuda.empty_cache()
        a = b
    return freq.cpu().numpy().astype("uint64"), shared.cpu().numpy().astype("uint64")


def measure(torch, L, T, docs, a, write_min_docs=None, check=False):
    import numpy as np
    dev = T.device
    n = T.numel()
    SA = torch.empty(n, dtype=torch.int32, device=dev)
    LCP = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    L.build_device(T.data_ptr(), n, SA.data_ptr(), LCP.data_ptr(), p=8000)
    del T
    print(f"built, n = {n}, {len(docs)} documents", file=sys.stderr, flush=True)
    wsb = L.coll_workspace_bytes(n, 32)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    S, Lp, W = SA.data_ptr(), LCP.data_ptr(), ws.data_ptr()
    res = {"n": n, "documents": len(docs), "workspace_bytes": wsb}
    got = {}
    res["yardstick_count_nonzero"] = _summary(_timed(torch, lambda: got.__setitem__("R", torch.count_nonzero(LCP < K)), a.warm, a.runs))
    res["coll_sharing"] = _summary(_timed(torch, lambda: got.__setitem__("s", L.coll_sharing_device(S, Lp, n, K, docs, W, wsb)), a.warm, a.runs))
    res["coll_kmers_count"] = _summary(_timed(torch, lambda: got.__setitem__("c", L.coll_kmers_device(S, Lp, n, K, docs, dWS_ptr=W, ws_bytes=wsb)),
                                              a.warm, a.runs))
    R = res["yardstick_count_nonzero"]["median_ms"]
    res["sharing_over_yardstick"] = round(res["coll_sharing"]["median_ms"] / R, 3)
    res["count_over_yardstick"] = round(res["coll_kmers_count"]["median_ms"] / R, 3)
    freq, shared = got["s"]
    res["collection_kmers"] = int(got["c"])
    res["freq"] = {str(c): int(freq[c]) for c in range(1, len(docs) + 1)}
    res["shared_diagonal"] = [int(shared[d, d]) for d in range(len(docs))]
    exact = {"count_equals_sum_of_freq": int(got["c"]) == int(freq.sum())}
    if write_min_docs:
        found = L.coll_kmers_device(S, Lp, n, K, docs, min_docs=write_min_docs, dWS_ptr=W, ws_bytes=wsb)
        rec = torch.empty((max(found, 1), 4), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        write = lambda: L.coll_kmers_device(S, Lp, n, K, docs, min_docs=write_min_docs, dRecords_ptr=rec.data_ptr(), capacity=found, dWS_ptr=W,
                                            ws_bytes=wsb)
        res[f"coll_kmers_write_min_docs_{write_min_docs}"] = _summary(_timed(torch, write, a.warm, a.runs))
        res[f"coll_kmers_write_min_docs_{write_min_docs}"]["records"] = found
        exact["records_equal_freq_of_all"] = found == int(freq[len(docs)])
        exact["records_carry_every_bit"] = bool((rec[:found, 3] == (1 << len(docs)) - 1).all())
        del rec
    if check:
        print("timed, checking", file=sys.stderr, flush=True)
        wf, wsh = truth(torch, SA, LCP, n, K, docs)
        exact["freq_equals_tensor_ops"] = bool(np.array_equal(freq, wf))
        exact["shared_equals_tensor_ops"] = bool(np.array_equal(shared, wsh))
    res["all_exact"] = exact
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--n-bases", type=int, default=3_000_000_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import caps_sa_amd
    from bench import make_text
    L = caps_sa_amd.lib()
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "warm": a.warm, "runs": a.runs, "measured_on": "MI355X (this run)", "k": K, "gate_factor": 2.5}
    T = make_text(torch, a.n_bases, 42, dev, "uniform")
    part = T.numel() // 24
    docs = [(d * part, part) for d in range(24)]
    w1 = measure(torch, L, T, docs, a)
    del T
    R = w1["yardstick_count_nonzero"]["median_ms"]
    w1["gate_sharing"] = w1["coll_sharing"]["median_ms"] <= 2.5 * R
    w1["gate_count"] = w1["coll_kmers_count"]["median_ms"] <= 2.5 * R
    res["c3_24_documents"] = w1
    torch.cuda.empty_cache()
    T, docs = eight_documents(torch, a.n_bases // 8, dev)
    res["eight_similar_documents"] = measure(torch, L, T, docs, a, write_min_docs=8, check=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
