"""Packed variable-length queries over the paged KV cache: timings, on tools/bench_paged.py's protocol.
bf16, head_dim 128, H 32 / H_kv 8.  Every leg of a comparison is timed in the same session with the legs ALTERNATING inside each of the
three repeats: device time per call of 20 calls captured in one CUDA graph, median of 5 replays per repeat, the median and the spread of
the three repeats (the *_graph_us / *_graph_spread_us fields); host-inclusive time around the Python call beside it (*_us), never
instead of it.  One JSON line per shape to profiles/varlen_paged/bench.jsonl (or --out).

  uniform: tools/bench_paged.py's shapes (every sequence at the full context, non-causal, Sq 1 and 4) --
           varlen_kvcache_attention against kvcache_attention on the same data (the same work plus the item-list pre-pass).
  mixed:   causal, page 16 and 64: 1 x 2048-token chunk + 63 decode at 8k context, 4 x 512 + 124 decode, 256 decode only --
           against (a) kvcache_attention on q padded to [B, max L_q] and (b) one kvcache_attention call per distinct L_q.
  --trace NAME: a few eager calls of one mixed shape and nothing else (for rocprofv3 --kernel-trace --stats)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "universal-metal-flash-attention_amd"))
import umfa_torch as um  # noqa: E402

H, HKV, D = 32, 8, 128
DT = torch.bfloat16


def host_timed(fns, warmup, iters):
    """{name: (median us, spread)} around the Python call; the legs alternate inside every repeat"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    meds = {n: [] for n in fns}
    for _ in range(3):
        for n, fn in fns.items():
            ts = []
            for _ in range(iters):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            meds[n].append(statistics.median(ts))
    return {n: (statistics.median(m), max(m) - min(m)) for n, m in meds.items()}


def graph_timed(fns, reps=3, calls=20):
    """{name: (median us per call, spread)} of device time: `calls` calls captured in one CUDA graph per leg, 5 replays per repeat, the
    legs alternating inside every repeat (every fn has run before: its scratch exists)"""
    graphs = {}
    for n, fn in fns.items():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(calls):
                fn()
        g.replay()
        torch.cuda.synchronize()
        graphs[n] = g
    meds = {n: [] for n in fns}
    for _ in range(reps):
        for n, g in graphs.items():
            ts = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                g.replay()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3 / calls)
            meds[n].append(statistics.median(ts))
    graphs.clear()
    return {n: (statistics.median(m), max(m) - min(m)) for n, m in meds.items()}


def pool(B, L, ps, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mp = (L + ps - 1) // ps
    kc = torch.randn(B * mp, ps, HKV, D, device="cuda", dtype=DT, generator=g)
    vc = torch.randn(B * mp, ps, HKV, D, device="cuda", dtype=DT, generator=g)
    bt = torch.randperm(B * mp, device="cuda", generator=g).to(torch.int32).view(B, mp)
    return kc, vc, bt, g


def measure(rec, fns, warmup, iters):
    host = host_timed(fns, warmup, iters)
    dev = graph_timed(fns)
    for n in fns:
        rec[f"{n}_us"], rec[f"{n}_spread_us"] = host[n]
        rec[f"{n}_graph_us"], rec[f"{n}_graph_spread_us"] = dev[n]
    return rec


def uniform(B, L, ps, Sq, warmup, iters):
    kc, vc, bt, g = pool(B, L, ps)
    q = torch.randn(B, Sq, H, D, device="cuda", dtype=DT, generator=g)
    qp = q.view(B * Sq, H, D)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * Sq
    rec = dict(kind="uniform", B=B, L=L, page_size=ps, Sq=Sq, H=H, H_kv=HKV, D=D, dtype="bf16")
    fns = {"kvcache": lambda: um.kvcache_attention(q, kc, vc, cache_seqlens=sl, block_table=bt),
           "varlen": lambda: um.varlen_kvcache_attention(qp, kc, vc, cu, Sq, sl, block_table=bt)}
    fns["varlen"]()
    rec["kernel"] = um.last_kernel()
    fns["kvcache"]()
    rec["kvcache_kernel"] = um.last_kernel()
    measure(rec, fns, warmup, iters)
    rec["graph_delta_us"] = rec["varlen_graph_us"] - rec["kvcache_graph_us"]
    rec["graph_ratio"] = rec["varlen_graph_us"] / rec["kvcache_graph_us"]
    return rec


MIXED = {"chunk2048_decode63": [2048] + [1] * 63, "chunk512x4_decode124": [512] * 4 + [1] * 124, "decode256": [1] * 256}


def mixed_setup(name, ps, L=8192):
    lq = MIXED[name]
    B, Tq = len(lq), sum(lq)
    kc, vc, bt, g = pool(B, L, ps)
    q = torch.randn(Tq, H, D, device="cuda", dtype=DT, generator=g)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    cu = torch.tensor([0] + list(torch.tensor(lq).cumsum(0)), dtype=torch.int32, device="cuda")
    return lq, q, kc, vc, bt, sl, cu


def mixed(name, ps, warmup, iters, L=8192):
    lq, q, kc, vc, bt, sl, cu = mixed_setup(name, ps, L)
    B, Tq, mx = len(lq), sum(lq), max(lq)
    rec = dict(kind="mixed", shape=name, B=B, T_q=Tq, max_seqlen_q=mx, L=L, page_size=ps, H=H, H_kv=HKV, D=D, dtype="bf16", causal=True)
    fns = {"varlen": lambda: um.varlen_kvcache_attention(q, kc, vc, cu, mx, sl, block_table=bt, causal=True)}
    if mx > 1:
        # (a) q padded to [B, max L_q] (at the front: bottom-right causal then gives the real rows their keys)
        qpad = torch.zeros(B, mx, H, D, device="cuda", dtype=DT)
        off = 0
        for b, l in enumerate(lq):
            qpad[b, mx - l:] = q[off:off + l]
            off += l
        fns["padded"] = lambda: um.kvcache_attention(qpad, kc, vc, cache_seqlens=sl, block_table=bt, causal=True)
        # (b) one call per distinct L_q (the groups' q, table rows and lengths are gathered outside the timing)
        groups, off = {}, 0
        for b, l in enumerate(lq):
            groups.setdefault(l, []).append((b, off))
            off += l
        calls = []
        for l, members in groups.items():
            idx = torch.tensor([b for b, _ in members], device="cuda")
            qg = torch.stack([q[o:o + l] for _, o in members])
            calls.append((qg, sl[idx].contiguous(), bt[idx].contiguous()))
        rec["groups"] = len(calls)

        def grouped():
            return [um.kvcache_attention(qg, kc, vc, cache_seqlens=s, block_table=t, causal=True) for qg, s, t in calls]

        fns["grouped"] = grouped
    else:
        q4 = q.view(B, 1, H, D)
        fns["kvcache"] = lambda: um.kvcache_attention(q4, kc, vc, cache_seqlens=sl, block_table=bt, causal=True)
    fns["varlen"]()
    rec["kernel"] = um.last_kernel()
    rec["items_decode"], rec["items_128row"] = um.ops.varlen_kvcache_item_counts()
    measure(rec, fns, warmup, iters)
    for n in fns:
        if n != "varlen":
            rec[f"graph_speedup_vs_{n}"] = rec[f"{n}_graph_us"] / rec["varlen_graph_us"]
    if mx == 1:
        bytes_kv = B * L * HKV * D * 2 * 2
        rec["varlen_graph_TBps"] = bytes_kv / rec["varlen_graph_us"] / 1e6
        rec["kvcache_graph_TBps"] = bytes_kv / rec["kvcache_graph_us"] / 1e6
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "varlen_paged" / "bench.jsonl"))
    ap.add_argument("--only", choices=["uniform", "mixed"], default=None)
    ap.add_argument("--trace", default="", help="a MIXED shape name: a few eager calls of it at page 64 and nothing else")
    a = ap.parse_args()
    if a.trace:
        lq, q, kc, vc, bt, sl, cu = mixed_setup(a.trace, 64)
        for _ in range(20):
            um.varlen_kvcache_attention(q, kc, vc, cu, max(lq), sl, block_table=bt, causal=True)
        torch.cuda.synchronize()
        print(um.last_kernel(), um.ops.varlen_kvcache_item_counts())
        return
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    out = open(a.out, "a")

    def emit(rec):
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
        out.flush()
        torch.cuda.empty_cache()

    if a.only != "mixed":
        for B, L in ((8, 2048), (8, 8192), (8, 32768), (32, 8192), (64, 2048), (64, 8192)):
            for ps in (16, 64, 256):
                for Sq in (1, 4):
                    emit(uniform(B, L, ps, Sq, a.warmup, a.iters))
    if a.only != "uniform":
        for name in MIXED:
            for ps in (16, 64):
                emit(mixed(name, ps, a.warmup, a.iters))
    out.close()


if __name__ == "__main__":
    main()
