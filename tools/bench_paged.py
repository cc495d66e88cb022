"""KV-cache attention timings: umfa_torch.kvcache_attention on a paged cache against (i) the dense GQA route
umfa_torch.scaled_dot_product_attention on an already contiguous cache, (ii) gathering the pages first + that route, (iii) torch's SDPA on
the gathered tensors.  bf16, head_dim 128, H 32 / H_kv 8, every sequence at the full context, non-causal (the same keys for every route).
One JSON line per shape to profiles/paged/bench.jsonl (or --out): medians of --iters timed calls after --warmup, three repeats, the
spread of the three medians; TB/s counts the K and V bytes the attention reads (sum L_k H_kv D 2 B x 2).  Every route is timed twice:
around the Python call (host dispatch included: the *_us fields) and as device time per call of 20 calls captured in one CUDA graph
(the *_graph_us fields).  --ab TAG: a subset of shapes, the paged route only (an A/B of two library builds, UMFA_LIBRARY)."""
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


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    meds = []
    for _ in range(3):
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        meds.append(statistics.median(ts))
    return statistics.median(meds), max(meds) - min(meds)


def graph_timed(fn, reps=3, calls=20):
    """device time per call without host dispatch: `calls` calls captured in one CUDA graph, replayed; median over 5 replays, three
    repeats (fn has run before: every scratch pool it needs exists)"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        for _ in range(calls):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    meds = []
    for _ in range(reps):
        ts = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / calls)
        meds.append(statistics.median(ts))
    del graph
    return statistics.median(meds), max(meds) - min(meds)


def shape(B, L, ps, Sq, warmup, iters, splits=0, baselines=True):
    dt = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    mp = (L + ps - 1) // ps
    q = torch.randn(B, Sq, H, D, device="cuda", dtype=dt, generator=g)
    kc = torch.randn(B * mp, ps, HKV, D, device="cuda", dtype=dt, generator=g)
    vc = torch.randn(B * mp, ps, HKV, D, device="cuda", dtype=dt, generator=g)
    bt = torch.randperm(B * mp, device="cuda", generator=g).to(torch.int32).view(B, mp)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    rec = dict(B=B, L=L, page_size=ps, Sq=Sq, H=H, H_kv=HKV, D=D, dtype="bf16", num_splits=splits)
    bytes_kv = B * L * HKV * D * 2 * 2
    f = lambda: um.kvcache_attention(q, kc, vc, cache_seqlens=sl, block_table=bt, num_splits=splits)  # noqa: E731
    rec["paged_us"], rec["paged_spread_us"] = timed(f, warmup, iters)
    rec["kernel"] = um.last_kernel()
    rec["paged_TBps"] = bytes_kv / rec["paged_us"] / 1e6
    rec["paged_graph_us"], rec["paged_graph_spread_us"] = graph_timed(f)
    rec["paged_graph_TBps"] = bytes_kv / rec["paged_graph_us"] / 1e6
    if baselines:
        qd = q.transpose(1, 2).contiguous()

        def gather():
            idx = bt.long()
            return (kc[idx].view(B, mp * ps, HKV, D)[:, :L].transpose(1, 2).contiguous(),
                    vc[idx].view(B, mp * ps, HKV, D)[:, :L].transpose(1, 2).contiguous())

        kd, vd = gather()
        dense = lambda: um.scaled_dot_product_attention(qd, kd, vd, enable_gqa=True)  # noqa: E731
        rec["dense_us"], rec["dense_spread_us"] = timed(dense, warmup, iters)
        rec["dense_kernel"] = um.last_kernel()
        rec["dense_graph_us"], rec["dense_graph_spread_us"] = graph_timed(dense)

        def gd():
            k2, v2 = gather()
            return um.scaled_dot_product_attention(qd, k2, v2, enable_gqa=True)

        rec["gather_dense_us"], rec["gather_dense_spread_us"] = timed(gd, warmup, iters)
        rec["gather_dense_graph_us"], rec["gather_dense_graph_spread_us"] = graph_timed(gd)

        def gt():
            k2, v2 = gather()
            return torch.nn.functional.scaled_dot_product_attention(qd, k2, v2, enable_gqa=True)

        rec["gather_torch_us"], rec["gather_torch_spread_us"] = timed(gt, warmup, iters)
        rec["vs_dense"] = rec["paged_us"] / rec["dense_us"]
        rec["vs_gather_dense"] = rec["paged_us"] / rec["gather_dense_us"]
        rec["graph_vs_dense"] = rec["paged_graph_us"] / rec["dense_graph_us"]
        rec["graph_vs_gather_dense"] = rec["paged_graph_us"] / rec["gather_dense_graph_us"]
        del kd, vd
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "paged" / "bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="one decode shape only (for a kernel trace)")
    ap.add_argument("--ab", default="", help="tag of an A/B leg: a subset of shapes, the paged route only, the tag in every record")
    a = ap.parse_args()
    if a.quick:
        shapes = [(8, 8192, 64, 1)]
    elif a.ab:
        shapes = [(8, 8192, 16, 1), (8, 32768, 64, 1), (64, 8192, 64, 1), (64, 8192, 16, 4)]
    else:
        shapes = [(B, L, ps, Sq) for (B, L) in ((8, 2048), (8, 8192), (8, 32768), (32, 8192), (64, 2048), (64, 8192))
                  for ps in (16, 64, 256) for Sq in (1, 4)]
    out = open(a.out, "a") if not a.quick else None
    for B, L, ps, Sq in shapes:
        rec = shape(B, L, ps, Sq, a.warmup, a.iters, baselines=not a.ab)
        if a.ab:
            rec["ab"] = a.ab
        print(json.dumps(rec), flush=True)
        if out:
            out.write(json.dumps(rec) + "\n")
        torch.cuda.empty_cache()
    if not a.quick:  # one long sequence, split over the CUs
        for ps in ((64,) if a.ab else (64, 256)):
            rec = shape(1, 131072, ps, 1, a.warmup, a.iters, baselines=not a.ab)
            if a.ab:
                rec["ab"] = a.ab
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
        out.close()


if __name__ == "__main__":
    main()
