"""fp8 KV-cache attention timings: umfa_torch.kvcache_attention on a float8_e4m3fn paged cache with per-head
descales against the unchanged 16-bit call on a bf16 cache of the same geometry, in one process and alternating (fp8, 16-bit, fp8, ...
per repeat).  bf16 q, head_dim 128, H 32 / H_kv 8, every sequence at the full context, non-causal.  Timing as tools/bench_paged.py: device
time per call from 20 calls captured in one graph (median of 5 replays, three repeats with their spread) and the host-inclusive time
around one Python call beside it.  One JSON line per shape to profiles/paged_fp8/bench.jsonl (or --out); TB/s counts the K and V bytes
each call reads (fp8: sum L_k H_kv D x 2 bytes; 16-bit: twice that).  --quick: one shape, nothing written (for a kernel trace, or an ablation
leg with --tag)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "universal-metal-flash-attention_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import umfa_torch as um  # noqa: E402
from bench_paged import timed  # noqa: E402

H, HKV, D = 32, 8, 128


def capture(fn, calls=20):
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
    return graph


def replay_us(graph, calls=20):
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / calls)
    return statistics.median(ts)


def shape(B, L, ps, Sq, warmup, iters, splits=0):
    g = torch.Generator(device="cuda").manual_seed(0)
    mp = (L + ps - 1) // ps
    q = torch.randn(B, Sq, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
    kc = torch.randn(B * mp, ps, HKV, D, device="cuda", dtype=torch.bfloat16, generator=g)
    vc = torch.randn(B * mp, ps, HKV, D, device="cuda", dtype=torch.bfloat16, generator=g)
    kd = torch.full((HKV,), 2.0 ** -5, device="cuda")
    vd = torch.full((HKV,), 2.0 ** -5, device="cuda")
    k8, v8 = (kc.float() * 32).to(torch.float8_e4m3fn), (vc.float() * 32).to(torch.float8_e4m3fn)
    bt = torch.randperm(B * mp, device="cuda", generator=g).to(torch.int32).view(B, mp)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    rec = dict(B=B, L=L, page_size=ps, Sq=Sq, H=H, H_kv=HKV, D=D, dtype="bf16", num_splits=splits)
    f8 = lambda: um.kvcache_attention(q, k8, v8, cache_seqlens=sl, block_table=bt, num_splits=splits, k_descale=kd, v_descale=vd)  # noqa: E731
    f16 = lambda: um.kvcache_attention(q, kc, vc, cache_seqlens=sl, block_table=bt, num_splits=splits)  # noqa: E731
    rec["fp8_us"], rec["fp8_spread_us"] = timed(f8, warmup, iters)
    rec["fp8_kernel"] = um.last_kernel()
    rec["bf16_us"], rec["bf16_spread_us"] = timed(f16, warmup, iters)
    rec["bf16_kernel"] = um.last_kernel()
    g8, g16 = capture(f8), capture(f16)
    m8, m16 = [], []
    for _ in range(3):  # alternating: both legs see the same clocks and neighbours
        m8.append(replay_us(g8))
        m16.append(replay_us(g16))
    rec["fp8_graph_us"], rec["fp8_graph_spread_us"] = statistics.median(m8), max(m8) - min(m8)
    rec["bf16_graph_us"], rec["bf16_graph_spread_us"] = statistics.median(m16), max(m16) - min(m16)
    rec["graph_ratio"] = rec["fp8_graph_us"] / rec["bf16_graph_us"]
    rec["ratio_lo"], rec["ratio_hi"] = min(m8) / max(m16), max(m8) / min(m16)
    bytes8 = B * L * HKV * D * 2
    rec["fp8_graph_TBps"] = bytes8 / rec["fp8_graph_us"] / 1e6
    rec["bf16_graph_TBps"] = 2 * bytes8 / rec["bf16_graph_us"] / 1e6
    del g8, g16
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "paged_fp8" / "bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="one decode shape only, nothing written (for a kernel trace)")
    ap.add_argument("--tag", default="", help="recorded in every line (an ablation leg: UMFA_LIBRARY names the build)")
    a = ap.parse_args()
    if a.quick:
        shapes = [(8, 32768, 64, 1)]
    else:
        shapes = [(B, L, ps, Sq) for (B, L) in ((8, 2048), (8, 8192), (8, 32768), (32, 8192), (64, 8192)) for ps in (16, 64) for Sq in (1, 4)]
        shapes += [(1, 131072, 64, 1), (1, 131072, 64, 4)]
    out = None if a.quick else open(a.out, "a")
    for B, L, ps, Sq in shapes:
        rec = shape(B, L, ps, Sq, a.warmup, a.iters)
        if a.tag:
            rec["tag"] = a.tag
        print(json.dumps(rec), flush=True)
        if out:
            out.write(json.dumps(rec) + "\n")
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
