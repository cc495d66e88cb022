"""Sliding-window attention for packed queries over the KV cache, timings:
umfa_torch.varlen_kvcache_window_attention against entries whose code the change leaves untouched.  bf16, head_dim 128, H 32 / H_kv 8,
64-key pages, causal.  Device time only, section 3.1m's method: 20 calls captured in one CUDA graph, the median of 5 replays, three
repeats with the two legs alternating, the spread of the three medians reported for each leg.

  1. uniform decode: B 8, L_q 1, W in {1023, 4095}, L in {8k, 32k, 8k + 64}, against kvcache_window_attention on the same caches.
     Expected: new - existing <= the item-list pre-pass (--prepass-us, traced in a kernel-trace run of its own) + the two legs' spreads.
  2. cost follows the band on packed decode: 256 decode sequences at context L against varlen_kvcache_attention over caches whose context
     is W + 1.  Expected: <= that x (s + 1) / s x 1.05, s = ceil((W + 1) / 128) (section 3.1m's bound).
  3. independence from the context: t(L = 32k) / t(L = 8k) inside the same 5 %, for a decode batch of 2 and for the mixed batch
     1 x 2048 + 63 decode.
  4. the mixed batch against varlen_kvcache_attention unwindowed over the full context: the ratio, beside the ratio of keys read.  No bound.

One JSON line per leg and one per verdict, to profiles/varlen_paged_window/bench.jsonl (or --out).  --quick: 21 eager calls of each leg of
experiment 1 at one shape and of 256 packed decode sequences, no file (the input of a kernel trace)."""
from __future__ import annotations

import argparse
import itertools
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "universal-metal-flash-attention_amd"))
import umfa_torch as um  # noqa: E402

H, HKV, D, PS = 32, 8, 128, 64
WINDOWS = (1023, 4095)
CONTEXTS = (8192, 32768)
STRADDLE = 8192 + 64  # the band starts half a step into a step: s + 1 steps visited
SPREAD = 1.05
CALLS = 20


def batch(lq, L):
    """packed q for the lengths lq, every sequence with L cached keys behind a randomly permuted table"""
    g = torch.Generator(device="cuda").manual_seed(0)
    B, mp = len(lq), (L + PS - 1) // PS
    q = torch.randn(sum(lq), H, D, device="cuda", dtype=torch.bfloat16, generator=g)
    kc = torch.randn(B * mp, PS, HKV, D, device="cuda", dtype=torch.bfloat16, generator=g)
    vc = torch.randn(B * mp, PS, HKV, D, device="cuda", dtype=torch.bfloat16, generator=g)
    bt = torch.randperm(B * mp, device="cuda", generator=g).to(torch.int32).view(B, mp)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    cu = torch.tensor([0] + list(itertools.accumulate(lq)), dtype=torch.int32, device="cuda")
    return q, kc, vc, bt, sl, cu, max(lq)


def capture(fn):
    """(graph of CALLS calls, the kernel's name); fn runs before the capture: every scratch pool it needs exists"""
    fn()
    torch.cuda.synchronize()
    name = um.last_kernel()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        for _ in range(CALLS):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph, name


def median5(graph):
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / CALLS)
    return statistics.median(ts)


def timed(*fns):
    """[(median of three medians in us, their spread, kernel)] per leg, the legs alternating within each of the three repeats"""
    legs = [capture(f) for f in fns]
    meds = [[] for _ in legs]
    for _ in range(3):
        for m, (graph, _) in zip(meds, legs):
            m.append(median5(graph))
    return [(statistics.median(m), max(m) - min(m), name) for m, (_, name) in zip(meds, legs)]


def windowed(b, W):
    q, kc, vc, bt, sl, cu, mq = b
    return lambda: um.varlen_kvcache_window_attention(q, kc, vc, cu, mq, sl, block_table=bt, causal=True, window_size=(W, 0))


def unwindowed(b):
    q, kc, vc, bt, sl, cu, mq = b
    return lambda: um.varlen_kvcache_attention(q, kc, vc, cu, mq, sl, block_table=bt, causal=True)


def dense_windowed(b, W):
    q, kc, vc, bt, sl, _, mq = b
    q4 = q.view(sl.numel(), mq, H, D)
    return lambda: um.kvcache_window_attention(q4, kc, vc, cache_seqlens=sl, block_table=bt, causal=True, window_size=(W, 0))


def keys_read(lq, L, W):
    """keys the work items of one KV head read, causal, every sequence at L keys: an item of tokens [t0, t1] reads keys [max(0, t0 + off -
    W), t1 + off] (W None: from key 0); a decode-form sequence is one item, any other ceil(g L_q / 128) items of 128 / g tokens"""
    g = H // HKV
    total = 0
    for l in lq:
        per = l if g * l <= 32 else 128 // g
        for t0 in range(0, l, per):
            t1, off = min(t0 + per, l) - 1, L - l
            total += t1 + off + 1 - (0 if W is None else max(0, t0 + off - W))
    return total


def leg(route, r, **kw):
    return dict(route=route, kernel=r[2], graph_us=r[0], graph_spread_us=r[1], **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "varlen_paged_window" / "bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="eager calls at one window and context, no file (for a kernel trace)")
    ap.add_argument("--prepass-us", type=float, default=None, help="the item-list pre-pass's traced time (experiment 1's allowance)")
    ap.add_argument("--only", type=int, default=0, help="run one experiment (1 .. 4) alone")
    a = ap.parse_args()
    shape = dict(H=H, H_kv=HKV, D=D, page_size=PS, dtype="bf16", causal=True)
    out = None
    if not a.quick:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        out = open(a.out, "a")

    def emit(rec):
        rec = {**shape, **rec}
        print(json.dumps(rec), flush=True)
        if out:
            out.write(json.dumps(rec) + "\n")
            out.flush()

    want = lambda n: not a.only or a.only == n  # noqa: E731
    if a.quick:  # 20 eager calls of each leg of experiment 1 (B 8, 8k, W 1023) and of 256 packed decode sequences: a kernel trace's input
        for lq in ([1] * 8, [1] * 256):
            b = batch(lq, CONTEXTS[0])
            for f in (windowed(b, WINDOWS[0]),) + ((dense_windowed(b, WINDOWS[0]),) if len(lq) == 8 else ()):
                for _ in range(CALLS + 1):
                    f()
                torch.cuda.synchronize()
                print(json.dumps(dict(route="trace", B=len(lq), L=CONTEXTS[0], W=WINDOWS[0], kernel=um.last_kernel())), flush=True)
        return
    # 1. uniform decode against the dense window entry
    if want(1):
        for W in WINDOWS:
            for L in CONTEXTS + (STRADDLE,):
                b = batch([1] * 8, L)
                new, old = timed(windowed(b, W), dense_windowed(b, W))
                emit(leg("packed_window", new, exp=1, B=8, L=L, W=W))
                emit(leg("dense_window", old, exp=1, B=8, L=L, W=W))
                if a.prepass_us is not None:
                    allow = a.prepass_us + new[1] + old[1]
                    emit(dict(route="verdict", exp=1, B=8, L=L, W=W, diff_us=new[0] - old[0], prepass_us=a.prepass_us, allowance_us=allow,
                              packing_costs_the_prepass="met" if new[0] - old[0] <= allow else "missed"))
                del b
                torch.cuda.empty_cache()
    # 2. 256 decode sequences at context L against the unwindowed packed entry at context W + 1
    if want(2):
        for W in WINDOWS:
            s = -(-(W + 1) // 128)
            for L in CONTEXTS + (STRADDLE,):
                bw, bu = batch([1] * 256, L), batch([1] * 256, W + 1)
                new, base = timed(windowed(bw, W), unwindowed(bu))
                bound = base[0] * (s + 1) / s * SPREAD
                emit(leg("packed_window", new, exp=2, B=256, L=L, W=W))
                emit(leg("packed_unwindowed_at_W+1", base, exp=2, B=256, L=W + 1, W=W))
                emit(dict(route="verdict", exp=2, B=256, L=L, W=W, steps=s, window_us=new[0], unwindowed_us=base[0], bound_us=bound,
                          ratio_to_unwindowed=new[0] / base[0], cost_follows_band="met" if new[0] <= bound else "missed"))
                del bw, bu
                torch.cuda.empty_cache()
    # 3. / 4. the decode batch of 2 and the mixed batch at both contexts; the mixed batch against the unwindowed full context
    mixes = {"decode2": [1, 1], "mixed_2048+63": [2048] + [1] * 63}
    if want(3) or want(4):  # (one pass serves both)
        for W in WINDOWS:
            for tag, lq in mixes.items():
                ts = {}
                for L in CONTEXTS:
                    b = batch(lq, L)
                    fns = [windowed(b, W)] + ([unwindowed(b)] if tag != "decode2" else [])
                    res = timed(*fns)
                    ts[L] = res[0][0]
                    emit(leg("packed_window", res[0], exp=3, batch=tag, L=L, W=W))
                    if len(res) > 1:
                        keys_w, keys_u = keys_read(lq, L, W), keys_read(lq, L, None)
                        emit(leg("packed_unwindowed_full", res[1], exp=4, batch=tag, L=L, W=W))
                        emit(dict(route="report", exp=4, batch=tag, L=L, W=W, window_us=res[0][0], unwindowed_us=res[1][0],
                                  time_ratio=res[0][0] / res[1][0], keys_ratio=keys_w / keys_u))
                    del b
                    torch.cuda.empty_cache()
                ratio = ts[CONTEXTS[1]] / ts[CONTEXTS[0]]
                emit(dict(route="verdict", exp=3, batch=tag, W=W, window_us={str(L): t for L, t in ts.items()}, context_ratio=ratio,
                          independent_of_context="met" if 1 / SPREAD <= ratio <= SPREAD else "missed"))
    if out:
        out.close()


if __name__ == "__main__":
    main()
