"""Sliding-window KV-cache attention timings: umfa_torch.kvcache_window_attention against the existing unwindowed
kernel, whose code the window leaves untouched.  bf16, head_dim 128, H 32 / H_kv 8, B 8, causal, Sq 1 (a decode step), 64-key pages, every
sequence at the full context L; windows W in {1023, 4095} (W + 1 keys) at L in {8k, 32k}.  Device time only: 20 calls captured in one
CUDA graph, the median of 5 replays, three repeats, the spread of the three medians.

Two comparisons, neither against the new code itself:
  (a) cost follows the band: t_window(L, W) against t_unwindowed at context W + 1, expected <= t_unwindowed x (s + 1) / s x 1.05 with
      s = ceil((W + 1) / 128) -- one more step for a band that straddles a step boundary, 5 % for the spread of this route;
  (b) independence from the context: t_window(32k, W) / t_window(8k, W), expected inside that same 5 %.
The fixed contexts start every band on a step boundary; one more context, L = 8k + 64, makes the band straddle one (s + 1 steps) and is
held to (a)'s bound in a record of its own.  One JSON line per (W, L) and one per W with the verdicts, to
profiles/paged_window/bench.jsonl (or --out).  --quick: one shape, no file (for a kernel trace)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "universal-metal-flash-attention_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import umfa_torch as um  # noqa: E402
from bench_paged import graph_timed  # noqa: E402

H, HKV, D, B, PS = 32, 8, 128, 8, 64
WINDOWS = (1023, 4095)
CONTEXTS = (8192, 32768)
STRADDLE = 8192 + 64  # the band starts half a step into a step: s + 1 steps visited
SPREAD = 1.05


def cache(L):
    g = torch.Generator(device="cuda").manual_seed(0)
    mp = (L + PS - 1) // PS
    q = torch.randn(B, 1, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
    kc = torch.randn(B * mp, PS, HKV, D, device="cuda", dtype=torch.bfloat16, generator=g)
    vc = torch.randn(B * mp, PS, HKV, D, device="cuda", dtype=torch.bfloat16, generator=g)
    bt = torch.randperm(B * mp, device="cuda", generator=g).to(torch.int32).view(B, mp)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    return q, kc, vc, bt, sl


def unwindowed(L):
    q, kc, vc, bt, sl = cache(L)
    f = lambda: um.kvcache_attention(q, kc, vc, cache_seqlens=sl, block_table=bt, causal=True)  # noqa: E731
    f()
    torch.cuda.synchronize()
    name = um.last_kernel()
    t, spread = graph_timed(f)
    return dict(route="unwindowed", L=L, kernel=name, graph_us=t, graph_spread_us=spread)


def windowed(L, W):
    q, kc, vc, bt, sl = cache(L)
    f = lambda: um.kvcache_window_attention(q, kc, vc, cache_seqlens=sl, block_table=bt, causal=True, window_size=(W, 0))  # noqa: E731
    f()
    torch.cuda.synchronize()
    name = um.last_kernel()
    t, spread = graph_timed(f)
    return dict(route="window", L=L, W=W, kernel=name, graph_us=t, graph_spread_us=spread,
                band_TBps=B * (W + 1) * HKV * D * 2 * 2 / t / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "paged_window" / "bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="one window at both contexts and its unwindowed yardstick, no file (for a kernel trace)")
    a = ap.parse_args()
    shape = dict(B=B, Sq=1, H=H, H_kv=HKV, D=D, page_size=PS, dtype="bf16", causal=True)
    out = None
    if not a.quick:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        out = open(a.out, "a")

    def emit(rec):
        rec = {**shape, **rec}
        print(json.dumps(rec), flush=True)
        if out:
            out.write(json.dumps(rec) + "\n")

    for W in WINDOWS[:1] if a.quick else WINDOWS:
        base = unwindowed(W + 1)
        emit(base)
        ts = {}
        for L in CONTEXTS:
            rec = windowed(L, W)
            ts[L] = rec["graph_us"]
            emit(rec)
            torch.cuda.empty_cache()
        s = -(-(W + 1) // 128)
        bound = base["graph_us"] * (s + 1) / s * SPREAD
        ratio = ts[CONTEXTS[1]] / ts[CONTEXTS[0]]
        emit(dict(route="verdict", W=W, steps=s, unwindowed_us=base["graph_us"], bound_us=bound,
                  window_us={str(L): t for L, t in ts.items()},
                  a_cost_follows_band={str(L): ("met" if t <= bound else "missed") for L, t in ts.items()},
                  a_ratio_to_unwindowed={str(L): t / base["graph_us"] for L, t in ts.items()},
                  b_context_ratio=ratio, b_independent_of_context="met" if 1 / SPREAD <= ratio <= SPREAD else "missed"))
        if not a.quick:
            rec = windowed(STRADDLE, W)
            emit(rec)
            emit(dict(route="verdict_straddle", W=W, L=STRADDLE, steps_visited=s + 1, unwindowed_us=base["graph_us"], bound_us=bound,
                      window_us=rec["graph_us"], a_ratio_to_unwindowed=rec["graph_us"] / base["graph_us"],
                      a_cost_follows_band="met" if rec["graph_us"] <= bound else "missed"))
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
