"""Packed variable-length queries over an fp8 (e4m3fn) paged KV cache: timings, on tools/bench_varlen_paged.py's
protocol and helpers.  bf16 q, head_dim 128, H 32 / H_kv 8, per-(sequence, KV head) descales.  Device time per call of 20 calls captured
in one CUDA graph, median of 5 replays per repeat, the median and the spread of three repeats with the legs ALTERNATING inside each
repeat.  Every yardstick is taken in the same session from code this feature does not touch.  One JSON line per shape to
profiles/varlen_paged_fp8/bench.jsonl (or --out).

  uniform: every sequence at the full context, non-causal, Sq 1 and 4; four legs -- varlen8 (the new entry), kvcache8 (kvcache_attention's
           fp8 call), varlen16 and kvcache16 (the 16-bit entries on a 16-bit pool of the same geometry).  Yardstick (a): varlen8 -
           kvcache8 against the allowance (varlen16 - kvcache16) + twice the larger spread.
  mixed:   tools/bench_varlen_paged.py's three causal shapes at 8k context, page 16 and 64: varlen8 against varlen16; on the decode-only
           shape kvcache8 against kvcache16 as well.  Yardstick (b): varlen8 / varlen16 of each shape against kvcache8 / kvcache16 of
           the decode-only shape at the same page size, margin = the two ratios' combined spread (the `summary` records).
  --trace NAME: a few eager calls of one mixed shape and nothing else (for rocprofv3 --kernel-trace --stats)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import bench_varlen_paged as bv  # noqa: E402  (puts the package on sys.path)

um = bv.um
H, HKV, D, DT = bv.H, bv.HKV, bv.D, bv.DT
F8 = torch.float8_e4m3fn


def pools(B, L, ps):
    """a 16-bit pool and an fp8 pool of the same geometry under one block table, [B, H_kv] descales"""
    kc, vc, bt, g = bv.pool(B, L, ps)
    k8, v8 = (kc * 4).clamp(-448, 448).to(F8), (vc * 4).clamp(-448, 448).to(F8)
    kd = torch.rand(B, HKV, device="cuda", generator=g) * 0.5 + 0.25
    vd = torch.rand(B, HKV, device="cuda", generator=g) * 0.5 + 0.25
    return kc, vc, k8, v8, bt, kd, vd, g


def graph_measure(rec, fns):
    for fn in fns.values():  # scratch grows outside the capture
        fn()
    torch.cuda.synchronize()
    for n, (med, spread) in bv.graph_timed(fns).items():
        rec[f"{n}_graph_us"], rec[f"{n}_graph_spread_us"] = med, spread
    return rec


def uniform(B, L, ps, Sq):
    kc, vc, k8, v8, bt, kd, vd, g = pools(B, L, ps)
    q = torch.randn(B, Sq, H, D, device="cuda", dtype=DT, generator=g)
    qp = q.view(B * Sq, H, D)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * Sq
    rec = dict(kind="uniform", B=B, L=L, page_size=ps, Sq=Sq, H=H, H_kv=HKV, D=D, dtype="bf16", cache="e4m3fn")
    fns = {"varlen8": lambda: um.varlen_kvcache_attention(qp, k8, v8, cu, Sq, sl, block_table=bt, k_descale=kd, v_descale=vd),
           "kvcache8": lambda: um.kvcache_attention(q, k8, v8, cache_seqlens=sl, block_table=bt, k_descale=kd, v_descale=vd),
           "varlen16": lambda: um.varlen_kvcache_attention(qp, kc, vc, cu, Sq, sl, block_table=bt),
           "kvcache16": lambda: um.kvcache_attention(q, kc, vc, cache_seqlens=sl, block_table=bt)}
    fns["varlen8"]()
    rec["kernel"] = um.last_kernel()
    graph_measure(rec, fns)
    spread = max(rec[f"{n}_graph_spread_us"] for n in fns)
    rec["gap8_us"] = rec["varlen8_graph_us"] - rec["kvcache8_graph_us"]
    rec["gap16_us"] = rec["varlen16_graph_us"] - rec["kvcache16_graph_us"]
    rec["allowance_us"] = rec["gap16_us"] + 2 * spread
    rec["met_a"] = rec["gap8_us"] <= rec["allowance_us"]
    rec["varlen8_over_varlen16"] = rec["varlen8_graph_us"] / rec["varlen16_graph_us"]
    return rec


def mixed(name, ps, L=8192):
    lq = bv.MIXED[name]
    B, Tq, mx = len(lq), sum(lq), max(lq)
    kc, vc, k8, v8, bt, kd, vd, g = pools(B, L, ps)
    q = torch.randn(Tq, H, D, device="cuda", dtype=DT, generator=g)
    sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    cu = torch.tensor([0] + list(torch.tensor(lq).cumsum(0)), dtype=torch.int32, device="cuda")
    rec = dict(kind="mixed", shape=name, B=B, T_q=Tq, max_seqlen_q=mx, L=L, page_size=ps, H=H, H_kv=HKV, D=D, dtype="bf16", cache="e4m3fn",
               causal=True)
    fns = {"varlen8": lambda: um.varlen_kvcache_attention(q, k8, v8, cu, mx, sl, block_table=bt, causal=True, k_descale=kd, v_descale=vd),
           "varlen16": lambda: um.varlen_kvcache_attention(q, kc, vc, cu, mx, sl, block_table=bt, causal=True)}
    if mx == 1:
        q4 = q.view(B, 1, H, D)
        fns["kvcache8"] = lambda: um.kvcache_attention(q4, k8, v8, cache_seqlens=sl, block_table=bt, causal=True, k_descale=kd, v_descale=vd)
        fns["kvcache16"] = lambda: um.kvcache_attention(q4, kc, vc, cache_seqlens=sl, block_table=bt, causal=True)
    fns["varlen8"]()
    rec["kernel"] = um.last_kernel()
    rec["items_decode"], rec["items_128row"] = um.ops.varlen_kvcache_item_counts()
    graph_measure(rec, fns)
    rec["varlen8_over_varlen16"] = rec["varlen8_graph_us"] / rec["varlen16_graph_us"]
    if mx == 1:
        rec["kvcache8_over_kvcache16"] = rec["kvcache8_graph_us"] / rec["kvcache16_graph_us"]
    return rec


def rel_spread(rec, a, b):
    """the spread of the ratio a / b, first order: the two legs' relative spreads added"""
    return rec[f"{a}_graph_spread_us"] / rec[f"{a}_graph_us"] + rec[f"{b}_graph_spread_us"] / rec[f"{b}_graph_us"]


def summary(recs, ps):
    """yardstick (b) at one page size: each mixed shape's varlen8 / varlen16 against kvcache8 / kvcache16 of the decode-only shape"""
    dec = next(r for r in recs if r["shape"] == "decode256" and r["page_size"] == ps)
    yard = dec["kvcache8_over_kvcache16"]
    out = dict(kind="summary", page_size=ps, kvcache8_over_kvcache16=yard, yardstick_rel_spread=rel_spread(dec, "kvcache8", "kvcache16"), shapes={})
    for r in recs:
        if r["page_size"] != ps:
            continue
        margin = yard * (out["yardstick_rel_spread"] + rel_spread(r, "varlen8", "varlen16"))
        out["shapes"][r["shape"]] = dict(varlen8_over_varlen16=r["varlen8_over_varlen16"], margin=margin,
                                         met_b=r["varlen8_over_varlen16"] <= yard + margin)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "varlen_paged_fp8" / "bench.jsonl"))
    ap.add_argument("--only", choices=["uniform", "mixed"], default=None)
    ap.add_argument("--trace", default="", help="a MIXED shape name: a few eager calls of it at page 64 and nothing else")
    a = ap.parse_args()
    if a.trace:
        lq = bv.MIXED[a.trace]
        B, mx = len(lq), max(lq)
        _, _, k8, v8, bt, kd, vd, g = pools(B, 8192, 64)
        q = torch.randn(sum(lq), H, D, device="cuda", dtype=DT, generator=g)
        kn, vn = (torch.randn(sum(lq), HKV, D, device="cuda", dtype=DT, generator=g) for _ in range(2))
        sl = torch.full((B,), 8192 - mx, dtype=torch.int32, device="cuda")
        cu = torch.tensor([0] + list(torch.tensor(lq).cumsum(0)), dtype=torch.int32, device="cuda")
        for _ in range(20):  # the serving call: append, item list, attention (and the fold when the launch splits)
            um.varlen_kvcache_attention(q, k8, v8, cu, mx, sl, block_table=bt, k=kn, v=vn, causal=True, k_descale=kd, v_descale=vd)
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
        return rec

    if a.only != "mixed":
        for B, L in ((8, 8192), (32, 8192), (64, 2048), (64, 8192)):
            for ps in (16, 64):
                for Sq in (1, 4):
                    emit(uniform(B, L, ps, Sq))
    if a.only != "uniform":
        recs = [emit(mixed(name, ps)) for name in bv.MIXED for ps in (16, 64)]
        for ps in (16, 64):
            emit(summary(recs, ps))
    out.close()


if __name__ == "__main__":
    main()
