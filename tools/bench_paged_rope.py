"""Rotary KV-cache attention timings: three legs per shape,
  (a) fused   kvcache_attention / varlen_kvcache_attention with rotary_cos / rotary_sin (one pre-pass launch + the attention),
  (b) seq     the parent sequence: ops.rope_rotate(q), ops.rope_rotate(k), then the existing appending call (the per-sequence tables are
              gathered outside the timing),
  (c) plain   the existing appending call without rotary.
bf16, head_dim 128, H 32 / H_kv 8, interleaved pairs over the full head_dim, fp32 tables, causal, every sequence at the full context.
Device time per call from 20 calls captured in one CUDA graph per leg: the median of 5 replays, three repeats with the legs alternating
inside each repeat, the median of the three and their spread.  One JSON line per shape to profiles/paged_rope/bench.jsonl (or --out).
qimg_us: the cost of writing and re-reading the q image from its bytes at --copy-tbps (section 3.1i's copy rate).  --quick: one decode
shape, the fused and the plain leg eagerly (for a kernel trace)."""
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


def capture(fn, calls=20):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()  # (every scratch pool the leg needs exists before the capture)
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


def legs_timed(legs, reps=3):
    graphs = {n: capture(f) for n, f in legs.items()}
    meds = {n: [] for n in legs}
    for _ in range(reps):
        for n in legs:  # the legs alternate inside each repeat
            meds[n].append(replay_us(graphs[n]))
    return {n: (statistics.median(m), max(m) - min(m)) for n, m in meds.items()}


def tables(seqlen_ro):
    g = torch.Generator(device="cuda").manual_seed(1)
    ang = torch.rand(seqlen_ro, D // 2, device="cuda", generator=g) * 6.2831853
    return torch.cos(ang), torch.sin(ang)


def dup(t, pos):
    return t[pos].repeat_interleave(2, dim=-1).contiguous()


def record(rec, res, q_rows, copy_tbps):
    for n, (us, spread) in res.items():
        rec[f"{n}_graph_us"], rec[f"{n}_graph_spread_us"] = us, spread
    rec["fused_minus_seq_us"] = rec["fused_graph_us"] - rec["seq_graph_us"]
    rec["fused_minus_plain_us"] = rec["fused_graph_us"] - rec["plain_graph_us"]
    rec["qimg_bytes"] = 2 * q_rows * H * D * 2  # written once, read once
    rec["qimg_us"] = rec["qimg_bytes"] / copy_tbps / 1e6
    return rec


def batched(B, L, ps, S, copy_tbps):
    dt = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    mp = (L + ps - 1) // ps
    q = torch.randn(B, S, H, D, device="cuda", dtype=dt, generator=g)
    kn, vn = (torch.randn(B, S, HKV, D, device="cuda", dtype=dt, generator=g) for _ in range(2))
    kc, vc = (torch.randn(B * mp, ps, HKV, D, device="cuda", dtype=dt, generator=g) for _ in range(2))
    bt = torch.randperm(B * mp, device="cuda", generator=g).to(torch.int32).view(B, mp)
    sl = torch.full((B,), L - S, dtype=torch.int32, device="cuda")
    cos, sin = tables(L)
    pos = (sl.long()[:, None] + torch.arange(S, device="cuda")[None, :])
    cq, sq = dup(cos, pos), dup(sin, pos)  # [B, S, D]: gathered outside the timing

    def fused():
        return um.kvcache_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt, causal=True, rotary_cos=cos, rotary_sin=sin,
                                    rotary_interleaved=True)

    def seq():
        rq = um.ops.rope_rotate(q.transpose(1, 2), cq, sq).transpose(1, 2)
        rk = um.ops.rope_rotate(kn.transpose(1, 2), cq, sq).transpose(1, 2)
        return um.kvcache_attention(rq, kc, vc, rk, vn, cache_seqlens=sl, block_table=bt, causal=True)

    def plain():
        return um.kvcache_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt, causal=True)

    rec = dict(form="batched", B=B, L=L, page_size=ps, Sq=S, S_new=S, H=H, H_kv=HKV, D=D, dtype="bf16")
    res = legs_timed(dict(fused=fused, seq=seq, plain=plain))
    rec["kernel"] = um.last_kernel()
    return record(rec, res, B * S, copy_tbps), (fused, plain)


def mixed(ps, copy_tbps):
    """one prefill chunk of 2048 tokens beside 63 decode sequences, all at 8k context"""
    dt = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    lq = [2048] + [1] * 63
    B, T, L = len(lq), sum(lq), 8192
    mp = (L + ps - 1) // ps
    q = torch.randn(T, H, D, device="cuda", dtype=dt, generator=g)
    kn, vn = (torch.randn(T, HKV, D, device="cuda", dtype=dt, generator=g) for _ in range(2))
    kc, vc = (torch.randn(B * mp, ps, HKV, D, device="cuda", dtype=dt, generator=g) for _ in range(2))
    bt = torch.randperm(B * mp, device="cuda", generator=g).to(torch.int32).view(B, mp)
    lqt = torch.tensor(lq, device="cuda")
    cu = torch.cat([torch.zeros(1, device="cuda", dtype=torch.long), lqt.cumsum(0)]).to(torch.int32)
    sl = (L - lqt).to(torch.int32)
    cos, sin = tables(L)
    pos = torch.cat([sl[b].long() + torch.arange(n, device="cuda") for b, n in enumerate(lq)])
    cq, sq = dup(cos, pos)[None], dup(sin, pos)[None]  # [1, T, D]
    kw = dict(block_table=bt, causal=True)

    def fused():
        return um.varlen_kvcache_attention(q, kc, vc, cu, 2048, sl, k=kn, v=vn, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=True, **kw)

    def seq():
        rq = um.ops.rope_rotate(q[None].transpose(1, 2), cq, sq).transpose(1, 2)[0]
        rk = um.ops.rope_rotate(kn[None].transpose(1, 2), cq, sq).transpose(1, 2)[0]
        return um.varlen_kvcache_attention(rq, kc, vc, cu, 2048, sl, k=rk, v=vn, **kw)

    def plain():
        return um.varlen_kvcache_attention(q, kc, vc, cu, 2048, sl, k=kn, v=vn, **kw)

    rec = dict(form="packed", lq="1x2048+63x1", L=L, page_size=ps, T_q=T, H=H, H_kv=HKV, D=D, dtype="bf16")
    res = legs_timed(dict(fused=fused, seq=seq, plain=plain))
    rec["kernel"] = um.last_kernel()
    return record(rec, res, T, copy_tbps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "paged_rope" / "bench.jsonl"))
    ap.add_argument("--copy-tbps", type=float, default=6.29, help="the device copy rate the q image's cost is stated at (TB/s; DESIGN.md section 3.1i: 6.29)")
    ap.add_argument("--quick", action="store_true", help="one decode shape, fused and plain legs eagerly (for a kernel trace)")
    a = ap.parse_args()
    if a.quick:
        _, (fused, plain) = batched(8, 8192, 64, 1, a.copy_tbps)
        for _ in range(20):
            fused()
            plain()
        torch.cuda.synchronize()
        return
    with open(a.out, "a") as out:
        for ps in (16, 64):
            for B, L, S in ((8, 2048, 1), (8, 8192, 1), (64, 8192, 1), (8, 8192, 4)):
                rec, _ = batched(B, L, ps, S, a.copy_tbps)
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
                torch.cuda.empty_cache()
            rec = mixed(ps, a.copy_tbps)
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
