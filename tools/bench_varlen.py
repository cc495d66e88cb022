"""Packed variable-length attention against the routes a caller has without it, all in one process:
  varlen   umfa_torch.varlen_attention on the packed tokens
  padded   [N, H, max_len, D] with a key-padding bool mask through umfa_torch.attention_forward
  blockmask  [1, H, T, D] with a block-diagonal bool mask [T, T] through umfa_torch.attention_forward
  perseq   the sum of one dense umfa_torch.attention_forward call per sequence
  torch    torch.nn.attention.varlen.varlen_attn (when it runs on this build)
The mask routes take expanded K / V heads for GQA (the expansion is outside the timing).  Time is the median of --reps timed calls
(CUDA events around each call), repeated --repeats times; TFLOP/s counts the visible work per sequence (4 D H per visible query-key
pair forward, 2.5 x that backward).  One JSON line per (shape, route, pass).

    python tools/bench_varlen.py [--reps 10] [--repeats 3] [--out profiles/varlen/bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "universal-metal-flash-attention_amd")]


def shapes():
    rng = np.random.default_rng(0)
    out = [dict(name="a", lens=rng.integers(1024, 4609, 8).tolist(), H=24, Hkv=24, D=128, dt=torch.bfloat16, causal=False, bwd=False)]
    nd = int(rng.integers(16, 65))
    cuts = np.sort(rng.choice(np.arange(1, 16384), nd - 1, replace=False))
    lens_b = np.diff(np.concatenate([[0], cuts, [16384]])).tolist()
    out.append(dict(name="b", lens=lens_b, H=32, Hkv=8, D=128, dt=torch.bfloat16, causal=True, bwd=True))
    out.append(dict(name="c", lens=rng.integers(128, 2049, 32).tolist(), H=16, Hkv=16, D=64, dt=torch.float16, causal=True, bwd=False))
    return out


def visible_pairs(lens, causal):
    return sum(L * (L + 1) // 2 if causal else L * L for L in lens)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated shape names")
    args = ap.parse_args()
    import umfa_torch as um
    from torch.nn.attention.varlen import varlen_attn

    lines = []
    for s in shapes():
        if args.only and s["name"] not in args.only.split(","):
            continue
        lens, H, Hkv, D, dt, causal = s["lens"], s["H"], s["Hkv"], s["D"], s["dt"], s["causal"]
        N, T, Lmax, G = len(lens), sum(lens), max(lens), H // Hkv
        torch.manual_seed(0)
        q = torch.randn(T, H, D, device="cuda", dtype=dt)
        k = torch.randn(T, Hkv, D, device="cuda", dtype=dt)
        v = torch.randn(T, Hkv, D, device="cuda", dtype=dt)
        cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")
        starts = np.concatenate([[0], np.cumsum(lens)])[:-1].tolist()
        ke, ve = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
        # padded batch + key-padding mask
        qp = torch.zeros(N, H, Lmax, D, device="cuda", dtype=dt)
        kp, vp = torch.zeros_like(qp), torch.zeros_like(qp)
        for n, (s0, L) in enumerate(zip(starts, lens)):
            qp[n, :, :L] = q[s0:s0 + L].transpose(0, 1)
            kp[n, :, :L] = ke[s0:s0 + L].transpose(0, 1)
            vp[n, :, :L] = ve[s0:s0 + L].transpose(0, 1)
        kpad = (torch.arange(Lmax, device="cuda")[None, :] < torch.tensor(lens, device="cuda")[:, None])[:, None, None, :]
        # one packed sequence + block-diagonal mask
        doc = torch.repeat_interleave(torch.arange(N, device="cuda"), torch.tensor(lens, device="cuda"))
        bmask = (doc[:, None] == doc[None, :])[None, None]
        q1, k1, v1 = (t.transpose(0, 1)[None].contiguous() for t in (q, ke, ve))
        perseq = [(q[s0:s0 + L].transpose(0, 1)[None].contiguous(), ke[s0:s0 + L].transpose(0, 1)[None].contiguous(),
                   ve[s0:s0 + L].transpose(0, 1)[None].contiguous()) for s0, L in zip(starts, lens)]
        routes = {
            "varlen": lambda: um.varlen_attention(q, k, v, cu, cu, Lmax, Lmax, causal),
            "padded": lambda: um.attention_forward(qp, kp, vp, causal=causal, mask=kpad),
            "blockmask": lambda: um.attention_forward(q1, k1, v1, causal=causal, mask=bmask),
            "perseq": lambda: [um.attention_forward(a, b, c, causal=causal) for a, b, c in perseq],
            "torch": lambda: varlen_attn(q, k.repeat_interleave(G, 1) if G > 1 else k, v.repeat_interleave(G, 1) if G > 1 else v,
                                         cu, cu, Lmax, Lmax, causal),
        }
        passes = [("fwd", routes)]
        if s["bwd"]:
            qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
            do = torch.randn_like(q)
            ke_t, ve_t = kg.repeat_interleave(G, 1).detach().requires_grad_(True), vg.repeat_interleave(G, 1).detach().requires_grad_(True)

            def vl_fb():
                o = um.varlen_attention(qg, kg, vg, cu, cu, Lmax, Lmax, causal)
                torch.autograd.grad(o, (qg, kg, vg), do)

            def t_fb():
                o = varlen_attn(qg, ke_t, ve_t, cu, cu, Lmax, Lmax, causal)
                torch.autograd.grad(o, (qg, ke_t, ve_t), do)
            passes.append(("fwd+bwd", {"varlen": vl_fb, "torch": t_fb}))
        flops_f = 4.0 * D * H * visible_pairs(lens, causal)
        for pname, rs in passes:
            fl = flops_f * (3.5 if pname == "fwd+bwd" else 1.0)
            for rname, fn in rs.items():
                rec = dict(shape=s["name"], route=rname, pass_=pname, N=N, T=T, max_len=Lmax, H=H, Hkv=Hkv, D=D, dtype=str(dt).split(".")[-1],
                           causal=causal)
                try:
                    ms = [timed(fn, args.reps) for _ in range(args.repeats)]
                    rec.update(ms_median=float(np.median(ms)), ms_min=min(ms), ms_max=max(ms),
                               tflops=fl / (float(np.median(ms)) * 1e-3) / 1e12)
                except Exception as e:  # noqa: BLE001  (a route this build cannot run: recorded, not fatal)
                    rec.update(error=f"{type(e).__name__}: {str(e)[:160]}")
                    torch.cuda.synchronize()
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
