"""Sliding-window packed variable-length attention against the routes a caller has without it, in one process:
  window   umfa_torch.varlen_attention(..., window_size=(left, right)) on the packed tokens
  causal   the same call without a window (causal varlen: the upper bound the window should undercut; non-causal shapes: all keys)
  perseq   the sum of one dense umfa_torch.sliding_window_attention call per sequence, K / V heads expanded (outside the timing)
Time is the median of --reps timed calls (CUDA events around each call), repeated --repeats times; TFLOP/s counts the visible work of
the window per sequence (4 D H per visible query-key pair forward, 3.5 x that forward + backward), for every route alike, so the
routes compare by time.  One JSON line per (shape, route, pass).

    python tools/bench_varlen_window.py [--reps 10] [--repeats 3] [--out profiles/varlen_window/bench.jsonl]
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
    return [
        dict(name="w1", lens=[8192] * 4, H=32, Hkv=8, D=128, dt=torch.bfloat16, causal=True, window=(4095, 0)),
        dict(name="w2", lens=[8192] * 4, H=32, Hkv=8, D=128, dt=torch.bfloat16, causal=True, window=(1023, 0)),
        dict(name="w3", lens=rng.integers(128, 2049, 64).tolist(), H=32, Hkv=8, D=64, dt=torch.float16, causal=True, window=(255, 0)),
        dict(name="w4", lens=[4096] * 8, H=16, Hkv=16, D=128, dt=torch.bfloat16, causal=False, window=(128, 128)),
    ]


def visible_pairs(lens, causal, window):
    left, right = window
    if causal:
        right = 0
    tot = 0
    for L in lens:
        i = np.arange(L)
        lo = np.maximum(0, i - left) if left >= 0 else np.zeros(L, np.int64)
        hi = np.minimum(L - 1, i + right) if right >= 0 else np.full(L, L - 1)
        tot += int(np.maximum(hi - lo + 1, 0).sum())
    return tot


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

    lines = []
    for s in shapes():
        if args.only and s["name"] not in args.only.split(","):
            continue
        lens, H, Hkv, D, dt, causal, window = s["lens"], s["H"], s["Hkv"], s["D"], s["dt"], s["causal"], s["window"]
        N, T, Lmax, G = len(lens), sum(lens), max(lens), H // Hkv
        torch.manual_seed(0)
        q = torch.randn(T, H, D, device="cuda", dtype=dt)
        k = torch.randn(T, Hkv, D, device="cuda", dtype=dt)
        v = torch.randn(T, Hkv, D, device="cuda", dtype=dt)
        cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")
        starts = np.concatenate([[0], np.cumsum(lens)])[:-1].tolist()
        ke, ve = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
        dense_win = (window[0] if window[0] >= 0 else Lmax, 0 if causal else (window[1] if window[1] >= 0 else Lmax))
        perseq = [tuple(t[s0:s0 + L].transpose(0, 1)[None].contiguous().requires_grad_(True) for t in (q, ke, ve))
                  for s0, L in zip(starts, lens)]
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
        do = torch.randn_like(q)
        dos = [do[s0:s0 + L].transpose(0, 1)[None].contiguous() for s0, L in zip(starts, lens)]

        def fwd(win):
            return lambda: um.varlen_attention(q, k, v, cu, cu, Lmax, Lmax, causal, window_size=win)

        def fb(win):
            def f():
                o = um.varlen_attention(qg, kg, vg, cu, cu, Lmax, Lmax, causal, window_size=win)
                torch.autograd.grad(o, (qg, kg, vg), do)
            return f

        def ps_fwd():
            with torch.no_grad():
                for a, b, c in perseq:
                    um.sliding_window_attention(a, b, c, dense_win, causal=causal)

        def ps_fb():
            for (a, b, c), g in zip(perseq, dos):
                o = um.sliding_window_attention(a, b, c, dense_win, causal=causal)
                torch.autograd.grad(o, (a, b, c), g)

        passes = [("fwd", {"window": fwd(window), "causal": fwd((-1, -1)), "perseq": ps_fwd}),
                  ("fwd+bwd", {"window": fb(window), "causal": fb((-1, -1)), "perseq": ps_fb})]
        flops_f = 4.0 * D * H * visible_pairs(lens, causal, window)
        for pname, rs in passes:
            fl = flops_f * (3.5 if pname == "fwd+bwd" else 1.0)
            for rname, fn in rs.items():
                rec = dict(shape=s["name"], route=rname, pass_=pname, N=N, T=T, max_len=Lmax, H=H, Hkv=Hkv, D=D, dtype=str(dt).split(".")[-1],
                           causal=causal, window=list(window),
                           band=visible_pairs(lens, causal, window) / visible_pairs(lens, causal, (-1, -1)))
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
