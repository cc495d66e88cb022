"""Attention dropout timings (bf16): forward and forward + backward at three shapes, three cases each --
p = 0 on today's route (umfa_torch.library.sdpa), p = 0.1 on the dropout kernels (umfa_torch.dropout_attention), torch's own SDPA at
p = 0.1.  Median of CUDA-event-timed iterations after a warm-up.  Prints one JSON line per (shape, case) and writes them to --out.

    python tools/bench_dropout.py --out profiles/dropout/bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "universal-metal-flash-attention_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import umfa_torch  # noqa: E402
from umfa_torch import library  # noqa: E402

SHAPES = [  # name, B, H, S, D, causal
    ("flux", 1, 24, 4096, 128, False),
    ("bert", 32, 12, 512, 64, False),
    ("gpt2_causal", 8, 12, 1024, 64, True),
]


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name, B, H, S, D, causal in SHAPES:
        q, k, v, do = (torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16) for _ in range(4))
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
        cases = {
            "umfa_p0": lambda x, y, z: library.sdpa(x, y, z, is_causal=causal),
            "umfa_drop_p0.1": lambda x, y, z: umfa_torch.dropout_attention(x, y, z, 0.1, causal=causal),
            "torch_p0.1": lambda x, y, z: library.native_sdpa(x, y, z, dropout_p=0.1, is_causal=causal),
        }
        for case, f in cases.items():
            with torch.no_grad():
                fwd = _time(lambda: f(q, k, v), a.warmup, a.iters)

            def step():
                o = f(qg, kg, vg)
                torch.autograd.grad(o, (qg, kg, vg), do)
            fb = _time(step, a.warmup, a.iters)
            r = {"shape": name, "B": B, "H": H, "S": S, "D": D, "causal": causal, "case": case, "fwd_us": round(fwd, 1),
                 "fwd_bwd_us": round(fb, 1)}
            if case.startswith("umfa_drop"):
                f(q, k, v)
                r["fwd_kernel"] = umfa_torch.last_kernel()
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
