#!/usr/bin/env python3
"""Masked / sliding-window backward timing: python tools/bench_masked_backward.py [out.jsonl]

Per case, device events around warmed-up launches (median over repeats, ms per call):
  bwd_masked      umfa_attention_backward_masked_stream on the forward's mask (kernels + the tile-flag pass)
  bwd_unmasked    the unmasked backward on the same tensors (no mask at all)
  bwd_open_mask   the masked backward with an all-true bool mask of the same shape, not stripped (every tile open)
  e2e_umfa        forward + backward through umfa_torch.scaled_dot_product_attention (or sliding_window_attention) with autograd
  e2e_torch       forward + backward through torch's own SDPA with the same mask -- the route masked training took before
One JSON line per case; `faster_than_torch` compares the two end-to-end columns."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "universal-metal-flash-attention_amd")]
import torch  # noqa: E402

import umfa_torch  # noqa: E402
from umfa_torch import library  # noqa: E402


def timed(fn, warm=3, reps=7, n=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / n)
    ts.sort()
    return round(ts[len(ts) // 2], 4)


def case(name, B, H, S, D, dt, mask_fn=None, window=None, note=""):
    torch.manual_seed(0)
    q, k, v, do = (torch.randn(B, H, S, D, device="cuda", dtype=dt) for _ in range(4))
    scale = D ** -0.5
    if window is not None:
        i = torch.arange(S, device="cuda").view(-1, 1)
        j = torch.arange(S, device="cuda").view(1, -1)
        tmask = ((j >= i - window[0]) & (j <= i + window[1]))  # torch's route needs the band as a tensor
        m = None
    else:
        m = mask_fn()
        tmask = m
    open_mask = torch.ones(torch.broadcast_shapes(tuple(tmask.shape), (1, 1, S, S)), dtype=torch.bool, device="cuda")
    out, lse = umfa_torch.attention_forward(q, k, v, scale=scale, mask=m, window=window, out_dtype=dt, return_lse=True)
    out0, lse0 = umfa_torch.attention_forward(q, k, v, scale=scale, out_dtype=dt, return_lse=True)
    outo, lseo = umfa_torch.attention_forward(q, k, v, scale=scale, mask=open_mask, out_dtype=dt, return_lse=True)
    r = dict(case=name, B=B, H=H, S=S, D=D, dtype=str(dt).replace("torch.", ""), note=note)
    r["bwd_masked"] = timed(lambda: umfa_torch.attention_backward(do, q, k, v, out, lse, scale=scale, mask=m, window=window))
    r["kernel"] = umfa_torch.last_kernel()
    r["bwd_unmasked"] = timed(lambda: umfa_torch.attention_backward(do, q, k, v, out0, lse0, scale=scale))
    r["kernel_unmasked"] = umfa_torch.last_kernel()
    r["bwd_open_mask"] = timed(lambda: umfa_torch.attention_backward(do, q, k, v, outo, lseo, scale=scale, mask=open_mask))
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))

    def e2e_umfa():
        for t in (qg, kg, vg):
            t.grad = None
        if window is not None:
            o = umfa_torch.sliding_window_attention(qg, kg, vg, window=window, scale=scale)
        else:
            o = umfa_torch.scaled_dot_product_attention(qg, kg, vg, attn_mask=m, scale=scale)
        o.backward(do)

    tm = tmask.float() if tmask.dtype in (torch.float16, torch.bfloat16) else tmask  # as the routing's torch fall-back passes it

    def e2e_torch():
        for t in (qg, kg, vg):
            t.grad = None
        library.native_sdpa(qg, kg, vg, attn_mask=tm, scale=scale).backward(do)

    umfa_torch.reset_dispatch_stats()
    r["e2e_umfa"] = timed(e2e_umfa, reps=5, n=3)
    r["umfa_route_fallbacks"] = umfa_torch.get_dispatch_stats()["pytorch_fallback"]
    r["e2e_torch"] = timed(e2e_torch, reps=5, n=3)
    r["masked_over_unmasked"] = round(r["bwd_masked"] / r["bwd_unmasked"], 3)
    r["masked_over_open_mask"] = round(r["bwd_masked"] / r["bwd_open_mask"], 3)
    r["faster_than_torch"] = r["e2e_umfa"] < r["e2e_torch"]
    print(json.dumps(r), flush=True)
    del q, k, v, do, out, lse, out0, lse0, outo, lseo, qg, kg, vg, m, tmask, open_mask
    torch.cuda.empty_cache()
    return r


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "masked_bwd" / "bench.jsonl"
    out.parent.mkdir(parents=True, exist_ok=True)
    S = 4096
    bf = torch.bfloat16

    def pad(B, S_, n):
        return lambda: (torch.arange(S_, device="cuda") < S_ - n).view(1, 1, 1, S_).expand(B, 1, 1, S_)

    def docs():
        d = torch.arange(S, device="cuda") // (S // 4)
        return (d.view(-1, 1) == d.view(1, -1)).view(1, 1, S, S)

    def bias():
        i = torch.arange(S, device="cuda", dtype=torch.float32)
        h = torch.arange(24, device="cuda", dtype=torch.float32).view(-1, 1, 1) + 1
        return (-(i.view(-1, 1) - i.view(1, -1)).abs() / (64 * h)).to(bf).view(1, 24, S, S)

    rows = [
        case("a_key_padding_512", 1, 24, S, 128, bf, pad(1, S, 512), note="bool [1,1,1,S], last 512 keys masked"),
        case("b_blockdiag_4docs", 1, 24, S, 128, bf, docs, note="bool [1,1,S,S], four documents"),
        case("c_bf16_bias", 1, 24, S, 128, bf, bias, note="bf16 additive [1,24,S,S], every tile mixed"),
        case("d_window_512", 1, 24, S, 128, bf, window=(512, 512), note="sliding_window_attention (512, 512)"),
        case("e_B4H16_S1024_D64_padding", 4, 16, 1024, 64, bf, pad(4, 1024, 200), note="bool [4,1,1,S], last 200 keys masked"),
        case("f_fp16_D128_padding", 2, 16, 2048, 128, torch.float16, pad(2, 2048, 300), note="fp16 operands"),
        case("g_fp32_D64_padding_exact", 1, 8, 1024, 64, torch.float32, pad(1, 1024, 200), note="fp32 operands: fp32-exact engine"),
        case("h_bf16_D96_padding_exact", 1, 8, 1024, 96, bf, pad(1, 1024, 200), note="head_dim 96: fp32-exact engine"),
        case("i_bf16_D256_padding", 1, 8, 2048, 256, bf, pad(1, 2048, 300), note="head_dim 256"),
    ]
    with out.open("w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
