#!/usr/bin/env python3
"""Bitwise A/B of the decode-form forward between two builds of libMFAFFI.so: does a change alter any output bit?

  python tools/lab/fwd_bitwise_ab.py <library A> <library B> [report.txt]

Each library runs in a child process of its own (UMFA_LIBRARY selects it) over the same fixed inputs -- head_dim 64 / 128, Sq 1 / 4 / 32,
with and without a forced split, bf16 with the fp16 P V product (in-kernel conversion; V far below fp16's range: the second sweep), bf16 P V,
fp16 -- and stores O, LSE and the kernel name; the parent compares them bit for bit and against fp64."""
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent

# (name, dtype, D, B, H, Sq, Skv, options, V scale)
CASES = [
    ("d128_sq1", "bf16", 128, 2, 8, 1, 4097, {}, 1.0),
    ("d128_sq1_split16", "bf16", 128, 2, 8, 1, 4097, {"force_split": 16}, 1.0),
    ("d128_sq4_split5", "bf16", 128, 5, 3, 4, 255, {"force_split": 5}, 1.0),
    ("d128_sq32", "bf16", 128, 1, 4, 32, 2048, {}, 1.0),
    ("d128_sq32_split32", "bf16", 128, 1, 4, 32, 2048, {"force_split": 32}, 1.0),
    ("d64_sq1", "bf16", 64, 1, 16, 1, 8192, {}, 1.0),
    ("d64_sq4_split2", "bf16", 64, 2, 4, 4, 129, {"force_split": 2}, 1.0),
    ("d64_sq32_split32", "bf16", 64, 2, 2, 32, 4097, {"force_split": 32}, 1.0),
    ("d128_sq4_tinyV_resweep", "bf16", 128, 2, 3, 4, 1000, {}, 1e-7),
    ("d64_sq1_bf16pv", "bf16", 64, 2, 3, 1, 1000, {"pv_fp16": 0, "force_split": 5}, 1.0),
    ("d128_sq8_fp16", "fp16", 128, 2, 3, 8, 1000, {"force_split": 2}, 1.0),
]


def child(out_path):
    sys.path[:0] = [str(ROOT), str(ROOT / "universal-metal-flash-attention_amd")]
    import torch
    import umfa_torch
    res = {}
    for idx, (name, dts, D, B, H, Sq, Skv, opts, vs) in enumerate(CASES):
        dt = torch.bfloat16 if dts == "bf16" else torch.float16
        g = torch.Generator(device="cuda").manual_seed(77 + idx)
        q = torch.randn(B, H, Sq, D, device="cuda", generator=g).to(dt)
        k = torch.randn(B, H, Skv, D, device="cuda", generator=g).to(dt)
        v = (torch.randn(B, H, Skv, D, device="cuda", generator=g) * vs).to(dt)
        with umfa_torch.options(decode_ks=1, **opts):
            o, lse = umfa_torch.attention_forward(q, k, v, out_dtype=torch.float32, return_lse=True)
            kern = umfa_torch.last_kernel()
        torch.cuda.synchronize()
        s = torch.matmul(q.double(), k.double().transpose(-1, -2)) * D ** -0.5
        ref = torch.matmul(torch.softmax(s, dim=-1), v.double())
        rel = ((o.double() - ref).abs().amax(dim=(2, 3)) / ref.abs().amax(dim=(2, 3)).clamp_min(1e-300)).max().item()
        res[name] = dict(o=o.cpu(), lse=lse.cpu(), kern=kern, rel=rel)
    torch.save(res, out_path)


def main():
    if sys.argv[1] == "--child":
        child(sys.argv[2])
        return 0
    libs = [os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])]
    report = sys.argv[3] if len(sys.argv) > 3 else None
    import torch
    got = []
    with tempfile.TemporaryDirectory() as td:
        for i, lib in enumerate(libs):
            out = os.path.join(td, f"{i}.pt")
            env = dict(os.environ, UMFA_LIBRARY=lib)
            try:
                r = subprocess.run([sys.executable, __file__, "--child", out], env=env, timeout=600)
            except subprocess.TimeoutExpired:
                print(f"child for {lib} timed out")
                return 124
            if r.returncode != 0:  # (not a difference: nothing more runs after this)
                print(f"child for {lib} exited {r.returncode}")
                return 3
            got.append(torch.load(out))
    lines = ["# decode-form forward, bitwise A/B: A = %s, B = %s" % tuple(Path(p).parent.name + "/" + Path(p).name for p in libs),
             "# case | kernel A | kernel B | O bitwise equal | LSE bitwise equal | rel vs fp64 A | rel vs fp64 B (per (b, h) slab)"]
    same = True
    for name, *_ in CASES:
        a, b = got[0][name], got[1][name]
        eo, el = torch.equal(a["o"], b["o"]), torch.equal(a["lse"], b["lse"])
        same = same and eo and el and a["kern"] == b["kern"]
        lines.append("%s | %s | %s | %s | %s | %.3e | %.3e" % (name, a["kern"], b["kern"], eo, el, a["rel"], b["rel"]))
    lines.append("all bitwise equal: %s" % same)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if report:
        Path(report).write_text(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
