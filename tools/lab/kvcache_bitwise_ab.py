#!/usr/bin/env python3
"""Two builds of the library against each other, bit for bit, over the six KV-cache forwards (dense and packed: plain, sliding window, fp8).

    python tools/lab/kvcache_bitwise_ab.py --a PARENT/libMFAFFI.so --b CHANGE/libMFAFFI.so [--record FILE]

One fresh child process per library (UMFA_LIBRARY selects it; this process never opens the GPU) runs every case on the same seeded
inputs and saves O, LSE and both caches after the append; this process then compares the two files byte for byte (the raw bytes, so
NaNs count too).  A child that fails ends the run: nothing more is started.  Exit status 0: no case differs.

Shapes: B = 2 (packed: 3 sequences), H = 8, H_kv = 2, page_size 16 with a permuted block table (static: a [B, 384, H_kv, D] cache),
cache_seqlens [300, 129] (packed: cu_seqlens_q [0, 1, 41, 44] over cache_seqlens [300, 129, 17]), the query's tokens appended by every
call.  {bf16, fp16} x D {64, 128} x Sq {1, 40} x causal x num_splits {1, 3} x output {fp32, operand type}; windows (100, 0) and (20, 5);
fp8 caches with per-(batch, head) descales; static caches; bf16 with V x 1e-9 (the range rule's second sweep)."""
import argparse
import itertools
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
H, HKV, PS, MP, CAP = 8, 2, 16, 24, 384
DENSE_LENS, PACKED_LENS, PACKED_LQ = [300, 129], [300, 129, 17], [1, 40, 3]
WINDOWS = ((100, 0), (20, 5))
ENTRIES = ("paged", "window", "fp8", "varlen", "varlen_window", "varlen_fp8")


def cases():
    """(entry, dtype, D, Sq (packed: None), causal, window, splits, fp32 out, static cache, tiny V)"""
    grid = lambda *a: itertools.product(("bf16", "fp16"), (64, 128), *a)  # noqa: E731
    for dt, D, Sq, causal, ns, f32 in grid((1, 40), (False, True), (1, 3), (True, False)):
        yield ("paged", dt, D, Sq, causal, None, ns, f32, False, False)
        yield ("fp8", dt, D, Sq, causal, None, ns, f32, False, False)
    for dt, D, Sq, win, ns, f32 in grid((1, 40), WINDOWS, (1, 3), (True, False)):
        yield ("window", dt, D, Sq, False, win, ns, f32, False, False)
    for dt, D, causal, ns, f32 in grid((False, True), (1, 3), (True, False)):
        yield ("varlen", dt, D, None, causal, None, ns, f32, False, False)
        yield ("varlen_fp8", dt, D, None, causal, None, ns, f32, False, False)
    for dt, D, win, ns, f32 in grid(WINDOWS, (1, 3), (True, False)):
        yield ("varlen_window", dt, D, None, False, win, ns, f32, False, False)
    for dt, D, Sq in grid((1, 40)):  # static caches
        yield ("paged", dt, D, Sq, True, None, 1, False, True, False)
        yield ("fp8", dt, D, Sq, True, None, 1, False, True, False)
        yield ("window", dt, D, Sq, False, WINDOWS[0], 1, False, True, False)
    for dt, D in grid():
        yield ("varlen", dt, D, None, True, None, 1, False, True, False)
        yield ("varlen_fp8", dt, D, None, True, None, 1, False, True, False)
        yield ("varlen_window", dt, D, None, False, WINDOWS[0], 1, False, True, False)
    for D, ns in itertools.product((64, 128), (1, 3)):  # bf16 V far below fp16's range: the second sweep
        for Sq in (1, 40):
            yield ("paged", "bf16", D, Sq, True, None, ns, True, False, True)
            yield ("window", "bf16", D, Sq, False, WINDOWS[1], ns, True, False, True)
        yield ("varlen", "bf16", D, None, True, None, ns, True, False, True)
        yield ("varlen_window", "bf16", D, None, False, WINDOWS[1], ns, True, False, True)


def name_of(c):
    entry, dt, D, Sq, causal, win, ns, f32, static, tiny = c
    return (f"{entry} {dt} D={D} Sq={Sq if Sq else 'packed'} causal={int(causal)} window={win} splits={ns} out={'fp32' if f32 else dt}"
            f"{' static' if static else ''}{' tinyV' if tiny else ''}")


def child(out_path):
    import torch
    sys.path.insert(0, str(ROOT / "universal-metal-flash-attention_amd"))
    from umfa_torch import ops

    res, kernels = {}, {}
    for idx, c in enumerate(cases()):
        entry, dt, D, Sq, causal, win, ns, f32, static, tiny = c
        T = torch.bfloat16 if dt == "bf16" else torch.float16
        packed, fp8 = entry.startswith("varlen"), entry.endswith("fp8")
        g = torch.Generator().manual_seed(1000 + idx)  # CPU generator: the same numbers in both processes
        rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        lens = PACKED_LENS if packed else DENSE_LENS
        B = len(lens)
        q = (rnd(sum(PACKED_LQ), H, D) if packed else rnd(B, Sq, H, D)).to(T).cuda()
        kn = (rnd(sum(PACKED_LQ), HKV, D) if packed else rnd(B, Sq, HKV, D)).to(T).cuda()
        vn = rnd(sum(PACKED_LQ), HKV, D) if packed else rnd(B, Sq, HKV, D)
        pool = (B, CAP, HKV, D) if static else (B * MP, PS, HKV, D)
        kc, vc = rnd(*pool), rnd(*pool)
        if tiny:
            vn, vc = vn * 1e-9, vc * 1e-9
        vn = vn.to(T).cuda()
        CT = torch.float8_e4m3fn if fp8 else T
        kc, vc = kc.to(CT).cuda(), vc.to(CT).cuda()
        bt = None if static else torch.randperm(B * MP, generator=g).to(torch.int32).view(B, MP).cuda()
        sl = torch.tensor(lens, dtype=torch.int32).cuda()
        kw = dict(block_table=bt, k_new=kn, v_new=vn, scale=D ** -0.5, causal=causal, num_splits=ns, out_dtype=torch.float32 if f32 else T)
        if win:
            kw["window"] = win
        pre = ()
        if packed:
            cu = torch.tensor([0] + list(itertools.accumulate(PACKED_LQ)), dtype=torch.int32).cuda()
            pre = (cu, max(PACKED_LQ))
        desc = ()
        if fp8:
            desc = ((0.5 + torch.rand(B, HKV, generator=g)).cuda(), (0.5 + torch.rand(B, HKV, generator=g)).cuda())
        fn = getattr(ops, ("varlen_" if packed else "") + "kvcache_attention_" + ("fp8_" if fp8 else "window_" if win else "") + "forward")
        o, lse = fn(q, kc, vc, *pre, sl, *desc, **kw)
        torch.cuda.synchronize()
        kernels[name_of(c)] = ops.last_kernel()
        res[name_of(c)] = [t.contiguous().view(torch.uint8).cpu() for t in (o, lse, kc, vc)]
    torch.save({"tensors": res, "kernels": kernels}, out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", help="the first library (the parent's build)")
    ap.add_argument("--b", help="the second library (the change's build)")
    ap.add_argument("--record", default="", help="write the record here too")
    ap.add_argument("--timeout", type=int, default=240, help="seconds allowed to each child")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    import torch  # (host tensors only in this process)
    with tempfile.TemporaryDirectory() as td:
        got = []
        for tag, lib in (("a", a.a), ("b", a.b)):
            path = str(Path(td) / f"{tag}.pt")
            r = subprocess.run([sys.executable, __file__, "--child", path], env={**os.environ, "UMFA_LIBRARY": str(Path(lib).resolve())},
                               timeout=a.timeout)
            if r.returncode != 0:
                print(f"the child of library {tag} ({lib}) ended with status {r.returncode}: nothing more is started")
                return 2
            got.append(torch.load(path))
    ta, tb = got[0]["tensors"], got[1]["tensors"]
    assert list(ta) == list(tb)
    lines, total, total_bad = [], 0, 0
    for entry in ENTRIES:
        names = [n for n in ta if n.split()[0] == entry]
        bad = [n for n in names if not all(torch.equal(x, y) for x, y in zip(ta[n], tb[n]))]
        ran = {got[1]["kernels"][n] for n in names}
        assert ran == {got[0]["kernels"][n] for n in names}
        lines.append(f"  {entry:14s} {len(names):3d} cases, {len(bad)} differ; {len(ran)} kernel instantiations ran")
        for n in bad:
            which = [w for w, x, y in zip(("O", "LSE", "k_cache", "v_cache"), ta[n], tb[n]) if not torch.equal(x, y)]
            lines.append(f"      differs in {', '.join(which)}: {n}")
        total += len(names)
        total_bad += len(bad)
    lines.append("")
    lines.append(f"{total} cases, {total_bad} differ" + (": every tensor bitwise equal." if not total_bad else "."))
    text = "\n".join(lines)
    print(text)
    if a.record:
        Path(a.record).parent.mkdir(parents=True, exist_ok=True)
        Path(a.record).write_text(text + "\n")
    return 1 if total_bad else 0


if __name__ == "__main__":
    sys.exit(main())
