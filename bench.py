#!/usr/bin/env python3
"""bench.py -- SDPA forward throughput on MI355X (BASELINE.json metric), 1 / 2 / 4 / 8 GPUs of one node.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]

`--gpus N` with N > 1 starts N ranks ITSELF (fresh child processes, spawned before this process imports torch or
touches a GPU; RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment, RCCL through torch.distributed "nccl");
under `python -m torch.distributed.run ... bench.py --gpus N` (WORLD_SIZE already set) it runs as one rank of that job.
A child that fails makes the whole run exit non-zero.

Headline (`value`, `scaling: "strong"`): ONE FLUX-shape problem B=1 H=24 S=4096 D=128, bf16, forward, through the in-stream
C-ABI entry (umfa_attention_forward_stream -> V cast pre-pass + fa_fwd16_w64<bf16,128,pv16>: the default bf16 arithmetic, P V
product in fp16, inside the stated 1e-3), fp32 O as the C ABI writes it, inputs resident in HBM.  At N = 1 the whole
problem on the GPU; at N > 1 its 24 heads dealt over the ranks and the full O assembled on EVERY rank by RCCL all-gathers
over xGMI that run on a side stream under the next head chunk's kernel (umfa_torch.parallel.overlapped_sharded_sdpa; the
north-star's split).  Exactly K steps between barrier + synchronize brackets, max over ranks; value = the problem's FLOPs
x K / that time.  The timed region is taken in the board's SUSTAINED power state: after the W warm-up steps the same K-step
region is repeated untimed for ~0.3 s (`settle`), because a region that starts from an idle board sits inside the
firmware's power-averaging transient (tools/lab/settle_probe.py: 0.213 ms per launch right after idle, 0.176 from the
25th replay on, and a synchronize between regions does not reset it); the cold region is reported beside it
(`cold_start`).
Beside it, on every run (not inside the timed region of `value`):
  weak          (N > 1) one FLUX batch element per rank, no collective: the embarrassingly parallel (batch x head) regime
  cfg5          BASELINE config 5: B=1 H=32 S=32768 D=128 head-sharded (32 / N heads per rank), same two numbers
  roofline      dominant kernel vs the 2.5 PFLOP/s dense bf16 MFMA peak: algorithmic FLOPs per launch / mean launch
                duration from HIP events on the launch stream
and on rank 0 of a 1-GPU run:
  configs       cfg2 (B4 H16 S1024 D64 causal forward), cfg3 backward and forward + backward, cfg5's 4-head shard
  int8          runtime-quantised block-wise forward vs the bf16 forward, FLUX and cfg4, both sides timed by the same
                events on the same stream, quantiser included
  parity        measured rel-err of every config at full size against the CPU oracle (row subset, all keys)
  cpu_baseline  PyTorch CPU SDPA (the reference's config-1 path, its declared ground truth) on the same FLUX shape on
                this box's host cores; the fp64 oracle port nested under it
"""
from __future__ import annotations

import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
for p in (str(ROOT), str(ROOT / "universal-metal-flash-attention_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_BF16_TFLOPS = 2500.0  # dense, MI355X_MICROARCH.md "Peak BF16/FP16 MFMA"
B, H, S, D = 1, 24, 4096, 128
FLOPS_PER_STEP = 4.0 * B * H * S * S * D  # 206.16 GFLOP
METRIC = "SDPA fwd TFLOPS (bf16) + int8 speedup, B=1 H=24 S=4096 D=128, 1/2/4/8 GPU"


# ------------------------------------------------------------------------------------------------------------------
# launcher: N fresh rank processes.  Nothing here imports torch or touches a GPU.
def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n: int, argv: list[str], timeout_s: float = 1500.0) -> int:
    env0 = dict(os.environ)
    env0.setdefault("MASTER_ADDR", "127.0.0.1")
    env0.setdefault("MASTER_PORT", str(free_port()))
    env0.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this driver (RCCL needs it)
    procs = []
    for r in range(n):
        env = dict(env0, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n))
        procs.append(subprocess.Popen([sys.executable, str(Path(__file__).resolve())] + argv, env=env))
    deadline = time.time() + timeout_s
    rc = 0
    pending = set(range(n))
    while pending:
        for r in sorted(pending):
            code = procs[r].poll()
            if code is not None:
                pending.discard(r)
                if code != 0 and rc == 0:
                    rc = code if code > 0 else 1
                    print(f"bench.py: rank {r} exited with {code}; stopping the other ranks", file=sys.stderr)
        if rc != 0 or time.time() > deadline:
            if time.time() > deadline and rc == 0:
                rc = 124
                print("bench.py: ranks did not finish in time", file=sys.stderr)
            for r in pending:  # exactly the processes started above
                procs[r].terminate()
            for r in pending:
                try:
                    procs[r].wait(timeout=10)
                except subprocess.TimeoutExpired:
                    procs[r].kill()
            break
        time.sleep(0.05)
    return rc


def launcher_selftest() -> None:
    """`--launcher-selftest`: the ranks rendezvous over gloo on the CPU and rank 0 prints what it saw -- the launcher and
    the env contract are testable without a GPU (tests/test_bench_launcher.py)."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    t = torch.tensor([float(rank + 1)])
    if world > 1:
        dist.all_reduce(t)
    from umfa_torch import parallel
    a, b = parallel.shard_range(H, world, rank)
    heads = torch.tensor([float(b - a)])
    if world > 1:
        dist.all_reduce(heads)
    if rank == 0:
        print(json.dumps({"selftest": "launcher", "n_gpus": world, "sum_of_rank_ids_plus_one": t.item(),
                          "heads_covered": int(heads.item()), "local_rank_env": os.environ.get("LOCAL_RANK")}), flush=True)
    if world > 1:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------------------
def torch_cpu_sdpa():
    """torch.nn.functional.scaled_dot_product_attention on the host cores, full FLUX shape, fp32 and bf16 (best of <= 3
    runs each, at most ~20 s in all)."""
    import torch
    import torch.nn.functional as F
    out = {"cores": torch.get_num_threads()}
    budget = time.perf_counter() + 20.0
    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        g = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(B, H, S, D, generator=g).to(dt) for _ in range(3))
        best = None
        for _ in range(3):
            if time.perf_counter() > budget and best is not None:
                break
            t0 = time.perf_counter()
            F.scaled_dot_product_attention(q, k, v)
            el = time.perf_counter() - t0
            best = el if best is None else min(best, el)
            if time.perf_counter() > budget:
                break
        out[name] = round(FLOPS_PER_STEP / best / 1e12, 4)
    return out


def oracle_port(cores: int):
    """The fp64 oracle (oracle/sdpa_ref.c, OpenMP) on a bounded sample of the workload."""
    import numpy as np

    from oracle import oracle
    os.environ.setdefault("OMP_NUM_THREADS", str(cores))
    heads, s_len = max(1, cores), 2048  # ~10-20 s of CPU work
    rng = np.random.default_rng(0)
    mk = lambda: oracle.f32_to_bf16_bits(rng.standard_normal((1, heads, s_len, D)).astype(np.float32))  # noqa: E731
    q, k, v = mk(), mk(), mk()
    oracle.lib()
    t0 = time.perf_counter()
    oracle.sdpa_forward(q, k, v)
    dt = time.perf_counter() - t0
    return {"value": round(4.0 * heads * s_len * s_len * D / dt / 1e12, 5), "unit": "TFLOP/s", "cores": cores, "kind": "port",
            "sample": f"B=1 H={heads} S={s_len} D={D} bf16 forward, oracle/sdpa_ref.c (fp64 accumulate, OpenMP), {dt:.1f} s"}


def cpu_baseline(cores: int):
    try:
        t = torch_cpu_sdpa()
        res = {"value": t["bf16"], "unit": "TFLOP/s", "cores": t["cores"], "kind": "reference",
               "sample": f"torch.nn.functional.scaled_dot_product_attention on CPU tensors, the FULL workload B={B} H={H} S={S} "
                         f"D={D} bf16, best of <= 3 runs (the reference's own CPU path, BASELINE configs[0], and its "
                         "declared ground truth: tests/conftest.py:165-182)",
               "fp32_value": t["fp32"]}
    except Exception as exc:  # noqa: BLE001
        res = {"value": None, "unit": "TFLOP/s", "cores": cores, "kind": "reference", "error": repr(exc)}
    try:
        res["oracle_port"] = oracle_port(cores)
    except Exception as exc:  # noqa: BLE001
        res["oracle_port"] = {"error": repr(exc)}
    return res


# ------------------------------------------------------------------------------------------------------------------
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, tensors: dict) -> None:
    """`--dump-outputs DIR`: each tensor as DIR/<name>.npy in float32 (the inputs are seeded, so two builds can be compared
    output for output).  A tensor that would take the files past 64 MB in all is replaced by a fixed, seeded sample of its
    elements (flat indices from numpy's default_rng(0), sorted) and written as <name>_sample.npy beside <name>_sample_index.npy."""
    import numpy as np

    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    budget = DUMP_LIMIT_BYTES
    for name, t in tensors.items():
        a = t.detach().float().cpu().numpy()
        if a.nbytes <= budget:
            np.save(d / f"{name}.npy", a)
            budget -= a.nbytes
            continue
        n = max(1, min(a.size, budget // 12))  # float32 value + int64 index per sampled element
        idx = np.sort(np.random.default_rng(0).choice(a.size, size=n, replace=False))
        np.save(d / f"{name}_sample.npy", a.reshape(-1)[idx])
        np.save(d / f"{name}_sample_index.npy", idx.astype(np.int64))
        budget -= n * 12


def run_rank(args) -> None:
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    # UMFA_BENCH_ONE_DEVICE=1 (code-path rehearsal on a 1-GPU box, never a measurement): every rank uses cuda:0 and the
    # process group is gloo (RCCL refuses two ranks on one device); the JSON line is marked `rehearsal`
    rehearsal = os.environ.get("UMFA_BENCH_ONE_DEVICE") == "1"
    if rehearsal:
        local_rank = 0
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} wants GPU {local_rank} but only {torch.cuda.device_count()} are visible")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    import umfa_torch
    from umfa_torch import parallel

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x: float) -> float:
        if world == 1:
            return x
        t = torch.tensor([x], device="cpu" if rehearsal else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def timed(fn, steps, warmup, graph=True, settle_s=0.3):
        """max-over-ranks wall seconds of exactly `steps` calls of fn between barrier + synchronize brackets, taken in the
        board's sustained power state.  Returns (seconds, {cold region, settle launches})."""
        g = None
        if graph:
            # warm-up AND capture on the same side stream: scratch pools are per (device, stream) and never grow while
            # a stream is capturing (runtime_internal.h), so the capture stream must have seen the shape first
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):
                    fn()
                side.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    for _ in range(steps):
                        fn()
            torch.cuda.current_stream(dev).wait_stream(side)
            g.replay()  # untimed: the first replay pays the graph upload
        else:
            for _ in range(warmup):
                fn()

        def region():
            barrier()
            t0 = time.perf_counter()
            if g is not None:
                g.replay()
            else:
                for _ in range(steps):
                    fn()
            barrier()
            return max_over_ranks(time.perf_counter() - t0)

        cold = region()  # what a K-step region sees right after the W warm-up steps (the board just left idle)
        n_settle = int(min(400, max(3, math.ceil(settle_s / max(cold, 1e-4)))))
        for _ in range(n_settle):  # untimed: the firmware's power limiter reaches its sustained state (~25 FLUX-size regions)
            if g is not None:
                g.replay()
            else:
                for _ in range(steps):
                    fn()
        dt = region()
        return dt, {"cold_start_ms_per_step": round(cold / steps * 1e3, 4), "settle_untimed_steps": n_settle * steps,
                    "untimed_steps_before_the_timed_region": max(1, warmup) + (steps if graph else 0) + steps + n_settle * steps,
                    "why": "a region started from an idle board sits in the firmware's power-averaging transient (tools/lab/settle_probe.py, "
                           "profiles/r3/lab_notes.md); `value` is the sustained state, the cold region is reported here"}

    def event_ms(fn, n, warmup=3):
        """per-launch milliseconds from HIP events on the launch stream (torch's current stream): sorted list"""
        for _ in range(warmup):
            fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in evs:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return sorted(a.elapsed_time(b) for a, b in evs)

    def graph_ms(fn, n, warmup=3, reps=3):
        """steady-state milliseconds per call: n calls captured in one hipGraph (warm-up and capture on one side stream, as
        in timed()), replayed once untimed, then timed with HIP events around `reps` more replays -- the same launch regime
        as the headline; per-launch eager events (event_ms) also contain the launch gaps between a call's kernels"""
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                fn()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(n):
                    fn()
            g.replay()
            side.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):  # back to back: one replay's launch latency (tens of us) is 10 % of twenty 0.1-ms calls, and not steady state
                g.replay()
            b.record()
            b.synchronize()
        torch.cuda.current_stream(dev).wait_stream(side)
        return a.elapsed_time(b) / (n * reps)

    # ---- headline: ONE FLUX problem (strong scaling).  N = 1: the whole problem on this GPU; N > 1: its heads dealt over the
    # ranks, the full O on every rank through all-gathers overlapped with the next head chunk
    torch.manual_seed(1234)  # the same full problem on every rank
    q, k, v = (torch.randn(B, H, S, D, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(3))
    # O in fp32: the C ABI's contract (mfa_attention_encode_mtl writes fp32 O, MFABridge.swift:1089) and the output the stated
    # tolerance is checked on (`parity.cfg3_flux_fp32O`); the fused bf16 cast-back epilogue is timed beside it (`configs`)
    out = torch.empty(B, H, S, D, device=dev, dtype=torch.float32)
    flops = FLOPS_PER_STEP * (0.5 if args.causal else 1.0)
    strong_ok = world > 1 and H % world == 0

    def attn(qc, kc, vc, out=None):
        return umfa_torch.attention_forward(qc, kc, vc, causal=args.causal, out=out)

    comm = torch.cuda.Stream(device=dev) if strong_ok else None

    def step():
        if strong_ok:
            parallel.overlapped_sharded_sdpa(q, k, v, out, attention_fn=attn, comm_stream=comm)
        else:
            umfa_torch.attention_forward(q, k, v, causal=args.causal, out=out)

    if world > 1 and not strong_ok:
        raise SystemExit(f"bench.py: {H} heads do not divide over {world} ranks")
    # RCCL collectives are launched eagerly (not captured): the N > 1 headline is an eager region
    dt, settle = timed(step, args.steps, args.warmup, graph=(world == 1 and not args.no_graph))
    kernel_name = umfa_torch.last_kernel()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"o": out})  # O of the last timed step: what a caller of the in-stream entry receives
    gathered_ok = None
    if strong_ok and rank == 0:
        # the assembled tensor is the full O: rank 0 recomputes its own first chunk and the first chunk of the LAST rank with
        # launches of the same shape (same work decomposition => the kernels are bitwise repeatable) and compares bit for bit
        gathered_ok = True
        for r_ in (0, world - 1):
            a_, b_, _, _ = parallel.owned_heads(H, world, r_)[0]
            chk = umfa_torch.attention_forward(q[:, a_:b_], k[:, a_:b_], v[:, a_:b_], causal=args.causal, out_dtype=out.dtype)
            torch.cuda.synchronize()
            gathered_ok = gathered_ok and bool(torch.equal(out[:, a_:b_], chk))

    # dominant kernel: this rank's launch(es) of one step, HIP events on the launch stream
    if strong_ok:
        spans = parallel.owned_heads(H, world, rank)
        local_flops = flops * (H // world) / H

        def local_step():
            for a_, b_, _, _ in spans:
                umfa_torch.attention_forward(q[:, a_:b_], k[:, a_:b_], v[:, a_:b_], causal=args.causal, out=out[:, a_:b_])
    else:
        local_flops, local_step = flops, step
    durs = event_ms(local_step, args.steps)
    mean_ms = sum(durs) / len(durs)
    achieved = local_flops / (mean_ms * 1e-3) / 1e12

    # ---- weak scaling (N > 1): one FLUX batch element per rank, no data-path collective
    def sharded_leg(Bx, Hx, Sx, steps):
        torch.manual_seed(1234)  # the same full problem on every rank; each computes the views of its heads
        fq, fk, fv = (torch.randn(Bx, Hx, Sx, D, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(3))
        mode, ql, kl, vl = parallel.local_slices(fq, fk, fv, world, rank)
        o_local = torch.empty(ql.shape, device=dev, dtype=torch.bfloat16)
        fl = 4.0 * Bx * Hx * Sx * Sx * D

        def compute():
            umfa_torch.attention_forward(ql, kl, vl, out=o_local)

        def compute_gather():
            umfa_torch.attention_forward(ql, kl, vl, out=o_local)
            parallel.all_gather_output(o_local, mode, (Bx, Hx, Sx, D))  # one all_gather_into_tensor; B = 1 head shards: a view of it IS O

        t_c, _ = timed(compute, steps, 3, graph=not args.no_graph, settle_s=0.1)
        res = {"workload": f"B={Bx} H={Hx} S={Sx} D={D} bf16 forward, ONE problem, {mode} sharded: {ql.shape[1]} heads on rank 0",
               "kernel": umfa_torch.last_kernel(), "ms_per_step": round(t_c / steps * 1e3, 4),
               "value": round(fl * steps / t_c / 1e12, 2), "unit": "TFLOP/s", "scaling": "strong"}
        if world > 1:
            t_g, _ = timed(compute_gather, steps, 3, graph=False, settle_s=0.1)  # RCCL collectives are launched eagerly
            res["with_allgather"] = {"ms_per_step": round(t_g / steps * 1e3, 4), "value": round(fl * steps / t_g / 1e12, 2),
                                     "bytes_per_rank": o_local.numel() * 2, "collective": "all_gather_into_tensor (RCCL), not overlapped"}
        del fq, fk, fv
        return res

    weak = None
    if world > 1 and not args.headline_only:
        torch.manual_seed(rank)
        wq, wk, wv = (torch.randn(B, H, S, D, device=dev, dtype=torch.float32).to(torch.bfloat16) for _ in range(3))
        wo = torch.empty_like(wq)
        t_w, _ = timed(lambda: umfa_torch.attention_forward(wq, wk, wv, causal=args.causal, out=wo), args.steps, args.warmup,
                       graph=not args.no_graph, settle_s=0.1)
        weak = {"workload": "one FLUX batch element per rank, no data-path collective", "scaling": "weak",
                "ms_per_step": round(t_w / args.steps * 1e3, 4), "value": round(flops * world * args.steps / t_w / 1e12, 2), "unit": "TFLOP/s"}
        del wq, wk, wv, wo
    cfg5 = None if args.headline_only else sharded_leg(1, 32, 32768, max(2, min(args.steps, 10 if world > 1 else 4)))

    extra = {}
    if world == 1 and rank == 0 and not args.headline_only:
        # ---- other BASELINE configs on one GPU (kernel time from HIP events, median)
        def med(ts):
            return ts[len(ts) // 2]

        configs = {}
        torch.manual_seed(0)
        c2 = [torch.randn(4, 16, 1024, 64, device=dev, dtype=torch.bfloat16) for _ in range(3)]
        o2 = torch.empty_like(c2[0])
        GT = "ms: one hipGraph of n calls, HIP events around its second replay (the headline's launch regime); ms_eager: median of per-call HIP events on eager launches"
        t_e = med(event_ms(lambda: umfa_torch.attention_forward(*c2, causal=True, out=o2), 30))
        t = graph_ms(lambda: umfa_torch.attention_forward(*c2, causal=True, out=o2), 100)
        f2 = 2.0 * 4 * 16 * 1024 * 1024 * 64  # causal convention: half of 4 B H S^2 D
        # this launch is HBM-bound, not MFMA-bound: 8.59 GFLOP over Q + K + V + O (bf16) = 33.5 MB is 256 FLOP / B, below the ridge (2500 / 8 = 312):
        # its floor is bytes / the measured device-to-device copy rate (6.29 TB/s), `frac_hbm` is that floor over the time
        b2 = 4.0 * (4 * 16 * 1024 * 64) * 2
        configs["cfg2_B4_H16_S1024_D64_bf16_causal_fwd"] = {"ms": round(t, 5), "ms_eager": round(t_e, 5), "tflops": round(f2 / t / 1e9, 1), "frac": round(f2 / t / 1e9 / PEAK_BF16_TFLOPS, 4),
                                                             "bound": "hbm", "bytes": b2, "hbm_floor_ms": round(b2 / 6.29e12 * 1e3, 5), "gbps": round(b2 / t / 1e6, 1),
                                                             "frac_hbm": round(b2 / 6.29e12 * 1e3 / t, 4),
                                                             "kernel": umfa_torch.last_kernel(), "flops": f2, "timer": GT}
        # short causal launches, round 6: the 128-row kernel's balanced causal pairs (option cbal; DESIGN.md section 3.1 "CBAL") against the unpaired
        # schedule, same process, same timer.  Config 2 itself is NOT routed there (forced here to show why: level / slower -- at head_dim 64 two
        # co-resident workgroups do not overlap, profiles/r6/cbal_stamps_config2.txt)
        try:
            cp = {}
            for (nm, B_, H_, S_, D_) in (("B1_H8_S4096_D128", 1, 8, 4096, 128), ("B2_H8_S2048_D128", 2, 8, 2048, 128), ("B4_H8_S1024_D128", 4, 8, 1024, 128),
                                          ("B1_H8_S4096_D64", 1, 8, 4096, 64), ("cfg2_B4_H16_S1024_D64", 4, 16, 1024, 64)):
                cq = [torch.randn(B_, H_, S_, D_, device=dev, dtype=torch.bfloat16) for _ in range(3)]
                co = torch.empty_like(cq[0])
                ent = {}
                for tag, opts in (("default", {}), ("paired", {"cbal": 1}), ("unpaired", {"cbal": 2})):
                    with umfa_torch.options(no_w64=1, **opts):
                        ent[tag + "_ms"] = round(graph_ms(lambda: umfa_torch.attention_forward(*cq, causal=True, out=co), 50), 5)
                ent["kernel"] = umfa_torch.last_kernel()
                ent["tflops_default"] = round(2.0 * B_ * H_ * S_ * S_ * D_ / ent["default_ms"] / 1e9, 1)
                cp[nm] = ent
            cp["note"] = "causal bf16 forward on the 128-row kernel (no_w64 = 1 for all three columns); default = what the plan picks (fwd_16_split_plan)"
            configs["causal_pairs_128row"] = cp
        except Exception as exc:  # noqa: BLE001
            configs["causal_pairs_128row"] = {"error": repr(exc)}
        # the headline shape in the two regimes that meet / sit on the stated tolerance, beside the headline's (lazy reference):
        # exact running max (bf16 at its operand-format floor) and fp16 (inside 1e-3)
        from oracle import parity as _par

        def _flux_regime(name, dt_, **opts):
            fq, fk, fv = (t.to(dt_) for t in (q, k, v))
            fo = torch.empty_like(fq)
            with umfa_torch.options(**opts):
                tg = graph_ms(lambda: umfa_torch.attention_forward(fq, fk, fv, out=fo), 40)
                kn = umfa_torch.last_kernel()
                o32 = umfa_torch.attention_forward(fq, fk, fv, out_dtype=torch.float32)
                torch.cuda.synchronize()
            pr = _par.forward_rel_err(fq, fk, fv, o32, floor_kind="fp16" if (dt_ == torch.float16 or ",pv16" in kn) else "bf16")
            configs[name] = {"ms": round(tg, 5), "tflops": round(FLOPS_PER_STEP / tg / 1e9, 1), "frac": round(FLOPS_PER_STEP / tg / 1e9 / PEAK_BF16_TFLOPS, 4),
                             "kernel": kn, "rel": pr["rel"], "rms": pr["rms"], "format_floor_rel": pr.get("format_floor"),
                             "format_floor_rms": pr.get("format_floor_rms"), "fp32_out_for_rel": True, "options": {k_: str(v_) for k_, v_ in opts.items()}}

        # the default (bf16 operands, P V product in fp16: inside 1e-3) with the bf16 cast-back epilogue -- `value` times fp32 O --,
        # then the bf16 P V kernels (pv_fp16 = 0: round 3's default and today's fall-back) in their three softmax-reference
        # regimes, then fp16 operands
        _flux_regime("cfg3_flux_bf16_default_bf16O", torch.bfloat16)
        _flux_regime("cfg3_flux_bf16_pvbf16_lazy", torch.bfloat16, pv_fp16=0)
        _flux_regime("cfg3_flux_bf16_pvbf16_exact", torch.bfloat16, pv_fp16=0, softmax_reference="exact")
        _flux_regime("cfg3_flux_fp16", torch.float16)
        # mask tensors at the FLUX shape (the north-star's "arbitrary-mask tile early-exit"): key padding [1,1,1,S] and a
        # block-diagonal mask [1,1,S,S] (four documents of 1024 tokens) -- the 128-row kernel with the tile-flag pre-pass (fully
        # masked tiles skipped, fully open ones without mask reads); rel on fp32 O against the oracle WITH the mask, row subset
        import numpy as _np
        from oracle import oracle as _orc
        _i = torch.arange(S, device=dev)
        _masks = {"cfg3_flux_bf16_mask_padding": ((_i < 3000)[None, None, None, :]).contiguous(),
                  "cfg3_flux_bf16_mask_blockdiag": ((_i[:, None] // 1024) == (_i[None, :] // 1024))[None, None].contiguous(),
                  # ADDITIVE masks (round 6: the one-wave-per-SIMD bias kernels, the mask tile by LDS-DMA straight from the caller's tensor): an fp16
                  # relative-position bias shared by the heads [1,1,S,S], every tile mixed; and a per-head one [1,H,S,S] (ALiBi-like slopes: 805 MB, read once)
                  "cfg3_flux_bf16_mask_additive_bias": (-(_i[:, None] - _i[None, :]).abs().to(torch.float16) / 256.0)[None, None].contiguous(),
                  "cfg3_flux_bf16_mask_additive_bias_per_head": (-(_i[:, None] - _i[None, :]).abs().float()[None] /
                                                                 (64.0 * (1 + torch.arange(H, device=dev)[:, None, None]))).to(torch.float16)[None].contiguous()}
        # fp32 ADDITIVE masks (end of round 6; what the reference's callers build: metal_sdpa_backend.cpp:3210-3231).  The classification pass writes an fp16 copy and
        # decides on the device whether it is exact; the bias kernel (on the copy) and the 128-row kernel (on the fp32 tensor) are both enqueued, guarded by that verdict.
        # "_fp32": the fp16 bias above widened (exact: the bias kernel runs); "_fp32_inexact": the same bias computed in fp32 (|i - j| / 256 above 2048 does not fit fp16:
        # the 128-row kernel runs, the pass and one empty launch are the cost); "_blockdiag_fp32": a bool mask as the reference's torch path converts it (0 / -inf)
        _masks["cfg3_flux_bf16_mask_additive_bias_fp32"] = _masks["cfg3_flux_bf16_mask_additive_bias"].float()
        _masks["cfg3_flux_bf16_mask_additive_bias_fp32_inexact"] = (-(_i[:, None] - _i[None, :]).abs().float() / 256.0)[None, None].contiguous()
        _masks["cfg3_flux_bf16_mask_blockdiag_fp32"] = torch.where(_masks["cfg3_flux_bf16_mask_blockdiag"], 0.0, float("-inf")).contiguous()
        for _name, _m in _masks.items():
            fo = torch.empty(B, H, S, D, device=dev, dtype=torch.float32)
            tg = graph_ms(lambda: umfa_torch.attention_forward(q, k, v, mask=_m, out=fo), 20)
            kn = umfa_torch.last_kernel()
            umfa_torch.attention_forward(q, k, v, mask=_m, out=fo)
            torch.cuda.synchronize()
            rows = _par.sample_rows(S)
            _add = _m.dtype != torch.bool
            _ridx = torch.as_tensor(rows if _m.shape[2] > 1 else [0] * len(rows), device=dev)
            if _m.shape[1] > 1:  # a mask with a head dimension of its own: [1, H, rows, S]
                mrows = _np.ascontiguousarray(_m[:, :, _ridx].float().cpu().numpy())
            else:
                mrows = _np.ascontiguousarray(_np.broadcast_to((_m[0, 0].float() if _add else _m[0, 0])[_ridx].cpu().numpy(), (len(rows), S)))
            ref = _orc.sdpa_forward(_np.ascontiguousarray(_par.bits(q)[:, :, rows]), _par.bits(k), _par.bits(v), mask=mrows,
                                    mask_type=_orc.MASK_ADDITIVE if _add else _orc.MASK_BOOL).astype(_np.float64)
            dd = fo[:, :, rows].cpu().numpy().astype(_np.float64) - ref
            vis = 1.0 if _add else float(_m.float().mean().item())  # fraction of (row, key) pairs that attend: the work a skipping kernel has to do
            if _add and bool(torch.isinf(_m).any().item()):
                vis = float((~torch.isinf(_m)).float().mean().item())
            configs[_name] = {"ms": round(tg, 5), "kernel": kn, "visible_fraction": round(vis, 4),
                              "tflops_of_visible_work": round(FLOPS_PER_STEP * vis / tg / 1e9, 1),
                              "frac_of_visible_work": round(FLOPS_PER_STEP * vis / tg / 1e9 / PEAK_BF16_TFLOPS, 4),
                              "rel": float(_np.abs(dd).max() / _np.abs(ref).max()), "fp32_out": True,
                              "mask": {"cfg3_flux_bf16_mask_padding": "bool [1,1,1,S], keys < 3000 attend", "cfg3_flux_bf16_mask_blockdiag": "bool [1,1,S,S], four blocks of 1024",
                                       "cfg3_flux_bf16_mask_additive_bias": "fp16 additive [1,1,S,S], -|i - j| / 256: every tile mixed",
                                       "cfg3_flux_bf16_mask_additive_bias_per_head": "fp16 additive [1,H,S,S], -|i - j| / (64 (h + 1)): 805 MB, every tile mixed, not classified",
                                       "cfg3_flux_bf16_mask_additive_bias_fp32": "fp32 additive [1,1,S,S]: the fp16 bias widened -- fp16 holds every value: the bias kernel of the guarded pair runs",
                                       "cfg3_flux_bf16_mask_additive_bias_fp32_inexact": "fp32 additive [1,1,S,S], -|i - j| / 256 in fp32 -- fp16 does not hold it: the 128-row kernel of the guarded pair runs",
                                       "cfg3_flux_bf16_mask_blockdiag_fp32": "fp32 additive [1,1,S,S], 0 / -inf, four blocks of 1024 (a bool mask as the reference's torch path converts it)"}[_name]}
            if _m.dtype == torch.float32:  # ... and the 128-row kernel alone (the route before this build)
                with umfa_torch.options(no_w64_f32_mask=1):
                    configs[_name]["ms_128row_alone"] = round(graph_ms(lambda: umfa_torch.attention_forward(q, k, v, mask=_m, out=fo), 20), 5)
                    configs[_name]["kernel_128row_alone"] = umfa_torch.last_kernel()
            del fo
        # sliding window WITHOUT a mask tensor (the in-stream entry's UMFA_MASK_TYPE_WINDOW; the north-star's "sliding-window tile early-exit"):
        # +-512 keys around the row -- the same band as the window TENSORS of the mask tests, with no S x S mask anywhere
        try:
            fo = torch.empty(B, H, S, D, device=dev, dtype=torch.float32)
            tg = graph_ms(lambda: umfa_torch.attention_forward(q, k, v, window=(512, 512), out=fo), 20)
            kn = umfa_torch.last_kernel()
            umfa_torch.attention_forward(q, k, v, window=(512, 512), out=fo)
            torch.cuda.synchronize()
            rows = _par.sample_rows(S)
            band = (_np.abs(_np.arange(S)[None, :] - _np.asarray(rows)[:, None]) <= 512)
            ref = _orc.sdpa_forward(_np.ascontiguousarray(_par.bits(q)[:, :, rows]), _par.bits(k), _par.bits(v), mask=_np.ascontiguousarray(band),
                                    mask_type=_orc.MASK_BOOL).astype(_np.float64)
            dd = fo[:, :, rows].cpu().numpy().astype(_np.float64) - ref
            _r = _np.arange(S)
            vis = float((_np.minimum(_r + 512, S - 1) - _np.maximum(_r - 512, 0) + 1).sum() / (S * S))
            configs["cfg3_flux_bf16_window512"] = {"ms": round(tg, 5), "kernel": kn, "visible_fraction": round(vis, 4),
                                                   "tflops_of_visible_work": round(FLOPS_PER_STEP * vis / tg / 1e9, 1),
                                                   "frac_of_visible_work": round(FLOPS_PER_STEP * vis / tg / 1e9 / PEAK_BF16_TFLOPS, 4),
                                                   "rel": float(_np.abs(dd).max() / _np.abs(ref).max()), "fp32_out": True,
                                                   "mask": "none: window = (512, 512) through UMFA_MASK_TYPE_WINDOW"}
            del fo
        except Exception as exc:  # noqa: BLE001
            configs["cfg3_flux_bf16_window512"] = {"error": repr(exc)}
        o3, lse3 = umfa_torch.attention_forward(q, k, v, return_lse=True)
        do3 = torch.randn_like(q)
        tb_e = med(event_ms(lambda: umfa_torch.attention_backward(do3, q, k, v, o3, lse3, scale=D ** -0.5), 20))
        tb = graph_ms(lambda: umfa_torch.attention_backward(do3, q, k, v, o3, lse3, scale=D ** -0.5), 40)
        configs["cfg3_flux_bf16_bwd"] = {"ms": round(tb, 5), "ms_eager": round(tb_e, 5), "tflops": round(2.5 * FLOPS_PER_STEP / tb / 1e9, 1),
                                         "frac": round(2.5 * FLOPS_PER_STEP / tb / 1e9 / PEAK_BF16_TFLOPS, 4), "kernel": umfa_torch.last_kernel(),
                                         "flops": 2.5 * FLOPS_PER_STEP, "note": "algorithmic 2.5 x forward FLOPs (SURVEY.md §8d); bf16 gradients, in-stream entry"}

        def fwd_bwd():
            oo, ll = umfa_torch.attention_forward(q, k, v, return_lse=True)
            umfa_torch.attention_backward(do3, q, k, v, oo, ll, scale=D ** -0.5)

        tfb_e = med(event_ms(fwd_bwd, 20))
        tfb = graph_ms(fwd_bwd, 40)
        configs["cfg3_flux_bf16_fwd_bwd"] = {"ms": round(tfb, 5), "ms_eager": round(tfb_e, 5), "tflops": round(3.5 * FLOPS_PER_STEP / tfb / 1e9, 1),
                                             "frac": round(3.5 * FLOPS_PER_STEP / tfb / 1e9 / PEAK_BF16_TFLOPS, 4), "flops": 3.5 * FLOPS_PER_STEP}
        del o3, lse3, do3
        c5 = [torch.randn(1, 4, 32768, 128, device=dev, dtype=torch.bfloat16) for _ in range(3)]
        o5 = torch.empty_like(c5[0])
        t5 = med(event_ms(lambda: umfa_torch.attention_forward(*c5, out=o5), 6, warmup=2))
        f5 = 4.0 * 4 * 32768 * 32768 * 128
        configs["cfg5_shard_B1_H4_S32768_D128_bf16_fwd"] = {"ms": round(t5, 4), "tflops": round(f5 / t5 / 1e9, 1), "frac": round(f5 / t5 / 1e9 / PEAK_BF16_TFLOPS, 4),
                                                             "kernel": umfa_torch.last_kernel(), "flops": f5}
        del c5, o5
        # config 4's quantised backward: quantiser + cast + the two 16-bit MFMA backward kernels on fp16 de-quantised operands
        try:
            q4, k4, v4, do4 = (torch.randn(1, 16, 8192, D, device=dev, dtype=torch.bfloat16) for _ in range(4))
            o4, l4 = umfa_torch.quantized_attention_forward_stream(q4, k4, v4, return_lse=True)
            tq = graph_ms(lambda: umfa_torch.quantized_attention_backward_stream(do4, q4, k4, v4, o4, l4), 10, warmup=2)
            f4 = 2.5 * 4.0 * 16 * 8192 * 8192 * D
            configs["cfg4_int8_bwd"] = {"ms": round(tq, 4), "tflops": round(f4 / tq / 1e9, 1), "frac": round(f4 / tq / 1e9 / PEAK_BF16_TFLOPS, 4),
                                        "kernel": umfa_torch.last_kernel(), "flops": f4,
                                        "note": "umfa_quantized_backward_stream, quantiser and dO cast inside; algorithmic 2.5 x forward FLOPs; round 2 ran this on the fp32-exact engine (42.5 ms)"}
            del q4, k4, v4, do4, o4, l4
        except Exception as exc:  # noqa: BLE001
            configs["cfg4_int8_bwd"] = {"error": repr(exc)}
        # config 4's quantised forward WITH a mask, the way the reference's quantised entry takes one: a dense fp32 additive
        # [B, H, Sq, Skv] tensor (MFABridge+Quantized.swift:227-358 -- 4.3 GB at this size: the call is bound by reading it once).
        # Block-diagonal, four documents of 2048 tokens; rel against the oracle's quantised restatement with the same mask on the
        # rows of four 64-row quantisation blocks of two heads.
        try:
            S4 = 8192
            q4, k4, v4 = (torch.randn(1, 16, S4, D, device=dev, dtype=torch.bfloat16) for _ in range(3))
            i4 = torch.arange(S4, device=dev)
            mb = ((i4[:, None] // 2048) == (i4[None, :] // 2048))
            m32 = torch.zeros(1, 16, S4, S4, device=dev, dtype=torch.float32).masked_fill_(~mb[None, None], float("-inf"))
            out4 = torch.empty(1, 16, S4, D, device=dev, dtype=torch.float32)
            lse4 = torch.empty(16 * S4, device=dev, dtype=torch.float32)
            fn4 = lambda: umfa_torch.quantized_attention_forward_stream(q4, k4, v4, mask=m32, out=out4, lse=lse4)  # noqa: E731
            tm = graph_ms(fn4, 6, warmup=2)
            kn4 = umfa_torch.last_kernel()
            fn4()
            torch.cuda.synchronize()
            from oracle import oracle as _orc4
            import numpy as _np4
            rows4 = _np4.concatenate([_np4.arange(b0, b0 + 64) for b0 in (0, 2048 + 640, 4096 + 1984, 8192 - 64)])
            rel4 = 0.0
            for h4 in (0, 9):
                rq = _np4.ascontiguousarray(_par.bits(q4[:, h4:h4 + 1])[:, :, rows4])
                mrow = _np4.ascontiguousarray(m32[0, h4][torch.as_tensor(rows4, device=dev)].cpu().numpy())[None, None]
                ref4, _ = _orc4.quantized_forward(rq, _par.bits(k4[:, h4:h4 + 1]), _par.bits(v4[:, h4:h4 + 1]), mask=mrow)
                got4 = out4[:, h4:h4 + 1][:, :, torch.as_tensor(rows4, device=dev)].cpu().numpy()
                rel4 = max(rel4, float(_np4.abs(got4 - ref4).max() / _np4.abs(ref4).max()))
            f4m = 4.0 * 16 * S4 * S4 * D
            configs["cfg4_int8_mask_blockdiag"] = {"ms": round(tm, 4), "kernel": kn4, "visible_fraction": 0.25,
                                                   "tflops_of_visible_work": round(f4m * 0.25 / tm / 1e9, 1),
                                                   "mask_bytes": int(m32.numel() * 4), "mask_read_tbps_if_read_once": round(m32.numel() * 4 / tm / 1e9, 2),
                                                   "rel_vs_quantised_oracle": rel4,
                                                   "mask": "fp32 additive [1,16,8192,8192] (0 / -inf, four documents of 2048): the reference ABI's form"}
            # ... and the same mask the way a torch caller HAS it -- bool [1, 1, S, S], 64 MB -- through umfa_quantized_forward_masked_stream
            # (read in place with its strides: nothing is expanded); same rows, same oracle
            mbool = mb[None, None].contiguous()
            fn4b = lambda: umfa_torch.quantized_attention_forward_stream(q4, k4, v4, mask=mbool, out=out4, lse=lse4)  # noqa: E731
            tmb = graph_ms(fn4b, 6, warmup=2)
            fn4b()
            torch.cuda.synchronize()
            rel4b = 0.0
            for h4 in (0, 9):
                rq = _np4.ascontiguousarray(_par.bits(q4[:, h4:h4 + 1])[:, :, rows4])
                mrow = _np4.ascontiguousarray(m32[0, h4][torch.as_tensor(rows4, device=dev)].cpu().numpy())[None, None]
                ref4, _ = _orc4.quantized_forward(rq, _par.bits(k4[:, h4:h4 + 1]), _par.bits(v4[:, h4:h4 + 1]), mask=mrow)
                got4 = out4[:, h4:h4 + 1][:, :, torch.as_tensor(rows4, device=dev)].cpu().numpy()
                rel4b = max(rel4b, float(_np4.abs(got4 - ref4).max() / _np4.abs(ref4).max()))
            configs["cfg4_int8_mask_blockdiag_bool"] = {"ms": round(tmb, 4), "kernel": umfa_torch.last_kernel(), "visible_fraction": 0.25,
                                                        "tflops_of_visible_work": round(f4m * 0.25 / tmb / 1e9, 1), "mask_bytes": int(mbool.numel()),
                                                        "rel_vs_quantised_oracle": rel4b,
                                                        "mask": "bool [1,1,8192,8192], the same four documents: umfa_quantized_forward_masked_stream (additive entry)"}
            del q4, k4, v4, m32, out4, lse4, mbool
        except Exception as exc:  # noqa: BLE001
            configs["cfg4_int8_mask_blockdiag"] = {"error": repr(exc)}
        extra["configs"] = configs
        try:
            extra["int8"] = bench_int8(torch, umfa_torch, event_ms, med, graph_ms)
        except Exception as exc:  # noqa: BLE001  reported, never silently replaced by another path
            extra["int8"] = {"error": repr(exc)}
        try:
            extra["host_boundary"] = bench_host_boundary(B, H, S, D)  # default options: one upload, the kernels, one download
            with umfa_torch.options(sync_chunks=0):  # opt-in: head chunks on side streams, pinned host ranges
                extra["host_boundary"]["chunked_opt_in_ms_per_call"] = bench_host_boundary(B, H, S, D)["ms_per_call"]
        except Exception as exc:  # noqa: BLE001
            extra["host_boundary"] = {"error": repr(exc)}
        if not args.no_parity:
            try:
                extra["parity"] = measure_parity(torch, umfa_torch)
            except Exception as exc:  # noqa: BLE001
                extra["parity"] = {"error": repr(exc)}

    if rank == 0:
        traffic, tsrc = None, None
        tfile = ROOT / "profiles" / "traffic_latest.json"
        if tfile.exists():
            try:
                tj = json.loads(tfile.read_text())
                traffic, tsrc = tj.get("hbm_bytes_per_launch"), f"static: profiles/traffic_latest.json ({tj.get('source', 'rocprofv3 PMC passes')}), not measured in this run"
            except Exception:  # noqa: BLE001
                traffic = None
        line = {
            "metric": METRIC,
            "value": round(flops * args.steps / dt / 1e12, 2),
            "unit": "TFLOP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,  # the CLI argument; every other untimed launch (graph upload, cold region, settle) is counted under `settle`
            "ms_per_step": round(dt / args.steps * 1e3, 4),
            "cold_start_ms_per_step": settle["cold_start_ms_per_step"],  # the same K steps right after the W warm-up steps, the board just out of idle
            "ms_eager": round(durs[len(durs) // 2], 5),  # median of per-call HIP events on EAGER launches of the same step (what a PyTorch-eager caller sees)
            "timer": {"version": 2, "headline": "wall clock around one hipGraph of K steps (barrier + synchronize on both sides), sustained state",
                      "configs": "graph_ms: HIP events around 3 back-to-back replays of one hipGraph of n calls, / (3 n) -- since round 5; rounds 1-4 timed ONE replay "
                                 "(one replay's launch latency, tens of us, was inside): not like-for-like with BENCH_r01 ... r04"},
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic N(0,1) Q/K/V, torch.manual_seed(1234) on every rank (one shared problem)",
            "config": {"workload": f"FLUX-shape SDPA forward B={B} H={H} S={S} D={D} bf16{' causal' if args.causal else ''}, "
                                   "ONE problem, fp32 O (the C ABI's contract), default options: P V product in fp16, V cast pre-pass inside the step" +
                                   (f", {H // world} heads per rank + RCCL all-gather of O to every rank" if world > 1 else ""),
                       "kernel": kernel_name, "entry": "umfa_attention_forward_stream (in-stream C ABI)",
                       "launch": ("eager launches (RCCL collectives are not captured)" if (world > 1 or args.no_graph) else
                                  f"one hipGraph of {args.steps} launches") + "; cold region, untimed settle, then the timed region (`settle`)",
                       "parallelism": ("single GPU" if world == 1 else
                                       f"heads dealt over {world} ranks in two chunks (umfa_torch.parallel.owned_heads), in-place all_gather_into_tensor "
                                       "per chunk on a side stream under the next chunk's kernel (RCCL over xGMI)"),
                       "gathered_equals_local": gathered_ok,
                       **({"all_gather_form": {True: "in-place", False: "staged (in-place form refused or wrong on this runtime)"}.get(
                           next(iter(parallel._INPLACE_OK.values()), None), "unknown")} if strong_ok and not rehearsal else {}),
                       "ranks": world},
            "settle": settle,
            **({"rehearsal": "UMFA_BENCH_ONE_DEVICE=1: all ranks on cuda:0 over gloo -- a code-path check, not a measurement"} if rehearsal else {}),
            "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
                         "frac_of_2516": round(achieved / 2516.0, 4),  # SURVEY.md section 8d quotes the dense bf16 peak as 2.516 PFLOP/s (256 CUs x 4096 FLOP/clk x 2.4 GHz)
                         "traffic": traffic, "traffic_source": tsrc,
                         "traffic_kind": "static",
                         "kernel_ms_mean": round(mean_ms, 5), "kernel_ms_min": round(durs[0], 5),
                         "flops_per_launch": local_flops,
                         "launch": "one step = the call's kernels on the launch stream: the V cast pre-pass (bf16 -> fp16, HBM-bound) + the attention "
                                   "kernel; HIP events around the call, so `achieved` prices BOTH against the attention kernel's FLOPs"},
        }
        if weak:
            line["weak"] = weak
        if cfg5:
            line["cfg5"] = cfg5
        line.update(extra)
        if world == 1 and not args.no_cpu_baseline and not args.headline_only:
            line["cpu_baseline"] = cpu_baseline(os.cpu_count() or 1)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


def bench_int8(torch, umfa_torch, event_ms, med, graph_ms):
    """int8 block-quantised forward (quantiser pre-pass INCLUDED) vs the bf16 forward with the same fp32 O, both through
    their in-stream entries on the same stream, both timed by the same HIP events."""
    res = {}
    for name, (Bx, Hx, Sx) in {"flux_B1_H24_S4096_D128": (1, 24, 4096), "cfg4_B1_H16_S8192_D128": (1, 16, 8192)}.items():
        torch.manual_seed(0)
        q, k, v = (torch.randn(Bx, Hx, Sx, D, device="cuda", dtype=torch.bfloat16) for _ in range(3))
        out = torch.empty(Bx, Hx, Sx, D, device="cuda", dtype=torch.float32)
        out8 = torch.empty(Bx, Hx, Sx, D, device="cuda", dtype=torch.float32)
        lse8 = torch.empty(Bx * Hx * Sx, device="cuda", dtype=torch.float32)
        # graph-replayed like the headline and the configs (round 5; per-call eager events until then: a call timed from an idle queue
        # carries its launch latency, and the three sides did not carry the same -- one box read the FLUX int8 call at 0.236 ms where
        # back-to-back launches of the same build measure 0.183).  Median of three graphs of 20 calls, the sides interleaved.
        fns = {"bf": lambda: umfa_torch.attention_forward(q, k, v, out=out),
               "i8": lambda: umfa_torch.quantized_attention_forward_stream(q, k, v, out=out8, lse=lse8),
               "f8": lambda: umfa_torch.quantized_attention_forward_stream(q, k, v, quant_mode="blockwise_fp8pv", out=out8, lse=lse8)}
        ts = {n_: [] for n_ in fns}
        for _ in range(3):
            for n_, fn_ in fns.items():
                ts[n_].append(graph_ms(fn_, 20))
        bf, i8, f8 = (med(ts[n_]) for n_ in ("bf", "i8", "f8"))
        fns["bf"]()
        kb = umfa_torch.last_kernel()
        fns["i8"]()
        k8 = umfa_torch.last_kernel()
        fns["f8"]()
        fl = 4.0 * Bx * Hx * Sx * Sx * D
        # mixed peak of the reference's int8 arithmetic: half the FLOPs (QK^T) on the int8 MFMA at 2x the
        # bf16 rate, half (P V) on the fp16 MFMA: time floor = flops / 2 / 5000 + flops / 2 / 2500 -> 3333 TFLOP/s
        mixed_peak = 1.0 / (0.5 / (2 * PEAK_BF16_TFLOPS) + 0.5 / PEAK_BF16_TFLOPS)
        res[name] = {"bf16_ms": round(bf, 4), "int8_ms_incl_quantiser": round(i8, 4), "speedup": round(bf / i8, 3),
                     "int8_TOPs": round(fl / i8 / 1e9, 1), "int8_mixed_peak_TOPs": round(mixed_peak, 1),
                     "int8_frac_of_mixed_peak_incl_quantiser": round(fl / i8 / 1e9 / mixed_peak, 4),
                     "fp32_out": True, "bf16_kernel": kb, "int8_kernel": k8,
                     "fp8pv_ms_incl_quantiser": round(f8, 4), "fp8pv_speedup": round(bf / f8, 3), "fp8pv_kernel": umfa_torch.last_kernel(),
                     "modes": "int8 = quant_mode 2, the reference's arithmetic (int8 Q K V block-wise, P and P V in fp16); fp8pv = quant_mode 3 "
                              "(opt-in: int8 Q K^T, fp8 e4m3 P and V on the 2x-rate MFMA; rel-err in parity.cfg4_fp8pv)",
                     "timer": "HIP events around hipGraph replays of 20 calls, median of 3 graphs, the three sides interleaved"}
        del q, k, v, out, out8, lse8
    try:
        fx, c4 = res["flux_B1_H24_S4096_D128"], res["cfg4_B1_H16_S8192_D128"]
        res["summary"] = (f"against the default bf16 forward, quantiser included: the reference's int8 arithmetic {c4['speedup']:.2f}x at config 4 "
                          f"({fx['speedup']:.2f}x at the FLUX shape); the SageAttention2-style fp8 P V mode {c4['fp8pv_speedup']:.2f}x "
                          f"({fx['fp8pv_speedup']:.2f}x) at 2x the quantisation error (parity.cfg4_fp8pv)")
        # why the north-star's >= 1.3x is not reachable under the reference's arithmetic (mode 2), with this line's own numbers
        res["why_not_1_3x"] = ("mode 2 keeps P V on a 1x-rate MFMA: K Q^T at 2x + P V at 1x = 3/4 of the bf16 kernel's matrix cycles, a ceiling of 1.33x for the KERNEL; "
                               f"the separate quantiser pass (~29 us: reads Q, K, V, writes int8 Q, K and the fp16 V image) is {29.0 / (fx['bf16_ms'] * 1e3):.0%} of the "
                               f"FLUX call, so the CALL's ceiling there is {1.0 / (0.75 + 29.0 / (fx['bf16_ms'] * 1e3)):.2f}x before any other cost, and both kernels sit on the "
                               "board's power cap, where 25 % fewer matrix cycles return ~12 % of time.  A 2x-rate P V with an accurate (int8) P needs P <= 1, i.e. the exact "
                               "running max: +46 % on the bf16 kernel (configs.cfg3_flux_bf16_pvbf16_exact against _lazy) for at most 1/6 of the matrix cycles -- not built. "
                               "Only the opt-in fp8 P V mode (3-bit mantissas for P and V) passes 1.3x, at config 4.")
    except Exception:  # noqa: BLE001
        pass
    return res


def bench_host_boundary(B, H, S, D, calls: int = 5):
    """The PCIe-inclusive rate of the reference ABI's SYNCHRONOUS entry: mfa_attention_forward on buffers that wrap HOST memory
    (mfa_buffer_from_ptr, MFABridge.swift:1074-1433) -- every call uploads Q, K, V, runs the same kernels as the headline and
    downloads the fp32 O.  Reported beside `value`, never as it: `value` starts with the operands resident in HBM."""
    import time

    import numpy as np
    import umfa
    from umfa import core as _core

    rng = np.random.default_rng(1234)
    # bf16 bit patterns of N(0,1) (the top halves of fp32 words)
    q, k, v = ((rng.standard_normal((B, H, S, D), dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16) for _ in range(3))
    o = np.zeros((B, H, S, D), np.float32)
    with umfa.MFAContext() as ctx:
        bufs = [_core.MFABuffer(ctx, a) for a in (q, k, v, o)]
        try:
            def call():
                _core._check_error(_core._lib.mfa_attention_forward(
                    ctx.handle, *(x.handle for x in bufs), B, S, S, H, D, float(D) ** -0.5, False, _core.MFA_PRECISION_BF16,
                    _core.MFA_PRECISION_BF16, _core.MFA_PRECISION_FP32, False, False, False, False, None, 0, None, None, 0,
                    _core.MFA_MASK_TYPE_NONE, _core.MFA_MASK_SCALAR_BYTE))
            call()  # (pools, pinned staging)
            ts = []
            for _ in range(calls):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            kern = ctx.last_kernel
        finally:
            for x in bufs:
                x.close()
    ts.sort()
    t = ts[len(ts) // 2]
    moved = q.nbytes * 3 + o.nbytes
    return {"entry": "mfa_attention_forward on mfa_buffer_from_ptr(host) buffers: upload Q, K, V + kernels + download fp32 O, synchronous "
                     "(default options: one upload, the kernels, one download; `chunked_opt_in_ms_per_call`: option sync_chunks = 0, DESIGN.md section 1)",
            "ms_per_call": round(t * 1e3, 3), "tflops_pcie_inclusive": round(4.0 * B * H * S * S * D / t / 1e12, 2),
            "host_bytes_moved": int(moved), "host_link_gbps": round(moved / t / 1e9, 2), "calls": calls, "kernel": kern,
            "finite": bool(np.isfinite(o).all() and np.abs(o).max() > 0),
            "note": "not `value`: the headline starts with the operands resident in HBM (the in-stream entry, as the reference's torch extension calls it)"}


def measure_parity(torch, umfa_torch):
    """rel = max|O - O_ref| / max|O_ref| (and rms) at FULL size, O_ref = the fp64 CPU oracle on the rounded inputs, on a
    row subset (8 groups of 32 rows, every head, all keys).  The oracle is the checker here, nothing else."""
    import numpy as np

    from oracle import oracle, parity
    res = {"metric": "max|O-Oref|/max|Oref| (rms: rms(O-Oref)/rms(Oref)); Oref = oracle/sdpa_ref.c fp64 on the rounded inputs; "
                     "rows = 8 groups of 32 per (batch, head), all keys"}
    bf, f32 = torch.bfloat16, torch.float32

    def run(name, Bx, Hx, Sx, Dx, causal, out_dtype):
        torch.manual_seed(0)
        q, k, v = (torch.randn(Bx, Hx, Sx, Dx, device="cuda", dtype=torch.float32).to(bf) for _ in range(3))
        o = umfa_torch.attention_forward(q, k, v, causal=causal, out_dtype=out_dtype)
        torch.cuda.synchronize()
        rows = parity.sample_rows(Sx)
        ref = oracle.sdpa_forward_rows(parity.bits(q), parity.bits(k), parity.bits(v), rows, causal=causal).astype(np.float64)
        d = o[:, :, rows].float().cpu().numpy().astype(np.float64) - ref
        res[name] = {"rel": float(np.abs(d).max() / np.abs(ref).max()), "rms": float(np.sqrt((d * d).mean() / (ref * ref).mean())),
                     "kernel": umfa_torch.last_kernel(), "rows": int(rows.size)}

    run("cfg2_B4_H16_S1024_D64_causal_fp32O", 4, 16, 1024, 64, True, f32)
    run("cfg3_flux_fp32O", 1, 24, 4096, 128, False, f32)
    run("cfg3_flux_bf16O", 1, 24, 4096, 128, False, bf)
    run("cfg5_shard_B1_H4_S32768_fp32O", 1, 4, 32768, 128, False, f32)
    run("cfg5_shard_B1_H4_S32768_bf16O", 1, 4, 32768, 128, False, bf)
    # cfg4: the int8 block-wise forward against the oracle's QUANTISED restatement (whole slabs fake-quantised with the
    # oracle's quantiser, then the fp64 forward) and against exact SDPA, three heads
    torch.manual_seed(0)
    Bx, Hx, Sx = 1, 16, 8192
    q, k, v = (torch.randn(Bx, Hx, Sx, D, device="cuda", dtype=torch.float32).to(bf) for _ in range(3))
    o8 = umfa_torch.quantized_attention_forward_stream(q, k, v)
    torch.cuda.synchronize()
    k8_name = umfa_torch.last_kernel()  # (read now: the fp8 run below changes it)
    hs, rows = [0, 7, 15], parity.sample_rows(Sx)

    def fake_quant(x):
        f = oracle.to_f32(x).reshape(len(hs), -1)
        o = np.empty_like(f)
        for i in range(len(hs)):
            qi, sc = oracle.quantize_symmetric(f[i], group=64 * D, bits=8)
            o[i] = oracle.dequantize(qi, sc, group=64 * D)
        return o.reshape(1, len(hs), -1, D)

    qs, ks, vs = (parity.bits(t[:, hs]) for t in (q, k, v))
    ref_q = oracle.sdpa_forward_rows(fake_quant(qs), fake_quant(ks), fake_quant(vs), rows)
    ref_x = oracle.sdpa_forward_rows(qs, ks, vs, rows)
    got = o8[:, hs][:, :, rows].cpu().numpy()
    o3 = umfa_torch.quantized_attention_forward_stream(q, k, v, quant_mode="blockwise_fp8pv")
    torch.cuda.synchronize()
    got3 = o3[:, hs][:, :, rows].cpu().numpy()
    ref3 = oracle.quantized_forward_fp8pv(qs, ks, vs, rows=rows)
    res["cfg4_fp8pv_B1_H16_S8192"] = {"rel_vs_its_restatement_exact_P": parity.rel_err(got3, ref3), "rel_vs_exact_sdpa": parity.rel_err(got3, ref_x),
                                      "rel_vs_int8_oracle": parity.rel_err(got3, ref_q), "kernel": umfa_torch.last_kernel(), "heads": hs, "rows": int(rows.size)}
    res["cfg4_int8_blockwise_B1_H16_S8192"] = {"rel_vs_quantized_oracle": parity.rel_err(got, ref_q), "rel_vs_exact_sdpa": parity.rel_err(got, ref_x),
                                               "quantisation_itself": parity.rel_err(ref_q, ref_x), "kernel": k8_name,
                                               "heads": hs, "rows": int(rows.size)}
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--headline-only", action="store_true", help="only the headline workload: no strong / cfg5 legs, no configs / int8 / parity / cpu_baseline (A/B and rocprof runs: "
                         "every fa_fwd16_w64 dispatch of the process is then a FLUX launch)")
    ap.add_argument("--causal", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="launch the K timed steps eagerly instead of as one hipGraph")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write the headline's output of its last step (fp32 O) "
                         "as DIR/<name>.npy: at most 64 MB, inputs seeded, so two builds can be compared output for output")
    ap.add_argument("--launcher-selftest", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))  # fresh child processes; this one never touches a GPU
    if args.launcher_selftest:
        launcher_selftest()
        return
    run_rank(args)


if __name__ == "__main__":
    main()
