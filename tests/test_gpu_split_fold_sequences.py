"""The three users of the split-KV fold's ticketed scratch block (runtime_internal.h StreamScratch::split), one after another on one stream.

The decode form of the 128-row kernel (fa_fwd_16_kernel.h KS = 4), the plain 128-row split (option decode_ks = 2 with a forced part count) and
the balanced causal pairs (option cbal) share one block of ticket / flag words and partial slots per stream.  Every launch must leave its
words zero for the next one -- nothing clears them between launches -- and the block is retired and replaced while a sequence runs
(ensure_ticketed: the ticket area grows with few items x few parts, then many items x 32 parts).  A word left non-zero makes the next fold
skip or repeat parts: here that is a deterministic VALUE failure of a named launch, not a repeatability flake.  Some launches carry V far below
fp16's range, so that the converting kernels' range check sends every workgroup through its second sweep (whose barriers and amax exchange use
the LDS words the epilogue reserves: fa_fwd_16_kernel.h FWD16_EPI_*), and some read K / V through a [B, Skv, H, D] cache viewed as [B, H, Skv, D].

Each launch is checked against an fp64 reference first (per (batch, head) slab, at the bounds of tests/test_gpu_decode.py and the fuzz's decode
leg; LSE to 2e-3), then run once more and compared bit for bit.  One sequence is also captured whole as a graph (after a warm-up pass on the
capture stream) and replayed twice against the eager outputs.  A fixed set of shapes: no seeds, no retries."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
NORTH_STAR = 1.0e-3
CEIL = {BF: 2.0 ** -8 * 1.5, FP: 2.0 ** -11 * 1.5}
LSE_TOL = 2.0e-3


# ---- launch specs ----
# vs: V's scale (1e-7: every output below 2^-11 -- the converting kernels' range check sends each workgroup through the second sweep, whose
# barriers and amax exchange use the words the epilogue reserves); strided: K / V are a [B, Skv, H, D] cache viewed as [B, H, Skv, D]
def dec(dt, D, B, H, Sq, Skv, split=0, pv=1, out=F32, vs=1.0, strided=False):
    """the decode form (at most 32 query rows per (batch, head); decode_ks = 1: whatever the CU count says about the plan's gate)"""
    return dict(kind="dec", dt=dt, D=D, B=B, H=H, Sq=Sq, Skv=Skv, out=out, vs=vs, strided=strided,
                opts=dict(decode_ks=1, pv_fp16=pv, **({"force_split": split} if split else {})))


def plain(dt, D, B, H, Sq, Skv, split, pv=1, vs=1.0):
    """the plain 128-row kernel's split (decode form off)"""
    return dict(kind="plain", dt=dt, D=D, B=B, H=H, Sq=Sq, Skv=Skv, out=F32, vs=vs, opts=dict(decode_ks=2, force_split=split, pv_fp16=pv))


def cbal(mode, dt, D, B, H, Sq, Skv, pv=1, out=F32, vs=1.0):
    """causal, the balanced pairs (cbal 1) or the unpaired schedule (cbal 2) of the 128-row kernel"""
    return dict(kind="cbal", dt=dt, D=D, B=B, H=H, Sq=Sq, Skv=Skv, out=out, vs=vs, opts=dict(cbal=mode, no_w64=1, pv_fp16=pv))


def gqa(dt, D, B, Hq, Hkv, Sq, Skv, split=0, packed=True):
    """grouped K / V heads the way the SDPA layer launches them (umfa_torch/sdpa.py _gqa_zero_copy): packed -- a KV head's query heads are
    the ROWS of one item; else -- the query heads are heads of a (batch x KV head) slab whose K / V head stride is 0"""
    return dict(kind="gqa_rows" if packed else "gqa_heads", dt=dt, D=D, B=B, H=Hq, Hkv=Hkv, Sq=Sq, Skv=Skv, out=F32,
                opts=dict(decode_ks=1, pv_fp16=1, **({"force_split": split} if split else {})))


# Each sequence: small launches (few items x few parts), then many items x 32 parts (the ticket area grows: a fresh block), then small
# launches again (they reuse the large block) with CBAL launches between decode launches.
SEQUENCES = {
    "bf16_d128_first": [
        dec(BF, 128, 1, 2, 1, 255, split=2),
        dec(BF, 128, 1, 2, 4, 33, split=5),
        dec(BF, 64, 1, 1, 1, 1),
        plain(BF, 128, 1, 2, 8, 300, split=2),
        dec(BF, 128, 2, 3, 4, 129, split=16),
        gqa(BF, 128, 1, 8, 2, 1, 1000, split=5),
        dec(BF, 128, 2, 8, 32, 4097, split=32),
        dec(BF, 128, 4, 8, 17, 4097, split=32),
        plain(BF, 128, 4, 8, 32, 2048, split=32),
        dec(BF, 64, 8, 8, 32, 4097, split=32),
        dec(BF, 128, 1, 1, 1, 127, split=2),
        dec(FP, 128, 1, 2, 3, 129, split=5),
        cbal(1, BF, 128, 2, 3, 512, 512),
        dec(BF, 128, 1, 2, 1, 255, split=16),
        cbal(1, FP, 64, 2, 2, 384, 1024),
        dec(BF, 64, 1, 3, 2, 33, split=2),
        dec(BF, 128, 2, 2, 8, 4097, split=32, pv=0),
        cbal(2, BF, 128, 2, 2, 1100, 1100),
        dec(BF, 128, 1, 4, 1, 4097),
        gqa(BF, 64, 2, 6, 3, 4, 255, split=16, packed=False),
        dec(BF, 128, 2, 3, 31, 129, split=2, out=BF),
        plain(FP, 64, 1, 2, 32, 127, split=5),
        cbal(1, BF, 64, 2, 3, 256, 256, pv=0),
        dec(FP, 64, 2, 2, 1, 1, split=5),
        dec(BF, 128, 1, 8, 16, 255, split=32),
        cbal(1, BF, 128, 1, 2, 1024, 1024, out=BF),
        dec(BF, 128, 2, 3, 1, 33),
    ],
    "mixed_d64_first": [
        dec(FP, 64, 1, 1, 1, 33, split=2),
        cbal(1, BF, 64, 2, 2, 256, 256),
        dec(BF, 64, 1, 2, 4, 127, split=5, pv=0),
        plain(BF, 64, 1, 3, 16, 255, split=2, pv=0),
        gqa(BF, 128, 2, 4, 1, 8, 129, split=2),
        dec(BF, 64, 1, 2, 32, 1, split=16),
        dec(FP, 128, 4, 8, 32, 4097, split=32),
        plain(BF, 64, 8, 8, 20, 4097, split=32),
        gqa(BF, 128, 4, 32, 8, 1, 4097, split=32),
        dec(BF, 128, 8, 8, 1, 4097, split=32),
        dec(BF, 64, 1, 1, 2, 129, split=2),
        cbal(1, BF, 128, 2, 2, 640, 200),
        dec(BF, 64, 1, 1, 2, 129, split=2),
        cbal(2, FP, 128, 2, 3, 512, 640),
        dec(BF, 128, 1, 3, 1, 4097, split=5),
        plain(BF, 128, 2, 2, 32, 33, split=16),
        cbal(1, BF, 128, 2, 2, 1152, 1152),
        dec(FP, 128, 1, 2, 8, 255, split=16, out=FP),
        gqa(BF, 64, 1, 8, 2, 2, 127, split=32, packed=False),
        dec(BF, 64, 2, 3, 31, 4097),
        cbal(1, FP, 128, 1, 3, 500, 500),
        dec(BF, 128, 1, 1, 1, 1, split=32),
        dec(BF, 128, 2, 2, 4, 255, split=2),
    ],
    "strided_and_second_sweep": [
        dec(BF, 128, 1, 2, 4, 255, split=2, vs=1e-7),
        dec(BF, 64, 2, 3, 1, 129, split=5, strided=True),
        cbal(1, BF, 128, 2, 2, 512, 512),
        dec(BF, 128, 1, 4, 8, 1000, vs=1e-7, strided=True),
        plain(BF, 128, 2, 2, 32, 4097, split=32, vs=1e-7),
        dec(BF, 64, 16, 8, 1, 4097, split=32),
        dec(BF, 128, 8, 8, 4, 4097, split=32, vs=1e-7),
        dec(FP, 64, 1, 2, 1, 33, split=2, strided=True),
        cbal(1, BF, 64, 2, 3, 384, 1024, vs=1e-7),
        dec(BF, 128, 1, 2, 2, 127, split=16, vs=1e-7),
        cbal(2, BF, 128, 1, 2, 1024, 1024),
        dec(BF, 128, 2, 2, 32, 4097, split=32, strided=True),
        gqa(BF, 128, 1, 8, 1, 4, 255, split=5),
        dec(BF, 64, 1, 1, 1, 1, vs=1e-7),
        cbal(1, BF, 128, 2, 3, 256, 256, vs=1e-7),
        dec(BF, 128, 2, 3, 17, 33, split=2),
    ],
}
GRAPH_SEQUENCE = [
    dec(BF, 128, 1, 2, 1, 255, split=2),
    cbal(1, BF, 128, 2, 2, 512, 512),
    dec(BF, 64, 1, 3, 4, 129, split=5),
    gqa(BF, 128, 2, 8, 2, 1, 1000, split=16),
    dec(BF, 128, 4, 8, 32, 4097, split=32),
    plain(BF, 128, 2, 4, 32, 2048, split=32),
    dec(FP, 128, 1, 2, 2, 33, split=16),
    cbal(1, FP, 64, 2, 2, 384, 1024),
    dec(BF, 128, 1, 2, 1, 4097, split=2, pv=0),
    dec(BF, 64, 2, 2, 17, 127),
]


def _bound(s):
    if s["out"] != F32:
        return 4.0e-3 if s["out"] == BF else 2.0e-3  # (the output type's own rounding: tests/test_gpu_decode.py, tests/test_gpu_cbal.py)
    if s["dt"] == FP or s["opts"].get("pv_fp16", 1) == 0:
        return CEIL[s["dt"]]
    return NORTH_STAR


def _inputs(s, idx):
    g = torch.Generator(device="cuda").manual_seed(1000 + idx)
    B, H, Sq, Skv, D, dt = s["B"], s["H"], s["Sq"], s["Skv"], s["D"], s["dt"]
    Hkv = s.get("Hkv", H)
    q = torch.randn(B, H, Sq, D, device="cuda", generator=g).to(dt)
    if s.get("strided"):
        k = torch.randn(B, Skv, Hkv, D, device="cuda", generator=g).to(dt).transpose(1, 2)
        v = (torch.randn(B, Skv, Hkv, D, device="cuda", generator=g) * s.get("vs", 1.0)).to(dt).transpose(1, 2)
    else:
        k = torch.randn(B, Hkv, Skv, D, device="cuda", generator=g).to(dt)
        v = (torch.randn(B, Hkv, Skv, D, device="cuda", generator=g) * s.get("vs", 1.0)).to(dt)
    return q, k, v


def _reference(s, q, k, v):
    g = s["H"] // k.shape[1]
    kk, vv = (k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)) if g > 1 else (k, v)
    sc = torch.matmul(q.double(), kk.double().transpose(-1, -2)) * s["D"] ** -0.5
    if s["kind"] == "cbal":
        i = torch.arange(s["Sq"], device="cuda")[:, None]
        j = torch.arange(s["Skv"], device="cuda")[None, :]
        sc = sc.masked_fill(~(j <= i), float("-inf"))
    return torch.matmul(torch.softmax(sc, dim=-1), vv.double()), torch.logsumexp(sc, dim=-1)


def _launch(umfa_torch, s, q, k, v, out=None):
    """one launch of the spec; returns (O [B, H, Sq, D], LSE [B, H, Sq], kernel name)"""
    B, H, Sq, Skv, D = s["B"], s["H"], s["Sq"], s["Skv"], s["D"]
    if out is None:
        out = torch.empty(B, H, Sq, D, device="cuda", dtype=s["out"])
    with umfa_torch.options(**s["opts"]):
        if s["kind"] in ("gqa_rows", "gqa_heads"):
            Hkv = k.shape[1]
            g = H // Hkv
            if s["kind"] == "gqa_rows":
                row_stride = q.stride(1) if Sq == 1 else q.stride(2)
                qp = q.as_strided((B * Hkv, 1, g * Sq, D), (g * q.stride(1), g * q.stride(1), row_stride, 1), q.storage_offset())
                kp = k.as_strided((B * Hkv, 1, Skv, D), (k.stride(1), k.stride(1), k.stride(2), 1), k.storage_offset())
                vp = v.as_strided((B * Hkv, 1, Skv, D), (v.stride(1), v.stride(1), v.stride(2), 1), v.storage_offset())
                ov = out.view(B * Hkv, 1, g * Sq, D)
            else:
                qp = q.as_strided((B * Hkv, g, Sq, D), (g * q.stride(1), q.stride(1), q.stride(2), 1), q.storage_offset())
                kp = k.as_strided((B * Hkv, g, Skv, D), (k.stride(1), 0, k.stride(2), 1), k.storage_offset())
                vp = v.as_strided((B * Hkv, g, Skv, D), (v.stride(1), 0, v.stride(2), 1), v.storage_offset())
                ov = out.view(B * Hkv, g, Sq, D)
            _, lse = umfa_torch.attention_forward(qp, kp, vp, out=ov, return_lse=True)
        else:
            _, lse = umfa_torch.attention_forward(q, k, v, causal=s["kind"] == "cbal", out=out, return_lse=True)
        kern = umfa_torch.last_kernel()
    return out, lse.view(B, H, Sq), kern


def _describe(s):
    return "%s %s D%d B%d H%d%s Sq%d Skv%d out %s%s%s" % (s["kind"], str(s["dt"])[6:], s["D"], s["B"], s["H"], "/%d" % s["Hkv"] if "Hkv" in s else "",
                                                         s["Sq"], s["Skv"], str(s["out"])[6:], " V x %g" % s["vs"] if s.get("vs", 1.0) != 1.0 else "",
                                                         " strided K/V" if s.get("strided") else "")


def _value_error(s, o, lse, ref, rl):
    """None, or the worst (b, h, row) of this launch against fp64 and its error (per (batch, head) slab), with the LSE error"""
    od = o.double()
    rowerr = ((od - ref).abs() / ref.abs().amax(dim=(2, 3), keepdim=True).clamp_min(1e-30)).amax(dim=-1)
    rowerr = torch.where(torch.isfinite(od).all(dim=-1), rowerr, torch.full_like(rowerr, float("inf")))
    lerr = (lse.double() - rl).abs().max().item()
    flat = int(torch.argmax(rowerr).item())
    H, Sq = rowerr.shape[1], rowerr.shape[2]
    wb, wh, wr = flat // (H * Sq), (flat // Sq) % H, flat % Sq
    rel = rowerr[wb, wh, wr].item()
    if rel <= _bound(s) and lerr <= LSE_TOL:  # (NaN compares false)
        return None
    return "worst (b %d, h %d, row %d) rel %.3e (bound %.1e), lse error %.3e (bound %.0e)" % (wb, wh, wr, rel, _bound(s), lerr, LSE_TOL)


def _check_kernel(s, kern):
    if not kern.startswith("fa_fwd16<"):
        return False
    if s["kind"] in ("dec", "gqa_rows", "gqa_heads"):
        return kern.endswith(",dec>")
    return not kern.endswith(",dec>")


def _run_sequence(umfa_torch, name, seq, stream):
    with torch.cuda.stream(stream):
        umfa_torch.release_scratch(stream)  # (the sequence grows this stream's block from nothing: no graph of this stream is live)
        for idx, s in enumerate(seq):
            q, k, v = _inputs(s, idx)
            ref, rl = _reference(s, q, k, v)
            o1, l1, kern = _launch(umfa_torch, s, q, k, v)
            where = "sequence %s launch %d: %s %s opts %s" % (name, idx, kern, _describe(s), s["opts"])
            assert _check_kernel(s, kern), "route: " + where
            err = _value_error(s, o1, l1, ref, rl)
            assert err is None, "values, first run: %s -- %s" % (where, err)  # values first
            o2, l2, _ = _launch(umfa_torch, s, q, k, v)
            err = _value_error(s, o2, l2, ref, rl)
            assert err is None, "values, second run: %s -- %s" % (where, err)
            assert torch.equal(o1, o2) and torch.equal(l1, l2), "not bitwise repeatable (both runs within bounds): " + where
        stream.synchronize()


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_split_fold_users_in_sequence(name):
    import umfa_torch
    _run_sequence(umfa_torch, name, SEQUENCES[name], torch.cuda.Stream())


def test_split_fold_sequence_captured_as_one_graph():
    """the whole sequence as one captured graph, after one warm-up pass on the capture stream (the block has its final size: nothing grows
    while capturing); two replays, each output bitwise the eager one and inside the fp64 bound"""
    import umfa_torch
    seq = GRAPH_SEQUENCE
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    data = [_inputs(s, 500 + idx) for idx, s in enumerate(seq)]
    refs = [_reference(s, *d) for s, d in zip(seq, data)]
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(side):
        umfa_torch.release_scratch(side)
        eager = []
        for idx, (s, d) in enumerate(zip(seq, data)):
            o, l, kern = _launch(umfa_torch, s, *d)
            where = "graph sequence launch %d (eager): %s %s opts %s" % (idx, kern, _describe(s), s["opts"])
            assert _check_kernel(s, kern), "route: " + where
            err = _value_error(s, o, l, *refs[idx])
            assert err is None, "values: %s -- %s" % (where, err)
            eager.append((o.clone(), l.clone(), kern))
        side.synchronize()
        outs = [torch.empty_like(e[0]) for e in eager]
        gr = torch.cuda.CUDAGraph()
        lses = []
        with torch.cuda.graph(gr, stream=side):
            for s, d, o in zip(seq, data, outs):
                lses.append(_launch(umfa_torch, s, *d, out=o)[1])
        for rep in range(2):
            for o in outs:
                o.fill_(float("nan"))
            gr.replay()
            side.synchronize()
            for idx, s in enumerate(seq):
                where = "graph sequence launch %d (replay %d): %s %s opts %s" % (idx, rep, eager[idx][2], _describe(s), s["opts"])
                err = _value_error(s, outs[idx], lses[idx], *refs[idx])
                assert err is None, "values: %s -- %s" % (where, err)
                assert torch.equal(outs[idx], eager[idx][0]) and torch.equal(lses[idx], eager[idx][1]), "replay differs from eager: " + where
    torch.cuda.current_stream().wait_stream(side)
    del gr
