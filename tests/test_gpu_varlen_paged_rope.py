"""Rotary embedding fused into varlen_kvcache_attention on the GPU: the rotated cache rows, O and LSE against
the fp64 reference (tests/paged_rope_ref.py) under the format bounds; O, LSE and both pools bit for bit against the parent sequence
(packed operands rotated by ops.rope_rotate, then the existing entry); both work-item forms in one launch; equal lengths against
kvcache_attention with rotary; device-side rules on cu_seqlens_q and cache_seqlens; graph replay; opcheck / torch.compile; refusals."""
import numpy as np
import pytest
import torch

import paged_ref
import paged_rope_ref as rr
import tolerances as tol
import varlen_paged_ref as vref
from paged_rope_gpu import DT, bits, check_rotated_rows, i32, np64, rotate_by_ops, tables

pytestmark = pytest.mark.gpu

GUARD = 2
H, HKV, PS, MAXP = 8, 2, 16, 6  # capacity 96
RO = 104
LQ = [1, 35, 2, 0]  # decode (g L_q = 4 rows), a prefill chunk in the 128-row form (140 rows), speculative decode, an idle sequence
SL = [47, 14, 0, 30]


def _umfa():
    import umfa_torch
    return umfa_torch


def _cu(lq):
    return np.concatenate([[0], np.cumsum(lq)]).astype(np.int64)


def _inputs(dt, D, lq, seed, pad=0, cache="paged"):
    B, Tq = len(lq), int(sum(lq)) + pad
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=DT[dt], generator=g)  # noqa: E731
    q, kn, vn = rnd(Tq, H, D), rnd(Tq, HKV, D), rnd(Tq, HKV, D)
    if cache == "paged":
        shape, bt = (B * MAXP + 2 * GUARD, PS, HKV, D), np.random.default_rng(seed).permutation(B * MAXP).reshape(B, MAXP) + GUARD
    else:
        shape, bt = ((B, PS * MAXP, HKV, D) if cache == "bshd" else (B, HKV, PS * MAXP, D)), None
    kc, vc = rnd(*shape), rnd(*shape)
    if cache == "bhsd":
        kc, vc = kc.transpose(1, 2), vc.transpose(1, 2)
    return q, kc, vc, None if bt is None else i32(bt), kn, vn


def _fused(um, q, kc, vc, kn, vn, cu, max_q, sl, bt, cos, sin, inter, causal, splits=0):
    kc, vc = kc.clone(), vc.clone()
    o, lse = um.varlen_kvcache_attention(q, kc, vc, cu, max_q, sl, block_table=bt, k=kn, v=vn, causal=causal, num_splits=splits,
                                         return_softmax_lse=True, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=inter)
    torch.cuda.synchronize()
    return o, lse, kc, vc, um.last_kernel()


def _sequence(um, q, kc, vc, kn, vn, cu, max_q, sl, bt, cos, sin, inter, causal, splits=0):
    """the parent commit's sequence: rope_rotate(q), rope_rotate(k) at the packed rows' positions, the existing entry"""
    cap = kc.shape[1] * (bt.shape[1] if bt is not None else 1)
    c, s = cu.cpu().numpy(), sl.cpu().numpy()
    pq, cov = rr.packed_positions(c, q.shape[0], max_q, s, cap, causal)
    pk, _ = rr.packed_positions(c, q.shape[0], max_q, s, cap, True)
    covt = torch.tensor(cov, device="cuda")[:, None, None]
    rq = torch.where(covt, rotate_by_ops(um, q, pq, cos, sin, inter), q)
    rk = torch.where(covt, rotate_by_ops(um, kn, pk, cos, sin, inter), kn)
    kc, vc = kc.clone(), vc.clone()
    o, lse = um.varlen_kvcache_attention(rq, kc, vc, cu, max_q, sl, block_table=bt, k=rk, v=vn, causal=causal, num_splits=splits,
                                         return_softmax_lse=True)
    torch.cuda.synchronize()
    return o, lse, kc, vc, um.last_kernel()


def _check_values(dt, q, kc0, vc0, kn, vn, cu, max_q, sl, bt, cos, sin, inter, causal, got, tag=""):
    o, lse, kc1, vc1, kernel = got
    rd = 2 * cos.shape[1]
    c, s, btn = cu.cpu().numpy(), sl.cpu().numpy(), None if bt is None else bt.cpu().numpy()
    ref = rr.forward_packed(np64(q), np64(kc0), np64(vc0), c, max_q, s, np64(cos), np64(sin), btn, np64(kn), np64(vn), causal, None, inter, dt)
    _, rk = rr.packed_operands(np64(q), np64(kn), kc0, c, max_q, s, np64(cos), np64(sin), btn, causal, inter)
    exact, _ = vref.append(np64(kc0), np64(vc0), rk, np64(vn), c, max_q, s, btn)  # the pool with the UNROUNDED rotation appended
    srcm, _ = vref.append(np.zeros(kc0.shape), np.zeros(kc0.shape), np64(kn), np64(vn), c, max_q, s, btn)
    wrote = (bits(kc0) != bits(kc1)).reshape(*kc0.shape[:3], -1).any(-1)
    assert (wrote == (ref[2] != np64(kc0)).any(-1)).all()  # exactly the reference's rows were written
    k1 = np64(kc1)
    check_rotated_rows(k1[wrote], exact[wrote], srcm[wrote], rd, inter, dt, tag)
    assert (k1[wrote][..., rd:] == srcm[wrote][..., rd:]).all() and (np64(vc1) == ref[3]).all()
    o_ref, lse_ref = ref[0], ref[1]
    live = np.isfinite(lse_ref)  # [H, T_q]
    o_, l_ = np64(o), np64(lse)
    cov = vref.covered(c, o_.shape[0], max_q)
    dead = ~live & cov[None, :]
    assert np.isfinite(o_[cov]).all() and (o_.transpose(1, 0, 2)[dead] == 0).all() and np.isneginf(l_[dead]).all()
    if live.any():
        print(f"{tag}: {kernel} lse max err {float(np.abs(l_[live] - lse_ref[live]).max()):.3e}")
        np.testing.assert_allclose(l_[live], lse_ref[live], rtol=0, atol=2e-3)
        tol.check_forward(o_.transpose(1, 0, 2)[live][None, None], o_ref.transpose(1, 0, 2)[live][None, None], DT[dt], kernel,
                          tag="varlen_paged_rope", out_dt=DT[dt])


def _check_bits(a, b, cov=None):
    assert a[4] == b[4], (a[4], b[4])
    for x, y, name in zip(a[:4], b[:4], ("O", "LSE", "k_cache", "v_cache")):
        if cov is not None and name in ("O", "LSE"):  # rows no sequence covers are not written
            x, y = (x[cov], y[cov]) if name == "O" else (x[:, cov], y[:, cov])
        assert (bits(x) == bits(y)).all(), (name, int((bits(x) != bits(y)).sum()))


# (dtype, head_dim, rotary_dim, interleaved, causal, fp32 tables, cache, num_splits, pad rows)
GRID = [("bf16", 128, 128, False, True, True, "paged", 0, 0), ("fp16", 64, 64, True, True, False, "paged", 0, 0),
        ("bf16", 64, 32, True, False, True, "paged", 0, 3), ("fp16", 128, 16, False, True, False, "paged", 0, 0),
        ("bf16", 128, 32, False, False, False, "paged", 2, 0), ("fp16", 128, 128, True, True, True, "paged", 2, 3),
        ("bf16", 128, 64, True, True, True, "bshd", 0, 0), ("fp16", 64, 16, False, False, True, "bhsd", 0, 0),
        ("bf16", 64, 64, False, True, False, "paged", 0, 0), ("fp16", 128, 32, True, False, False, "bshd", 2, 0)]


@pytest.mark.parametrize("dt,D,rd,inter,causal,f32,cache,splits,pad", GRID)
def test_values_then_bits_with_both_forms_in_one_launch(dt, D, rd, inter, causal, f32, cache, splits, pad):
    um = _umfa()
    seed = 200 + GRID.index((dt, D, rd, inter, causal, f32, cache, splits, pad))
    q, kc, vc, bt, kn, vn = _inputs(dt, D, LQ, seed, pad=pad, cache=cache)
    cos, sin = tables(RO, rd, torch.float32 if f32 else DT[dt], seed, pad=8 if pad else 0)
    cu, sl = i32(_cu(LQ)), i32(SL)
    args = (q, kc, vc, kn, vn, cu, max(LQ), sl, bt, cos, sin, inter, causal, splits)
    got = _fused(um, *args)
    assert um.ops.varlen_kvcache_item_counts() == (2 * HKV, 2 * HKV), "decode-form and 128-row items in one launch"
    assert got[4].startswith("fa_fwd16_paged_varlen<") and ("split" in got[4]) == (splits > 1), got[4]
    _check_values(dt, q, kc, vc, kn, vn, cu, max(LQ), sl, bt, cos, sin, inter, causal, got, tag=f"{dt}-{D}-{rd}-{cache}")
    cov = torch.tensor(vref.covered(_cu(LQ), q.shape[0], max(LQ)), device="cuda")
    _check_bits(got, _sequence(um, *args), cov)


@pytest.mark.parametrize("causal,inter", [(True, False), (False, True)])
def test_equal_lengths_agree_bitwise_with_kvcache_attention(causal, inter):
    um = _umfa()
    B, L, D, dt = 3, 4, 128, "bf16"
    q, kc, vc, bt, kn, vn = _inputs(dt, D, [L] * B, 301)
    cos, sin = tables(RO, 64, torch.float32, 302)
    cu, sl = i32(_cu([L] * B)), i32([14, 0, 47])
    got = _fused(um, q, kc, vc, kn, vn, cu, L, sl, bt, cos, sin, inter, causal, 2)
    kc2, vc2 = kc.clone(), vc.clone()
    o, lse = um.kvcache_attention(q.view(B, L, H, D), kc2, vc2, kn.view(B, L, HKV, D), vn.view(B, L, HKV, D), cache_seqlens=sl, block_table=bt,
                                  causal=causal, num_splits=2, return_softmax_lse=True, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=inter)
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(B, L, H, D), o) and torch.equal(got[1].view(H, B, L).transpose(0, 1), lse)
    assert torch.equal(got[2], kc2) and torch.equal(got[3], vc2)


@pytest.mark.parametrize("inter", [False, True])
def test_device_side_rules(inter):
    """positions come from cu_seqlens_q and cache_seqlens on the device: the last table row exactly and one past it, lengths -5 and
    1e9, table entries -1 and num_pages on the append's page, an append that overflows the capacity, rows behind cu[B] (not appended,
    not used), guard pages, untouched inputs"""
    um = _umfa()
    dt, D, rd, ro = "fp16", 64, 32, 40
    lq = [2, 2, 3, 2, 2, 2, 3]
    q, kc, vc, bt, kn, vn = _inputs(dt, D, lq, 311, pad=2)
    #      last row = ro - 1 | one past | negative | huge | page entry -1 | page entry num_pages | overflows the capacity (95 + 3 > 96)
    sl = i32([ro - 2, ro - 1, -5, 10 ** 9, 16, 30, 95])
    btn = bt.cpu().numpy()
    btn[4, 1] = -1
    btn[5, 1] = kc.shape[0]  # positions 30, 31 lie on logical page 1
    bt = i32(btn)
    cos, sin = tables(ro, rd, DT[dt], 312)
    cu = i32(_cu(lq))
    keep = [t.clone() for t in (q, kn, vn, cos, sin, sl, bt, cu)]
    cov = torch.tensor(vref.covered(_cu(lq), q.shape[0], 3), device="cuda")
    for causal in (True, False):
        args = (q, kc, vc, kn, vn, cu, 3, sl, bt, cos, sin, inter, causal)
        got = _fused(um, *args)
        wrote = (bits(kc) != bits(got[2])).reshape(*kc.shape[:3], -1).any(-1)
        assert not wrote[:GUARD].any() and not wrote[-GUARD:].any() and not wrote[btn[3]].any()
        assert not wrote[btn[4, 0]].any() and not wrote[btn[5, 0]].any()  # the rows of the two bad entries were dropped, not misplaced
        _check_values(dt, q, kc, vc, kn, vn, cu, 3, sl, bt, cos, sin, inter, causal, got, tag=f"rules-{inter}-{causal}")
        _check_bits(got, _sequence(um, *args), cov)
    for t, k in zip((q, kn, vn, cos, sin, sl, bt, cu), keep):
        assert torch.equal(t, k)


@pytest.mark.parametrize("splits", [0, 2])
def test_output_guard_bands_and_uncovered_rows_come_back_bit_identical(splits):
    """O and LSE written into the middle of sentinel-filled buffers (the ops entry takes the caller's buffers): the bands on both sides
    and the rows no sequence covers (pad rows behind cu[B]) keep every bit, and the rows in between are the public call's.  The q image
    itself lives in the library's pooled workspace, which no caller can see, so no sentinel can be placed beside it: the tally, the item list
    and the split partials lie in front of it and nothing behind, and the attention launches rewrite all three after the pre-pass, so this
    test does NOT catch a pre-pass that wrote outside the image.  What is checked of the image is its own rows, through O."""
    um = _umfa()
    dt, D, G, pad = "bf16", 128, 64, 3
    q, kc, vc, bt, kn, vn = _inputs(dt, D, LQ, 351, pad=pad)
    cos, sin = tables(RO, 64, torch.float32, 352)
    cu, sl = i32(_cu(LQ)), i32(SL)
    Tq = q.shape[0]
    want = _fused(um, q, kc, vc, kn, vn, cu, max(LQ), sl, bt, cos, sin, False, True, splits)
    bo = torch.full((Tq * H * D + 2 * G,), -7.5, dtype=DT[dt], device="cuda")
    bl = torch.full((H * Tq + 2 * G,), -7.5, dtype=torch.float32, device="cuda")
    kc2, vc2 = kc.clone(), vc.clone()
    o, lse = um.ops.varlen_kvcache_attention_rope_forward(q, kc2, vc2, cu, max(LQ), sl, cos, sin, bt, kn, vn, scale=D ** -0.5, causal=True,
                                                          num_splits=splits, out=bo[G:-G].view(Tq, H, D), lse=bl[G:-G].view(H, Tq))
    torch.cuda.synchronize()
    assert o.data_ptr() == bo[G:].data_ptr() and lse.data_ptr() == bl[G:].data_ptr()
    for b in (bo, bl):
        assert (b[:G] == -7.5).all() and (b[-G:] == -7.5).all()
    cov = torch.tensor(vref.covered(_cu(LQ), Tq, max(LQ)), device="cuda")
    assert (~cov).sum() == pad
    assert (o[~cov] == -7.5).all() and (lse[:, ~cov] == -7.5).all()  # rows no sequence covers are not written
    assert torch.equal(o[cov], want[0][cov]) and torch.equal(lse[:, cov], want[1][:, cov])
    assert torch.equal(kc2, want[2]) and torch.equal(vc2, want[3])


def test_graph_replay_follows_lengths_and_cu():
    um = _umfa()
    dt, D = "bf16", 128
    q, kc, vc, bt, kn, vn = _inputs(dt, D, LQ, 321)
    cos, sin = tables(RO, D, torch.float32, 322)
    cu, sl = i32(_cu(LQ)), i32(SL)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def step():
        return um.varlen_kvcache_attention(q, kc, vc, cu, 35, sl, block_table=bt, k=kn, v=vn, causal=True, return_softmax_lse=True,
                                           rotary_cos=cos, rotary_sin=sin)

    kc0, vc0 = kc.clone(), vc.clone()
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        res = step()
    kc.copy_(kc0)
    vc.copy_(vc0)
    for it, lq in enumerate(([1, 35, 2, 0], [3, 30, 0, 5], [35, 1, 1, 1])):  # the same T_q, other sequences
        cu.copy_(i32(_cu(lq)))
        before = (kc.clone(), vc.clone())
        graph.replay()
        torch.cuda.synchronize()
        got = (res[0].clone(), res[1].clone(), kc.clone(), vc.clone(), um.last_kernel())
        _check_values(dt, q, before[0], before[1], kn, vn, cu, 35, sl, bt, cos, sin, False, True, got, tag=f"replay {it}")
        _check_bits(got, _fused(um, q, before[0], before[1], kn, vn, cu, 35, sl, bt, cos, sin, False, True))
        sl.add_(i32(lq))  # the server advances the lengths on the device


def test_opcheck_and_compile():
    um = _umfa()
    q, kc, vc, bt, kn, vn = _inputs("bf16", 64, LQ, 331)
    cos, sin = tables(RO, 32, torch.float32, 332)
    cu, sl = i32(_cu(LQ)), i32(SL)
    torch.library.opcheck(torch.ops.umfa.varlen_kvcache_rope_forward_append.default,
                          (q, kc, vc, kn, vn, cu, 35, sl, cos, sin, True, bt, True, 0.125, 2))
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    def f(q, kc, vc, kn, vn):
        return um.varlen_kvcache_attention(q, kc, vc, cu, 35, sl, block_table=bt, k=kn, v=vn, causal=True, rotary_cos=cos, rotary_sin=sin)

    kc_e, vc_e = kc.clone(), vc.clone()
    torch._dynamo.reset()
    oc = torch.compile(f, fullgraph=True, backend=backend)(q, kc, vc, kn, vn)
    oe = f(q, kc_e, vc_e, kn, vn)
    torch.cuda.synchronize()
    assert len(graphs) == 1
    calls = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function" and "umfa" in str(n.target)]
    assert calls == ["umfa.varlen_kvcache_rope_forward_append"], calls
    assert torch.equal(oc, oe) and torch.equal(kc, kc_e) and torch.equal(vc, vc_e)
    assert um.last_kernel().startswith("fa_fwd16_paged_varlen<bf16,64,causal"), um.last_kernel()


def test_refusals_and_no_backward():
    um = _umfa()
    q, kc, vc, bt, kn, vn = _inputs("bf16", 128, LQ, 341)
    cos, sin = tables(RO, 64, torch.float32, 342)
    cu, sl = i32(_cu(LQ)), i32(SL)
    call = lambda **kw: um.varlen_kvcache_attention(q, kc.clone(), vc.clone(), cu, 35, sl, block_table=bt, k=kw.pop("k", kn),  # noqa: E731
                                                    v=kw.pop("v", vn), causal=True, **kw)
    assert call(rotary_cos=cos, rotary_sin=sin).shape == q.shape
    assert call(rotary_interleaved=True).shape == q.shape
    wide = torch.zeros(RO, 40, device="cuda")
    bad = [dict(rotary_cos=cos), dict(rotary_sin=sin), dict(rotary_cos=cos, rotary_sin=sin, k=None, v=None),
           dict(rotary_cos=cos.cpu(), rotary_sin=sin.cpu()), dict(rotary_cos=cos[0], rotary_sin=sin[0]),
           dict(rotary_cos=cos, rotary_sin=sin[:, :16]), dict(rotary_cos=cos, rotary_sin=sin.bfloat16()),
           dict(rotary_cos=cos.half(), rotary_sin=sin.half()),
           dict(rotary_cos=cos.t().contiguous().t(), rotary_sin=sin.t().contiguous().t()),
           dict(rotary_cos=wide[:, 1:33], rotary_sin=wide[:, 1:33]), dict(rotary_cos=wide[:, :4], rotary_sin=wide[:, :4]),
           dict(rotary_cos=wide[:, :12], rotary_sin=wide[:, :12]),
           dict(rotary_cos=torch.zeros(RO, 72, device="cuda"), rotary_sin=torch.zeros(RO, 72, device="cuda")),
           dict(rotary_cos=cos[:0], rotary_sin=sin[:0])]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):  # the malformed table of the existing tests
        um.varlen_kvcache_attention(q, kc, vc, cu, 35, sl, block_table=bt, rotary_cos=torch.zeros(1))
    f8 = torch.float8_e4m3fn
    with pytest.raises(ValueError):  # fp8 caches stay with kvcache_attention
        um.varlen_kvcache_attention(q, kc.to(f8), vc.to(f8), cu, 35, sl, block_table=bt, k=kn, v=vn, rotary_cos=cos, rotary_sin=sin)
    o = um.varlen_kvcache_attention(q.clone().requires_grad_(True), kc.clone(), vc.clone(), cu, 35, sl, block_table=bt, k=kn, v=vn,
                                    rotary_cos=cos, rotary_sin=sin)
    with pytest.raises(RuntimeError):
        o.float().sum().backward()
