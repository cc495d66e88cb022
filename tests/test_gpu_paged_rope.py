"""Rotary embedding fused into kvcache_attention on the GPU: the rotated cache rows, O and LSE against the fp64
reference (tests/paged_rope_ref.py) under the format bounds; O, LSE and both pools bit for bit against the parent sequence (operands
rotated by ops.rope_rotate, then the existing entry); the device-side rules (the table's last row, out-of-range lengths and table
entries, overflow, guard pages, guard bands around O and LSE, untouched inputs); graph replay with advancing lengths and the capture rule; the custom ops under
opcheck / torch.compile; the refusals."""
import numpy as np
import pytest
import torch

import paged_fp8_ref as f8ref
import paged_ref
import paged_rope_ref as rr
import tolerances as tol
from paged_rope_gpu import DT, bits, check_rotated_rows, fp32_slack, i32, np64, rotate_by_ops, tables

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
GUARD = 2  # pages at each end of a pool that no table names: they must come back unchanged
B, H, HKV, PS, MAXP = 3, 8, 2, 16, 4  # capacity 64
RO = 72  # table rows: past every position the grid reaches


def _umfa():
    import umfa_torch
    return umfa_torch


def _inputs(dt, D, Sq, Sn, seed, cache="paged", fp8=False, B=B):
    """q, k_cache, v_cache, block table (None: static), k_new, v_new"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device="cuda", dtype=DT[dt], generator=g)  # noqa: E731
    q, kn, vn = rnd(B, Sq, H, D), rnd(B, Sn, HKV, D), rnd(B, Sn, HKV, D)
    if cache == "paged":
        shape, bt = (B * MAXP + 2 * GUARD, PS, HKV, D), np.random.default_rng(seed).permutation(B * MAXP).reshape(B, MAXP) + GUARD
    else:
        shape, bt = ((B, PS * MAXP, HKV, D) if cache == "bshd" else (B, HKV, PS * MAXP, D)), None
    if fp8:
        kc, vc = ((torch.randn(shape, device="cuda", generator=g) * 4).clamp(-448, 448).to(F8) for _ in range(2))
    else:
        kc, vc = rnd(*shape), rnd(*shape)
    if cache == "bhsd":  # HF's [B, H_kv, S_max, D], handed over as its [B, S_max, H_kv, D] view
        kc, vc = kc.transpose(1, 2), vc.transpose(1, 2)
    return q, kc, vc, None if bt is None else i32(bt), kn, vn


def _descales(seed):
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.7, 1.4, (B, HKV))
    e = np.where((np.arange(HKV)[None, :] + np.arange(B)[:, None]) % 2 == 0, 2.0 ** -3, 2.0 ** 3)
    dev = lambda a: torch.tensor(a.astype(np.float32), device="cuda")  # noqa: E731
    return dev(base * e), dev(base[::-1, ::-1] / e)


def _fused(um, q, kc, vc, kn, vn, sl, bt, cos, sin, inter, causal, splits=0, kd=None, vd=None):
    kc, vc = kc.clone(), vc.clone()
    o, lse = um.kvcache_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt, causal=causal, num_splits=splits,
                                  return_softmax_lse=True, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=inter, k_descale=kd,
                                  v_descale=vd)
    torch.cuda.synchronize()
    return o, lse, kc, vc, um.last_kernel()


def _sequence(um, q, kc, vc, kn, vn, sl, bt, cos, sin, inter, causal, splits=0, kd=None, vd=None):
    """the parent commit's sequence: rope_rotate(q), rope_rotate(k), the existing entry"""
    cap = kc.shape[1] * (bt.shape[1] if bt is not None else 1)
    s = sl.cpu().numpy()
    rq = rotate_by_ops(um, q, rr.positions(s, q.shape[1], cap, causal), cos, sin, inter)
    rk = rotate_by_ops(um, kn, rr.positions(s, kn.shape[1], cap, True), cos, sin, inter)
    kc, vc = kc.clone(), vc.clone()
    o, lse = um.kvcache_attention(rq, kc, vc, rk, vn, cache_seqlens=sl, block_table=bt, causal=causal, num_splits=splits,
                                  return_softmax_lse=True, k_descale=kd, v_descale=vd)
    torch.cuda.synchronize()
    return o, lse, kc, vc, um.last_kernel()


def _appended(kc_before, kc_after):
    """mask [.., D] of the cache rows the call wrote (random inputs: a written row differs from what was there)"""
    return (bits(kc_before) != bits(kc_after)).reshape(*kc_before.shape[:3], -1).any(-1)


def _check_values(dt, q, kc0, vc0, kn, vn, sl, bt, cos, sin, inter, causal, got, kd=None, vd=None, tag=""):
    """1. values against fp64: the rotated cache rows under the format bound (fp8: the reference quantiser's byte, a neighbour only at
    a 16-bit rounding tie), then O and LSE against the reference run on its own rounded rotated operands"""
    o, lse, kc1, vc1, kernel = got
    rd = 2 * cos.shape[1]
    s, btn = sl.cpu().numpy(), None if bt is None else bt.cpu().numpy()
    fp8 = kd is not None
    rq, rk = rr.operands(np64(q), np64(kn), kc0, s, np64(cos), np64(sin), btn, causal, inter)
    if fp8:
        ref = rr.forward_fp8(np64(q), bits(kc0), bits(vc0), s, kd.cpu().numpy(), vd.cpu().numpy(), np64(cos), np64(sin), btn, np64(kn),
                             np64(vn), causal, None, inter, dt)
        kdn = kd.cpu().numpy().astype(np.float32)[:, None, :, None]
        lo = np.floor(rk / rr.ulp(rk, dt)) * rr.ulp(rk, dt)  # the two 16-bit neighbours of the exact rotation
        hi = lo + rr.ulp(rk, dt)
        tie = np.abs(rk - (lo + hi) / 2) <= fp32_slack(np64(kn), rd, inter, dt)
        near = (f8ref.quantise(lo, kdn), f8ref.quantise(hi, kdn))
        want = f8ref.quantise(rr.round_operand(rk, dt), kdn)
        # the bytes the call stored, row by row through the reference's own append of distinguishable markers
        idx = np.arange(rk.size, dtype=np.float64).reshape(rk.shape)
        where, _ = paged_ref.append(np.full(kc0.shape, -1.0), np.full(kc0.shape, -1.0), idx, idx, s, btn)
        sel = where >= 0
        src = where[sel].astype(np.int64)
        gotb = bits(kc1).reshape(kc0.shape)[sel]
        exact = gotb == want.ravel()[src]
        share = float(tie.ravel()[src].mean()) if src.size else 0.0
        print(f"{tag}: fp8 bytes off the reference quantiser {int((~exact).sum())} of {src.size}; tie-sensitive share {share:.5f}")
        assert share < 0.01
        assert (exact | (tie.ravel()[src] & ((gotb == near[0].ravel()[src]) | (gotb == near[1].ravel()[src])))).all()
        assert (bits(vc1) == ref[3]).all()  # V: the existing quantiser, unrotated
        assert (bits(kc1).reshape(kc0.shape)[~sel] == bits(kc0).reshape(kc0.shape)[~sel]).all()
    else:
        ref = rr.forward(np64(q), np64(kc0), np64(vc0), s, np64(cos), np64(sin), btn, np64(kn), np64(vn), causal, None, inter, dt)
        exact, _ = paged_ref.append(np64(kc0), np64(vc0), rk, np64(vn), s, btn)  # the pool with the UNROUNDED rotation appended
        srcm, _ = paged_ref.append(np.zeros(kc0.shape), np.zeros(kc0.shape), np64(kn), np64(vn), s, btn)
        wrote = _appended(kc0, kc1)
        k1 = np64(kc1)
        check_rotated_rows(k1[wrote], exact[wrote], srcm[wrote], rd, inter, dt, tag)
        assert (k1[wrote][..., rd:] == srcm[wrote][..., rd:]).all()  # the pass-through tail is a copy
        assert (k1[~wrote] == np64(kc0)[~wrote]).all()
        assert (np64(vc1) == ref[3]).all()  # V: appended unrotated, bit for bit
    o_ref, lse_ref = ref[0], ref[1]
    o_, l_ = np64(o), np64(lse)
    live = np.isfinite(lse_ref)
    live_o = live.transpose(0, 2, 1)
    assert np.isfinite(o_).all() and (o_[~live_o] == 0).all() and np.isneginf(l_[~live]).all()
    if not live.any():
        return
    print(f"{tag}: {kernel} lse max err {float(np.abs(l_[live] - lse_ref[live]).max()):.3e}")
    np.testing.assert_allclose(l_[live], lse_ref[live], rtol=0, atol=2e-3)
    for b in range(o_.shape[0]):  # (check_forward normalises by max |O|: one (batch, KV head) group at a time)
        for hk in range(HKV):
            hs = slice(hk * (H // HKV), (hk + 1) * (H // HKV))
            m = live_o[b, :, hs]
            if m.any():
                tol.check_forward(o_[b, :, hs][m][None, None], o_ref[b, :, hs][m][None, None], DT[dt], kernel, tag="paged_rope", out_dt=DT[dt])


def _check_bits(a, b):
    """2. bits against the sequence: O, LSE and both pools"""
    assert a[4] == b[4], (a[4], b[4])  # the unchanged attention kernel
    for x, y, name in zip(a[:4], b[:4], ("O", "LSE", "k_cache", "v_cache")):
        assert (bits(x) == bits(y)).all(), (name, int((bits(x) != bits(y)).sum()))


# (dtype, head_dim, rotary_dim, interleaved, causal, fp32 tables, shape, num_splits)
#   decode: Sq = S_new = 1 at lengths [0, 14, 47] (the empty cache, just under a page boundary, a third page); chunk: Sq = S_new = 4 from
#   14 (the append crosses a page); q2k5: Sq 2 with S_new 5; bshd / bhsd: the static cache in both layouts; fp8: an fp8 cache
GRID = [("bf16", 128, 128, False, True, True, "decode", 0), ("fp16", 64, 64, True, True, False, "decode", 0),
        ("bf16", 64, 32, True, False, True, "chunk", 0), ("fp16", 128, 16, False, True, False, "chunk", 0),
        ("bf16", 128, 32, False, False, False, "q2k5", 0), ("fp16", 128, 128, True, True, True, "q2k5", 0),
        ("bf16", 128, 128, True, True, True, "bshd", 0), ("fp16", 64, 16, False, False, True, "bhsd", 0),
        ("bf16", 128, 64, False, True, True, "decode", 2), ("bf16", 64, 64, False, True, False, "chunk", 2),
        ("bf16", 128, 128, False, True, True, "fp8", 0), ("fp16", 64, 32, True, False, False, "fp8", 2)]
SHAPES = {"decode": (1, 1, [0, 14, 47]), "chunk": (4, 4, [14, 14, 30]), "q2k5": (2, 5, [0, 14, 47]), "bshd": (4, 4, [14, 0, 47]),
          "bhsd": (1, 1, [0, 14, 47]), "fp8": (4, 4, [14, 0, 47])}


@pytest.mark.parametrize("dt,D,rd,inter,causal,f32,shape,splits", GRID)
def test_values_then_bits(dt, D, rd, inter, causal, f32, shape, splits):
    um = _umfa()
    Sq, Sn, lens = SHAPES[shape]
    seed = 100 + GRID.index((dt, D, rd, inter, causal, f32, shape, splits))
    fp8 = shape == "fp8"
    q, kc, vc, bt, kn, vn = _inputs(dt, D, Sq, Sn, seed, cache=shape if shape in ("bshd", "bhsd") else "paged", fp8=fp8)
    kd, vd = _descales(seed) if fp8 else (None, None)
    cos, sin = tables(RO, rd, torch.float32 if f32 else DT[dt], seed, pad=8 if shape == "chunk" else 0)
    sl = i32(lens)
    args = (q, kc, vc, kn, vn, sl, bt, cos, sin, inter, causal, splits, kd, vd)
    got = _fused(um, *args)
    assert got[4].startswith("fa_fwd16_paged_fp8<" if fp8 else "fa_fwd16_paged<") and ("split" in got[4]) == (splits > 1), got[4]
    _check_values(dt, q, kc, vc, kn, vn, sl, bt, cos, sin, inter, causal, got, kd, vd, tag=f"{dt}-{D}-{rd}-{shape}")
    _check_bits(got, _sequence(um, *args))


@pytest.mark.parametrize("inter", [False, True])
def test_device_side_rules(inter):
    """the last table row exactly and one past it (the clamped row), lengths -5 and 1e9, table entries -1 and num_pages on the append's
    page (rows dropped, the rest of the pool bit-identical), an append that overflows the capacity, guard pages, untouched inputs"""
    um = _umfa()
    dt, D, rd, Sq, Sn = "bf16", 128, 64, 2, 2
    ro = 40
    q, kc, vc, bt, kn, vn = _inputs(dt, D, Sq, Sn, 31, B=7)
    #      last row = ro - 1 | one past | negative | huge | page entry -1 | page entry num_pages | overflows the capacity (63 + 2 > 64)
    sl = i32([ro - Sn, ro - Sn + 1, -5, 10 ** 9, 16, 30, 63])
    btn = bt.cpu().numpy()
    btn[4, 1] = -1
    btn[5, 1] = kc.shape[0]  # position 30, 31 lie on logical page 1; 32 would lie on page 2
    bt = i32(btn)
    cos, sin = tables(ro, rd, torch.float32, 32)
    keep = [t.clone() for t in (q, kn, vn, cos, sin, sl, bt)]
    for causal in (True, False):
        args = (q, kc, vc, kn, vn, sl, bt, cos, sin, inter, causal)
        got = _fused(um, *args)
        ref = rr.forward(np64(q), np64(kc), np64(vc), sl.cpu().numpy(), np64(cos), np64(sin), btn, np64(kn), np64(vn), causal, None, inter, dt)
        wrote = _appended(kc, got[2])
        want_wrote = (ref[2] != np64(kc)).any(-1)
        assert (wrote == want_wrote).all()  # dropped rows are dropped, nothing else is written (guard pages included)
        assert not wrote[:GUARD].any() and not wrote[-GUARD:].any()
        _check_values(dt, q, kc, vc, kn, vn, sl, bt, cos, sin, inter, causal, got, tag=f"rules-{inter}-{causal}")
        _check_bits(got, _sequence(um, *args))
    for t, k in zip((q, kn, vn, cos, sin, sl, bt), keep):
        assert torch.equal(t, k)
    # sequence 1's second new key sits one past the table and takes its last row: the same bits as the key rotated at ro - 1
    k_at = rotate_by_ops(um, kn, np.full((7, Sn), ro - 1), cos, sin, inter)
    pos = ro - Sn + 1 + 1
    assert torch.equal(got[2][btn[1, pos // PS], pos % PS], k_at[1, 1])


@pytest.mark.parametrize("shape,splits", [("decode", 0), ("chunk", 2), ("fp8", 0)])
def test_output_guard_bands_come_back_bit_identical(shape, splits):
    """O and LSE written into the middle of sentinel-filled buffers (the ops entry takes the caller's buffers): the bands on both sides
    keep every bit and the rows in between are the public call's.  The q image itself lives in the library's pooled workspace, which no
    caller can see, so no sentinel can be placed beside it: its only neighbour there is the block of split partials, which the attention
    launch rewrites before it reads them, so this test does NOT catch a pre-pass that wrote past the image.  What is checked of the
    image is its own rows, through O, in every case of this file."""
    um = _umfa()
    dt, D, G = "bf16", 128, 64
    Sq, Sn, lens = SHAPES[shape]
    fp8 = shape == "fp8"
    q, kc, vc, bt, kn, vn = _inputs(dt, D, Sq, Sn, 81, fp8=fp8)
    kd, vd = _descales(82) if fp8 else (None, None)
    cos, sin = tables(RO, 64, torch.float32, 83)
    sl = i32(lens)
    want = _fused(um, q, kc, vc, kn, vn, sl, bt, cos, sin, False, True, splits, kd, vd)
    bo = torch.full((B * Sq * H * D + 2 * G,), -7.5, dtype=DT[dt], device="cuda")
    bl = torch.full((B * H * Sq + 2 * G,), -7.5, dtype=torch.float32, device="cuda")
    kc2, vc2 = kc.clone(), vc.clone()
    o, lse = um.ops.kvcache_attention_rope_forward(q, kc2, vc2, sl, cos, sin, bt, kn, vn, scale=D ** -0.5, causal=True, num_splits=splits,
                                                   k_descale=kd, v_descale=vd, out=bo[G:-G].view(B, Sq, H, D), lse=bl[G:-G].view(B, H, Sq))
    torch.cuda.synchronize()
    assert o.data_ptr() == bo[G:].data_ptr() and lse.data_ptr() == bl[G:].data_ptr()
    for b in (bo, bl):
        assert (b[:G] == -7.5).all() and (b[-G:] == -7.5).all()
    assert torch.equal(o, want[0]) and torch.equal(lse, want[1])
    assert (bits(kc2) == bits(want[2])).all() and (bits(vc2) == bits(want[3])).all()
    with pytest.raises(ValueError):  # a buffer of another shape is refused, not written
        um.ops.kvcache_attention_rope_forward(q, kc2, vc2, sl, cos, sin, bt, kn, vn, scale=D ** -0.5, k_descale=kd, v_descale=vd,
                                              out=bo[G:-G].view(B * Sq, H, D))


def test_graph_replay_follows_the_lengths_and_capture_needs_a_warm_up():
    um = _umfa()
    dt, D, rd = "bf16", 128, 128
    q, kc, vc, bt, kn, vn = _inputs(dt, D, 1, 1, 41)
    cos, sin = tables(RO, rd, torch.float32, 42)
    sl = i32([0, 14, 47])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def step():
        return um.kvcache_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt, causal=True, num_splits=2, return_softmax_lse=True,
                                    rotary_cos=cos, rotary_sin=sin)

    # a capture on a stream whose pool would have to grow: the allocation error, and nothing launched
    kc0, vc0 = kc.clone(), vc.clone()
    cold = torch.cuda.Stream()
    cold.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    um.release_scratch(stream=cold)  # (torch hands out pooled streams: an earlier test may have warmed this one)
    mark = torch.zeros(4, device="cuda")
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0, stream=cold):
        mark.add_(1.0)  # (the graph holds one node of torch's, so that it can be replayed)
        with pytest.raises(um.ops.MFAError) as e:
            step()
    assert e.value.code == 2, e.value.code  # MFA_ERROR_MEMORY_ALLOCATION
    g0.replay()
    torch.cuda.synchronize()
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up: the pool grows outside the capture
            step()
    torch.cuda.current_stream().wait_stream(s)
    kc.copy_(kc0)
    vc.copy_(vc0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        res = step()
    kc.copy_(kc0)
    vc.copy_(vc0)
    g = torch.Generator(device="cuda").manual_seed(43)
    for it in range(3):
        for t in (q, kn, vn):
            t.copy_(torch.randn(t.shape, device="cuda", dtype=t.dtype, generator=g))
        before = (kc.clone(), vc.clone())
        graph.replay()
        torch.cuda.synchronize()
        got = (res[0].clone(), res[1].clone(), kc.clone(), vc.clone(), um.last_kernel())
        _check_values(dt, q, before[0], before[1], kn, vn, sl, bt, cos, sin, False, True, got, tag=f"replay {it}")
        _check_bits(got, _fused(um, q, before[0], before[1], kn, vn, sl, bt, cos, sin, False, True, 2))
        sl.add_(1)  # the decode loop advances the lengths on the device


def test_opcheck_custom_ops():
    _umfa()
    q, kc, vc, bt, kn, vn = _inputs("bf16", 64, 2, 2, 51)
    cos, sin = tables(RO, 32, torch.float32, 52)
    sl = i32([5, 33, 14])
    torch.library.opcheck(torch.ops.umfa.kvcache_rope_forward_append.default, (q, kc, vc, kn, vn, sl, cos, sin, False, bt, True, 0.125, 2))
    q, k8, v8, bt, kn, vn = _inputs("fp16", 64, 2, 2, 53, fp8=True)
    kd, vd = _descales(54)
    cos, sin = tables(RO, 64, torch.float16, 55)
    torch.library.opcheck(torch.ops.umfa.kvcache_fp8_rope_forward_append.default,
                          (q, k8.view(torch.uint8), v8.view(torch.uint8), kn, vn, sl, kd, vd, cos, sin, True, bt, True, 0.125, 0))


def test_compile_fullgraph_single_node():
    um = _umfa()
    q, kc, vc, bt, kn, vn = _inputs("fp16", 128, 1, 1, 61)
    cos, sin = tables(RO, 128, torch.float32, 62)
    sl = i32([30, 47, 0])
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    def f(q, kc, vc, kn, vn):
        return um.kvcache_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt, causal=True, rotary_cos=cos, rotary_sin=sin,
                                    rotary_interleaved=True)

    kc_e, vc_e = kc.clone(), vc.clone()
    torch._dynamo.reset()
    oc = torch.compile(f, fullgraph=True, backend=backend)(q, kc, vc, kn, vn)
    oe = f(q, kc_e, vc_e, kn, vn)
    torch.cuda.synchronize()
    assert len(graphs) == 1
    calls = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function" and "umfa" in str(n.target)]
    assert calls == ["umfa.kvcache_rope_forward_append"], calls
    assert torch.equal(oc, oe) and torch.equal(kc, kc_e) and torch.equal(vc, vc_e)
    assert um.last_kernel().startswith("fa_fwd16_paged<fp16,128,causal"), um.last_kernel()


def test_refusals_and_no_backward():
    um = _umfa()
    q, kc, vc, bt, kn, vn = _inputs("bf16", 128, 1, 1, 71)
    cos, sin = tables(RO, 64, torch.float32, 72)
    sl = i32([3, 14, 47])
    call = lambda **kw: um.kvcache_attention(q, kc.clone(), vc.clone(), kw.pop("k", kn), kw.pop("v", vn), cache_seqlens=sl, block_table=bt,  # noqa: E731
                                             causal=True, **kw)
    assert call(rotary_cos=cos, rotary_sin=sin).shape == q.shape
    assert call(rotary_interleaved=True).shape == q.shape  # without tables the flag means nothing, as before
    wide = torch.zeros(RO, 40, device="cuda")
    bad = [dict(rotary_cos=cos), dict(rotary_sin=sin),  # only one of the two
           dict(rotary_cos=cos, rotary_sin=sin, k=None, v=None),  # no new tokens
           dict(rotary_cos=cos, rotary_sin=sin, k=kn[:, :0], v=vn[:, :0]),  # empty new tokens
           dict(rotary_cos=cos.cpu(), rotary_sin=sin.cpu()), dict(rotary_cos=cos[0], rotary_sin=sin[0]),  # not 2-D device tensors
           dict(rotary_cos=cos[None], rotary_sin=sin[None]),
           dict(rotary_cos=cos, rotary_sin=sin[:, :16]), dict(rotary_cos=cos, rotary_sin=sin.bfloat16()),  # shape / dtype differ
           dict(rotary_cos=cos.half(), rotary_sin=sin.half()), dict(rotary_cos=cos.double(), rotary_sin=sin.double()),  # neither fp32 nor q's
           dict(rotary_cos=cos.t().contiguous().t(), rotary_sin=sin.t().contiguous().t()),  # column stride != 1
           dict(rotary_cos=wide[:, 1:33], rotary_sin=wide[:, 1:33]),  # rows not 16-byte aligned
           dict(rotary_cos=wide[:, :4], rotary_sin=wide[:, :4]),  # rotary_dim 8
           dict(rotary_cos=wide[:, :12], rotary_sin=wide[:, :12]),  # rotary_dim 24: not a multiple of 16
           dict(rotary_cos=torch.zeros(RO, 72, device="cuda"), rotary_sin=torch.zeros(RO, 72, device="cuda")),  # rotary_dim 144 > D
           dict(rotary_cos=cos[:0], rotary_sin=sin[:0])]  # seqlen_ro = 0
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):  # the malformed table of the existing tests
        um.kvcache_attention(q, kc, vc, cache_seqlens=10, block_table=bt, rotary_cos=torch.zeros(1))
    with pytest.raises(um.ops.MFAError):  # the C entry refuses what it cannot run: there is no fall-back
        um.ops.kvcache_attention_rope_forward(q, kc.clone(), vc.clone(), sl, wide[:, :12], wide[:, :12], bt, kn, vn, scale=0.1)
    qg = q.clone().requires_grad_(True)
    o = um.kvcache_attention(qg, kc.clone(), vc.clone(), kn, vn, cache_seqlens=sl, block_table=bt, causal=True, rotary_cos=cos, rotary_sin=sin)
    with pytest.raises(RuntimeError):
        o.float().sum().backward()
    q8, k8, v8, bt8, kn8, vn8 = _inputs("bf16", 128, 1, 1, 73, fp8=True)
    o = um.kvcache_attention(q8.clone().requires_grad_(True), k8, v8, kn8, vn8, cache_seqlens=sl, block_table=bt8, rotary_cos=cos,
                             rotary_sin=sin, k_descale=0.5, v_descale=2.0)
    with pytest.raises(RuntimeError):
        o.float().sum().backward()
