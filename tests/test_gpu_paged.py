"""KV-cache attention on the GPU (umfa_torch.kvcache_attention): values against the fp64 reference
(tests/paged_ref.py) under the format bounds of tests/tolerances.py for paged and static caches, the in-place append (bitwise, nothing
else in the pool touched), out-of-range table entries and lengths, rows that see no key, forced split-KV parts, bf16 V far from fp16's
range, agreement with the gather + dense route, graph replay with advancing lengths and a rewritten table, opcheck / torch.compile and
the refused arguments."""
import numpy as np
import pytest
import torch

import paged_ref as ref
import tolerances as tol

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
GUARD = 2  # pages at each end of a pool that no table names: they must come back unchanged


def _umfa():
    import umfa_torch
    return umfa_torch


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _bits(t):
    return t.detach().cpu().view(torch.int16).numpy()


def _paged(B, Sq, H, Hkv, D, ps, max_pages, dt, seed, S_new=0, share=True):
    """q, k_cache, v_cache (GUARD free pages at each end), a randomly permuted block table (sequence 1 shares sequence 0's first page
    when `share`), k_new / v_new"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    num_pages = B * max_pages + 2 * GUARD
    q = torch.randn(B, Sq, H, D, device="cuda", dtype=dt, generator=g)
    kc = torch.randn(num_pages, ps, Hkv, D, device="cuda", dtype=dt, generator=g)
    vc = torch.randn(num_pages, ps, Hkv, D, device="cuda", dtype=dt, generator=g)
    perm = np.random.default_rng(seed).permutation(B * max_pages) + GUARD
    bt = perm.reshape(B, max_pages).astype(np.int32)
    if share and B > 1:
        bt[1, 0] = bt[0, 0]
    kn = torch.randn(B, S_new, Hkv, D, device="cuda", dtype=dt, generator=g) if S_new else None
    vn = torch.randn(B, S_new, Hkv, D, device="cuda", dtype=dt, generator=g) if S_new else None
    return q, kc, vc, torch.tensor(bt, device="cuda"), kn, vn


def _seqlens(vals):
    return torch.tensor(vals, dtype=torch.int32, device="cuda")


def _run(q, kc, vc, sl, bt, kn=None, vn=None, causal=False, num_splits=0, scale=None, out_dtype=torch.float32):
    um = _umfa()
    sc = q.shape[-1] ** -0.5 if scale is None else scale
    o, lse = um.ops.kvcache_attention_forward(q, kc, vc, sl, bt, kn, vn, scale=sc, causal=causal, num_splits=num_splits,
                                              out_dtype=out_dtype)
    torch.cuda.synchronize()
    return o, lse, um.last_kernel()


def _check(q, kc0, vc0, sl, bt, o, lse, kernel, kn=None, vn=None, causal=False, scale=None, dt="bf16", out_dt=None):
    """values and LSE against the fp64 reference (run on the caches as they were before the call)"""
    o_ref, lse_ref, _, _ = ref.forward(_np(q), _np(kc0), _np(vc0), sl.cpu().numpy(), None if bt is None else bt.cpu().numpy(),
                                       None if kn is None else _np(kn), None if vn is None else _np(vn), causal, scale)
    o_, l_ = _np(o), _np(lse)
    assert np.isfinite(o_).all()
    live = np.isfinite(lse_ref)  # [B, H, Sq]
    live_o = live.transpose(0, 2, 1)  # [B, Sq, H]
    assert (o_[~live_o] == 0).all() and np.isneginf(l_[~live]).all()
    if not live.any():
        return
    np.testing.assert_allclose(l_[live], lse_ref[live], rtol=0, atol=2e-3)
    got = o_[live_o][None, None]
    want = o_ref[live_o][None, None]
    tol.check_forward(got, want, DT[dt], kernel, tag="paged", out_dt=out_dt)


# (page_size, g, Sq, causal, dtype, head_dim)
CASES = [(16, 1, 1, False, "bf16", 128), (16, 4, 1, True, "fp16", 128), (16, 8, 4, True, "bf16", 64), (32, 4, 16, False, "bf16", 128),
         (32, 8, 1, False, "fp16", 64), (64, 1, 200, True, "bf16", 128), (64, 4, 4, True, "bf16", 128), (64, 8, 16, True, "fp16", 128),
         (256, 4, 1, False, "bf16", 128), (256, 1, 16, True, "fp16", 64), (256, 8, 200, False, "bf16", 64), (16, 4, 200, True, "bf16", 128)]


@pytest.mark.parametrize("ps,g,Sq,causal,dt,D", CASES)
def test_paged_values(ps, g, Sq, causal, dt, D):
    Hkv, max_pages = 2, max(2, 640 // ps)
    cap = ps * max_pages
    q, kc, vc, bt, _, _ = _paged(4, Sq, g * Hkv, Hkv, D, ps, max_pages, DT[dt], seed=ps + g + Sq)
    sl = _seqlens([0, 1, ps + 5, cap])  # empty, one key, not a page multiple, exactly at capacity
    o, lse, kernel = _run(q, kc, vc, sl, bt, causal=causal)
    _check(q, kc, vc, sl, bt, o, lse, kernel, causal=causal, dt=dt)


# the unsplit kernel with more than 32 rows per (batch, KV head): each wave owns 32 rows of one or more 128-row blocks (chunked prefill
# with many sequences takes it: the work items fill the CUs and the automatic count is 1)
@pytest.mark.parametrize("ps,g,Sq,dt,D", [(16, 8, 16, "bf16", 128), (64, 1, 200, "fp16", 128), (32, 4, 200, "bf16", 64)])
@pytest.mark.parametrize("causal", [False, True])
def test_unsplit_many_rows(ps, g, Sq, dt, D, causal):
    Hkv, max_pages = 2, 640 // ps
    q, kc, vc, bt, _, _ = _paged(4, Sq, g * Hkv, Hkv, D, ps, max_pages, DT[dt], seed=ps + g + Sq + 1)
    sl = _seqlens([0, 150, ps + 5, 640])
    for out_dtype in (torch.float32, DT[dt]):
        o, lse, kernel = _run(q, kc, vc, sl, bt, causal=causal, num_splits=1, out_dtype=out_dtype)
        assert "split" not in kernel, kernel
        _check(q, kc, vc, sl, bt, o, lse, kernel, causal=causal, dt=dt, out_dt=None if out_dtype == torch.float32 else out_dtype)


@pytest.mark.parametrize("layout", ["bshd", "bhsd"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_static_cache_values(layout, dt):
    B, Smax, H, Hkv, D = 3, 300, 8, 2, 128
    g = torch.Generator(device="cuda").manual_seed(7)
    q = torch.randn(B, 4, H, D, device="cuda", dtype=DT[dt], generator=g)
    if layout == "bshd":
        kc = torch.randn(B, Smax, Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        vc = torch.randn(B, Smax, Hkv, D, device="cuda", dtype=DT[dt], generator=g)
    else:  # HF StaticCache: [B, H_kv, S_max, D], handed over as its [B, S_max, H_kv, D] view
        kc = torch.randn(B, Hkv, Smax, D, device="cuda", dtype=DT[dt], generator=g).transpose(1, 2)
        vc = torch.randn(B, Hkv, Smax, D, device="cuda", dtype=DT[dt], generator=g).transpose(1, 2)
    sl = _seqlens([17, 300, 129])
    for causal in (False, True):
        o, lse, kernel = _run(q, kc, vc, sl, None, causal=causal)
        _check(q, kc, vc, sl, None, o, lse, kernel, causal=causal, dt=dt)


def test_public_entry_output_dtype_and_lse():
    um = _umfa()
    q, kc, vc, bt, _, _ = _paged(2, 3, 8, 2, 128, 64, 4, torch.bfloat16, seed=3)
    sl = _seqlens([100, 7])
    o, lse = um.kvcache_attention(q, kc, vc, cache_seqlens=sl, block_table=bt, causal=True, return_softmax_lse=True)
    torch.cuda.synchronize()
    assert o.dtype == torch.bfloat16 and o.shape == q.shape and lse.shape == (2, 8, 3)
    _check(q, kc, vc, sl, bt, o, lse, um.last_kernel(), causal=True, out_dt=torch.bfloat16)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("static", [False, "bshd", "bhsd"])
def test_append_writes_rows_bitwise_and_nothing_else(dt, static):
    B, Hkv, D, S_new = 3, 2, 64, 5
    if static:
        g = torch.Generator(device="cuda").manual_seed(11)
        q = torch.randn(B, 5, 8, D, device="cuda", dtype=DT[dt], generator=g)
        if static == "bshd":
            kc = torch.randn(B, 40, Hkv, D, device="cuda", dtype=DT[dt], generator=g)
            vc = torch.randn(B, 40, Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        else:  # HF StaticCache [B, H_kv, S_max, D], appended through its [B, S_max, H_kv, D] view
            kc = torch.randn(B, Hkv, 40, D, device="cuda", dtype=DT[dt], generator=g).transpose(1, 2)
            vc = torch.randn(B, Hkv, 40, D, device="cuda", dtype=DT[dt], generator=g).transpose(1, 2)
        kn = torch.randn(B, S_new, Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        vn = torch.randn(B, S_new, Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        bt = None
        sl = _seqlens([0, 14, 37])  # the last one runs past S_max = 40: two rows dropped
    else:
        q, kc, vc, bt, kn, vn = _paged(B, 5, 8, Hkv, D, 16, 3, DT[dt], seed=12, S_new=S_new, share=False)
        sl = _seqlens([0, 14, 46])  # page crossing; the last one past the capacity of 48
    kc0, vc0 = kc.clone(), vc.clone()
    base_k = kc.transpose(1, 2) if static == "bhsd" else kc  # (the storage as allocated: every byte of it is compared)
    o, lse, kernel = _run(q, kc, vc, sl, bt, kn, vn, causal=True)
    if static == "bhsd":
        assert base_k.is_contiguous() and base_k.data_ptr() == kc.data_ptr()
    btn = None if bt is None else bt.cpu().numpy()
    kw, vw = ref.append(_bits(kc0), _bits(vc0), _bits(kn), _bits(vn), sl.cpu().numpy(), btn)
    assert (_bits(kc) == kw).all() and (_bits(vc) == vw).all()  # the rows written, bitwise, and every other byte unchanged
    assert not (kw == _bits(kc0)).all()
    if not static:
        assert (_bits(kc)[:GUARD] == _bits(kc0)[:GUARD]).all() and (_bits(kc)[-GUARD:] == _bits(kc0)[-GUARD:]).all()
    _check(q, kc0, vc0, sl, bt, o, lse, kernel, kn, vn, causal=True, dt=dt)
    assert (sl.cpu().numpy() == ([0, 14, 37] if static else [0, 14, 46])).all()  # cache_seqlens is not advanced


def test_strided_cache_seqlens_and_tables_are_refused():
    um = _umfa()
    q, kc, vc, bt, kn, vn = _paged(3, 1, 8, 2, 128, 16, 4, torch.bfloat16, seed=22, S_new=1, share=False)
    kc0 = kc.clone()
    one = torch.tensor([20], dtype=torch.int32, device="cuda")
    lens = torch.tensor([[20, 1], [30, 2], [40, 3]], dtype=torch.int32, device="cuda")
    for sl in (one.expand(3), lens[:, 0]):  # stride 0, stride 2: the kernels would read the wrong lengths
        with pytest.raises(ValueError, match="cache_seqlens"):
            um.kvcache_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt)
        with pytest.raises(ValueError):
            um.ops.kvcache_attention_forward(q, kc, vc, sl, bt, kn, vn, scale=0.1)
    with pytest.raises(ValueError, match="block_table"):  # rows that overlap
        um.kvcache_attention(q, kc, vc, cache_seqlens=10, block_table=bt[:1].expand(3, 4))
    torch.cuda.synchronize()
    assert torch.equal(kc, kc0)  # nothing was appended
    o = um.kvcache_attention(q, kc, vc, kn, vn, cache_seqlens=lens[:, 0].contiguous(), block_table=bt)
    o2 = um.kvcache_attention(q, kc0, vc.clone(), kn, vn, cache_seqlens=torch.tensor([20, 30, 40], dtype=torch.int32, device="cuda"),
                              block_table=bt)
    torch.cuda.synchronize()
    assert torch.equal(o, o2)


def test_rows_without_keys_are_exact_zeros():
    q, kc, vc, bt, _, _ = _paged(3, 8, 8, 2, 128, 16, 4, torch.bfloat16, seed=13)
    sl = _seqlens([0, 3, 40])  # no key at all; causal with L_k = 3 < Sq = 8
    o, lse, kernel = _run(q, kc, vc, sl, bt, causal=True)
    assert (o[0] == 0).all() and torch.isneginf(lse[0]).all()
    assert (o[1, :5] == 0).all() and torch.isneginf(lse[1, :, :5]).all()
    _check(q, kc, vc, sl, bt, o, lse, kernel, causal=True)


@pytest.mark.parametrize("num_splits", [0, 3])
def test_out_of_range_entries_and_lengths(num_splits):
    B, Hkv, D = 4, 2, 128
    q, kc, vc, bt, kn, vn = _paged(B, 2, 8, Hkv, D, 16, 4, torch.bfloat16, seed=14, S_new=3, share=False)
    btn = bt.cpu().numpy()
    num_pages = kc.shape[0]
    btn[0, :] = -1                                  # no page the pool holds
    btn[1, 1], btn[1, 3] = num_pages, 2 ** 31 - 1   # one past the pool, far past it
    btn[2, 2] = -(2 ** 31)
    bt = torch.tensor(btn, device="cuda")
    sl = _seqlens([20, 30, -7, 10 ** 9])            # a negative and a huge length: clamped into [0, 64]
    kc0, vc0 = kc.clone(), vc.clone()
    o, lse, kernel = _run(q, kc, vc, sl, bt, kn, vn, causal=False, num_splits=num_splits)
    kw, vw = ref.append(_bits(kc0), _bits(vc0), _bits(kn), _bits(vn), sl.cpu().numpy(), btn)
    assert (_bits(kc) == kw).all() and (_bits(vc) == vw).all()
    assert (o[0] == 0).all() and torch.isneginf(lse[0]).all()
    _check(q, kc0, vc0, sl, bt, o, lse, kernel, kn, vn)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_forced_splits_within_bounds_and_repeatable(dt):
    q, kc, vc, bt, _, _ = _paged(2, 1, 32, 8, 128, 64, 40, DT[dt], seed=15)
    sl = _seqlens([2500, 1111])
    for n in range(1, 9):
        o, lse, kernel = _run(q, kc, vc, sl, bt, causal=True, num_splits=n)
        assert (n > 1) == ("split" in kernel), kernel
        _check(q, kc, vc, sl, bt, o, lse, kernel, causal=True, dt=dt)
        o2, lse2, _ = _run(q, kc, vc, sl, bt, causal=True, num_splits=n)
        assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("mag", [1e-9, 1e20])
@pytest.mark.parametrize("num_splits", [1, 4])
def test_bf16_v_far_from_fp16_range(mag, num_splits):
    q, kc, vc, bt, _, _ = _paged(2, 4, 8, 2, 128, 32, 20, torch.bfloat16, seed=16)
    vc = (vc.float() * mag).to(torch.bfloat16)
    sl = _seqlens([600, 77])
    o, lse, kernel = _run(q, kc, vc, sl, bt, num_splits=num_splits)
    assert torch.isfinite(o).all()
    _check(q, kc, vc, sl, bt, o, lse, kernel)


@pytest.mark.parametrize("causal", [False, True])
def test_agrees_with_gather_and_dense_route(causal):
    um = _umfa()
    B, Sq, H, Hkv, D, ps = 2, 4, 16, 4, 128, 16
    q, kc, vc, bt, _, _ = _paged(B, Sq, H, Hkv, D, ps, 64, torch.float16, seed=17, share=False)
    L = 1000
    sl = _seqlens([L, L])
    o, _, _ = _run(q, kc, vc, sl, bt, causal=causal, out_dtype=torch.float32)
    idx = bt[:, :(L + ps - 1) // ps].long()
    kg = kc[idx].reshape(B, -1, Hkv, D)[:, :L].transpose(1, 2).contiguous()
    vg = vc[idx].reshape(B, -1, Hkv, D)[:, :L].transpose(1, 2).contiguous()
    qd = q.transpose(1, 2).contiguous()
    if causal:  # bottom-right: query i sees keys j <= i + L - Sq
        mask = torch.arange(L, device="cuda")[None, :] <= torch.arange(Sq, device="cuda")[:, None] + (L - Sq)
        od = um.scaled_dot_product_attention(qd, kg, vg, attn_mask=mask, enable_gqa=True)
    else:
        od = um.scaled_dot_product_attention(qd, kg, vg, enable_gqa=True)
    torch.cuda.synchronize()
    a, b = _np(o), _np(od.transpose(1, 2))
    assert np.abs(a - b).max() <= 4 * tol.ULP_AT_ONE["fp16"] * np.abs(b).max(), np.abs(a - b).max()


def test_graph_replay_follows_lengths_and_table():
    um = _umfa()
    B, H, Hkv, D, ps = 2, 8, 2, 128, 16
    q, kc, vc, bt, kn, vn = _paged(B, 1, H, Hkv, D, ps, 16, torch.bfloat16, seed=18, S_new=1, share=False)
    sl = _seqlens([40, 100])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def step():
        return um.kvcache_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt, causal=True, num_splits=3,
                                    return_softmax_lse=True)

    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up: scratch grows outside the capture
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        res = step()
    perm = torch.tensor(np.random.default_rng(0).permutation(bt.cpu().numpy().ravel()).reshape(bt.shape), device="cuda")
    for it in range(4):
        sl.add_(37)
        if it == 2:
            bt.copy_(perm)
        kc0, vc0 = kc.clone(), vc.clone()
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in res]
        kr, vr = kc.clone(), vc.clone()
        kc.copy_(kc0)
        vc.copy_(vc0)
        want = step()
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), it
        assert torch.equal(kr, kc) and torch.equal(vr, vc), it
        _check(q, kc0, vc0, sl, bt, got[0], got[1], um.last_kernel(), kn, vn, causal=True, out_dt=torch.bfloat16)


def test_opcheck_custom_ops():
    _umfa()
    q, kc, vc, bt, kn, vn = _paged(2, 2, 8, 2, 64, 16, 4, torch.bfloat16, seed=19, S_new=2)
    sl = _seqlens([5, 33])
    torch.library.opcheck(torch.ops.umfa.kvcache_forward.default, (q, kc, vc, sl, bt, True, 0.125, 0))
    torch.library.opcheck(torch.ops.umfa.kvcache_forward_append.default, (q, kc, vc, kn, vn, sl, bt, True, 0.125, 2))


def test_compile_fullgraph_single_node():
    um = _umfa()
    q, kc, vc, bt, kn, vn = _paged(2, 1, 8, 2, 128, 16, 8, torch.float16, seed=20, S_new=1)
    sl = _seqlens([30, 64])
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    def f(q, kc, vc, kn, vn):
        return um.kvcache_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt, causal=True)

    kc_e, vc_e = kc.clone(), vc.clone()
    torch._dynamo.reset()
    oc = torch.compile(f, fullgraph=True, backend=backend)(q, kc, vc, kn, vn)
    oe = f(q, kc_e, vc_e, kn, vn)
    torch.cuda.synchronize()
    assert len(graphs) == 1
    calls = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function" and "umfa" in str(n.target)]
    assert calls == ["umfa.kvcache_forward_append"], calls
    assert torch.equal(oc, oe)
    assert torch.equal(kc, kc_e) and torch.equal(vc, vc_e)  # the compiled call appended in place too


def test_refused_arguments():
    um = _umfa()
    q, kc, vc, bt, _, _ = _paged(2, 1, 8, 2, 128, 16, 4, torch.bfloat16, seed=21)
    for kw in (dict(rotary_cos=torch.zeros(1)), dict(cache_batch_idx=torch.zeros(2, dtype=torch.int32, device="cuda")),
               dict(cache_leftpad=torch.zeros(2, dtype=torch.int32, device="cuda")), dict(window_size=(8, 0)), dict(softcap=30.0),
               dict(alibi_slopes=torch.zeros(8))):
        with pytest.raises(ValueError):
            um.kvcache_attention(q, kc, vc, cache_seqlens=10, block_table=bt, **kw)
    o = um.kvcache_attention(q, kc, vc, cache_seqlens=10, block_table=bt, window_size=(-1, -1), softcap=0.0, rotary_interleaved=True)
    assert o.shape == q.shape
    with pytest.raises(ValueError):  # head_dim 96
        um.kvcache_attention(q[..., :96].contiguous(), kc[..., :96].contiguous(), vc[..., :96].contiguous(), cache_seqlens=10,
                             block_table=bt)
    with pytest.raises(ValueError):  # fp32
        um.kvcache_attention(q.float(), kc.float(), vc.float(), cache_seqlens=10, block_table=bt)
    with pytest.raises(ValueError):  # a paged cache whose page_size is not a multiple of 16
        um.kvcache_attention(q, kc[:, :8].contiguous(), vc[:, :8].contiguous(), cache_seqlens=4, block_table=bt)
    qg = q.clone().requires_grad_(True)
    o = um.kvcache_attention(qg, kc, vc, cache_seqlens=10, block_table=bt)
    with pytest.raises(RuntimeError):  # inference only: no backward
        o.float().sum().backward()
