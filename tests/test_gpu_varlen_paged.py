"""Packed variable-length queries over the KV cache on the GPU (umfa_torch.varlen_kvcache_attention): mixed
batches (prefill chunks beside decode) against the fp64 reference (tests/varlen_paged_ref.py) under the format bounds of
tests/tolerances.py, bitwise agreement with kvcache_attention when every L_q is equal, the packed in-place append (bitwise, nothing else
in the pool touched), forced split-KV parts, both forms in one launch (the kernel's own tally), bf16 V far from fp16's range, hostile
table entries / lengths / cu values (guards and canaries), a strided q, graph replay with rewritten cu / lengths / table,
opcheck / torch.compile and the refused arguments."""
import ctypes

import numpy as np
import pytest
import torch

import tolerances as tol
import varlen_paged_ref as ref

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


def _i32(vals):
    return torch.tensor(np.asarray(vals, np.int64).astype(np.int32), dtype=torch.int32, device="cuda")


def _cu(lq):
    return np.concatenate([[0], np.cumsum(lq)]).astype(np.int64)


def _setup(lq, H, Hkv, D, ps, max_pages, dt, seed, new=False, share=True, pad=0):
    """packed q [T_q + pad, H, D] (pad rows no sequence covers), k_cache / v_cache with GUARD free pages at each end, a randomly
    permuted block table (sequence 1 shares sequence 0's first page when `share`), packed k_new / v_new"""
    B, Tq = len(lq), int(sum(lq)) + pad
    g = torch.Generator(device="cuda").manual_seed(seed)
    num_pages = B * max_pages + 2 * GUARD
    q = torch.randn(Tq, H, D, device="cuda", dtype=dt, generator=g)
    kc = torch.randn(num_pages, ps, Hkv, D, device="cuda", dtype=dt, generator=g)
    vc = torch.randn(num_pages, ps, Hkv, D, device="cuda", dtype=dt, generator=g)
    bt = (np.random.default_rng(seed).permutation(B * max_pages) + GUARD).reshape(B, max_pages).astype(np.int32)
    if share and B > 1:
        bt[1, 0] = bt[0, 0]
    kn = torch.randn(Tq, Hkv, D, device="cuda", dtype=dt, generator=g) if new else None
    vn = torch.randn(Tq, Hkv, D, device="cuda", dtype=dt, generator=g) if new else None
    return q, kc, vc, torch.tensor(bt, device="cuda"), kn, vn


def _run(q, kc, vc, cu, max_q, sl, bt, kn=None, vn=None, causal=False, num_splits=0, scale=None, out_dtype=torch.float32):
    um = _umfa()
    sc = q.shape[-1] ** -0.5 if scale is None else scale
    o, lse = um.ops.varlen_kvcache_attention_forward(q, kc, vc, cu, max_q, sl, bt, kn, vn, scale=sc, causal=causal, num_splits=num_splits,
                                                     out_dtype=out_dtype)
    torch.cuda.synchronize()
    return o, lse, um.last_kernel()


def _reference(q, kc0, vc0, cu, max_q, sl, bt, kn=None, vn=None, causal=False, scale=None, min_live=0.5):
    """the fp64 reference on the caches as they were before the call; asserts -- on the reference alone -- that at least `min_live`
    of the query rows are live"""
    o_ref, lse_ref, _, _ = ref.forward(_np(q), _np(kc0), _np(vc0), cu.cpu().numpy(), max_q, sl.cpu().numpy(),
                                       None if bt is None else bt.cpu().numpy(), None if kn is None else _np(kn),
                                       None if vn is None else _np(vn), causal, scale)
    live = np.isfinite(lse_ref)  # [H, T_q]
    assert live.mean() >= min_live, f"the case holds too few live rows ({live.mean():.2f})"
    return o_ref, lse_ref, live


def _check(refs, cu, max_q, o, lse, kernel, dt="bf16", out_dt=None):
    """values and LSE of the live rows against the reference; dead rows of covered sequences exactly 0 / -inf"""
    o_ref, lse_ref, live = refs
    o_, l_ = _np(o), _np(lse)
    cov = ref.covered(cu.cpu().numpy(), o_.shape[0], max_q)  # [T_q]
    assert np.isfinite(o_[cov]).all()
    dead = ~live & cov[None, :]
    assert (o_.transpose(1, 0, 2)[dead] == 0).all() and np.isneginf(l_[dead]).all()
    if not live.any():
        return
    np.testing.assert_allclose(l_[live], lse_ref[live], rtol=0, atol=2e-3)
    got = o_.transpose(1, 0, 2)[live][None, None]
    want = o_ref.transpose(1, 0, 2)[live][None, None]
    tol.check_forward(got, want, DT[dt], kernel, tag="varlen_paged", out_dt=out_dt)


def _mixed(g, ps, cap):
    """per call: L_q of 0, 1, 4, g L_q at 32 (the last decode-form count) and just above it, rows just below / at / just above 128 (exactly
    127 / 128 / 129 for g = 1), and one of several hundred tokens; cache lengths of 0, 1, not a page multiple and exactly the capacity"""
    lo = 32 // g
    lq = [0, 1, 4, lo, lo + 1, 128 // g - 1, 128 // g, 128 // g + 1, 300]
    sl = [5, 0, 1, ps + 5, cap, 200, 333, 150, 500]
    return lq, sl


def _items(lq, g, Hkv):
    """(decode-form items, 128-row items) a launch over these lengths runs"""
    dec = sum(Hkv for l in lq if 0 < g * l <= 32)
    blk = sum(Hkv * ((g * l + 127) // 128) for l in lq if g * l > 32)
    return dec, blk


# (page_size, g, head_dim, dtype, causal)
CASES = [(16, 1, 128, "bf16", True), (16, 4, 64, "fp16", False), (64, 4, 128, "bf16", True), (64, 8, 128, "fp16", True),
         (256, 8, 64, "bf16", False), (256, 1, 128, "fp16", True), (16, 8, 128, "bf16", False), (64, 1, 64, "bf16", True)]


@pytest.mark.parametrize("ps,g,D,dt,causal", CASES)
def test_mixed_batch_values(ps, g, D, dt, causal):
    um = _umfa()
    Hkv, max_pages = 2, max(2, 640 // ps)
    cap = ps * max_pages
    lq, slv = _mixed(g, ps, cap)
    q, kc, vc, bt, _, _ = _setup(lq, g * Hkv, Hkv, D, ps, max_pages, DT[dt], seed=ps + g + D)
    cu, sl = _i32(_cu(lq)), _i32(slv)
    refs = _reference(q, kc, vc, cu, max(lq), sl, bt, causal=causal)
    for out_dtype in (torch.float32, DT[dt]):
        o, lse, kernel = _run(q, kc, vc, cu, max(lq), sl, bt, causal=causal, num_splits=1, out_dtype=out_dtype)
        assert kernel.startswith("fa_fwd16_paged_varlen<") and "split" not in kernel and ("causal" in kernel) == causal, kernel
        assert um.ops.varlen_kvcache_item_counts() == _items(lq, g, Hkv)  # both forms, in this one launch
        _check(refs, cu, max(lq), o, lse, kernel, dt=dt, out_dt=None if out_dtype == torch.float32 else out_dtype)


@pytest.mark.parametrize("static", ["bshd", "bhsd"])
def test_static_cache_mixed_batch(static):
    lq, H, Hkv, D, Smax = [1, 200, 0, 4, 33], 8, 2, 128, 300
    g = torch.Generator(device="cuda").manual_seed(5)
    q = torch.randn(sum(lq), H, D, device="cuda", dtype=torch.bfloat16, generator=g)
    if static == "bshd":
        kc = torch.randn(len(lq), Smax, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
        vc = torch.randn(len(lq), Smax, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
    else:  # HF StaticCache: [B, H_kv, S_max, D], handed over as its [B, S_max, H_kv, D] view
        kc = torch.randn(len(lq), Hkv, Smax, D, device="cuda", dtype=torch.bfloat16, generator=g).transpose(1, 2)
        vc = torch.randn(len(lq), Hkv, Smax, D, device="cuda", dtype=torch.bfloat16, generator=g).transpose(1, 2)
    cu, sl = _i32(_cu(lq)), _i32([17, 300, 129, 0, 250])
    for causal in (False, True):
        refs = _reference(q, kc, vc, cu, 200, sl, None, causal=causal)
        o, lse, kernel = _run(q, kc, vc, cu, 200, sl, None, causal=causal)
        _check(refs, cu, 200, o, lse, kernel)


@pytest.mark.parametrize("Sq,new", [(1, False), (4, True), (40, False), (40, True)])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("num_splits", [1, 3])
def test_equal_lengths_agree_bitwise_with_kvcache_attention(Sq, new, dt, num_splits):
    """every L_q equal: the arithmetic and its order are kvcache_attention's (same rows per wave, same steps, same parts, same fold)"""
    um = _umfa()
    B, H, Hkv, D, ps, mp = 4, 8, 2, 128, 16, 40
    q, kc, vc, bt, kn, vn = _setup([Sq] * B, H, Hkv, D, ps, mp, DT[dt], seed=30 + Sq, new=new, share=False)
    cu, sl = _i32(_cu([Sq] * B)), _i32([0, 150, ps + 5, 600])
    kc2, vc2 = kc.clone(), vc.clone()
    o, lse, kernel = _run(q, kc, vc, cu, Sq, sl, bt, kn, vn, causal=True, num_splits=num_splits)
    r = lambda t: None if t is None else t.view(B, Sq, *t.shape[1:])  # noqa: E731
    o2, lse2 = um.ops.kvcache_attention_forward(r(q), kc2, vc2, sl, bt, r(kn), r(vn), scale=D ** -0.5, causal=True, num_splits=num_splits,
                                                out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert um.last_kernel() == kernel.replace("_varlen", "")
    assert torch.equal(o.view(B, Sq, H, D), o2)
    assert torch.equal(lse.view(H, B, Sq).permute(1, 0, 2), lse2)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("static", [False, True])
def test_append_writes_rows_bitwise_and_nothing_else(dt, static):
    lq, H, Hkv, D = [5, 0, 1, 40, 3], 8, 2, 64
    if static:
        g = torch.Generator(device="cuda").manual_seed(11)
        q = torch.randn(sum(lq), H, D, device="cuda", dtype=DT[dt], generator=g)
        kc = torch.randn(len(lq), 48, Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        vc = torch.randn(len(lq), 48, Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        kn = torch.randn(sum(lq), Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        vn = torch.randn(sum(lq), Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        bt = None
    else:
        q, kc, vc, bt, kn, vn = _setup(lq, H, Hkv, D, 16, 3, DT[dt], seed=12, new=True, share=False)
    cu, sl = _i32(_cu(lq)), _i32([14, 7, 47, 3, 46])  # page crossings; the last one runs past the capacity of 48: one row dropped
    kc0, vc0 = kc.clone(), vc.clone()
    refs = _reference(q, kc0, vc0, cu, 40, sl, bt, kn, vn, causal=True)
    o, lse, kernel = _run(q, kc, vc, cu, 40, sl, bt, kn, vn, causal=True)
    btn = None if bt is None else bt.cpu().numpy()
    kw, vw = ref.append(_bits(kc0), _bits(vc0), _bits(kn), _bits(vn), cu.cpu().numpy(), 40, sl.cpu().numpy(), btn)
    assert (_bits(kc) == kw).all() and (_bits(vc) == vw).all()  # the rows written, bitwise, and every other byte unchanged
    assert not (kw == _bits(kc0)).all()
    if not static:
        assert (_bits(kc)[:GUARD] == _bits(kc0)[:GUARD]).all() and (_bits(kc)[-GUARD:] == _bits(kc0)[-GUARD:]).all()
    _check(refs, cu, 40, o, lse, kernel, dt=dt)
    assert (sl.cpu().numpy() == [14, 7, 47, 3, 46]).all()  # cache_seqlens is not advanced
    # append + attention = attention on a pre-appended cache with the advanced lengths (clamped at the capacity)
    sl2 = _i32(np.minimum(np.array([14, 7, 47, 3, 46]) + np.array(lq), 48))
    o2, lse2, _ = _run(q, kc, vc, cu, 40, sl2, bt, causal=True)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("mix", ["decode", "mixed"])
def test_forced_and_automatic_splits(dt, mix):
    H, Hkv, D, ps, mp = 32, 8, 128, 64, 40
    lq = [1, 1, 2, 1] if mix == "decode" else [1, 150, 0, 2, 40]
    slv = [2500, 1111, 64, 0] if mix == "decode" else [2500, 1111, 9, 777, 2560]
    q, kc, vc, bt, _, _ = _setup(lq, H, Hkv, D, ps, mp, DT[dt], seed=15)
    cu, sl = _i32(_cu(lq)), _i32(slv)
    refs = _reference(q, kc, vc, cu, max(lq), sl, bt, causal=True)
    for n in (1, 2, 5, 0):
        o, lse, kernel = _run(q, kc, vc, cu, max(lq), sl, bt, causal=True, num_splits=n)
        if n:
            assert (n > 1) == ("split" in kernel), kernel
        _check(refs, cu, max(lq), o, lse, kernel, dt=dt)
        o2, lse2, _ = _run(q, kc, vc, cu, max(lq), sl, bt, causal=True, num_splits=n)
        assert torch.equal(o, o2) and torch.equal(lse, lse2)  # the fold takes the parts in order: bitwise repeatable


def test_both_forms_in_one_launch():
    um = _umfa()
    H, Hkv, D, ps, mp = 8, 2, 128, 16, 20
    for lq in ([1, 1, 1], [300, 129], [1, 300, 4, 9, 0, 128]):
        g = H // Hkv
        q, kc, vc, bt, _, _ = _setup(lq, H, Hkv, D, ps, mp, torch.bfloat16, seed=len(lq))
        for n in (1, 3):
            _, _, kernel = _run(q, kc, vc, _i32(_cu(lq)), max(lq), _i32([300] * len(lq)), bt, causal=True, num_splits=n)
            dec, blk = um.ops.varlen_kvcache_item_counts()
            assert (dec, blk) == _items(lq, g, Hkv), (lq, n, dec, blk)
            assert kernel == "fa_fwd16_paged_varlen<bf16,128,causal,pv16" + (",split>" if n > 1 else ">")
    assert _items([1, 300, 4, 9, 0, 128], 4, 2) == (4, 2 * (10 + 1 + 4))  # (decode: L_q 1 and 4; 128-row: 300, 9 and 128 tokens)


@pytest.mark.parametrize("mag", [1e-9, 1e20])
@pytest.mark.parametrize("num_splits", [1, 4])
def test_bf16_v_far_from_fp16_range(mag, num_splits):
    lq = [4, 1, 150]
    q, kc, vc, bt, _, _ = _setup(lq, 8, 2, 128, 32, 20, torch.bfloat16, seed=16)
    vc = (vc.float() * mag).to(torch.bfloat16)
    cu, sl = _i32(_cu(lq)), _i32([600, 77, 333])
    refs = _reference(q, kc, vc, cu, 150, sl, bt)
    o, lse, kernel = _run(q, kc, vc, cu, 150, sl, bt, num_splits=num_splits)
    assert torch.isfinite(o).all()
    _check(refs, cu, 150, o, lse, kernel)


def _raw_call(q, kc, vc, cu, max_q, sl, bt, kn, vn, out, lse, Tq, causal, num_splits):
    """the C entry on caller-owned O / LSE blocks (so that canary rows can surround them)"""
    from umfa_torch import ops
    H, D = q.shape[1], q.shape[2]
    new = [None, None, None, None]
    if kn is not None:
        new = [ctypes.c_void_p(kn.data_ptr()), ops._i64(kn.stride()[:2]), ctypes.c_void_p(vn.data_ptr()), ops._i64(vn.stride()[:2])]
    stream = torch.cuda.current_stream().cuda_stream
    return ops._lib.umfa_varlen_kvcache_attention_forward_stream(
        ops.context(), ctypes.c_void_p(stream), ctypes.c_void_p(q.data_ptr()), ops._i64(q.stride()[:2]), ctypes.c_void_p(kc.data_ptr()),
        ops._i64(kc.stride()[:3]), ctypes.c_void_p(vc.data_ptr()), ops._i64(vc.stride()[:3]), *new, ctypes.c_void_p(bt.data_ptr()),
        int(bt.stride(0)), ctypes.c_void_p(sl.data_ptr()), Tq, cu.numel() - 1, int(max_q), ctypes.c_void_p(cu.data_ptr()), kn is not None, H,
        kc.shape[2], D, kc.shape[1], kc.shape[0], bt.shape[1], float(D ** -0.5), bool(causal), ops._PREC[q.dtype],
        ctypes.c_void_p(out.data_ptr()), ops._PREC[out.dtype], ctypes.c_void_p(lse.data_ptr()), int(num_splits))


@pytest.mark.parametrize("num_splits", [0, 3])
@pytest.mark.parametrize("cu_kind", ["good", "non_monotone", "beyond"])
def test_hostile_contents_touch_nothing_else(num_splits, cu_kind):
    """table entries -1 / num_pages / 2^31 - 1 / -2^31, lengths negative and 10^9, cu non-monotone and beyond T_q: safe by construction
    (every index is clamped or range-checked on the device) -- the guard pages and the canary rows come back bit-identical"""
    H, Hkv, D, ps, mp, C = 8, 2, 128, 16, 4, 8  # C canary rows around q / O / LSE
    lq = [3, 2, 40, 1, 5]
    Tq, B = sum(lq), len(lq)
    _, kc, vc, bt, _, _ = _setup(lq, H, Hkv, D, ps, mp, torch.bfloat16, seed=14, share=False)
    g = torch.Generator(device="cuda").manual_seed(77)
    q_big = torch.randn(Tq + 2 * C, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
    kn_big = torch.randn(Tq + 2 * C, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
    vn_big = torch.randn(Tq + 2 * C, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
    o_big = torch.full((Tq + 2 * C, H, D), 7.0, device="cuda", dtype=torch.float32)
    lse_big = torch.full(((H + 2 * C) * Tq,), 7.0, device="cuda", dtype=torch.float32)
    q, kn, vn, out, lse = q_big[C:C + Tq], kn_big[C:C + Tq], vn_big[C:C + Tq], o_big[C:C + Tq], lse_big[C * Tq:(C + H) * Tq]
    btn = bt.cpu().numpy()
    num_pages = kc.shape[0]
    btn[0, :] = -1
    btn[1, 1], btn[1, 3] = num_pages, 2 ** 31 - 1
    btn[2, 2] = -(2 ** 31)
    bt = torch.tensor(btn, device="cuda")
    sl = _i32([20, 30, -7, 10 ** 9, 60])
    cuv = {"good": _cu(lq), "non_monotone": np.array([0, 40, 3, 45, 20, Tq]), "beyond": np.array([-9, 5, 10 ** 9, 7, 2 ** 31 - 1, Tq + 50])}[cu_kind]
    cu = _i32(cuv)
    kc0, vc0, q0, kn0, vn0 = kc.clone(), vc.clone(), q_big.clone(), kn_big.clone(), vn_big.clone()
    rc = _raw_call(q, kc, vc, cu, 40, sl, bt, kn, vn, out, lse, Tq, True, num_splits)
    torch.cuda.synchronize()
    assert rc == 0  # the call returns; values are not checked here
    assert torch.equal(kc[:GUARD], kc0[:GUARD]) and torch.equal(kc[-GUARD:], kc0[-GUARD:])
    assert torch.equal(vc[:GUARD], vc0[:GUARD]) and torch.equal(vc[-GUARD:], vc0[-GUARD:])
    assert torch.equal(q_big, q0) and torch.equal(kn_big, kn0) and torch.equal(vn_big, vn0)
    assert (o_big[:C] == 7.0).all() and (o_big[C + Tq:] == 7.0).all()
    assert (lse_big[:C * Tq] == 7.0).all() and (lse_big[(C + H) * Tq:] == 7.0).all()
    if cu_kind == "good":  # defined results: the pools equal the reference's append, the values its attention
        kw, vw = ref.append(_bits(kc0), _bits(vc0), _bits(kn), _bits(vn), cuv, 40, sl.cpu().numpy(), btn)
        assert (_bits(kc) == kw).all() and (_bits(vc) == vw).all()
        refs = _reference(q, kc0, vc0, cu, 40, sl, bt, kn, vn, causal=True, min_live=0.0)
        _check(refs, cu, 40, out, lse.view(H, Tq), "fa_fwd16_paged_varlen<bf16,128,causal,pv16>")


def test_uncovered_rows_are_not_written():
    lq, pad = [3, 50, 1], 6  # max_seqlen_q = 20 caps the 50-token sequence: its rows 20 .. 49 and the 6 pad rows belong to nobody
    q, kc, vc, bt, _, _ = _setup(lq, 8, 2, 64, 16, 8, torch.float16, seed=23, pad=pad)
    Tq = q.shape[0]
    out = torch.full((Tq, 8, 64), 7.0, device="cuda", dtype=torch.float32)
    lse = torch.full((8, Tq), 7.0, device="cuda", dtype=torch.float32)
    cu, sl = _i32(_cu(lq)), _i32([100, 90, 128])
    for n in (1, 2):
        assert _raw_call(q, kc, vc, cu, 20, sl, bt, None, None, out, lse, Tq, False, n) == 0
        torch.cuda.synchronize()
        cov = torch.tensor(ref.covered(_cu(lq), Tq, 20), device="cuda")
        assert cov.sum().item() == 3 + 20 + 1
        assert (out[~cov] == 7.0).all() and (lse[:, ~cov] == 7.0).all()
        refs = _reference(q, kc, vc, cu, 20, sl, bt, min_live=0.0)
        _check(refs, cu, 20, out, lse, "fa_fwd16_paged_varlen<fp16,64>", dt="fp16")


def test_strided_q_from_a_fused_projection():
    um = _umfa()
    lq, H, Hkv, D = [1, 70, 4, 9], 8, 2, 128
    _, kc, vc, bt, _, _ = _setup(lq, H, Hkv, D, 16, 8, torch.bfloat16, seed=24)
    g = torch.Generator(device="cuda").manual_seed(25)
    qkv = torch.randn(sum(lq), (H + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16, generator=g)
    q = qkv[:, :H * D].view(sum(lq), H, D)
    k = qkv[:, H * D:(H + Hkv) * D].view(sum(lq), Hkv, D)
    v = qkv[:, (H + Hkv) * D:].view(sum(lq), Hkv, D)
    assert not q.is_contiguous() and q.stride(0) == (H + 2 * Hkv) * D
    cu, sl = _i32(_cu(lq)), _i32([17, 30, 0, 100])
    kc0, vc0 = kc.clone(), vc.clone()
    refs = _reference(q, kc0, vc0, cu, 70, sl, bt, k, v, causal=True)
    o, lse = um.varlen_kvcache_attention(q, kc, vc, cu, 70, sl, block_table=bt, k=k, v=v, causal=True, return_softmax_lse=True)
    torch.cuda.synchronize()
    assert o.dtype == torch.bfloat16 and o.shape == q.shape and o.is_contiguous() and lse.shape == (H, sum(lq))
    _check(refs, cu, 70, o, lse, um.last_kernel(), out_dt=torch.bfloat16)
    o2, lse2, _ = _run(q.contiguous(), kc0, vc0, cu, 70, sl, bt, k.contiguous(), v.contiguous(), causal=True, out_dtype=torch.bfloat16)
    assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(kc, kc0) and torch.equal(vc, vc0)  # the strides, not a copy


def test_graph_replay_follows_cu_lengths_and_table():
    um = _umfa()
    H, Hkv, D, ps, mp, B, Tq, max_q = 8, 2, 128, 16, 16, 4, 120, 100
    heavy, light = [100, 18, 1, 1], [1, 1, 2, 1]  # prefill-heavy, then decode-heavy at the same T_q, B and max_seqlen_q
    q, kc, vc, bt, kn, vn = _setup(heavy, H, Hkv, D, ps, mp, torch.bfloat16, seed=18, new=True, share=False)
    assert q.shape[0] == Tq
    cu, sl = _i32(_cu(heavy)), _i32([40, 100, 7, 0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def step():
        return um.varlen_kvcache_attention(q, kc, vc, cu, max_q, sl, block_table=bt, k=kn, v=vn, causal=True, num_splits=3,
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
        sl.add_(29)
        if it >= 1:
            cu.copy_(_i32(_cu(light)))
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
        cov = torch.tensor(ref.covered(cu.cpu().numpy(), Tq, max_q), device="cuda")
        assert torch.equal(got[0][cov], want[0][cov]) and torch.equal(got[1][:, cov], want[1][:, cov]), it
        assert torch.equal(kr, kc) and torch.equal(vr, vc), it
        refs = _reference(q, kc0, vc0, cu, max_q, sl, bt, kn, vn, causal=True, min_live=0.0)
        _check(refs, cu, max_q, got[0], got[1], um.last_kernel(), out_dt=torch.bfloat16)
        assert int(cov.sum()) == (Tq if it == 0 else 5)


def test_opcheck_custom_ops():
    _umfa()
    lq = [2, 40, 1]
    q, kc, vc, bt, kn, vn = _setup(lq, 8, 2, 64, 16, 4, torch.bfloat16, seed=19, new=True)
    cu, sl = _i32(_cu(lq)), _i32([5, 20, 33])
    torch.library.opcheck(torch.ops.umfa.varlen_kvcache_forward.default, (q, kc, vc, cu, 40, sl, bt, True, 0.125, 0))
    torch.library.opcheck(torch.ops.umfa.varlen_kvcache_forward_append.default, (q, kc, vc, kn, vn, cu, 40, sl, bt, True, 0.125, 2))


def test_compile_fullgraph_single_node():
    um = _umfa()
    lq = [1, 35, 2]
    q, kc, vc, bt, kn, vn = _setup(lq, 8, 2, 128, 16, 8, torch.float16, seed=20, new=True)
    cu, sl = _i32(_cu(lq)), _i32([30, 64, 1])
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    def f(q, kc, vc, kn, vn):
        return um.varlen_kvcache_attention(q, kc, vc, cu, 35, sl, block_table=bt, k=kn, v=vn, causal=True)

    kc_e, vc_e = kc.clone(), vc.clone()
    torch._dynamo.reset()
    oc = torch.compile(f, fullgraph=True, backend=backend)(q, kc, vc, kn, vn)
    oe = f(q, kc_e, vc_e, kn, vn)
    torch.cuda.synchronize()
    assert len(graphs) == 1
    calls = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function" and "umfa" in str(n.target)]
    assert calls == ["umfa.varlen_kvcache_forward_append"], calls
    assert torch.equal(oc, oe)
    assert torch.equal(kc, kc_e) and torch.equal(vc, vc_e)  # the compiled call appended in place too


def test_refused_arguments_and_malformed_tensors():
    um = _umfa()
    lq = [1, 20, 3]
    q, kc, vc, bt, kn, vn = _setup(lq, 8, 2, 128, 16, 4, torch.bfloat16, seed=21, new=True)
    cu, sl = _i32(_cu(lq)), _i32([10, 20, 30])
    call = lambda *a, **kw: um.varlen_kvcache_attention(*a, **kw)  # noqa: E731
    for kw in (dict(rotary_cos=torch.zeros(1)), dict(cache_batch_idx=torch.zeros(3, dtype=torch.int32, device="cuda")),
               dict(cache_leftpad=torch.zeros(3, dtype=torch.int32, device="cuda")), dict(window_size=(8, 0)), dict(softcap=30.0),
               dict(alibi_slopes=torch.zeros(8)), dict(seqused_k=sl), dict(dropout_p=0.1)):
        with pytest.raises(ValueError):
            call(q, kc, vc, cu, 20, sl, block_table=bt, **kw)
    with pytest.raises(TypeError):
        call(q, kc, vc, cu, 20, sl, block_table=bt, no_such_argument=1)
    o = call(q, kc, vc, cu, 20, sl, block_table=bt, window_size=(-1, -1), softcap=0.0, rotary_interleaved=True)
    assert o.shape == q.shape
    kc0 = kc.clone()
    two = torch.stack([cu, cu], 1)
    bad = [
        dict(q=q[None]),                                                          # a dense 4-D q
        dict(q=q.float(), k_cache=kc.float(), v_cache=vc.float()),                # fp32
        dict(q=q[..., :96].contiguous(), k_cache=kc[..., :96].contiguous(), v_cache=vc[..., :96].contiguous()),  # head_dim 96
        dict(q=q.half()),                                                         # q and the cache differ in dtype
        dict(k_cache=kc.view(torch.int16).view(torch.float8_e4m3fn)[..., :128].contiguous(),
             v_cache=vc.view(torch.int16).view(torch.float8_e4m3fn)[..., :128].contiguous()),  # fp8 caches: kvcache_attention's
        dict(k_cache=kc[:, :8].contiguous(), v_cache=vc[:, :8].contiguous()),     # page_size not a multiple of 16
        dict(cu_seqlens_q=cu.long()), dict(cu_seqlens_q=cu.cpu()), dict(cu_seqlens_q=cu[:-1]), dict(cu_seqlens_q=two[:, 0]),  # dtype, device, [B + 1], stride
        dict(cu_seqlens_q=cu[None]),
        dict(max_seqlen_q=-1), dict(max_seqlen_q=q.shape[0] + 1), dict(max_seqlen_q=20.0),
        dict(cache_seqlens=sl[:2]), dict(cache_seqlens=sl.long()), dict(cache_seqlens=sl[:1].expand(3)), dict(cache_seqlens=10),
        dict(block_table=bt[:2]), dict(block_table=bt.long()), dict(block_table=bt[:1].expand(3, 4)), dict(block_table=bt.t().contiguous().t()),
        dict(k=kn, v=None), dict(k=kn[:-1], v=vn[:-1]), dict(k=kn.half(), v=vn.half()), dict(k=kn[None], v=vn[None]),
        dict(q=q[:, :7], k=None, v=None),                                         # 7 heads over 2 KV heads
        dict(softmax_scale=0.0),
    ]
    base = dict(q=q, k_cache=kc, v_cache=vc, cu_seqlens_q=cu, max_seqlen_q=20, cache_seqlens=sl, block_table=bt, k=kn, v=vn)
    for i, change in enumerate(bad):
        args = {**base, **change}
        with pytest.raises(ValueError):
            call(**args)
            pytest.fail(f"malformed case {i} was accepted: {list(change)}")
    torch.cuda.synchronize()
    assert torch.equal(kc, kc0)  # nothing was appended by a refused call
    with pytest.raises(ValueError):  # a static cache with fewer rows than sequences
        call(q, kc[:2], vc[:2], cu, 20, sl)
    qg = q.clone().requires_grad_(True)
    o = call(qg, kc, vc, cu, 20, sl, block_table=bt)
    with pytest.raises(RuntimeError):  # inference only: no backward
        o.float().sum().backward()
