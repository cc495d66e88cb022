"""KV-cache attention over fp8 (e4m3fn) caches on the GPU (umfa_torch.kvcache_attention with k_descale / v_descale; DESIGN.md section
3.1j), mirroring tests/test_gpu_paged.py: values against the fp64 reference on the dequantised caches (tests/paged_fp8_ref.py) under the
unchanged format bounds of tests/tolerances.py for paged and static caches, per-(batch, head) descales that differ by 2^+-6 between
heads, scalar and [H_kv] descales through stride 0, the quantising append bitwise against the CPU quantiser with nothing else touched,
out-of-range table entries and lengths, forced split-KV parts, agreement with the 16-bit route on the dequantised cache, graph replay
following lengths, table and descales, opcheck / torch.compile and the refused arguments.

Why the 16-bit bounds hold unchanged: the reference sees the same dequantised numbers, the kernel's expansions to its operand types are
exact, and P is rounded to fp16 once as in the 16-bit kernel; the only arithmetic added is two fp32 products with the scales."""
import numpy as np
import pytest
import torch

import paged_fp8_ref as ref
import tolerances as tol

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
F8 = torch.float8_e4m3fn
GUARD = 2  # pages at each end of a pool that no table names: they must come back unchanged


def _umfa():
    import umfa_torch
    return umfa_torch


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _bytes(t):
    return t.detach().cpu().view(torch.uint8).numpy()


def _f8(shape, g):
    """random finite e4m3fn values with a normal-like spread (rounded from N(0, 1) x 4; no NaN bytes)"""
    return (torch.randn(shape, device="cuda", generator=g) * 4).clamp(-448, 448).to(F8)


def _dev(x):
    return torch.tensor(np.asarray(x, np.float32), device="cuda")


def _paged(B, Sq, H, Hkv, D, ps, max_pages, dt, seed, S_new=0, share=True):
    g = torch.Generator(device="cuda").manual_seed(seed)
    num_pages = B * max_pages + 2 * GUARD
    q = torch.randn(B, Sq, H, D, device="cuda", dtype=dt, generator=g)
    kc, vc = _f8((num_pages, ps, Hkv, D), g), _f8((num_pages, ps, Hkv, D), g)
    perm = np.random.default_rng(seed).permutation(B * max_pages) + GUARD
    bt = perm.reshape(B, max_pages).astype(np.int32)
    if share and B > 1:
        bt[1, 0] = bt[0, 0]
    kn = torch.randn(B, S_new, Hkv, D, device="cuda", dtype=dt, generator=g) if S_new else None
    vn = torch.randn(B, S_new, Hkv, D, device="cuda", dtype=dt, generator=g) if S_new else None
    return q, kc, vc, torch.tensor(bt, device="cuda"), kn, vn


def _descales(B, Hkv, seed):
    """[B, H_kv] descales whose neighbouring heads differ by 2^+-6 (a kernel reading the wrong head's scale is off by far more than any
    bound), not powers of two themselves"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.7, 1.4, (B, Hkv))
    e = np.where((np.arange(Hkv)[None, :] + np.arange(B)[:, None]) % 2 == 0, 2.0 ** -3, 2.0 ** 3)
    return (base * e).astype(np.float32), (base[::-1, ::-1] / e).astype(np.float32)


def _seqlens(vals):
    return torch.tensor(vals, dtype=torch.int32, device="cuda")


def _run(q, kc, vc, sl, bt, kd, vd, kn=None, vn=None, causal=False, num_splits=0, scale=None, out_dtype=torch.float32):
    um = _umfa()
    sc = q.shape[-1] ** -0.5 if scale is None else scale
    o, lse = um.ops.kvcache_attention_fp8_forward(q, kc, vc, sl, kd, vd, bt, kn, vn, scale=sc, causal=causal, num_splits=num_splits,
                                                  out_dtype=out_dtype)
    torch.cuda.synchronize()
    k = um.last_kernel()
    assert k.startswith("fa_fwd16_paged_fp8<"), k
    return o, lse, k


def _check(q, kc0, vc0, sl, bt, kd, vd, o, lse, kernel, kn=None, vn=None, causal=False, scale=None, dt="bf16", out_dt=None):
    """values and LSE against the fp64 reference (run on the byte caches as they were before the call)"""
    o_ref, lse_ref, _, _ = ref.forward(_np(q), _bytes(kc0), _bytes(vc0), sl.cpu().numpy(), kd.cpu().numpy(), vd.cpu().numpy(),
                                       None if bt is None else bt.cpu().numpy(), None if kn is None else _np(kn),
                                       None if vn is None else _np(vn), causal, scale)
    o_, l_ = _np(o), _np(lse)
    assert np.isfinite(o_).all()
    live = np.isfinite(lse_ref)  # [B, H, Sq]
    live_o = live.transpose(0, 2, 1)  # [B, Sq, H]
    assert (o_[~live_o] == 0).all() and np.isneginf(l_[~live]).all()
    if not live.any():
        return
    print("fp8 paged", kernel, "lse max err", float(np.abs(l_[live] - lse_ref[live]).max()))
    np.testing.assert_allclose(l_[live], lse_ref[live], rtol=0, atol=2e-3)
    # (check_forward normalises by max |O|: one (batch, head) group at a time, its descale sets its magnitude)
    B, H = live.shape[0], live.shape[1]
    Hkv = kc0.shape[2]
    for b in range(B):
        for hk in range(Hkv):
            hs = slice(hk * (H // Hkv), (hk + 1) * (H // Hkv))
            m = live_o[b, :, hs]
            if m.any():
                tol.check_forward(o_[b, :, hs][m][None, None], o_ref[b, :, hs][m][None, None], DT[dt], kernel, tag="paged_fp8", out_dt=out_dt)


# (page_size, g, Sq, causal, dtype, head_dim): the grid of test_gpu_paged.py
CASES = [(16, 1, 1, False, "bf16", 128), (16, 4, 1, True, "fp16", 128), (16, 8, 4, True, "bf16", 64), (32, 4, 16, False, "bf16", 128),
         (32, 8, 1, False, "fp16", 64), (64, 1, 200, True, "bf16", 128), (64, 4, 4, True, "bf16", 128), (64, 8, 16, True, "fp16", 128),
         (256, 4, 1, False, "bf16", 128), (256, 1, 16, True, "fp16", 64), (256, 8, 200, False, "bf16", 64), (16, 4, 200, True, "bf16", 128)]


@pytest.mark.parametrize("ps,g,Sq,causal,dt,D", CASES)
def test_paged_values(ps, g, Sq, causal, dt, D):
    Hkv, max_pages = 2, max(2, 640 // ps)
    cap = ps * max_pages
    q, kc, vc, bt, _, _ = _paged(4, Sq, g * Hkv, Hkv, D, ps, max_pages, DT[dt], seed=ps + g + Sq)
    kd, vd = (_dev(x) for x in _descales(4, Hkv, seed=ps + g))
    sl = _seqlens([0, 1, ps + 5, cap])  # empty, one key, not a page multiple, exactly at capacity
    o, lse, kernel = _run(q, kc, vc, sl, bt, kd, vd, causal=causal)
    assert ("pv16" in kernel) == (dt == "bf16") and (",causal" in kernel) == causal, kernel
    _check(q, kc, vc, sl, bt, kd, vd, o, lse, kernel, causal=causal, dt=dt)


@pytest.mark.parametrize("ps,g,Sq,dt,D", [(16, 8, 16, "bf16", 128), (64, 1, 200, "fp16", 128), (32, 4, 200, "bf16", 64)])
@pytest.mark.parametrize("causal", [False, True])
def test_unsplit_many_rows(ps, g, Sq, dt, D, causal):
    Hkv, max_pages = 2, 640 // ps
    q, kc, vc, bt, _, _ = _paged(4, Sq, g * Hkv, Hkv, D, ps, max_pages, DT[dt], seed=ps + g + Sq + 1)
    kd, vd = (_dev(x) for x in _descales(4, Hkv, seed=g))
    sl = _seqlens([0, 150, ps + 5, 640])
    for out_dtype in (torch.float32, DT[dt]):
        o, lse, kernel = _run(q, kc, vc, sl, bt, kd, vd, causal=causal, num_splits=1, out_dtype=out_dtype)
        assert "split" not in kernel, kernel
        _check(q, kc, vc, sl, bt, kd, vd, o, lse, kernel, causal=causal, dt=dt, out_dt=None if out_dtype == torch.float32 else out_dtype)


def _static(layout, B, Smax, Hkv, D, g):
    if layout == "bshd":
        return _f8((B, Smax, Hkv, D), g), _f8((B, Smax, Hkv, D), g)
    return _f8((B, Hkv, Smax, D), g).transpose(1, 2), _f8((B, Hkv, Smax, D), g).transpose(1, 2)  # HF StaticCache's view


@pytest.mark.parametrize("layout", ["bshd", "bhsd"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_static_cache_values(layout, dt):
    B, Smax, H, Hkv, D = 3, 300, 8, 2, 128
    g = torch.Generator(device="cuda").manual_seed(7)
    q = torch.randn(B, 4, H, D, device="cuda", dtype=DT[dt], generator=g)
    kc, vc = _static(layout, B, Smax, Hkv, D, g)
    kd, vd = (_dev(x) for x in _descales(B, Hkv, seed=7))
    sl = _seqlens([17, 300, 129])
    for causal in (False, True):
        o, lse, kernel = _run(q, kc, vc, sl, None, kd, vd, causal=causal)
        _check(q, kc, vc, sl, None, kd, vd, o, lse, kernel, causal=causal, dt=dt)


@pytest.mark.parametrize("form", ["scalar", "heads", "batch", "float", "default"])
def test_descale_forms_through_stride_zero(form):
    um = _umfa()
    B, Hkv = 3, 2
    q, kc, vc, bt, _, _ = _paged(B, 2, 8, Hkv, 128, 16, 4, torch.bfloat16, seed=31)
    sl = _seqlens([40, 7, 64])
    full_k, full_v = _descales(B, Hkv, seed=31)
    if form == "scalar":
        kd, vd = _dev(0.37).reshape(()), _dev([2.5])
    elif form == "heads":
        kd, vd = _dev(full_k[0]), _dev(full_v[0])
    elif form == "batch":
        kd, vd = _dev(full_k[:, :1]), _dev(full_v[:, :1])
    elif form == "float":
        kd, vd = 0.37, 2.5
    else:
        kd = vd = None
    o, lse = um.kvcache_attention(q, kc, vc, cache_seqlens=sl, block_table=bt, causal=True, return_softmax_lse=True, k_descale=kd,
                                  v_descale=vd)
    torch.cuda.synchronize()
    assert o.dtype == torch.bfloat16 and o.shape == q.shape and lse.shape == (B, 8, 2)
    as_t = lambda d: _dev(1.0 if d is None else d) if not isinstance(d, torch.Tensor) else d  # noqa: E731
    _check(q, kc, vc, sl, bt, as_t(kd), as_t(vd), o, lse, um.last_kernel(), causal=True, out_dt=torch.bfloat16)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("static", [False, "bshd", "bhsd"])
def test_append_quantises_rows_bitwise_and_nothing_else(dt, static):
    B, Hkv, D, S_new = 3, 2, 64, 5
    if static:
        g = torch.Generator(device="cuda").manual_seed(11)
        q = torch.randn(B, 5, 8, D, device="cuda", dtype=DT[dt], generator=g)
        kc, vc = _static(static, B, 40, Hkv, D, g)
        kn = torch.randn(B, S_new, Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        vn = torch.randn(B, S_new, Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        bt = None
        lens = [0, 14, 37]  # the last one runs past S_max = 40: two rows dropped
    else:
        q, kc, vc, bt, kn, vn = _paged(B, 5, 8, Hkv, D, 16, 3, DT[dt], seed=12, S_new=S_new, share=False)
        lens = [0, 14, 46]  # page crossing; the last one past the capacity of 48
    kn[0, 0, 0, :4] = torch.tensor([1e4, -1e4, 0.0, -0.0], dtype=DT[dt])  # beyond +-448 descale: saturates
    sl = _seqlens(lens)
    kd, vd = (_dev(x) for x in _descales(B, Hkv, seed=12))  # arbitrary (not power-of-two) descales: the division must be IEEE
    kc0, vc0 = kc.clone(), vc.clone()
    o, lse, kernel = _run(q, kc, vc, sl, bt, kd, vd, kn, vn, causal=True)
    btn = None if bt is None else bt.cpu().numpy()
    kw, vw = ref.append(_bytes(kc0), _bytes(vc0), _np(kn), _np(vn), sl.cpu().numpy(), kd.cpu().numpy(), vd.cpu().numpy(), btn)
    # the CPU quantiser is torch's own cast, bit for bit
    tq = (kn.float().cpu() / kd.cpu()[:, None, :, None]).clamp(-448, 448).to(F8).view(torch.uint8).numpy()
    assert (ref.quantise(_np(kn), kd.cpu().numpy()[:, None, :, None]) == tq).all()
    assert (_bytes(kc) == kw).all() and (_bytes(vc) == vw).all()  # the rows written, bitwise, and every other byte unchanged
    assert not (kw == _bytes(kc0)).all()
    if static == "bhsd":  # the storage as allocated: every byte of it
        assert (_bytes(kc.transpose(1, 2)) == kw.transpose(0, 2, 1, 3)).all()
    if not static:
        assert (_bytes(kc)[:GUARD] == _bytes(kc0)[:GUARD]).all() and (_bytes(kc)[-GUARD:] == _bytes(kc0)[-GUARD:]).all()
    _check(q, kc0, vc0, sl, bt, kd, vd, o, lse, kernel, kn, vn, causal=True, dt=dt)
    assert (sl.cpu().numpy() == lens).all()  # cache_seqlens is not advanced


def test_rows_without_keys_are_exact_zeros():
    q, kc, vc, bt, _, _ = _paged(3, 8, 8, 2, 128, 16, 4, torch.bfloat16, seed=13)
    kd, vd = (_dev(x) for x in _descales(3, 2, seed=13))
    sl = _seqlens([0, 3, 40])  # no key at all; causal with L_k = 3 < Sq = 8
    o, lse, kernel = _run(q, kc, vc, sl, bt, kd, vd, causal=True)
    assert (o[0] == 0).all() and torch.isneginf(lse[0]).all()
    assert (o[1, :5] == 0).all() and torch.isneginf(lse[1, :, :5]).all()
    _check(q, kc, vc, sl, bt, kd, vd, o, lse, kernel, causal=True)


@pytest.mark.parametrize("num_splits", [0, 3])
def test_out_of_range_entries_and_lengths(num_splits):
    B, Hkv, D = 4, 2, 128
    q, kc, vc, bt, kn, vn = _paged(B, 2, 8, Hkv, D, 16, 4, torch.bfloat16, seed=14, S_new=3, share=False)
    kd, vd = (_dev(x) for x in _descales(B, Hkv, seed=14))
    btn = bt.cpu().numpy()
    num_pages = kc.shape[0]
    btn[0, :] = -1                                  # no page the pool holds
    btn[1, 1], btn[1, 3] = num_pages, 2 ** 31 - 1   # one past the pool, far past it
    btn[2, 2] = -(2 ** 31)
    bt = torch.tensor(btn, device="cuda")
    sl = _seqlens([20, 30, -7, 10 ** 9])            # a negative and a huge length: clamped into [0, 64]
    kc0, vc0 = kc.clone(), vc.clone()
    o, lse, kernel = _run(q, kc, vc, sl, bt, kd, vd, kn, vn, causal=False, num_splits=num_splits)
    kw, vw = ref.append(_bytes(kc0), _bytes(vc0), _np(kn), _np(vn), sl.cpu().numpy(), kd.cpu().numpy(), vd.cpu().numpy(), btn)
    assert (_bytes(kc) == kw).all() and (_bytes(vc) == vw).all()
    assert (o[0] == 0).all() and torch.isneginf(lse[0]).all()
    _check(q, kc0, vc0, sl, bt, kd, vd, o, lse, kernel, kn, vn)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_forced_splits_within_bounds_and_repeatable(dt):
    q, kc, vc, bt, _, _ = _paged(2, 1, 32, 8, 128, 64, 40, DT[dt], seed=15)
    kd, vd = (_dev(x) for x in _descales(2, 8, seed=15))
    sl = _seqlens([2500, 1111])
    for n in range(1, 9):
        o, lse, kernel = _run(q, kc, vc, sl, bt, kd, vd, causal=True, num_splits=n)
        assert (n > 1) == ("split" in kernel), kernel
        _check(q, kc, vc, sl, bt, kd, vd, o, lse, kernel, causal=True, dt=dt)
        o2, lse2, _ = _run(q, kc, vc, sl, bt, kd, vd, causal=True, num_splits=n)
        assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True])
def test_agrees_with_the_16bit_route_on_the_dequantised_cache(dt, causal):
    """power-of-two descales: k8.to(dt) * d is exact, so the 16-bit kvcache_attention sees the very numbers the fp8 call stands for"""
    um = _umfa()
    B, Sq, H, Hkv, D, ps = 2, 4, 16, 4, 128, 16
    q, kc, vc, bt, _, _ = _paged(B, Sq, H, Hkv, D, ps, 64, DT[dt], seed=17, share=False)
    kd = _dev(2.0 ** np.array([-3, 1, -6, 0]))
    vd = _dev(2.0 ** np.array([2, -5, 0, -1]))
    sl = _seqlens([1000, 333])
    o, _, _ = _run(q, kc, vc, sl, bt, kd, vd, causal=causal)
    k16 = (kc.to(DT[dt]) * kd.to(DT[dt])[None, None, :, None])
    v16 = (vc.to(DT[dt]) * vd.to(DT[dt])[None, None, :, None])
    assert torch.equal(k16.double(), kc.double() * kd.double()[None, None, :, None])
    o16, _ = um.ops.kvcache_attention_forward(q, k16, v16, sl, bt, scale=D ** -0.5, causal=causal, out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert um.last_kernel().startswith("fa_fwd16_paged<")
    a, b = _np(o), _np(o16)
    for hk in range(Hkv):  # (each KV head's outputs at its own scale)
        hs = slice(hk * (H // Hkv), (hk + 1) * (H // Hkv))
        err = np.abs(a[:, :, hs] - b[:, :, hs]).max()
        assert err <= 4 * tol.ULP_AT_ONE["fp16"] * np.abs(b[:, :, hs]).max(), (hk, err)


def test_graph_replay_follows_lengths_table_and_descales():
    um = _umfa()
    B, H, Hkv, D, ps = 2, 8, 2, 128, 16
    q, kc, vc, bt, kn, vn = _paged(B, 1, H, Hkv, D, ps, 16, torch.bfloat16, seed=18, S_new=1, share=False)
    kd, vd = (_dev(x) for x in _descales(B, Hkv, seed=18))
    sl = _seqlens([40, 100])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def step():
        return um.kvcache_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt, causal=True, num_splits=3,
                                    return_softmax_lse=True, k_descale=kd, v_descale=vd)

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
        if it % 2 == 1:  # the descales are device data too: the replay reads what they hold now
            kd.mul_(1.7)
            vd.copy_(vd.flip(0, 1) * 0.3)
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
        assert torch.equal(kr.view(torch.uint8), kc.view(torch.uint8)) and torch.equal(vr.view(torch.uint8), vc.view(torch.uint8)), it
        _check(q, kc0, vc0, sl, bt, kd, vd, got[0], got[1], um.last_kernel(), kn, vn, causal=True, out_dt=torch.bfloat16)


def test_opcheck_custom_ops():
    _umfa()
    q, kc, vc, bt, kn, vn = _paged(2, 2, 8, 2, 64, 16, 4, torch.bfloat16, seed=19, S_new=2)
    kd, vd = (_dev(x) for x in _descales(2, 2, seed=19))
    sl = _seqlens([5, 33])
    k8, v8 = kc.view(torch.uint8), vc.view(torch.uint8)  # the ops take the caches' bytes (torch's schema check has no float8 kernels)
    torch.library.opcheck(torch.ops.umfa.kvcache_fp8_forward.default, (q, k8, v8, sl, kd, vd, bt, True, 0.125, 0))
    torch.library.opcheck(torch.ops.umfa.kvcache_fp8_forward_append.default, (q, k8, v8, kn, vn, sl, kd, vd, bt, True, 0.125, 2))


def test_compile_fullgraph_single_node():
    um = _umfa()
    q, kc, vc, bt, kn, vn = _paged(2, 1, 8, 2, 128, 16, 8, torch.float16, seed=20, S_new=1)
    kd, vd = (_dev(x) for x in _descales(2, 2, seed=20))
    sl = _seqlens([30, 64])
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    def f(q, kc, vc, kn, vn):
        return um.kvcache_attention(q, kc, vc, kn, vn, cache_seqlens=sl, block_table=bt, causal=True, k_descale=kd, v_descale=vd)

    kc_e, vc_e = kc.clone(), vc.clone()
    torch._dynamo.reset()
    oc = torch.compile(f, fullgraph=True, backend=backend)(q, kc, vc, kn, vn)
    oe = f(q, kc_e, vc_e, kn, vn)
    torch.cuda.synchronize()
    assert len(graphs) == 1
    calls = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function" and "umfa" in str(n.target)]
    assert calls == ["umfa.kvcache_fp8_forward_append"], calls
    assert torch.equal(oc, oe)
    assert torch.equal(kc.view(torch.uint8), kc_e.view(torch.uint8)) and torch.equal(vc.view(torch.uint8), vc_e.view(torch.uint8))


def test_refused_arguments():
    um = _umfa()
    q, kc, vc, bt, _, _ = _paged(2, 1, 8, 2, 128, 16, 4, torch.bfloat16, seed=21)
    kd = _dev([0.5, 2.0])
    call = lambda k_, v_, **kw: um.kvcache_attention(q, k_, v_, cache_seqlens=10, block_table=bt, **kw)  # noqa: E731
    raw = kc.view(torch.uint8)
    for k_, v_ in ((raw.view(torch.float8_e4m3fnuz), raw.view(torch.float8_e4m3fnuz)), (raw.view(torch.float8_e5m2), raw.view(torch.float8_e5m2)),
                   (raw, raw), (kc, vc.to(torch.bfloat16)), (kc.to(torch.bfloat16), vc)):  # other 8-bit formats; mixed K / V formats
        with pytest.raises(ValueError):
            call(k_, v_)
    for bad in (kd.double(), kd.cpu(), _dev([1.0, 2.0, 3.0]), _dev(np.ones((3, 2))), _dev(np.ones((2, 2, 1))), kd.to(torch.bfloat16), "1.0"):
        with pytest.raises(ValueError):  # descales of the wrong dtype / device / shape
            call(kc, vc, k_descale=bad)
        with pytest.raises(ValueError):
            call(kc, vc, v_descale=bad)
    with pytest.raises(ValueError):  # descales with a 16-bit cache
        call(kc.to(torch.bfloat16), vc.to(torch.bfloat16), k_descale=kd)
    with pytest.raises(ValueError):
        call(kc.to(torch.bfloat16), vc.to(torch.bfloat16), v_descale=1.0)
    with pytest.raises(ValueError):  # head_dim 96
        um.kvcache_attention(q[..., :96].contiguous(), kc[..., :96].contiguous(), vc[..., :96].contiguous(), cache_seqlens=10, block_table=bt)
    with pytest.raises(ValueError):  # a paged cache whose page_size is not a multiple of 16
        call(kc[:, :8].contiguous(), vc[:, :8].contiguous())
    with pytest.raises(ValueError):  # a token stride that is not a multiple of 16 bytes
        pool = torch.zeros(kc.shape[0], 16, 2, 136, device="cuda", dtype=torch.uint8).view(F8)
        call(pool[..., :128], pool[..., :128])
    with pytest.raises(ValueError):  # fp32 q
        um.kvcache_attention(q.float(), kc, vc, cache_seqlens=10, block_table=bt)
    for kw in (dict(window_size=(8, 0)), dict(softcap=30.0), dict(rotary_cos=torch.zeros(1))):
        with pytest.raises(ValueError):
            call(kc, vc, **kw)
    with pytest.raises(ValueError):  # the ops entry refuses the same formats: there is no fall-back
        um.ops.kvcache_attention_fp8_forward(q, kc.to(torch.bfloat16), vc.to(torch.bfloat16), _seqlens([1, 1]), kd, kd, bt, scale=0.1)
    o = call(kc, vc, k_descale=kd, v_descale=0.5)
    torch.cuda.synchronize()
    assert o.shape == q.shape and um.last_kernel().startswith("fa_fwd16_paged_fp8<bf16,128")
    qg = q.clone().requires_grad_(True)
    o = um.kvcache_attention(qg, kc, vc, cache_seqlens=10, block_table=bt)
    with pytest.raises(RuntimeError):  # inference only: no backward
        o.float().sum().backward()
