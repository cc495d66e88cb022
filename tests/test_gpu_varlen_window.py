"""Sliding-window packed variable-length attention on the GPU (umfa_torch.varlen_attention(window_size=...)):
values per sequence against the fp64 reference (tests/varlen_window_ref.py) and the format bounds of tests/tolerances.py, LSE, the
backward, exact zeros for rows that see no key and keys no row sees, agreement with the dense sliding window, routing of windows that
bound nothing to the unwindowed kernels bit for bit, strided views, no writes past T_q, repeatability, graph replay with rewritten
offsets, opcheck / torch.compile, and the refusal of values below -1."""
import numpy as np
import pytest
import torch

import tolerances as tol
import varlen_window_ref as ref
from oracle import oracle

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
# lengths that cross 32-key tiles and 128-row blocks, L_q > L_k and L_q < L_k, equal, and empty sides
LENS_Q = (1, 31, 127, 128, 129, 300, 0, 64, 200)
LENS_K = (1, 40, 100, 128, 300, 129, 5, 0, 200)
WINDOWS = [(0, 0), (1, 0), (31, 0), (32, 0), (100, 17), (-1, 40), (40, -1), (127, 128)]


def _umfa():
    import umfa_torch
    return umfa_torch


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")


def _case(lens_q, lens_k, H, Hkv, D, dt, seed, packed=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    Tq, Tk = int(sum(lens_q)), int(sum(lens_k))
    if packed:  # q, k, v as views of one [T, 3, H, D] projection
        qkv = torch.randn(Tq, 3, H, D, device="cuda", dtype=dt, generator=g)
        return qkv[:, 0], qkv[:, 1], qkv[:, 2], _cu(lens_q), _cu(lens_k)
    q = torch.randn(Tq, H, D, device="cuda", dtype=dt, generator=g)
    k = torch.randn(Tk, Hkv, D, device="cuda", dtype=dt, generator=g)
    v = torch.randn(Tk, Hkv, D, device="cuda", dtype=dt, generator=g)
    return q, k, v, _cu(lens_q), _cu(lens_k)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _oracle_in(t):
    """[L, H, D] -> [1, H, L, D] as the oracle takes it (bf16 as uint16 bits)"""
    t = t.detach().transpose(0, 1).contiguous()[None].cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def _check_forward(q, k, v, cu_q, cu_k, causal, window, out, lse, kernel, out_dt=None, scale=None):
    D = q.shape[-1]
    scale = D ** -0.5 if scale is None else scale
    cq, ck = cu_q.cpu().numpy(), cu_k.cpu().numpy()
    o_ref, lse_ref = ref.forward(_np(q), _np(k), _np(v), cq, ck, causal, window, scale)
    o, l = _np(out), _np(lse)
    assert np.isfinite(o).all()
    for q0, Lq, k0, Lk in ref.seqs(cq, ck):
        if Lq == 0:
            continue
        live = ref.visible(Lq, Lk, causal, window).any(1)
        rows = np.arange(q0, q0 + Lq)
        # rows that see no key: O = 0 exactly, LSE = -inf
        assert (o[rows[~live]] == 0).all() and np.isneginf(l[:, rows[~live]]).all(), (q0, Lq, Lk, window)
        if not live.any():
            continue
        np.testing.assert_allclose(l[:, rows[live]], lse_ref[:, rows[live]], rtol=0, atol=2e-3)
        got = o[rows[live]].transpose(1, 0, 2)[None]
        want = o_ref[rows[live]].transpose(1, 0, 2)[None]
        tol.check_forward(got, want, q.dtype, kernel, tag=f"varlen window {window} Lq={Lq} Lk={Lk}", out_dt=out_dt)


def _check_backward(q, k, v, cu_q, cu_k, causal, window, out, lse, do, grads, kernel):
    D = q.shape[-1]
    G = q.shape[1] // k.shape[1]
    kind = "bf16" if q.dtype == torch.bfloat16 else "fp16"
    dq, dk, dv = (_np(t) for t in grads)
    lse_np = lse.detach().cpu().numpy()
    for q0, Lq, k0, Lk in ref.seqs(cu_q.cpu().numpy(), cu_k.cpu().numpy()):
        vis = ref.visible(Lq, Lk, causal, window)
        # rows that see no key: dQ = 0 exactly; keys no row sees: dK = dV = 0 exactly
        dead_q, dead_k = q0 + np.nonzero(~vis.any(1))[0], k0 + np.nonzero(~vis.any(0))[0]
        assert (dq[dead_q] == 0).all() and (dk[dead_k] == 0).all() and (dv[dead_k] == 0).all(), (Lq, Lk, window)
        if not vis.any():
            continue
        sl = slice(q0, q0 + Lq)
        fl = oracle.flash_backward_format_floor(
            _oracle_in(do[sl]), _oracle_in(q[sl]), _oracle_in(k[k0:k0 + Lk]), _oracle_in(v[k0:k0 + Lk]),
            _np(out[sl]).transpose(1, 0, 2)[None], lse_np[:, sl][None], kind, scale=D ** -0.5,
            term=np.where(vis, 0.0, -np.inf)[None, None], kv_group=G)
        got = (dq[sl].transpose(1, 0, 2)[None], dk[k0:k0 + Lk].transpose(1, 0, 2)[None], dv[k0:k0 + Lk].transpose(1, 0, 2)[None])
        tol.check_backward(got, fl, q.dtype, tag=f"varlen window bwd {window} Lq={Lq} Lk={Lk}", kernel=kernel, grad_dt=q.dtype)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("window", WINDOWS)
def test_forward_windows(window, causal):
    um = _umfa()
    q, k, v, cu_q, cu_k = _case(LENS_Q, LENS_K, 4, 2, 128, torch.bfloat16, seed=3 + causal)
    out, lse = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, max(LENS_Q), max(LENS_K), scale=128 ** -0.5, causal=causal,
                                               out_dtype=torch.float32, window=window)
    torch.cuda.synchronize()
    kern = um.last_kernel()
    banded = not (window[0] == -1 and (causal or window[1] == 0))  # ((-1, x) with causal is bottom-right causal: the unwindowed kernel)
    assert kern.startswith("fa_fwd16_varlen_window<" if banded else "fa_fwd16_varlen<"), kern
    _check_forward(q, k, v, cu_q, cu_k, causal, window, out, lse, kern)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("out_f32", [True, False])
def test_forward_types(dt, D, out_f32):
    um = _umfa()
    q, k, v, cu_q, cu_k = _case(LENS_Q, LENS_K, 4, 4, D, DT[dt], seed=D + out_f32)
    for causal, window in ((False, (100, 17)), (True, (31, -1))):
        out, lse = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, max(LENS_Q), max(LENS_K), scale=D ** -0.5, causal=causal,
                                                   out_dtype=torch.float32 if out_f32 else None, window=window)
        torch.cuda.synchronize()
        kern = um.last_kernel()
        assert kern.startswith("fa_fwd16_varlen_window<") and f",{D}" in kern, kern
        _check_forward(q, k, v, cu_q, cu_k, causal, window, out, lse, kern, out_dt=None if out_f32 else DT[dt])


@pytest.mark.parametrize("g", [1, 2, 4, 8])
def test_forward_gqa(g):
    um = _umfa()
    lens = (129, 1, 300, 64)
    q, k, v, cu_q, cu_k = _case(lens, lens, 8, 8 // g, 128, torch.bfloat16, seed=40 + g)
    out, lse = um.varlen_attention(q, k, v, cu_q, cu_k, max(lens), max(lens), True, return_lse=True, window_size=(50, -1))
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and lse.shape == (8, sum(lens))
    _check_forward(q, k, v, cu_q, cu_k, True, (50, 0), out, lse, um.last_kernel(), out_dt=torch.bfloat16)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("window", WINDOWS)
def test_backward_windows(window, causal):
    um = _umfa()
    lens_q, lens_k = (1, 31, 129, 0, 200, 64, 100), (1, 40, 100, 7, 200, 0, 260)
    q, k, v, cu_q, cu_k = _case(lens_q, lens_k, 4, 2, 64, torch.float16, seed=100 + causal)
    do = torch.randn_like(q)
    kw = dict(scale=64 ** -0.5, causal=causal, window=window)
    out, lse = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, 200, 260, **kw)
    grads = um.ops.varlen_attention_backward(do, q, k, v, out, lse, cu_q, cu_k, 200, 260, **kw)
    torch.cuda.synchronize()
    kern = um.last_kernel()
    banded = not (window[0] == -1 and (causal or window[1] == 0))
    assert kern.startswith("bwd16_dq+dkdv_varlen_window<" if banded else "bwd16_dq+dkdv_varlen<"), kern
    _check_backward(q, k, v, cu_q, cu_k, causal, window, out, lse, do, grads, kern)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_backward_types(dt, D):
    um = _umfa()
    lens_q, lens_k = (129, 300, 31), (100, 300, 64)
    q, k, v, cu_q, cu_k = _case(lens_q, lens_k, 4, 2, D, DT[dt], seed=300 + D)
    do = torch.randn_like(q)
    kw = dict(scale=D ** -0.5, causal=False, window=(100, 17))
    out, lse = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, 300, 300, **kw)
    grads = um.ops.varlen_attention_backward(do, q, k, v, out, lse, cu_q, cu_k, 300, 300, **kw)
    torch.cuda.synchronize()
    _check_backward(q, k, v, cu_q, cu_k, False, (100, 17), out, lse, do, grads, um.last_kernel())


@pytest.mark.parametrize("g", [1, 2, 4, 8])
def test_backward_gqa_autograd(g):
    um = _umfa()
    lens_q, lens_k = (129, 64, 200), (129, 300, 150)
    q, k, v, cu_q, cu_k = _case(lens_q, lens_k, 8, 8 // g, 128, torch.bfloat16, seed=200 + g)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    do = torch.randn_like(q)
    out, lse = um.varlen_attention(qg, kg, vg, cu_q, cu_k, 200, 300, True, return_lse=True, window_size=(40, -1))
    grads = torch.autograd.grad(out, (qg, kg, vg), do)
    torch.cuda.synchronize()
    assert um.last_kernel().startswith("bwd16_dq+dkdv_varlen_window<"), um.last_kernel()
    _check_backward(q, k, v, cu_q, cu_k, True, (40, 0), out, lse, do, grads, um.last_kernel())


def test_exact_zeros_outside_the_band():
    """rows with no key in their band: O = 0, LSE = -inf, dQ = 0 exactly; keys in no row's band: dK = dV = 0 exactly"""
    um = _umfa()
    # seq 0: L_q 200 > L_k 50 with causal and left 10 -> rows 0 .. 149 see nothing; seq 1: window (0, 0) with L_q 40 < L_k 300 ->
    # keys 0 .. 259 are in no row's band; seq 2: no keys
    lens_q, lens_k = (200, 40, 64), (50, 300, 0)
    q, k, v, cu_q, cu_k = _case(lens_q, lens_k, 2, 2, 128, torch.bfloat16, seed=9)
    for causal, window in ((True, (10, -1)), (False, (0, 0))):
        qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
        out, lse = um.varlen_attention(qg, kg, vg, cu_q, cu_k, 200, 300, causal, return_lse=True, window_size=window)
        dq, dk, dv = torch.autograd.grad(out, (qg, kg, vg), torch.randn_like(out))
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in (out, dq, dk, dv))
        dead = np.r_[0:150, 240:304]
        assert (out[dead] == 0).all() and torch.isneginf(lse[:, dead]).all() and (dq[dead] == 0).all()
        assert (out[150:240].abs().amax(-1) > 0).all()
        if not causal:
            assert (dk[50:310] == 0).all() and (dv[50:310] == 0).all()
            assert (dv[310:350].abs().amax(-1) > 0).all()  # (one key per row: P = 1, so dV = dO there and dK cancels)


@pytest.mark.parametrize("window", [(0, 0), (31, 0), (100, 17), (-1, 40), (127, 128)])
def test_equal_lengths_agree_with_dense_sliding_window(window):
    um = _umfa()
    N, L, H, D = 3, 384, 4, 128
    q, k, v, cu_q, cu_k = _case((L,) * N, (L,) * N, H, H, D, torch.float16, seed=21)
    o, _ = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, L, L, scale=D ** -0.5, out_dtype=torch.float32, window=window)
    dense = lambda t: t.view(N, L, H, D).transpose(1, 2).contiguous()  # noqa: E731
    od = um.sliding_window_attention(dense(q), dense(k), dense(v), window=tuple(L if w < 0 else w for w in window))
    torch.cuda.synchronize()
    a, b = _np(o.view(N, L, H, D).transpose(1, 2)), _np(od)
    ulp = tol.ULP_AT_ONE["fp16"]
    assert np.abs(a - b).max() <= 4 * ulp * np.abs(b).max(), np.abs(a - b).max()


@pytest.mark.parametrize("causal,window", [(False, (-1, -1)), (False, (300, 1000)), (True, (-1, -1)), (True, (2 ** 31 - 1, 0)),
                                           (True, (300, 5)), (False, (-1, 0))])
def test_unbounded_windows_take_the_unwindowed_kernels_bitwise(causal, window):
    um = _umfa()
    q, k, v, cu_q, cu_k = _case(LENS_Q, LENS_K, 4, 2, 128, torch.bfloat16, seed=31)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    do = torch.randn_like(q)
    as_causal = causal or window == (-1, 0)
    o1, l1 = um.varlen_attention(qg, kg, vg, cu_q, cu_k, 300, 300, causal, return_lse=True, window_size=window)
    torch.cuda.synchronize()
    assert um.last_kernel().startswith("fa_fwd16_varlen<") and ("causal" in um.last_kernel()) == as_causal, um.last_kernel()
    g1 = torch.autograd.grad(o1, (qg, kg, vg), do)
    torch.cuda.synchronize()
    assert um.last_kernel().startswith("bwd16_dq+dkdv_varlen<"), um.last_kernel()
    o2, l2 = um.varlen_attention(qg, kg, vg, cu_q, cu_k, 300, 300, as_causal, return_lse=True)
    g2 = torch.autograd.grad(o2, (qg, kg, vg), do)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    # a real band reaches the window kernels
    um.varlen_attention(q, k, v, cu_q, cu_k, 300, 300, causal, window_size=(299, 5))
    torch.cuda.synchronize()
    assert um.last_kernel().startswith("fa_fwd16_varlen_window<"), um.last_kernel()


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_strided_qkv_views(dt):
    um = _umfa()
    lens = (200, 0, 77, 128)
    q, k, v, cu_q, cu_k = _case(lens, lens, 4, 4, 64, DT[dt], seed=7, packed=True)
    assert not q.is_contiguous()
    kw = dict(return_lse=True, scale=0.1, window_size=(33, 4))
    o1, l1 = um.varlen_attention(q, k, v, cu_q, cu_k, 200, 200, False, **kw)
    o2, l2 = um.varlen_attention(q.contiguous(), k.contiguous(), v.contiguous(), cu_q, cu_k, 200, 200, False, **kw)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    _check_forward(q, k, v, cu_q, cu_k, False, (33, 4), o1.float(), l1, um.last_kernel(), out_dt=DT[dt], scale=0.1)


def test_no_writes_past_t_q():
    um = _umfa()
    lens = (129, 3, 256)
    q, k, v, cu_q, cu_k = _case(lens, lens, 4, 4, 64, torch.float16, seed=3)
    T = sum(lens)
    buf = torch.full((T + 64, 4, 64), 1234.5, dtype=torch.float32, device="cuda")
    um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, 256, 256, scale=0.125, causal=True, out=buf[:T], window=(20, -1))
    torch.cuda.synchronize()
    assert (buf[T:] == 1234.5).all()
    assert not (buf[:T] == 1234.5).any()


def test_bitwise_repeatable():
    um = _umfa()
    q, k, v, cu_q, cu_k = _case(LENS_Q, LENS_K, 8, 2, 128, torch.bfloat16, seed=5)
    do = torch.randn_like(q)
    kw = dict(scale=0.088, causal=False, window=(64, 64))
    res = []
    for _ in range(2):
        out, lse = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, 300, 300, **kw)
        res.append((out, lse) + um.ops.varlen_attention_backward(do, q, k, v, out, lse, cu_q, cu_k, 300, 300, **kw))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_graph_replay_follows_rewritten_offsets():
    um = _umfa()
    H, D = 4, 64
    lens_a, lens_b = (100, 300, 200), (250, 50, 300)  # same N, same max
    q, k, v, cu_q, cu_k = _case(lens_a, lens_a, H, H, D, torch.bfloat16, seed=8)
    do = torch.randn_like(q)
    kw = dict(scale=0.125, causal=True, window=(70, -1))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def step():
        out, lse = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, 300, 300, **kw)
        return (out, lse) + um.ops.varlen_attention_backward(do, q, k, v, out, lse, cu_q, cu_k, 300, 300, **kw)

    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up: scratch grows outside the capture
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        res = step()
    for lens in (lens_b, lens_a):
        cu_q.copy_(_cu(lens))
        cu_k.copy_(_cu(lens))
        graph.replay()
        torch.cuda.synchronize()
        want = step()
        torch.cuda.synchronize()
        for a, b in zip(res, want):
            assert torch.equal(a, b), lens
    o_ref, _ = ref.forward(_np(q), _np(k), _np(v), _cu(lens_a).cpu().numpy(), _cu(lens_a).cpu().numpy(), True, (70, -1), 0.125)
    assert np.abs(_np(res[0]) - o_ref).max() <= 4e-3 * np.abs(o_ref).max()
    o_b, _ = ref.forward(_np(q), _np(k), _np(v), _cu(lens_b).cpu().numpy(), _cu(lens_b).cpu().numpy(), True, (70, -1), 0.125)
    assert np.abs(o_b - o_ref).max() > 0.1 * np.abs(o_ref).max()


def test_opcheck_custom_ops():
    _umfa()
    lens = (70, 0, 129)
    q, k, v, cu_q, cu_k = _case(lens, lens, 4, 2, 64, torch.bfloat16, seed=2)
    torch.library.opcheck(torch.ops.umfa.varlen_window_forward.default, (q, k, v, cu_q, cu_k, 129, 129, True, 0.125, 20, 0))
    o, lse = torch.ops.umfa.varlen_window_forward(q, k, v, cu_q, cu_k, 129, 129, True, 0.125, 20, 0)
    do = torch.randn_like(o)
    torch.library.opcheck(torch.ops.umfa.varlen_window_backward.default, (do, q, k, v, o, lse, cu_q, cu_k, 129, 129, True, 0.125, 20, 0))


def test_compile_fullgraph_single_node():
    um = _umfa()
    lens = (100, 28, 256)
    q, k, v, cu_q, cu_k = _case(lens, lens, 4, 4, 128, torch.float16, seed=4)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    def f(q, k, v):
        return um.varlen_attention(q, k, v, cu_q, cu_k, 256, 256, is_causal=True, window_size=(63, -1))

    torch._dynamo.reset()
    oc = torch.compile(f, fullgraph=True, backend=backend)(qg, kg, vg)
    oc.float().sum().backward()
    oe = f(q, k, v)
    torch.cuda.synchronize()
    assert len(graphs) == 1
    calls = [n for n in graphs[0].graph.nodes if n.op == "call_function"]
    assert [str(n.target) for n in calls if "umfa" in str(n.target)] == ["umfa.varlen_window_forward"], [str(n.target) for n in calls]
    assert torch.equal(oc, oe)
    assert all(torch.isfinite(t.grad).all() for t in (qg, kg, vg))


@pytest.mark.parametrize("window", [(-2, 0), (0, -2), (-5, -5)])
def test_values_below_minus_one_are_refused(window):
    um = _umfa()
    q, k, v, cu_q, cu_k = _case((16,), (16,), 2, 2, 64, torch.float16, seed=1)
    with pytest.raises(ValueError):
        um.varlen_attention(q, k, v, cu_q, cu_k, 16, 16, window_size=window)
    with pytest.raises(Exception, match="Invalid arguments"):  # the C entry refuses them too (MFA_ERROR_INVALID_ARGS)
        um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, 16, 16, scale=0.125, window=window)
