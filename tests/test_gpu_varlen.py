"""Packed variable-length attention on the GPU (umfa_torch.varlen_attention): values per sequence against the
fp64 reference and the format floors (tests/tolerances.py), LSE, the backward, rows that see no key, no writes past T_q, agreement with
the dense path, bitwise repeatability, graph replay with rewritten offsets, opcheck / torch.compile, and torch's own varlen_attn."""
import numpy as np
import pytest
import torch

import tolerances as tol
import varlen_ref as ref
from oracle import oracle

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
LENS_Q = (1, 31, 127, 128, 129, 1000, 0, 64)
LENS_K = (1, 40, 100, 128, 300, 1000, 5, 0)  # L_q > L_k, L_q < L_k, L_q == L_k, an empty side


def _umfa():
    import umfa_torch
    return umfa_torch


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")


def _case(lens_q, lens_k, H, Hkv, D, dt, seed, packed=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    Tq, Tk = int(sum(lens_q)), int(sum(lens_k))
    if packed:  # q, k, v as views of one [T, 3, H, D] projection (self-attention: equal lengths, equal head counts)
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


def _check_forward(q, k, v, cu_q, cu_k, causal, out, lse, kernel, out_dt=None, scale=None):
    D = q.shape[-1]
    scale = D ** -0.5 if scale is None else scale
    o_ref, lse_ref = ref.forward(_np(q), _np(k), _np(v), cu_q.cpu().numpy(), cu_k.cpu().numpy(), causal, scale)
    o, l = _np(out), _np(lse)
    assert np.isfinite(o).all()
    for q0, Lq, k0, Lk in ref.seqs(cu_q.cpu().numpy(), cu_k.cpu().numpy()):
        if Lq == 0:
            continue
        live = ref.visible(Lq, Lk, causal).any(1)
        rows = np.arange(q0, q0 + Lq)
        # rows that see no key: O = 0 exactly, LSE = -inf
        assert (o[rows[~live]] == 0).all() and np.isneginf(l[:, rows[~live]]).all(), (q0, Lq, Lk)
        if not live.any():
            continue
        # LSE against fp64 (exact scores of the rounded inputs; the kernel's fp32 sums)
        np.testing.assert_allclose(l[:, rows[live]], lse_ref[:, rows[live]], rtol=0, atol=2e-3)
        got = o[rows[live]].transpose(1, 0, 2)[None]
        want = o_ref[rows[live]].transpose(1, 0, 2)[None]
        qs, ks, vs = q[q0:q0 + Lq], k[k0:k0 + Lk], v[k0:k0 + Lk]
        kv_h = torch.repeat_interleave  # the floor takes equal head counts: expand the grouped K / V heads
        G = q.shape[1] // k.shape[1]
        ks, vs = kv_h(ks, G, 1), kv_h(vs, G, 1)
        if causal:
            # bottom-right causal as the floor's top-left form: live row i sits at index i + (Lk - Lq) of a zero-padded Q of Lk rows
            off = Lk - Lq
            qpad = torch.zeros(Lk, qs.shape[1], D, dtype=qs.dtype, device=qs.device)
            li = np.nonzero(live)[0]
            qpad[li + off] = qs[li]
            inputs, frows = (_oracle_in(qpad), _oracle_in(ks), _oracle_in(vs)), li + off
        else:
            inputs, frows = (_oracle_in(qs), _oracle_in(ks), _oracle_in(vs)), None
        tol.check_forward(got, want, q.dtype, kernel, tag=f"varlen Lq={Lq} Lk={Lk}", out_dt=out_dt,
                          inputs=inputs if out_dt is None else None, rows=frows, causal=causal, scale=scale)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("out_f32", [True, False])
def test_forward_values(dt, D, causal, out_f32):
    um = _umfa()
    q, k, v, cu_q, cu_k = _case(LENS_Q, LENS_K, 4, 2, D, DT[dt], seed=D + causal)
    out, lse = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, max(LENS_Q), max(LENS_K), scale=D ** -0.5, causal=causal,
                                               out_dtype=torch.float32 if out_f32 else None)
    torch.cuda.synchronize()
    kern = um.last_kernel()
    assert kern.startswith("fa_fwd16_varlen<") and ("causal" in kern) == causal, kern
    _check_forward(q, k, v, cu_q, cu_k, causal, out, lse, kern, out_dt=None if out_f32 else DT[dt])


@pytest.mark.parametrize("g", [1, 2, 4, 8])
def test_forward_gqa(g):
    um = _umfa()
    lens = (129, 1, 300, 64)
    q, k, v, cu_q, cu_k = _case(lens, lens, 8, 8 // g, 128, torch.bfloat16, seed=40 + g)
    out, lse = um.varlen_attention(q, k, v, cu_q, cu_k, max(lens), max(lens), True, return_lse=True)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and lse.shape == (8, sum(lens))
    _check_forward(q, k, v, cu_q, cu_k, True, out, lse, um.last_kernel(), out_dt=torch.bfloat16)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_forward_strided_qkv_views(dt, D):
    """qkv[:, i] views of a [T, 3, H, D] projection go to the kernels as they are and give the contiguous call's bits"""
    um = _umfa()
    lens = (200, 0, 77, 128)
    q, k, v, cu_q, cu_k = _case(lens, lens, 4, 4, D, DT[dt], seed=7, packed=True)
    assert not q.is_contiguous() and q.stride(0) == 3 * 4 * D
    o1, l1 = um.varlen_attention(q, k, v, cu_q, cu_k, 200, 200, True, return_lse=True, scale=0.1)
    o2, l2 = um.varlen_attention(q.contiguous(), k.contiguous(), v.contiguous(), cu_q, cu_k, 200, 200, True, return_lse=True, scale=0.1)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    _check_forward(q, k, v, cu_q, cu_k, True, o1.float(), l1, um.last_kernel(), out_dt=DT[dt], scale=0.1)


def _check_backward(q, k, v, cu_q, cu_k, causal, out, lse, do, grads, kernel):
    D = q.shape[-1]
    G = q.shape[1] // k.shape[1]
    kind = "bf16" if q.dtype == torch.bfloat16 else "fp16"
    dq, dk, dv = (_np(t) for t in grads)
    lse_np = lse.detach().cpu().numpy()
    for q0, Lq, k0, Lk in ref.seqs(cu_q.cpu().numpy(), cu_k.cpu().numpy()):
        if Lq == 0 or Lk == 0:
            # nothing seen: dQ of a sequence without keys, dK / dV of one without queries are exactly zero
            assert (dq[q0:q0 + Lq] == 0).all() and (dk[k0:k0 + Lk] == 0).all() and (dv[k0:k0 + Lk] == 0).all()
            continue
        vis = ref.visible(Lq, Lk, causal)
        term = np.where(vis, 0.0, -np.inf)[None, None] if causal else None
        sl = slice(q0, q0 + Lq)
        fl = oracle.flash_backward_format_floor(
            _oracle_in(do[sl]), _oracle_in(q[sl]), _oracle_in(k[k0:k0 + Lk]), _oracle_in(v[k0:k0 + Lk]),
            _np(out[sl]).transpose(1, 0, 2)[None], lse_np[:, sl][None], kind, scale=D ** -0.5, term=term, kv_group=G)
        got = (dq[sl].transpose(1, 0, 2)[None], dk[k0:k0 + Lk].transpose(1, 0, 2)[None], dv[k0:k0 + Lk].transpose(1, 0, 2)[None])
        tol.check_backward(got, fl, q.dtype, tag=f"varlen bwd Lq={Lq} Lk={Lk}", kernel=kernel, grad_dt=q.dtype)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_backward_values(dt, D, causal):
    um = _umfa()
    lens_q, lens_k = (1, 31, 129, 0, 300, 64), (1, 40, 100, 7, 300, 0)
    q, k, v, cu_q, cu_k = _case(lens_q, lens_k, 4, 2, D, DT[dt], seed=100 + D + causal)
    do = torch.randn_like(q)
    out, lse = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, 300, 300, scale=D ** -0.5, causal=causal)
    grads = um.ops.varlen_attention_backward(do, q, k, v, out, lse, cu_q, cu_k, 300, 300, scale=D ** -0.5, causal=causal)
    torch.cuda.synchronize()
    kern = um.last_kernel()
    assert kern.startswith("bwd16_dq+dkdv_varlen<"), kern
    _check_backward(q, k, v, cu_q, cu_k, causal, out, lse, do, grads, kern)


@pytest.mark.parametrize("g", [1, 4, 8])
def test_backward_gqa(g):
    um = _umfa()
    lens_q, lens_k = (129, 64, 200), (129, 300, 150)
    q, k, v, cu_q, cu_k = _case(lens_q, lens_k, 8, 8 // g, 128, torch.bfloat16, seed=200 + g)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    do = torch.randn_like(q)
    out, lse = um.varlen_attention(qg, kg, vg, cu_q, cu_k, 200, 300, True, return_lse=True)
    grads = torch.autograd.grad(out, (qg, kg, vg), do)
    torch.cuda.synchronize()
    _check_backward(q, k, v, cu_q, cu_k, True, out, lse, do, grads, um.last_kernel())


def test_rows_without_keys_are_exact_zeros():
    um = _umfa()
    lens_q, lens_k = (64, 200, 50), (0, 50, 50)  # no keys at all; causal with L_q > L_k (rows 0 .. 149 see nothing)
    q, k, v, cu_q, cu_k = _case(lens_q, lens_k, 2, 2, 128, torch.bfloat16, seed=9)
    qg = q.clone().requires_grad_(True)
    out, lse = um.varlen_attention(qg, k, v, cu_q, cu_k, 200, 50, True, return_lse=True)
    (dq,) = torch.autograd.grad(out, (qg,), torch.randn_like(out))
    torch.cuda.synchronize()
    dead = np.r_[0:64, 64:214]
    assert (out[dead] == 0).all() and torch.isneginf(lse[:, dead]).all() and (dq[dead] == 0).all()
    assert torch.isfinite(out).all() and torch.isfinite(dq).all()
    # (row 214 sees one key: O = V there and its dQ cancels to rounding noise)
    assert (out[214:264].abs().amax(-1) > 0).all() and (dq[215:264].abs().amax(-1) > 0).all()


@pytest.mark.parametrize("causal", [False, True])
def test_no_writes_past_t_q(causal):
    um = _umfa()
    lens = (129, 3, 256)
    q, k, v, cu_q, cu_k = _case(lens, lens, 4, 4, 64, torch.float16, seed=3)
    T = sum(lens)
    buf = torch.full((T + 64, 4, 64), 1234.5, dtype=torch.float32, device="cuda")
    um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, 256, 256, scale=0.125, causal=causal, out=buf[:T])
    torch.cuda.synchronize()
    assert (buf[T:] == 1234.5).all()
    assert not (buf[:T] == 1234.5).any()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_equal_lengths_agree_with_dense_path(causal, dt):
    um = _umfa()
    N, L, H, D = 3, 384, 4, 128
    q, k, v, cu_q, cu_k = _case((L,) * N, (L,) * N, H, H, D, DT[dt], seed=21)
    o, _ = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, L, L, scale=D ** -0.5, causal=causal, out_dtype=torch.float32)
    dense = lambda t: t.view(N, L, H, D).transpose(1, 2).contiguous()  # noqa: E731
    od = um.attention_forward(dense(q), dense(k), dense(v), causal=causal, out_dtype=torch.float32)
    torch.cuda.synchronize()
    a = _np(o.view(N, L, H, D).transpose(1, 2))
    b = _np(od)
    ulp = tol.ULP_AT_ONE["fp16"]  # both P V products in fp16
    assert np.abs(a - b).max() <= 2 * ulp * np.abs(b).max(), np.abs(a - b).max()


def test_bitwise_repeatable():
    um = _umfa()
    q, k, v, cu_q, cu_k = _case(LENS_Q, LENS_K, 8, 2, 128, torch.bfloat16, seed=5)
    do = torch.randn_like(q)
    res = []
    for _ in range(2):
        out, lse = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, 1000, 1000, scale=0.088, causal=True)
        res.append((out, lse) + um.ops.varlen_attention_backward(do, q, k, v, out, lse, cu_q, cu_k, 1000, 1000, scale=0.088, causal=True))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_graph_replay_follows_rewritten_offsets():
    um = _umfa()
    H, D, T = 4, 64, 600
    lens_a, lens_b = (100, 300, 200), (250, 50, 300)  # same N, same max
    q, k, v, cu_q, cu_k = _case(lens_a, lens_a, H, H, D, torch.bfloat16, seed=8)
    do = torch.randn_like(q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def step():
        out, lse = um.ops.varlen_attention_forward(q, k, v, cu_q, cu_k, 300, 300, scale=0.125, causal=True)
        return (out, lse) + um.ops.varlen_attention_backward(do, q, k, v, out, lse, cu_q, cu_k, 300, 300, scale=0.125, causal=True)

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
    # the replayed values are the new offsets' attention (not the captured ones')
    o_ref, _ = ref.forward(_np(q), _np(k), _np(v), _cu(lens_a).cpu().numpy(), _cu(lens_a).cpu().numpy(), True, 0.125)
    assert np.abs(_np(res[0]) - o_ref).max() <= 4e-3 * np.abs(o_ref).max()
    o_b, _ = ref.forward(_np(q), _np(k), _np(v), _cu(lens_b).cpu().numpy(), _cu(lens_b).cpu().numpy(), True, 0.125)
    assert np.abs(o_b - o_ref).max() > 0.1 * np.abs(o_ref).max()  # (the two offset sets give different attention)


def test_opcheck_custom_ops():
    _umfa()
    lens = (70, 0, 129)
    q, k, v, cu_q, cu_k = _case(lens, lens, 4, 2, 64, torch.bfloat16, seed=2)
    torch.library.opcheck(torch.ops.umfa.varlen_forward.default, (q, k, v, cu_q, cu_k, 129, 129, True, 0.125))
    o, lse = torch.ops.umfa.varlen_forward(q, k, v, cu_q, cu_k, 129, 129, True, 0.125)
    do = torch.randn_like(o)
    torch.library.opcheck(torch.ops.umfa.varlen_backward.default, (do, q, k, v, o, lse, cu_q, cu_k, 129, 129, True, 0.125))


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
        return um.varlen_attention(q, k, v, cu_q, cu_k, 256, 256, is_causal=True)

    torch._dynamo.reset()
    oc = torch.compile(f, fullgraph=True, backend=backend)(qg, kg, vg)
    oc.float().sum().backward()
    oe = f(q, k, v)
    torch.cuda.synchronize()
    assert len(graphs) == 1
    calls = [n for n in graphs[0].graph.nodes if n.op == "call_function"]
    assert [str(n.target) for n in calls if "umfa" in str(n.target)] == ["umfa.varlen_forward"], [str(n.target) for n in calls]
    assert torch.equal(oc, oe)
    assert all(torch.isfinite(t.grad).all() for t in (qg, kg, vg))


def test_against_torch_varlen_attn():
    um = _umfa()
    from torch.nn.attention.varlen import AuxRequest, varlen_attn
    lens_q = lens_k = (129, 1, 300, 64)
    q, k, v, cu_q, cu_k = _case(lens_q, lens_k, 4, 4, 128, torch.bfloat16, seed=12)
    try:
        o_t, l_t = varlen_attn(q, k, v, cu_q, cu_k, 300, 300, True, return_aux=AuxRequest(lse=True))
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001  (torch's kernel is not built for every ROCm target)
        pytest.skip(f"torch's varlen_attn does not run on this build: {type(e).__name__}: {e}")
    o, l = um.varlen_attention(q, k, v, cu_q, cu_k, 300, 300, True, return_lse=True)
    torch.cuda.synchronize()
    assert o.shape == o_t.shape and o.dtype == o_t.dtype
    assert (o.float() - o_t.float()).abs().max() <= 2e-2 * o_t.float().abs().max()
    if l_t.shape == l.shape:
        assert (l - l_t.float()).abs().max() <= 1e-2
