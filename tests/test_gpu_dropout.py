"""Attention dropout on the MI355X: the keep mask of every kernel read back bitwise against the materialiser (and the materialiser against
the numpy restatement), values against fp64 with the materialised mask and the dropout-aware format floor, statistics, repeatability and
the torch integration (generator, graph capture, custom ops, routing option)."""
import math

import numpy as np
import pytest
import torch

import dropout_ref as ref
import tolerances as tol

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
SEQS = (1, 31, 130, 257, 1000)


def _umfa():
    import umfa_torch
    return umfa_torch


def _rs(seed, offset):
    return torch.tensor([seed, offset], dtype=torch.int64, device="cuda")


def _keep(B, H, Sq, Skv, p, rs):
    return _umfa().ops.dropout_keep_mask(B, H, Sq, Skv, p, rs).cpu().numpy().astype(bool)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ materialiser
@pytest.mark.parametrize("B,H,Sq,Skv", [(1, 1, 1, 1), (2, 3, 31, 130), (1, 2, 257, 1000), (2, 1, 1000, 33)])
@pytest.mark.parametrize("seed,offset", [(0, 0), (123456789, 5), (-(2 ** 62) + 11, 2 ** 40 + 1)])
def test_materialiser_matches_restatement(B, H, Sq, Skv, seed, offset):
    for p in (0.1, 0.5, 0.9):
        got = _keep(B, H, Sq, Skv, p, _rs(seed, offset))
        want = ref.keep_mask(B, H, Sq, Skv, p, seed, offset)
        assert np.array_equal(got, want), (B, H, Sq, Skv, p, int((got != want).sum()))


# ------------------------------------------------------------------------------------------------ mask read-back through the kernels
def _onehot(H, S, D, t):
    """[1, H, S, D]: row h D + d of head h is e_d (rows past S: none)"""
    a = np.zeros((1, H, S, D), np.float32)
    for h in range(H):
        n = min(D, S - h * D)
        if n > 0:
            a[0, h, h * D + np.arange(n), np.arange(n)] = 1.0
    return torch.from_numpy(a).to(device="cuda", dtype=t)


def _visible(Sq, Skv, causal):
    vis = np.ones((Sq, Skv), bool)
    if causal:
        vis = np.arange(Skv)[None, :] <= np.arange(Sq)[:, None]
    return vis


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Sq", SEQS)
@pytest.mark.parametrize("Skv", SEQS)
def test_mask_readback_all_kernels(dt, D, causal, Sq, Skv):
    """forward: Q = K = 0 (P uniform over the visible keys), V one-hot over the keys [hD, hD + D) of head h -> O != 0 exactly where kept.
    dK / dV: dO one-hot over the rows [hD, hD + D) -> dV != 0 exactly where kept.  dQ: K one-hot over the keys of head h, V = dO = e0 ->
    dS > 0 where kept, < 0 where dropped (rows with both)."""
    um = _umfa()
    t = DT[dt]
    p = 0.5
    H = max(math.ceil(Sq / D), math.ceil(Skv / D))
    rs = _rs(0x5EED0000 + Sq * 7 + Skv, Sq + 3 * Skv)
    keep = _keep(1, H, Sq, Skv, p, rs)
    vis = _visible(Sq, Skv, causal)
    s = ref.keep_scale(p)
    scale = D ** -0.5
    z_q = torch.zeros(1, H, Sq, D, dtype=t, device="cuda")
    z_k = torch.zeros(1, H, Skv, D, dtype=t, device="cuda")
    v = _onehot(H, Skv, D, t)
    o, lse = um.ops.attention_forward_dropout(z_q, z_k, v, p, rs, scale=scale, causal=causal, out_dtype=torch.float32)
    assert um.last_kernel().startswith("fa_fwd16_drop"), um.last_kernel()
    o = o.cpu().numpy()
    for h in range(H):
        ks = np.arange(h * D, min(h * D + D, Skv))
        if ks.size == 0:
            continue
        got = o[0, h][:, : ks.size] != 0
        want = keep[0, h][:, ks] & vis[:, ks]
        assert np.array_equal(got, want), ("fwd", h, int((got != want).sum()))
    # dK / dV
    do = _onehot(H, Sq, D, t)
    out_t = torch.zeros(1, H, Sq, D, dtype=t, device="cuda")  # (D_i = dO . O: zero here -- dV does not read it)
    dq, dk, dv = um.ops.attention_backward_dropout(do, z_q, z_k, z_k.clone(), out_t, lse, p, rs, scale=scale, causal=causal)
    assert um.last_kernel().startswith("bwd16_dq_drop"), um.last_kernel()
    dv = dv.float().cpu().numpy()
    for h in range(H):
        rows = np.arange(h * D, min(h * D + D, Sq))
        if rows.size == 0:
            continue
        got = dv[0, h][:, : rows.size].T != 0  # [rows, keys]
        want = keep[0, h][rows, :] & vis[rows, :]
        assert np.array_equal(got, want), ("dv", h, int((got != want).sum()))
    # dQ
    kk = _onehot(H, Skv, D, t)
    e0 = torch.zeros(1, H, Skv, D, dtype=t, device="cuda")
    e0[..., 0] = 1.0
    do0 = torch.zeros(1, H, Sq, D, dtype=t, device="cuda")
    do0[..., 0] = 1.0
    # O of the forward with these operands (K one-hot, Q = 0: S = 0 still): O_i = s * sum_j keep P V_j = (s * kept fraction) e0
    n = vis.sum(1).astype(np.float64)
    frac = (keep[0] & vis[None]).sum(-1) / n[None]  # [H, Sq]
    o0 = np.zeros((1, H, Sq, D), np.float32)
    o0[0, :, :, 0] = s * frac
    o0_t = torch.from_numpy(o0).cuda()
    lse0 = torch.from_numpy(np.log(n)[None, :].repeat(H, 0).reshape(-1).astype(np.float32)).cuda()
    dq, dk, dv = um.ops.attention_backward_dropout(do0, z_q, kk, e0, o0_t, lse0, p, rs, scale=scale, causal=causal)
    dq = dq.float().cpu().numpy()
    for h in range(H):
        ks = np.arange(h * D, min(h * D + D, Skv))
        if ks.size == 0:
            continue
        kv = keep[0, h][:, ks] & vis[:, ks]
        mixed = (frac[h] > 0) & (frac[h] < 1)
        g = dq[0, h][:, : ks.size]
        sel = mixed[:, None] & vis[:, ks]
        assert np.array_equal((g > 0)[sel], kv[sel]), ("dq", h)
        assert np.all(g[~vis[:, ks]] == 0), ("dq invisible", h)


# ------------------------------------------------------------------------------------------------ values
VALUE_CASES = [  # B, H, Sq, Skv, D, causal, p
    (2, 3, 256, 256, 64, False, 0.1), (1, 4, 130, 1000, 128, False, 0.5), (2, 2, 1000, 257, 64, True, 0.9),
    (1, 2, 1024, 1024, 128, True, 0.1), (1, 1, 2048, 2048, 64, False, 0.5), (1, 1, 4096, 4096, 64, True, 0.1),
]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("B,H,Sq,Skv,D,causal,p", VALUE_CASES)
def test_values_against_fp64(dt, B, H, Sq, Skv, D, causal, p):
    um = _umfa()
    t = DT[dt]
    g = torch.Generator(device="cuda").manual_seed(Sq * 31 + Skv + D)
    q, k, v, do = (torch.randn(B, H, S, D, generator=g, device="cuda").to(t) for S in (Sq, Skv, Skv, Sq))
    rs = _rs(977 + Sq, 13 * Skv)
    scale = D ** -0.5
    keep = _keep(B, H, Sq, Skv, p, rs)
    o32, lse = um.ops.attention_forward_dropout(q, k, v, p, rs, scale=scale, causal=causal, out_dtype=torch.float32)
    o16, lse16 = um.ops.attention_forward_dropout(q, k, v, p, rs, scale=scale, causal=causal)
    ro, rl = ref.forward(_np(q), _np(k), _np(v), keep, p, scale=scale, causal=causal)
    mx = np.abs(ro).max()
    assert np.abs(o32.cpu().numpy() - ro).max() / mx <= 1e-3
    assert np.abs(_np(o16) - ro).max() / mx <= (5e-3 if dt == "bf16" else 1e-3)
    assert np.abs(lse.cpu().numpy().reshape(B, H, Sq) - rl).max() <= 1e-3 * max(1.0, np.abs(rl).max())
    assert torch.equal(lse, lse16)
    # the floor models the 16-bit backward up to its epilogue: compare the fp32 gradients, and the operand-type ones as those rounded once
    g16 = um.ops.attention_backward_dropout(do, q, k, v, o16, lse16, p, rs, scale=scale, causal=causal)
    dq, dk, dv = um.ops.attention_backward_dropout(do, q, k, v, o16, lse16, p, rs, scale=scale, causal=causal, grads_in_input_type=False)
    assert all(torch.equal(a, b.to(t)) for a, b in zip(g16, (dq, dk, dv)))
    args = (_np(do), _np(q), _np(k), _np(v), _np(o16), keep, p)
    ex = ref.backward(*args, scale=scale, causal=causal)
    fl = ref.backward(*args, scale=scale, causal=causal, kind=dt)
    rows = tol.sample_rows(Sq, B, H, seed=Sq + Skv)
    for name, got, e, f in zip(("dq", "dk", "dv"), (dq, dk, dv), ex, fl):
        got = _np(got)
        if name == "dq":
            sel = lambda a: np.take_along_axis(a, np.asarray(rows).reshape(B, H, -1, 1), 2) if np.asarray(rows).ndim == 3 else a[:, :, rows]  # noqa: E731
            got, e, f = sel(got), sel(e), sel(f)
        scale_ref = np.abs(e).max()
        err = np.abs(got - e)
        ferr = np.abs(f - e)
        assert err.max() <= tol.BWD_CEILING[dt] * scale_ref, (name, err.max() / scale_ref)
        assert err.max() <= 1.10 * ferr.max() + tol.BWD_EPS * scale_ref, (name, err.max(), ferr.max())
        rms = lambda a: float(np.sqrt(np.mean(a * a)))  # noqa: E731
        assert rms(err) <= 1.05 * rms(ferr) + tol.BWD_EPS * scale_ref, (name, rms(err), rms(ferr))


# ------------------------------------------------------------------------------------------------ statistics, repeatability
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_fraction(p):
    B, H, S = 1, 16, 1024  # 2^24 elements
    keep = _umfa().ops.dropout_keep_mask(B, H, S, S, p, _rs(42, 0)).float()
    n = keep.numel()
    sig = math.sqrt(p * (1 - p) / n)
    assert abs(keep.mean().item() - (1 - p)) <= 6 * sig
    per = keep.mean(dim=(2, 3)).flatten().cpu().numpy()
    sig_s = math.sqrt(p * (1 - p) / (S * S))
    assert np.all(np.abs(per - (1 - p)) <= 6 * sig_s), per


def test_masks_differ_by_seed_offset_head():
    um = _umfa()
    a = um.ops.dropout_keep_mask(1, 2, 64, 64, 0.5, _rs(1, 0))
    assert not torch.equal(a, um.ops.dropout_keep_mask(1, 2, 64, 64, 0.5, _rs(2, 0)))
    assert not torch.equal(a, um.ops.dropout_keep_mask(1, 2, 64, 64, 0.5, _rs(1, 1)))
    assert not torch.equal(a[0, 0], a[0, 1])


@pytest.mark.parametrize("causal", [False, True])
def test_bitwise_repeatable(causal):
    um = _umfa()
    q, k, v, do = (torch.randn(2, 4, 700, 128, device="cuda", dtype=torch.bfloat16) for _ in range(4))
    rs = _rs(7, 9)
    r1 = um.ops.attention_forward_dropout(q, k, v, 0.3, rs, scale=0.1, causal=causal)
    r2 = um.ops.attention_forward_dropout(q, k, v, 0.3, rs, scale=0.1, causal=causal)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))
    g1 = um.ops.attention_backward_dropout(do, q, k, v, r1[0], r1[1], 0.3, rs, scale=0.1, causal=causal)
    g2 = um.ops.attention_backward_dropout(do, q, k, v, r1[0], r1[1], 0.3, rs, scale=0.1, causal=causal)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_scope_is_invalid_args():
    from umfa._ffi import MFAError
    um = _umfa()
    q = torch.randn(1, 2, 64, 64, device="cuda", dtype=torch.bfloat16)
    rs = _rs(1, 2)
    with pytest.raises(MFAError):
        um.ops.attention_forward_dropout(q.float(), q.float(), q.float(), 0.1, rs, scale=0.1)
    q96 = torch.randn(1, 2, 64, 96, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(MFAError):
        um.ops.attention_forward_dropout(q96, q96, q96, 0.1, rs, scale=0.1)
    for bad in (0.0, 1.0, -0.5):
        with pytest.raises(MFAError):
            um.ops.attention_forward_dropout(q, q, q, bad, rs, scale=0.1)
    with pytest.raises(ValueError):
        um.dropout_attention(q.float(), q.float(), q.float(), 0.1)


# ------------------------------------------------------------------------------------------------ torch integration
def test_manual_seed_reproduces():
    um = _umfa()
    q, k, v = (torch.randn(2, 3, 300, 64, device="cuda", dtype=torch.float16, requires_grad=True) for _ in range(3))
    outs = []
    for _ in range(2):
        torch.manual_seed(1234)
        o = um.dropout_attention(q, k, v, 0.2, causal=True)
        o.sum().backward()
        outs.append((o.detach().clone(), q.grad.clone(), k.grad.clone(), v.grad.clone()))
        q.grad = k.grad = v.grad = None
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    torch.manual_seed(99)
    assert not torch.equal(um.dropout_attention(q, k, v, 0.2, causal=True), outs[0][0])


def test_graph_capture_rewritten_rng_state():
    um = _umfa()
    B, H, S, D, p = 1, 2, 256, 64, 0.3
    q, k, v = (torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16, requires_grad=True) for _ in range(3))
    do = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
    rs = _rs(5, 6)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up: scratch grows outside the capture
            o = um.dropout_attention(q, k, v, p, rng_state=rs)
            gq, gk, gv = torch.autograd.grad(o, (q, k, v), do)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):  # (the stream whose scratch the warm-up grew)
        o = um.dropout_attention(q, k, v, p, rng_state=rs)
        gq, gk, gv = torch.autograd.grad(o, (q, k, v), do)
    for seed, off in ((11, 0), (12, 3), (-5, 2 ** 33)):
        rs.copy_(_rs(seed, off))
        graph.replay()
        torch.cuda.synchronize()
        keep = ref.keep_mask(B, H, S, S, p, seed, off)
        ro, _ = ref.forward(_np(q), _np(k), _np(v), keep, p, scale=D ** -0.5)
        assert np.abs(_np(o) - ro).max() / np.abs(ro).max() <= 5e-3
        ex = ref.backward(_np(do), _np(q), _np(k), _np(v), _np(o), keep, p, scale=D ** -0.5)
        for got, e in zip((gq, gk, gv), ex):
            assert np.abs(_np(got) - e).max() <= tol.BWD_CEILING["bf16"] * np.abs(e).max()


def test_opcheck_custom_ops():
    _umfa()
    q, k, v, do = (torch.randn(1, 2, 128, 64, device="cuda", dtype=torch.bfloat16) for _ in range(4))
    rs = _rs(3, 4)
    torch.library.opcheck(torch.ops.umfa.sdpa_forward_dropout.default, (q, k, v, False, 0.125, 0.1, rs))
    o, lse = torch.ops.umfa.sdpa_forward_dropout(q, k, v, False, 0.125, 0.1, rs)
    torch.library.opcheck(torch.ops.umfa.sdpa_backward_dropout.default, (do, q, k, v, o, lse, False, 0.125, 0.1, rs))


def test_routing_option():
    import torch.nn.functional as F
    um = _umfa()
    q, k, v = (torch.randn(2, 4, 256, 64, device="cuda", dtype=torch.bfloat16, requires_grad=True) for _ in range(3))
    with um.options(sdpa_dropout=1):
        um.reset_dispatch_stats()
        with um.use_umfa_sdpa():
            o = F.scaled_dot_product_attention(q, k, v, dropout_p=0.1)
            assert um.last_kernel().startswith("fa_fwd16_drop"), um.last_kernel()
            o.float().pow(2).sum().backward()
            assert um.last_kernel().startswith("bwd16_dq_drop"), um.last_kernel()
            st = um.get_dispatch_stats()
            assert st["fp32_autograd"] == 1 and st["pytorch_fallback"] == 0, st
            assert all(torch.isfinite(t.grad).all() for t in (q, k, v))
            F.scaled_dot_product_attention(q.detach(), k.detach(), v.detach(), dropout_p=0.1, is_causal=True)
            assert um.get_dispatch_stats()["fp32_instream"] == 1
            # outside the scope: torch's own
            m = torch.ones(256, 256, dtype=torch.bool, device="cuda").tril()
            F.scaled_dot_product_attention(q, k, v, attn_mask=m, dropout_p=0.1)
            F.scaled_dot_product_attention(q.float(), k.float(), v.float(), dropout_p=0.1)
            q256 = torch.randn(1, 2, 64, 256, device="cuda", dtype=torch.bfloat16)
            F.scaled_dot_product_attention(q256, q256, q256, dropout_p=0.1)
            assert um.get_dispatch_stats()["pytorch_fallback"] == 3
    # a short training run through the routing
    with um.options(sdpa_dropout=1):
        w = torch.nn.Linear(64, 64, device="cuda", dtype=torch.bfloat16)
        opt = torch.optim.SGD(w.parameters(), lr=1e-2)
        x = torch.randn(2, 4, 128, 64, device="cuda", dtype=torch.bfloat16)
        with um.use_umfa_sdpa():
            for _ in range(3):
                y = w(x)
                loss = F.scaled_dot_product_attention(y, y, y, dropout_p=0.1).float().pow(2).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
        assert torch.isfinite(loss)
