"""Masked and sliding-window attention backward (umfa_attention_backward_masked_stream, fa_bwd_16_mask.hip, fa_bwd.hip).

Reference: fp64 CPU autograd written out by hand on the already-rounded inputs -- scores + additive term, softmax with rows that
see nothing set to 0 (as ref_of in test_gpu_sdpa.py).  Gradient bounds as the unmasked fuzz (test_gpu_fuzz.py): bf16 3e-2, fp16
8e-3, fp32 1e-4 of max|ref|; bf16 head_dim 128 at moderate sizes 8e-3 (BWD16_TOL)."""
import itertools
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 3e-2, torch.float16: 8e-3, torch.float32: 1e-4}
BWD16_TOL = 8e-3


@pytest.fixture(scope="module")
def ut():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import umfa_torch
    return umfa_torch


def term_of(mask, shape4):
    """additive fp64 term of a mask (bool: -inf where False), broadcast to [B, H, Sq, Skv], on the CPU"""
    m = mask.detach().cpu()
    t = torch.zeros(m.shape, dtype=torch.float64).masked_fill(~m, float("-inf")) if m.dtype == torch.bool else m.double()
    return t.expand(shape4)


def window_term(Sq, Skv, left, right):
    i = torch.arange(Sq).view(-1, 1)
    j = torch.arange(Skv).view(1, -1)
    return torch.zeros(Sq, Skv, dtype=torch.float64).masked_fill(~((j >= i - left) & (j <= i + right)), float("-inf"))


def ref_grads(q, k, v, dout, term, causal, scale):
    qd, kd, vd = (t.detach().cpu().double().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bhqd,bhkd->bhqk", qd, kd) * scale + term
    if causal:
        Sq, Skv = s.shape[-2:]
        s = s.masked_fill(torch.ones(Sq, Skv, dtype=torch.bool).triu(1), float("-inf"))
    seen = torch.isfinite(s).any(-1, keepdim=True)
    p = torch.softmax(torch.where(seen, s, torch.zeros_like(s)), -1) * seen
    o = torch.einsum("bhqk,bhkd->bhqd", p, vd)
    o.backward(dout.detach().cpu().double())
    return qd.grad, kd.grad, vd.grad


def run(ut, q, k, v, dout, scale, causal, mask=None, window=None, with_fwd=False):
    out, lse = ut.attention_forward(q, k, v, scale=scale, causal=causal, mask=mask, window=window, out_dtype=q.dtype, return_lse=True)
    g = ut.attention_backward(dout, q, k, v, out, lse, scale=scale, causal=causal, mask=mask, window=window)
    torch.cuda.synchronize()
    return (g, out, lse) if with_fwd else g


def rel_err(g, r):
    return float((g.detach().double().cpu() - r).abs().max() / r.abs().max().clamp_min(1e-30))


# ----------------------------------------------------------------------------------------------------------------- ABI / ops level
SHAPES = {  # name: (B, H, Sq, Skv, causal)
    "2d": (2, 2, 200, 200, False),
    "keypad": (2, 3, 256, 256, False),
    "perhead": (1, 3, 192, 192, False),
    "blockdiag": (2, 2, 320, 320, False),
    "expanded": (2, 2, 160, 224, False),
    "view": (1, 2, 136, 200, False),
    "ragged": (1, 2, 1000, 777, False),
    "sq_ne_skv": (2, 2, 130, 300, False),
    "causal": (1, 2, 256, 256, True),
}
KINDS = ("bool", "f32", "f16", "bf16", "window")
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
HEADS = (64, 128, 256, 96)


def make_mask(kind, shape, B, H, Sq, Skv, gen):
    """a mask of the given dtype kind and layout; every layout keeps some rows fully open and some keys closed"""
    def vals(*dims):
        if kind == "bool":
            return torch.rand(*dims, generator=gen) < 0.7
        x = torch.randn(*dims, generator=gen)
        x = x.masked_fill(torch.rand(*dims, generator=gen) < 0.3, float("-inf"))
        return x.to({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[kind])

    def from_bool(b):
        if kind == "bool":
            return b
        z = torch.zeros(b.shape).masked_fill(~b, float("-inf"))
        return (z + 0.25 * torch.randn(b.shape, generator=gen)).to({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[kind])

    if shape in ("2d", "ragged", "sq_ne_skv", "causal"):
        m = vals(Sq, Skv)
    elif shape == "keypad":
        lens = [Skv - 37, Skv - 128][:B]
        m = from_bool(torch.stack([torch.arange(Skv) < n for n in lens]).view(B, 1, 1, Skv))
    elif shape == "perhead":
        m = vals(1, H, Sq, Skv)
    elif shape == "blockdiag":
        doc = torch.stack([torch.arange(Sq) * (2 + b) // Sq for b in range(B)])  # B documents layouts
        m = from_bool((doc.view(B, 1, Sq, 1) == doc.view(B, 1, 1, Skv)))
    elif shape == "expanded":
        return vals(1, 1, 1, Skv).cuda().expand(B, H, Sq, Skv)  # stride 0 in three dims
    elif shape == "view":
        return vals(Sq, Skv + 7).cuda()[:, 3:Skv + 3]  # rows not aligned to four elements, a view
    return m.cuda()


def _cases():
    out = []
    for dt, D, kind in itertools.product(DTYPES, HEADS, KINDS):
        names = sorted(SHAPES)
        h = zlib.crc32(f"{dt}{D}{kind}".encode())
        picked = {names[h % len(names)], names[(h // 7) % len(names)], names[(h // 49) % len(names)]}
        for s in sorted(picked):
            out.append((dt, D, kind, s))
    return out


@pytest.mark.parametrize("dt,D,kind,shape", _cases(), ids=lambda x: str(x).replace("torch.", ""))
def test_masked_backward_matches_fp64(ut, dt, D, kind, shape):
    B, H, Sq, Skv, causal = SHAPES[shape]
    gen = torch.Generator().manual_seed(zlib.crc32(f"{dt}{D}{kind}{shape}".encode()))
    q, k, v, dout = (torch.randn(B, H, n, D, generator=gen).to(dt).cuda() for n in (Sq, Skv, Skv, Sq))
    scale = D ** -0.5
    if kind == "window":
        win = (int(torch.randint(0, 80, (1,), generator=gen)), int(torch.randint(0, 80, (1,), generator=gen)))
        g, out, lse = run(ut, q, k, v, dout, scale, causal, window=win, with_fwd=True)
        term = window_term(Sq, Skv, *win).expand(B, H, Sq, Skv)
        want = "window"
    else:
        m = make_mask(kind, shape, B, H, Sq, Skv, gen)
        g, out, lse = run(ut, q, k, v, dout, scale, causal, mask=m, with_fwd=True)
        term = term_of(m, (B, H, Sq, Skv))
        want = "mask"
    kern = ut.last_kernel()
    if dt != torch.float32 and D in (64, 128, 256):
        assert kern == f"fa_bwd16<{'bf16' if dt == torch.bfloat16 else 'fp16'},{D},{want}>", kern
    else:
        assert kern.startswith("fa_bwd_exact"), kern
    r = ref_grads(q, k, v, dout, term, causal, scale)
    for name, gi, ri in zip("qkv", g, r):
        assert torch.isfinite(gi).all(), name
        assert rel_err(gi, ri) <= TOL[dt], (name, rel_err(gi, ri))
    if kern.startswith("fa_bwd16<"):  # and the gradient format floor on the O (operand type) and LSE the kernel was handed
        import tolerances
        from oracle import oracle
        kd = "bf16" if dt == torch.bfloat16 else "fp16"
        npy = lambda t: t.detach().float().cpu().numpy()  # noqa: E731
        fl = oracle.flash_backward_format_floor(npy(dout), npy(q), npy(k), npy(v), npy(out), npy(lse), kd, scale=scale, causal=causal,
                                                term=term.numpy())
        tolerances.check_backward([npy(gi) for gi in g], fl, kd, tag=f"masked {kind} {shape} d{D}", kernel=kern, grad_dt=kd,
                                  ceiling={kd: TOL[dt]})


def test_bf16_d128_moderate_size_within_bwd16_tol(ut):
    gen = torch.Generator().manual_seed(5)
    B, H, S, D = 2, 4, 512, 128
    q, k, v, dout = (torch.randn(B, H, S, D, generator=gen).to(torch.bfloat16).cuda() for _ in range(4))
    lens = torch.tensor([S - 100, S - 300])
    m = (torch.arange(S).view(1, 1, 1, S) < lens.view(B, 1, 1, 1)).cuda()
    g = run(ut, q, k, v, dout, D ** -0.5, False, mask=m)
    assert ut.last_kernel() == "fa_bwd16<bf16,128,mask>"
    r = ref_grads(q, k, v, dout, term_of(m, (B, H, S, S)), False, D ** -0.5)
    for gi, ri in zip(g, r):
        assert rel_err(gi, ri) <= BWD16_TOL


# ----------------------------------------------------------------------------------------------------------------- edge rows and keys
@pytest.mark.parametrize("dt,D", [(torch.bfloat16, 128), (torch.float16, 64), (torch.bfloat16, 256), (torch.float32, 64), (torch.bfloat16, 96)])
def test_fully_masked_rows_and_keys_give_exact_zeros(ut, dt, D):
    gen = torch.Generator().manual_seed(D)
    B, H, Sq, Skv = 1, 2, 192, 256
    q, k, v, dout = (torch.randn(B, H, n, D, generator=gen).to(dt).cuda() for n in (Sq, Skv, Skv, Sq))
    m = torch.rand(Sq, Skv, generator=gen) < 0.8
    m[5:40] = False          # rows that see nothing
    m[:, 3] = False          # keys nobody sees
    m[:, 70:140] = False
    m = m.cuda()
    dq, dk, dv = run(ut, q, k, v, dout, D ** -0.5, False, mask=m)
    for t in (dq, dk, dv):
        assert torch.isfinite(t).all()
    assert (dq[:, :, 5:40] == 0).all()
    for t in (dk, dv):
        assert (t[:, :, 3] == 0).all() and (t[:, :, 70:140] == 0).all()
    r = ref_grads(q, k, v, dout, term_of(m, (B, H, Sq, Skv)), False, D ** -0.5)
    for gi, ri in zip((dq, dk, dv), r):
        assert rel_err(gi, ri) <= TOL[dt]


@pytest.mark.parametrize("mdt", [torch.float32, torch.bfloat16])
def test_finfo_min_padding_matches_torch(ut, mdt):
    gen = torch.Generator().manual_seed(11)
    B, H, S, D = 2, 2, 256, 128
    q, k, v, dout = (torch.randn(B, H, S, D, generator=gen).to(torch.bfloat16).cuda() for _ in range(4))
    m = torch.zeros(B, 1, 1, S, dtype=mdt)
    m[0, ..., 200:] = torch.finfo(mdt).min
    m[1, ..., 1:] = torch.finfo(mdt).min  # one visible key
    m = m.cuda()
    g = run(ut, q, k, v, dout, D ** -0.5, False, mask=m)
    assert ut.last_kernel() == "fa_bwd16<bf16,128,mask>"
    qr, kr, vr = (t.float().requires_grad_(True) for t in (q, k, v))
    o = torch.nn.functional.scaled_dot_product_attention(qr, kr, vr, attn_mask=m.float())
    o.backward(dout.float())
    for gi, ri in zip(g, (qr.grad, kr.grad, vr.grad)):
        assert torch.isfinite(gi).all()
        assert rel_err(gi, ri.double().cpu()) <= TOL[torch.bfloat16]


# ----------------------------------------------------------------------------------------------------------------- routing
def _train_inputs(seed=3, S=256, D=128, B=2, H=2):
    gen = torch.Generator().manual_seed(seed)
    q, k, v, w = (torch.randn(B, H, S, D, generator=gen).to(torch.bfloat16).cuda() for _ in range(4))
    m = (torch.arange(S).view(1, 1, 1, S) < torch.tensor([S - 40, S - 97])[:B].view(B, 1, 1, 1)).cuda()
    return q, k, v, w, m


def _grads(fn, q, k, v, w, m):
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    (fn(qg, kg, vg, m).float() * w.float()).sum().backward()
    torch.cuda.synchronize()
    return qg.grad, kg.grad, vg.grad


def test_masked_training_routes_to_masked_bwd16(ut):
    from umfa_torch import sdpa
    q, k, v, w, m = _train_inputs()
    sdpa.reset_dispatch_stats()
    g = _grads(lambda a, b, c, mm: ut.scaled_dot_product_attention(a, b, c, attn_mask=mm), q, k, v, w, m)
    st = sdpa.get_dispatch_stats()
    assert st["pytorch_fallback"] == 0 and st["fp32_autograd"] == 1, st
    assert ut.last_kernel() == "fa_bwd16<bf16,128,mask>", ut.last_kernel()
    r = ref_grads(q, k, v, w, term_of(m, (2, 2, 256, 256)), False, 128 ** -0.5)
    for gi, ri in zip(g, r):
        assert rel_err(gi, ri) <= BWD16_TOL


def test_masked_training_through_aten_override_and_compile(ut):
    import torch.nn.functional as F
    q, k, v, w, m = _train_inputs(seed=4)
    eager = _grads(lambda a, b, c, mm: ut.scaled_dot_product_attention(a, b, c, attn_mask=mm), q, k, v, w, m)
    ut.unregister_backend()
    ut.library.override_aten_sdpa(True)
    try:
        ut.reset_dispatch_stats()
        via_aten = _grads(lambda a, b, c, mm: F.scaled_dot_product_attention(a, b, c, attn_mask=mm), q, k, v, w, m)
        assert ut.get_dispatch_stats()["pytorch_fallback"] == 0
        assert ut.last_kernel() == "fa_bwd16<bf16,128,mask>"
    finally:
        ut.library.override_aten_sdpa(False)
    fn = torch.compile(lambda a, b, c, mm: ut.scaled_dot_product_attention(a, b, c, attn_mask=mm), fullgraph=True)
    ut.reset_dispatch_stats()
    compiled = _grads(fn, q, k, v, w, m)
    assert ut.get_dispatch_stats()["pytorch_fallback"] == 0
    assert ut.last_kernel() == "fa_bwd16<bf16,128,mask>"
    for a, b, c in zip(eager, via_aten, compiled):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_routing_edges_keep_torch(ut):
    from umfa_torch import sdpa
    q, k, v, w, m = _train_inputs(seed=6)
    # a learnable mask: torch, which supplies its gradient
    mb = torch.zeros(m.shape, device="cuda").masked_fill(~m, float("-inf")).to(torch.bfloat16).requires_grad_(True)
    sdpa.reset_dispatch_stats()
    qg = q.clone().requires_grad_(True)
    (ut.scaled_dot_product_attention(qg, k, v, attn_mask=mb).float() * w.float()).sum().backward()
    assert sdpa.get_dispatch_stats()["pytorch_fallback"] == 1 and mb.grad is not None
    # the A/B switch
    with ut.options(no_bwd_mask=1):
        sdpa.reset_dispatch_stats()
        _grads(lambda a, b, c, mm: ut.scaled_dot_product_attention(a, b, c, attn_mask=mm), q, k, v, w, m)
        assert sdpa.get_dispatch_stats()["pytorch_fallback"] == 1
    # head_dim 384 (no masked wide backward); head_dim 256, 96 and fp32 operands (measured slower than torch end to end)
    for D, dt in ((384, torch.bfloat16), (256, torch.bfloat16), (96, torch.float16), (64, torch.float32)):
        q3, k3, v3, w3, m3 = _train_inputs(seed=7, S=64, D=D, B=1, H=2)
        q3, k3, v3, w3 = (t.to(dt) for t in (q3, k3, v3, w3))
        sdpa.reset_dispatch_stats()
        _grads(lambda a, b, c, mm: ut.scaled_dot_product_attention(a, b, c, attn_mask=mm), q3, k3, v3, w3, m3)
        assert sdpa.get_dispatch_stats()["pytorch_fallback"] == 1, (D, dt)


# ----------------------------------------------------------------------------------------------------------------- sliding window
@pytest.mark.parametrize("dt,D,win,causal", [(torch.bfloat16, 128, (100, 100), False), (torch.float16, 64, (64, 0), True),
                                            (torch.bfloat16, 256, (0, 33), False), (torch.float32, 64, (50, 20), False)])
def test_sliding_window_attention_equals_band_mask(ut, dt, D, win, causal):
    gen = torch.Generator().manual_seed(D + win[0])
    B, H, S = 1, 2, 384
    q, k, v, w = (torch.randn(B, H, S, D, generator=gen).to(dt).cuda() for _ in range(4))
    band = torch.isfinite(window_term(S, S, *win)).cuda()
    gw = _grads(lambda a, b, c, _: ut.sliding_window_attention(a, b, c, window=win, causal=causal), q, k, v, w, None)
    if dt != torch.float32:
        assert ut.last_kernel().endswith(",window>"), ut.last_kernel()
    gm = run(ut, q, k, v, w, D ** -0.5, causal, mask=band)
    r = ref_grads(q, k, v, w, window_term(S, S, *win).expand(B, H, S, S), causal, D ** -0.5)
    for a, b, ri in zip(gw, gm, r):
        assert rel_err(a, ri) <= TOL[dt] and rel_err(b, ri) <= TOL[dt]


# ----------------------------------------------------------------------------------------------------------------- repeatability, capture
def test_masked_backward_is_bitwise_repeatable(ut):
    q, k, v, w, m = _train_inputs(seed=8, S=1000)
    a = run(ut, q, k, v, w, 128 ** -0.5, False, mask=m)
    b = run(ut, q, k, v, w, 128 ** -0.5, False, mask=m)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    a = run(ut, q, k, v, w, 128 ** -0.5, True, window=(200, 0))
    b = run(ut, q, k, v, w, 128 ** -0.5, True, window=(200, 0))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_masked_forward_backward_graph_replays_to_eager(ut):
    q, k, v, w, m = _train_inputs(seed=9, S=512)
    mf = torch.zeros(m.shape, device="cuda").masked_fill(~m, float("-inf")).to(torch.bfloat16)
    scale = 128 ** -0.5

    def step():
        out, lse = ut.attention_forward(q, k, v, scale=scale, mask=mf, out_dtype=q.dtype, return_lse=True)
        return ut.attention_backward(w, q, k, v, out, lse, scale=scale, mask=mf)

    eager = step()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up on the capturing stream: its scratch exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        graphed = step()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, graphed):
        assert torch.equal(x, y)
