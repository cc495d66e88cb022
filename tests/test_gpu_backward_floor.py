"""The 16-bit attention backward (fa_bwd16, fa_bwd16_mask) held to the gradient format floor (tolerances.check_backward).

O and LSE come from the GPU forward (fp32 O); the gradients from ops.attention_backward, fp32 unless the case is about 16-bit
output.  The reference is oracle.flash_backward_format_floor on the CPU: fp64 gradients on the O and LSE the kernel was handed,
and the ideal 16-bit backward's (P and dS rounded once).  Full tensors where B H Sq Skv is small, else tolerances.sample_rows:
both edges of every 128-row (key) block of every (batch, head) slab plus seeded interior rows.

Test ids name the shape; the causal grid-shape cases also name the block count and the grid (causal_rank,
fa_bwd_16_common.h: odd block count / even count paired two per CU / more than 512 workgroups)."""
import numpy as np
import pytest
import torch

import tolerances as tol

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
FULL = 1 << 21  # B H Sq Skv up to which the reference covers every element


@pytest.fixture(scope="module")
def ut():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a device: the product path has no CPU fallback")
    import umfa_torch
    return umfa_torch


def _orc():
    from oracle import oracle
    return oracle


def _np(t):
    return t.detach().float().cpu().numpy()


def make(B, H, Sq, Skv, D, kind, seed, Hkv=None, qk_gain=1.0, v_off=0.0, per_slab=False):
    """q, dO [B, H, Sq, D], k, v [B, Hkv, Skv, D] in the operand type, on the device (generated on the CPU: reproducible)"""
    g = torch.Generator().manual_seed(seed)
    Hkv = Hkv or H
    q, k, v, do = (torch.randn(B, h, n, D, generator=g) for h, n in ((H, Sq), (Hkv, Skv), (Hkv, Skv), (H, Sq)))
    q, k, v = q * qk_gain, k * qk_gain, v + v_off
    if per_slab:  # distinct scale and offset per (batch, head): a slab mix-up cannot hide in matching statistics
        def sl(h, lo, hi):
            return torch.empty(B, h, 1, 1).uniform_(lo, hi, generator=g)
        q, k = q * sl(H, 0.5, 2.0), k * sl(Hkv, 0.5, 2.0)
        v, do = v * sl(Hkv, 0.25, 4.0) + sl(Hkv, -4.0, 4.0), do * sl(H, 0.25, 4.0)
    return [t.to(DT[kind]).cuda() for t in (q, k, v, do)]


def forward(ut, q, k, v, causal, scale, group=1, **kw):
    if group > 1:
        k, v = (t.repeat_interleave(group, dim=1) for t in (k, v))
    o, lse = ut.attention_forward(q, k, v, scale=scale, causal=causal, out_dtype=torch.float32, return_lse=True, **kw)
    return o, lse


def floor_of(q, k, v, do, o, lse, kind, scale, causal, group=1, term=None, sample=None, seed=0):
    """the format floor on all elements, or (sample=True) on sampled rows and keys; returns (floor, rows, keys)"""
    B, H, Sq, _ = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    if sample is None:
        sample = B * H * Sq * Skv > FULL
    rows = tol.sample_rows(Sq, B, H, seed) if sample else None
    keys = tol.sample_rows(Skv, B, Hkv, seed + 1) if sample else None
    fl = _orc().flash_backward_format_floor(_np(do), _np(q), _np(k), _np(v), _np(o), _np(lse), kind, scale=scale, causal=causal,
                                            term=term, kv_group=group, rows=rows, keys=keys)
    return fl, rows, keys


def picked(g, rows, keys):
    return (tol.gather_rows(_np(g[0]), rows), tol.gather_rows(_np(g[1]), keys), tol.gather_rows(_np(g[2]), keys))


def check(ut, g, fl, rows, keys, kind, tag, grad_dt=None, kernel=None, ceiling=None, scale_max=1.0):
    kernel = kernel or ut.last_kernel()
    return tol.check_backward(picked(g, rows, keys), fl, kind, tag=tag, kernel=kernel, grad_dt=grad_dt, ceiling=ceiling,
                              scale_max=scale_max)


def bwd(ut, q, k, v, do, o, lse, scale, causal, **kw):
    from umfa_torch import ops
    kw.setdefault("keep_fp32", True)
    g = ops.attention_backward(do, q, k, v, o, lse, scale=scale, causal=causal, **kw)
    torch.cuda.synchronize()
    return g


def run(ut, B, H, Sq, Skv, D, kind, causal, tag, seed=0, sample=None, **mk):
    scale = D ** -0.5
    q, k, v, do = make(B, H, Sq, Skv, D, kind, seed, **mk)
    o, lse = forward(ut, q, k, v, causal, scale)
    g = bwd(ut, q, k, v, do, o, lse, scale, causal)
    kern = ut.last_kernel()
    assert kern.startswith(f"fa_bwd16<{kind},{D}"), kern
    fl, rows, keys = floor_of(q, k, v, do, o, lse, kind, scale, causal, sample=sample, seed=seed)
    check(ut, g, fl, rows, keys, kind, tag, kernel=kern)
    return g, fl


# ----------------------------------------------------------------------------------------------------------------- base matrix
SHAPES = [(1, 257), (7, 64), (31, 33), (129, 127), (200, 1100), (1100, 200), (333, 333), (1024, 1024)]


@pytest.mark.parametrize("Sq,Skv", SHAPES, ids=[f"Sq{a}_Skv{b}" for a, b in SHAPES])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128, 256], ids=["d64", "d128", "d256"])
def test_base_matrix(ut, D, kind, causal, Sq, Skv):
    g, _ = run(ut, 2, 3, Sq, Skv, D, kind, causal, f"base d{D} {kind} causal={causal} {Sq}x{Skv}", seed=Sq * 31 + Skv + D)
    if causal and Sq < Skv:  # top-left causal: keys no query reaches get exactly zero gradients
        assert torch.count_nonzero(g[1][:, :, Sq:]) == 0 and torch.count_nonzero(g[2][:, :, Sq:]) == 0


# ----------------------------------------------------------------------------------------------------------------- grid shapes
GRIDS = [  # D, B, H, S; causal_rank branch of the dQ kernel
    pytest.param(64, 2, 32, 2048, id="d64_B2H32S2048_blk16_grid1024_over512"),
    pytest.param(64, 1, 3, 1920, id="d64_B1H3S1920_blk15_grid45_odd"),
    pytest.param(128, 4, 16, 1024, id="d128_B4H16S1024_blk8_grid512_paired"),
    pytest.param(128, 4, 17, 1024, id="d128_B4H17S1024_blk8_grid544_over512"),
    pytest.param(256, 2, 8, 2048, id="d256_B2H8S2048_blk16_grid256_one_per_cu"),
]


@pytest.mark.parametrize("D,B,H,S", GRIDS)
def test_causal_grid_branches(ut, D, B, H, S):
    run(ut, B, H, S, S, D, "bf16", True, f"grid d{D} B{B}H{H}S{S}", seed=S + H)


# ----------------------------------------------------------------------------------------------------------------- long context
@pytest.mark.parametrize("S,causal", [pytest.param(32768, True, id="causal_B1H2S32768"),
                                      pytest.param(16384, False, id="full_B1H2S16384")])
def test_long_context_bf16_d128(ut, S, causal):
    run(ut, 1, 2, S, S, 128, "bf16", causal, f"long S{S} causal={causal}", seed=7, sample=True)


# ----------------------------------------------------------------------------------------------------------------- hostile inputs
STRESS = {"peaked": dict(qk_gain=3.0), "v_mean8": dict(v_off=8.0), "per_slab": dict(per_slab=True)}


@pytest.mark.parametrize("what", sorted(STRESS))
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("D,B,H,Sq,Skv,causal", [pytest.param(128, 2, 3, 400, 700, True, id="d128_B2H3_400x700_causal"),
                                                 pytest.param(64, 2, 4, 333, 300, False, id="d64_B2H4_333x300")])
def test_inputs_that_stress_the_format(ut, D, B, H, Sq, Skv, causal, kind, what):
    run(ut, B, H, Sq, Skv, D, kind, causal, f"stress {what} d{D} {kind}", seed=17, **STRESS[what])


# ----------------------------------------------------------------------------------------------------------------- linearity in dO
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128, 256], ids=["d64", "d128", "d256"])
def test_power_of_two_linearity_in_dout(ut, D, kind, causal):
    """bwd(2^k dO) == 2^k bwd(dO) bitwise: every step scales exactly (dP, D, dS in fp32, dS rounded to the operand type) as long
    as nothing is subnormal.  fp16: dO is first scaled so that 2^k max|dS| sits near 2^14 (and 2^k max|dO| below 2^15), which
    leaves very few dS below fp16's normal range at the base scale; a row (dQ) or key (dK) holding one of those (from the fp64
    reference, with a factor-2 margin) is excused from the bitwise check -- its subnormal dS does not scale exactly -- and only
    held to the floor.  dV = P^T dO never sees dS: bitwise everywhere."""
    B, H, Sq, Skv, scale = 1, 2, 257, 300, D ** -0.5
    q, k, v, do = make(B, H, Sq, Skv, D, kind, seed=100 + D + causal)
    o, lse = forward(ut, q, k, v, causal, scale)
    fl, _, _ = floor_of(q, k, v, do, o, lse, kind, scale, causal, sample=False)
    if kind == "fp16":
        c = 2.0 ** np.floor(np.log2(min(2.0 ** 12 / fl["ds_max"], 2.0 ** 13 / float(do.abs().max()))))
        kexp = 2
        do = (do.float() * c).to(do.dtype)  # exact: a power of two, no overflow
        fl, _, _ = floor_of(q, k, v, do, o, lse, kind, scale, causal, sample=False)
    else:
        kexp = 5
    g1 = bwd(ut, q, k, v, do, o, lse, scale, causal)
    check(ut, g1, fl, None, None, kind, f"linearity base d{D} {kind}")
    g2 = bwd(ut, q, k, v, (do.float() * 2.0 ** kexp).to(do.dtype), o, lse, scale, causal)
    ok_q = np.ones(Sq, bool)
    ok_k = np.ones(Skv, bool)
    excused = {}
    if kind == "fp16":
        Q, K, V, dO = (_np(t).astype(np.float64) for t in (q, k, v, do))
        for h in range(H):
            s = Q[0, h] @ K[0, h].T * scale
            if causal:
                s = np.where(np.arange(Skv)[None, :] <= np.arange(Sq)[:, None], s, -np.inf)
            p = np.exp(s - _np(lse).reshape(B, H, Sq)[0, h][:, None].astype(np.float64))
            ds = p * (dO[0, h] @ V[0, h].T - (dO[0, h] * _np(o)[0, h]).sum(-1)[:, None])
            sub = (p > 0) & (np.abs(ds) < 2.0 ** -13)
            ok_q &= ~sub.any(1)
            ok_k &= ~sub.any(0)
        excused = dict(rows=int((~ok_q).sum()), keys=int((~ok_k).sum()))
        assert excused["rows"] <= 8 and excused["keys"] <= 8, excused  # the scaling keeps them rare
    tol.record(f"linearity d{D} {kind} causal={causal}", k=kexp, **excused)
    for a, b, ok, name in ((g1[0], g2[0], ok_q, "dq"), (g1[1], g2[1], ok_k, "dk"), (g1[2], g2[2], np.ones(Skv, bool), "dv")):
        want = a * 2.0 ** kexp
        sel = torch.from_numpy(ok).cuda()
        assert torch.equal(b[:, :, sel], want[:, :, sel]), (name, float((b - want)[:, :, sel].abs().max()))


# ----------------------------------------------------------------------------------------------------------------- launcher options
@pytest.mark.parametrize("Sq,Skv", [(333, 500), (500, 333)], ids=["333x500", "500x333"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("which", ["1", "2"], ids=["dq1_two_per_cu", "dq2_one_per_cu"])
def test_both_dq_kernels(ut, umfa_opts, which, causal, Sq, Skv):
    umfa_opts(bwd_dq=which)
    run(ut, 2, 3, Sq, Skv, 128, "bf16", causal, f"bwd_dq={which} causal={causal} {Sq}x{Skv}", seed=int(which) + Sq)


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_persistent_dkdv_grid(ut, umfa_opts, kind):
    """bwd_persist: bwd16_dkdv on one workgroup per CU, items stepped by gridDim.x, LDS reused between items; B2 H24 S1024 is
    384 items, more than the CUs"""
    B, H, S, D, scale = 2, 24, 1024, 128, 128 ** -0.5
    q, k, v, do = make(B, H, S, S, D, kind, seed=31)
    o, lse = forward(ut, q, k, v, False, scale)
    ref = bwd(ut, q, k, v, do, o, lse, scale, False)
    umfa_opts(bwd_persist=1)
    g = bwd(ut, q, k, v, do, o, lse, scale, False)
    fl, rows, keys = floor_of(q, k, v, do, o, lse, kind, scale, False, seed=31)
    check(ut, g, fl, rows, keys, kind, f"bwd_persist {kind} B{B}H{H}S{S}")
    for a, b, name in zip(g, ref, "qkv"):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("D,causal", [(128, False), (64, True)], ids=["d128_full", "d64_causal"])
def test_separate_delta(ut, umfa_opts, D, causal):
    umfa_opts(bwd_separate_delta=1)
    run(ut, 2, 3, 333, 300, D, "fp16", causal, f"bwd_separate_delta d{D}", seed=5)


# ----------------------------------------------------------------------------------------------------------------- grouped heads
GQA = [pytest.param(2, 8, 2, 256, 320, 64, False, id="B2_Hq8_Hkv2_256x320_d64_full"),
       pytest.param(2, 8, 2, 256, 320, 64, True, id="B2_Hq8_Hkv2_256x320_d64_causal"),
       pytest.param(1, 12, 4, 333, 333, 128, True, id="B1_Hq12_Hkv4_333_d128_causal"),
       pytest.param(1, 8, 1, 129, 1024, 256, False, id="B1_Hq8_Hkv1_129x1024_d256_full")]


def gqa_case(ut, B, Hq, Hkv, Sq, Skv, D, causal, kind, seed):
    from umfa_torch import ops
    scale, grp = D ** -0.5, Hq // Hkv
    q, k, v, do = make(B, Hq, Sq, Skv, D, kind, seed, Hkv=Hkv)
    o, lse = forward(ut, q, k, v, causal, scale, group=grp)
    fl, rows, keys = floor_of(q, k, v, do, o, lse, kind, scale, causal, group=grp, seed=seed)

    def launch():
        g = ops.attention_backward_gqa(do, q, k, v, o, lse, scale=scale, causal=causal)
        torch.cuda.synchronize()
        assert g is not None and g[1].shape == k.shape
        return g
    return launch, fl, rows, keys


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("B,Hq,Hkv,Sq,Skv,D,causal", GQA)
def test_gqa_entry(ut, B, Hq, Hkv, Sq, Skv, D, causal, kind):
    """umfa_attention_backward_gqa_stream (K / V read in place, gradients in the operand type) against the group-summed floor"""
    launch, fl, rows, keys = gqa_case(ut, B, Hq, Hkv, Sq, Skv, D, causal, kind, seed=Hq + Skv)
    g = launch()
    assert g[0].dtype == DT[kind]
    check(ut, g, fl, rows, keys, kind, f"gqa {kind} B{B} Hq{Hq} Hkv{Hkv} {Sq}x{Skv} d{D}", grad_dt=kind, kernel="gqa:" + ut.last_kernel())


# ----------------------------------------------------------------------------------------------------------------- output types
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("D,causal", [(128, True), (64, False), (256, False)], ids=["d128_causal", "d64_full", "d256_full"])
def test_gradients_in_the_operand_type(ut, D, causal, kind):
    B, H, Sq, Skv, scale = 2, 3, 300, 333, D ** -0.5
    q, k, v, do = make(B, H, Sq, Skv, D, kind, seed=D)
    o, lse = forward(ut, q, k, v, causal, scale)
    g = bwd(ut, q, k, v, do, o, lse, scale, causal, keep_fp32=False, grads_in_input_type=True)
    assert g[0].dtype == DT[kind] and ut.last_kernel().startswith("fa_bwd16")
    fl, rows, keys = floor_of(q, k, v, do, o, lse, kind, scale, causal)
    check(ut, g, fl, rows, keys, kind, f"grads in {kind} d{D}", grad_dt=kind)


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("D,causal", [(128, False), (64, True)], ids=["d128_full", "d64_causal"])
def test_out_in_the_operand_type(ut, D, causal, kind):
    """O handed over in the operand type: D = rowsum(dO o O) comes from the rounded O, so the floor does too"""
    B, H, Sq, Skv, scale = 1, 3, 384, 300, D ** -0.5
    q, k, v, do = make(B, H, Sq, Skv, D, kind, seed=D + 1)
    o, lse = forward(ut, q, k, v, causal, scale)
    o16 = o.to(DT[kind])
    g = bwd(ut, q, k, v, do, o16, lse, scale, causal)
    fl, rows, keys = floor_of(q, k, v, do, o16, lse, kind, scale, causal)
    check(ut, g, fl, rows, keys, kind, f"O in {kind} d{D}")


# ----------------------------------------------------------------------------------------------------------------- masked backward
def _window_term(Sq, Skv, left, right):
    i, j = np.arange(Sq)[:, None], np.arange(Skv)[None, :]
    return np.where((j >= i - left) & (j <= i + right), 0.0, -np.inf)


MASKS = ["keypad", "perhead", "bias_f32", "window64_causal", "window33_17"]


@pytest.mark.parametrize("what", MASKS)
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("D,B,H,Sq,Skv", [pytest.param(64, 2, 3, 333, 277, id="d64_B2H3_333x277"),
                                          pytest.param(128, 1, 2, 200, 450, id="d128_B1H2_200x450")])
def test_masked_backward(ut, D, B, H, Sq, Skv, kind, what):
    scale = D ** -0.5
    q, k, v, do = make(B, H, Sq, Skv, D, kind, seed=D + Sq)
    gen = torch.Generator().manual_seed(D + Skv)
    kw, causal = {}, False
    if what == "keypad":
        lens = torch.tensor([Skv - 37, Skv - 128][:B])
        m = torch.arange(Skv).view(1, 1, 1, Skv) < lens.view(B, 1, 1, 1)
        kw["mask"] = m.cuda()
        term = np.where(m.numpy(), 0.0, -np.inf)
    elif what == "perhead":
        m = torch.rand(1, H, Sq, Skv, generator=gen) < 0.7
        m[0, 0, 5] = False  # a row the mask hides entirely: zero dQ, nothing into dK / dV
        kw["mask"] = m.cuda()
        term = np.where(m.numpy(), 0.0, -np.inf)
    elif what == "bias_f32":
        m = 2.0 * torch.randn(1, H, Sq, Skv, generator=gen)
        kw["mask"] = m.cuda()
        term = m.double().numpy()
    else:
        win, causal = ((64, 0), True) if what == "window64_causal" else ((33, 17), False)
        kw["window"] = win
        term = _window_term(Sq, Skv, *win)
    o, lse = forward(ut, q, k, v, causal, scale, **kw)
    g = bwd(ut, q, k, v, do, o, lse, scale, causal, **kw)
    kern = ut.last_kernel()
    assert kern == f"fa_bwd16<{kind},{D},{'window' if 'window' in kw else 'mask'}>", kern
    fl, rows, keys = floor_of(q, k, v, do, o, lse, kind, scale, causal, term=term)
    rec = check(ut, g, fl, rows, keys, kind, f"masked {what} d{D} {kind}", kernel=kern)
    if what == "perhead":
        assert fl["dead"][0][:, 0, 5].all() and rec["dq"]["n"] > 0


# ----------------------------------------------------------------------------------------------------------------- repeatability
def test_repeatable_d64_causal_grid1024(ut):
    B, H, S, D, scale = 2, 32, 2048, 64, 64 ** -0.5
    q, k, v, do = make(B, H, S, S, D, "bf16", seed=77)
    o, lse = forward(ut, q, k, v, True, scale)
    fl, rows, keys = floor_of(q, k, v, do, o, lse, "bf16", scale, True, seed=77)
    g1 = bwd(ut, q, k, v, do, o, lse, scale, True)
    check(ut, g1, fl, rows, keys, "bf16", "repeat d64 grid1024, first launch")
    g2 = bwd(ut, q, k, v, do, o, lse, scale, True)
    check(ut, g2, fl, rows, keys, "bf16", "repeat d64 grid1024, second launch")
    for a, b, name in zip(g1, g2, "qkv"):
        assert torch.equal(a, b), name


def test_repeatable_gqa_d128(ut):
    launch, fl, rows, keys = gqa_case(ut, 1, 12, 4, 333, 333, 128, True, "bf16", seed=78)
    g1 = launch()
    check(ut, g1, fl, rows, keys, "bf16", "repeat gqa d128, first launch", grad_dt="bf16")
    g2 = launch()
    check(ut, g2, fl, rows, keys, "bf16", "repeat gqa d128, second launch", grad_dt="bf16")
    for a, b, name in zip(g1, g2, "qkv"):
        assert torch.equal(a, b), name
