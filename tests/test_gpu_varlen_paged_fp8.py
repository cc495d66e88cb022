"""Packed variable-length queries over fp8 (e4m3fn) KV caches on the GPU (umfa_torch.varlen_kvcache_attention with k_descale /
v_descale), with the helpers of tests/test_gpu_varlen_paged.py and tests/test_gpu_paged_fp8.py: mixed batches
against the fp64 reference (tests/varlen_paged_fp8_ref.py) under the unchanged format bounds of tests/tolerances.py, the format floor of
both work-item forms, a sequence across the block-table reload boundary, bitwise agreement with kvcache_attention's fp8 call when every
L_q is equal (with and without rotary), the packed quantising append (bitwise, nothing else touched), NaN bytes where no key lives,
hostile cu / lengths / table entries, static layouts, a strided q, uncovered rows, both forms in one launch, forced and automatic
splits, the fused rotary bit for bit against the plain call on rotated operands, graph replay with rewritten cu / lengths / table /
descales, opcheck / torch.compile and the refused arguments.

Why the 16-bit bounds hold unchanged: test_gpu_paged_fp8.py's reason -- the reference sees the same dequantised numbers, the kernel's
expansions are exact and P is rounded to fp16 once; O rows are divided by their (sequence, KV head) group's v_descale so that
check_forward's normalisation by max |O| compares every group at one scale."""
import numpy as np
import pytest
import torch

import forward_floor_ref as ffr
import paged_rope_ref as rr
import test_gpu_paged_fp8 as tf
import test_gpu_varlen_paged as tv
import tolerances as tol
import varlen_paged_fp8_ref as ref
import varlen_paged_ref as vref
from paged_rope_gpu import rotate_by_ops, tables

pytestmark = pytest.mark.gpu

DT = tv.DT
F8 = torch.float8_e4m3fn
GUARD = tv.GUARD
PREFIX = "fa_fwd16_paged_varlen_fp8<"
_np, _bytes, _dev, _i32, _cu = tv._np, tf._bytes, tf._dev, tv._i32, tv._cu


def _umfa():
    import umfa_torch
    return umfa_torch


def _setup(lq, H, Hkv, D, ps, max_pages, dt, seed, new=False, share=True, pad=0):
    """tv._setup with e4m3fn pools (no NaN bytes): packed q, pools with GUARD free pages at each end, a permuted block table"""
    B, Tq = len(lq), int(sum(lq)) + pad
    g = torch.Generator(device="cuda").manual_seed(seed)
    num_pages = B * max_pages + 2 * GUARD
    q = torch.randn(Tq, H, D, device="cuda", dtype=dt, generator=g)
    kc, vc = tf._f8((num_pages, ps, Hkv, D), g), tf._f8((num_pages, ps, Hkv, D), g)
    bt = (np.random.default_rng(seed).permutation(B * max_pages) + GUARD).reshape(B, max_pages).astype(np.int32)
    if share and B > 1:
        bt[1, 0] = bt[0, 0]
    kn = torch.randn(Tq, Hkv, D, device="cuda", dtype=dt, generator=g) if new else None
    vn = torch.randn(Tq, Hkv, D, device="cuda", dtype=dt, generator=g) if new else None
    return q, kc, vc, torch.tensor(bt, device="cuda"), kn, vn


def _descales(B, Hkv, seed):
    return tuple(_dev(x) for x in tf._descales(B, Hkv, seed))


def _run(q, kc, vc, cu, max_q, sl, bt, kd, vd, kn=None, vn=None, causal=False, num_splits=0, scale=None, out_dtype=torch.float32, **kw):
    um = _umfa()
    sc = q.shape[-1] ** -0.5 if scale is None else scale
    o, lse = um.ops.varlen_kvcache_attention_fp8_forward(q, kc, vc, cu, max_q, sl, kd, vd, bt, kn, vn, scale=sc, causal=causal,
                                                         num_splits=num_splits, out_dtype=out_dtype, **kw)
    torch.cuda.synchronize()
    k = um.last_kernel()
    assert k.startswith(PREFIX), k
    return o, lse, k


def _reference(q, kc0, vc0, cu, max_q, sl, bt, kd, vd, kn=None, vn=None, causal=False, scale=None, min_live=0.5, kind=None):
    """the fp64 reference on the byte caches as they were before the call; asserts -- on the reference alone -- the live share"""
    o_ref, lse_ref, k8, v8 = ref.forward(_np(q), _bytes(kc0), _bytes(vc0), cu.cpu().numpy(), max_q, sl.cpu().numpy(), kd.cpu().numpy(),
                                         vd.cpu().numpy(), None if bt is None else bt.cpu().numpy(), None if kn is None else _np(kn),
                                         None if vn is None else _np(vn), causal, scale, kind)
    live = np.isfinite(lse_ref)  # [H, T_q]
    assert live.mean() >= min_live, f"the case holds too few live rows ({live.mean():.2f})"
    return o_ref, lse_ref, live, k8, v8


def _vd_rows(vd, cu, Tq, max_q, H):
    """[T_q, H, 1] the v_descale of each output row's (sequence, KV head) group (1 on rows no sequence covers)"""
    B = cu.numel() - 1
    v = vd.cpu().numpy().astype(np.float64)
    Hkv = v.shape[-1] if v.ndim else 1
    v = np.broadcast_to(v, (B, Hkv))
    rows = np.ones((Tq, H, 1))
    for b, (q0, Lq) in enumerate(vref.ranges(cu.cpu().numpy(), Tq, max_q)):
        rows[q0:q0 + Lq, :, 0] = np.repeat(v[b], H // Hkv)[None, :]
    return rows


def _check(refs, cu, max_q, vd, o, lse, kernel, dt="bf16", out_dt=None):
    """values (divided by the group's v_descale) and LSE of the live rows against the reference; dead rows of covered sequences 0 / -inf"""
    o_ref, lse_ref, live = refs[:3]
    o_, l_ = _np(o), _np(lse)
    cov = vref.covered(cu.cpu().numpy(), o_.shape[0], max_q)
    assert np.isfinite(o_[cov]).all()
    dead = ~live & cov[None, :]
    assert (o_.transpose(1, 0, 2)[dead] == 0).all() and np.isneginf(l_[dead]).all()
    if not live.any():
        return
    print("varlen fp8", kernel, "lse max err", float(np.abs(l_[live] - lse_ref[live]).max()))
    np.testing.assert_allclose(l_[live], lse_ref[live], rtol=0, atol=2e-3)
    div = _vd_rows(vd, cu, o_.shape[0], max_q, o_.shape[1])
    got = (o_ / div).transpose(1, 0, 2)[live][None, None]
    want = (o_ref / div).transpose(1, 0, 2)[live][None, None]
    tol.check_forward(got, want, DT[dt], kernel, tag="varlen_paged_fp8", out_dt=out_dt)


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("new", [False, True], ids=["cached", "append"])
@pytest.mark.parametrize("ps,g,D,dt,causal", tv.CASES)
def test_mixed_batch_values(ps, g, D, dt, causal, new):
    um = _umfa()
    Hkv, max_pages = 2, max(2, 640 // ps)
    cap = ps * max_pages
    lq, slv = tv._mixed(g, ps, cap)
    q, kc, vc, bt, kn, vn = _setup(lq, g * Hkv, Hkv, D, ps, max_pages, DT[dt], seed=ps + g + D, new=new, share=not new)
    kd, vd = _descales(len(lq), Hkv, seed=ps + g)
    cu, sl = _i32(_cu(lq)), _i32(slv)
    kc0, vc0 = kc.clone(), vc.clone()
    refs = _reference(q, kc0, vc0, cu, max(lq), sl, bt, kd, vd, kn, vn, causal=causal)
    for out_dtype in (torch.float32, DT[dt]):
        kc.copy_(kc0)
        vc.copy_(vc0)
        o, lse, kernel = _run(q, kc, vc, cu, max(lq), sl, bt, kd, vd, kn, vn, causal=causal, num_splits=1, out_dtype=out_dtype)
        assert "split" not in kernel and ("causal" in kernel) == causal and ("pv16" in kernel) == (dt == "bf16"), kernel
        assert um.ops.varlen_kvcache_item_counts() == tv._items(lq, g, Hkv)  # both forms, in this one launch
        _check(refs, cu, max(lq), vd, o, lse, kernel, dt=dt, out_dt=None if out_dtype == torch.float32 else out_dtype)
        assert (_bytes(kc) == refs[3]).all() and (_bytes(vc) == refs[4]).all()


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("num_splits", [0, 1, 3], ids=["auto", "unsplit", "splits3"])
def test_format_floor_of_both_forms(dt, D, num_splits):
    """test_gpu_forward_floor.py::test_packed_queries on fp8 caches: decode-form items (L_q 1, 1, 5) and 128-row items (130, 200, 32, 33)
    of one launch, pooled separately against the fp16-P floor; visibility does not depend on the values, so the pools are that case's"""
    g, Hkv, ps = ffr.PACKED_G, ffr.PACKED_HKV, 16
    lq, cache = ffr.PACKED_LQ, ffr.PACKED_CACHE
    H = g * Hkv
    q, kc, vc, bt, _, _ = _setup(lq, H, Hkv, D, ps, -(-max(cache) // ps), DT[dt], seed=90 + D)
    kd, vd = _descales(len(lq), Hkv, seed=90 + D)
    cu, sl = _i32(_cu(lq)), _i32(cache)
    o, _, kernel = _run(q, kc, vc, cu, max(lq), sl, bt, kd, vd, causal=True, num_splits=num_splits)
    if num_splits:
        assert ("split" in kernel) == (num_splits > 1), kernel
    want, lse = _reference(q, kc, vc, cu, max(lq), sl, bt, kd, vd, causal=True)[:2]
    floor = _reference(q, kc, vc, cu, max(lq), sl, bt, kd, vd, causal=True, kind=ffr.KIND)[0]
    div = _vd_rows(vd, cu, sum(lq), max(lq), H)
    got = _np(o)
    nk = np.zeros(sum(lq), np.int64)
    decode = np.zeros(sum(lq), bool)
    for (q0, Lq), L in zip(vref.ranges(cu.cpu().numpy(), sum(lq), max(lq)), cache):
        nk[q0:q0 + Lq] = np.clip(np.arange(Lq) + L - Lq + 1, 0, L)  # bottom-right causal, every page in the pool
        decode[q0:q0 + Lq] = g * Lq <= 32
    for dec in (True, False):
        sel = decode == dec
        rows = lambda a: (a / div)[sel].reshape(-1, D)  # noqa: E731
        ffr.check_pool(rows(got), rows(want), rows(floor), np.repeat(nk[sel], H), dt, kernel,
                       f"packed fp8 {'decode' if dec else '128-row'} items {dt}", ffr.form_regime(32 if dec else 128, "split" in kernel),
                       live=np.isfinite(lse).T[sel])


@pytest.mark.parametrize("dt,D", [("bf16", 128), ("fp16", 64)])
@pytest.mark.parametrize("num_splits", [1, 3])
def test_table_reload_boundary(dt, D, num_splits):
    """L_k in (1024, 1300]: the kernel reloads its block-table vector every 8 steps (1024 keys) and requests stages two steps ahead, so
    these sequences cross a reload with requests in flight; 1100 / 1300 beside short ones, both forms"""
    g, Hkv, ps = 4, 2, 16
    lq, slv = [1, 40, 3, 130, 2], [1100, 1300, 20, 1050, 1024]
    q, kc, vc, bt, _, _ = _setup(lq, g * Hkv, Hkv, D, ps, 82, DT[dt], seed=41 + D)
    kd, vd = _descales(len(lq), Hkv, seed=41)
    cu, sl = _i32(_cu(lq)), _i32(slv)
    refs = _reference(q, kc, vc, cu, max(lq), sl, bt, kd, vd, causal=True)
    o, lse, kernel = _run(q, kc, vc, cu, max(lq), sl, bt, kd, vd, causal=True, num_splits=num_splits)
    assert ("split" in kernel) == (num_splits > 1), kernel
    _check(refs, cu, max(lq), vd, o, lse, kernel, dt=dt)


# ------------------------------------------------------------------------------------------------ bitwise agreement at equal lengths
@pytest.mark.parametrize("Sq,new", [(1, False), (1, True), (4, False), (4, True), (40, False), (40, True)])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("num_splits", [1, 3])
def test_equal_lengths_agree_bitwise_with_kvcache_attention(Sq, new, dt, num_splits):
    """every L_q equal: the arithmetic and its order are kvcache_attention's fp8 call's (same rows per wave, steps, parts and fold)"""
    um = _umfa()
    B, H, Hkv, D, ps, mp = 4, 8, 2, 128, 16, 40
    q, kc, vc, bt, kn, vn = _setup([Sq] * B, H, Hkv, D, ps, mp, DT[dt], seed=30 + Sq, new=new, share=False)
    kd, vd = _descales(B, Hkv, seed=30)
    cu, sl = _i32(_cu([Sq] * B)), _i32([0, 150, ps + 5, 600])
    kc0, kc2, vc2 = kc.clone(), kc.clone(), vc.clone()
    o, lse, kernel = _run(q, kc, vc, cu, Sq, sl, bt, kd, vd, kn, vn, causal=True, num_splits=num_splits)
    r = lambda t: None if t is None else t.view(B, Sq, *t.shape[1:])  # noqa: E731
    o2, lse2 = um.ops.kvcache_attention_fp8_forward(r(q), kc2, vc2, sl, kd, vd, bt, r(kn), r(vn), scale=D ** -0.5, causal=True,
                                                    num_splits=num_splits, out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert um.last_kernel() == kernel.replace("_varlen", "")
    assert torch.equal(o.view(B, Sq, H, D), o2)
    assert torch.equal(lse.view(H, B, Sq).permute(1, 0, 2), lse2)
    assert (_bytes(kc) == _bytes(kc2)).all() and (_bytes(vc) == _bytes(vc2)).all()
    assert (_bytes(kc) == _bytes(kc0)).all() != new  # (and something was appended)


@pytest.mark.parametrize("causal,inter,dt", [(True, False, "bf16"), (False, True, "fp16")])
def test_equal_lengths_with_rotary_agree_bitwise_with_kvcache_attention(causal, inter, dt):
    um = _umfa()
    B, L, H, Hkv, D, ps, mp = 3, 4, 8, 2, 128, 16, 6
    q, kc, vc, bt, kn, vn = _setup([L] * B, H, Hkv, D, ps, mp, DT[dt], seed=301, new=True, share=False)
    kd, vd = _descales(B, Hkv, seed=301)
    cos, sin = tables(104, 64, torch.float32, 302)
    cu, sl = _i32(_cu([L] * B)), _i32([14, 0, 47])
    kc2, vc2 = kc.clone(), vc.clone()
    o, lse, kernel = _run(q, kc, vc, cu, L, sl, bt, kd, vd, kn, vn, causal=causal, num_splits=2, rotary_cos=cos, rotary_sin=sin,
                          rotary_interleaved=inter)
    o2, lse2 = um.ops.kvcache_attention_rope_forward(q.view(B, L, H, D), kc2, vc2, sl, cos, sin, bt, kn.view(B, L, Hkv, D),
                                                     vn.view(B, L, Hkv, D), scale=D ** -0.5, causal=causal, num_splits=2,
                                                     rotary_interleaved=inter, k_descale=kd, v_descale=vd, out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert um.last_kernel() == kernel.replace("_varlen", "")
    assert torch.equal(o.view(B, L, H, D), o2) and torch.equal(lse.view(H, B, L).transpose(0, 1), lse2)
    assert (_bytes(kc) == _bytes(kc2)).all() and (_bytes(vc) == _bytes(vc2)).all()


# ------------------------------------------------------------------------------------------------ append
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("static", [False, "bshd", "bhsd"])
def test_append_quantises_rows_bitwise_and_nothing_else(dt, static):
    lq, H, Hkv, D = [5, 0, 1, 40, 3], 8, 2, 64
    if static:
        g = torch.Generator(device="cuda").manual_seed(11)
        q = torch.randn(sum(lq), H, D, device="cuda", dtype=DT[dt], generator=g)
        kc, vc = tf._static(static, len(lq), 48, Hkv, D, g)
        kn = torch.randn(sum(lq), Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        vn = torch.randn(sum(lq), Hkv, D, device="cuda", dtype=DT[dt], generator=g)
        bt = None
    else:
        q, kc, vc, bt, kn, vn = _setup(lq, H, Hkv, D, 16, 3, DT[dt], seed=12, new=True, share=False)
    kn[0, 0, :4] = torch.tensor([1e4, -1e4, 0.0, -0.0], dtype=DT[dt])  # beyond +-448 descale: saturates; both zeros
    vn[6, 1, :4] = torch.tensor([-3e4, 3e4, -0.0, 0.0], dtype=DT[dt])
    kd, vd = _descales(len(lq), Hkv, seed=12)  # arbitrary (not power-of-two) descales: the division must be IEEE
    cu, sl = _i32(_cu(lq)), _i32([14, 7, 47, 3, 46])  # page crossings; the last one runs past the capacity of 48: one row dropped
    kc0, vc0 = kc.clone(), vc.clone()
    refs = _reference(q, kc0, vc0, cu, 40, sl, bt, kd, vd, kn, vn, causal=True)
    o, lse, kernel = _run(q, kc, vc, cu, 40, sl, bt, kd, vd, kn, vn, causal=True)
    kw, vw = refs[3], refs[4]
    assert (_bytes(kc) == kw).all() and (_bytes(vc) == vw).all()  # the rows written, bitwise, and every other byte unchanged
    changed = (kw != _bytes(kc0)).reshape(*kw.shape[:2], -1).any(-1)
    assert changed.sum() == sum(lq) - 1  # every row but the dropped one
    if static == "bhsd":  # the storage as allocated: every byte of it
        assert (_bytes(kc.transpose(1, 2)) == kw.transpose(0, 2, 1, 3)).all()
    if not static:
        assert (_bytes(kc)[:GUARD] == _bytes(kc0)[:GUARD]).all() and (_bytes(kc)[-GUARD:] == _bytes(kc0)[-GUARD:]).all()
        assert (_bytes(vc)[:GUARD] == _bytes(vc0)[:GUARD]).all() and (_bytes(vc)[-GUARD:] == _bytes(vc0)[-GUARD:]).all()
        pg, row = int(bt[0, 0]), 14
    else:
        pg, row = 0, 14
    assert _bytes(kc)[pg, row, 0, :4].tolist() == [0x7e, 0xfe, 0x00, 0x80]  # +-448, +0, -0
    _check(refs, cu, 40, vd, o, lse, kernel, dt=dt)
    assert (sl.cpu().numpy() == [14, 7, 47, 3, 46]).all()  # cache_seqlens is not advanced
    # append + attention = attention on the appended cache with the advanced lengths (clamped at the capacity)
    sl2 = _i32(np.minimum(np.array([14, 7, 47, 3, 46]) + np.array(lq), 48))
    o2, lse2, _ = _run(q, kc, vc, cu, 40, sl2, bt, kd, vd, causal=True)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


def test_append_drops_rows_past_the_capacity_and_outside_the_pool():
    lq, H, Hkv, D, ps, mp = [3, 2, 4, 1], 8, 2, 128, 16, 4
    q, kc, vc, bt, kn, vn = _setup(lq, H, Hkv, D, ps, mp, torch.bfloat16, seed=13, new=True, share=False)
    kd, vd = _descales(len(lq), Hkv, seed=13)
    btn = bt.cpu().numpy()
    btn[1, 1] = kc.shape[0]  # sequence 1 appends at 30, 31: logical page 1, one past the pool
    btn[2, 0] = -1           # sequence 2 appends at 14 .. 17: rows 14, 15 dropped, 16, 17 land on page 1
    bt = torch.tensor(btn, device="cuda")
    cu, sl = _i32(_cu(lq)), _i32([62, 30, 14, 10 ** 9])  # sequence 0: row 2 past the capacity of 64; sequence 3: all of it
    kc0, vc0 = kc.clone(), vc.clone()
    refs = _reference(q, kc0, vc0, cu, 4, sl, bt, kd, vd, kn, vn, causal=True, min_live=0.0)
    o, lse, kernel = _run(q, kc, vc, cu, 4, sl, bt, kd, vd, kn, vn, causal=True)
    assert (_bytes(kc) == refs[3]).all() and (_bytes(vc) == refs[4]).all()
    wrote = (_bytes(kc) != _bytes(kc0)).reshape(*kc.shape[:2], -1).any(-1)
    assert wrote.sum() == 2 + 0 + 2 + 0 and not wrote[:GUARD].any() and not wrote[-GUARD:].any()
    _check(refs, cu, 4, vd, o, lse, kernel)


# ------------------------------------------------------------------------------------------------ poison and clamps
@pytest.mark.parametrize("num_splits", [1, 3])
@pytest.mark.parametrize("causal", [False, True])
def test_nan_bytes_where_no_key_lives_change_nothing(num_splits, causal):
    """0x7f / 0xff (e4m3fn's NaNs) in the rows at and past L_k of each sequence's last page and in every page no table names: O and LSE
    are bit-identical to the same call with zeros there (masked keys never reach the sums, rows past L_k are never fetched)"""
    g, Hkv, D, ps, mp = 4, 2, 128, 16, 6
    lq, slv = [1, 40, 3, 0, 9], [37, 70, 96, 50, 5]
    q, kc, vc, bt, _, _ = _setup(lq, g * Hkv, Hkv, D, ps, mp, torch.bfloat16, seed=51, share=False)
    kd, vd = _descales(len(lq), Hkv, seed=51)
    cu, sl = _i32(_cu(lq)), _i32(slv)
    btn = bt.cpu().numpy()
    dead = torch.zeros(kc.shape[:2], dtype=torch.bool, device="cuda")
    dead[:GUARD] = True
    dead[-GUARD:] = True
    for b, L in enumerate(slv):
        for lp in range(mp):
            lo = min(max(L - lp * ps, 0), ps)  # rows of this page below L_k
            dead[btn[b, lp], lo:] = True
    assert dead.any(1).sum() >= 2 * GUARD + len(lq)
    res = []
    for fill in (0x00, 0x7f, 0xff):
        k2, v2 = kc.clone(), vc.clone()
        k2.view(torch.uint8)[dead] = fill
        v2.view(torch.uint8)[dead] = fill
        res.append(_run(q, k2, v2, cu, max(lq), sl, bt, kd, vd, causal=causal, num_splits=num_splits))
    for o, lse, _ in res[1:]:
        assert torch.equal(o.view(torch.int32), res[0][0].view(torch.int32)) and torch.equal(lse.view(torch.int32), res[0][1].view(torch.int32))
    refs = _reference(q, kc, vc, cu, max(lq), sl, bt, kd, vd, causal=causal)
    _check(refs, cu, max(lq), vd, *res[0])


@pytest.mark.parametrize("num_splits", [0, 3])
@pytest.mark.parametrize("cu_kind", ["good", "non_monotone", "beyond"])
def test_hostile_contents_touch_nothing_else(num_splits, cu_kind):
    """test_gpu_varlen_paged.py's hostile case on fp8 pools: table entries -1 / num_pages / 2^31 - 1 / -2^31, lengths negative and 10^9,
    cu non-monotone and beyond T_q -- the outputs are finite, the guard pages and the canary rows round q / k / v / O / LSE unchanged"""
    um = _umfa()
    H, Hkv, D, ps, mp, C = 8, 2, 128, 16, 4, 8
    lq = [3, 2, 40, 1, 5]
    Tq = sum(lq)
    _, kc, vc, bt, _, _ = _setup(lq, H, Hkv, D, ps, mp, torch.bfloat16, seed=14, share=False)
    kd, vd = _descales(len(lq), Hkv, seed=14)
    g = torch.Generator(device="cuda").manual_seed(77)
    q_big = torch.randn(Tq + 2 * C, H, D, device="cuda", dtype=torch.bfloat16, generator=g)
    kn_big = torch.randn(Tq + 2 * C, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
    vn_big = torch.randn(Tq + 2 * C, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
    o_big = torch.full((Tq + 2 * C, H, D), 7.0, device="cuda", dtype=torch.float32)
    lse_big = torch.full(((H + 2 * C) * Tq,), 7.0, device="cuda", dtype=torch.float32)
    q, kn, vn, out, lse = q_big[C:C + Tq], kn_big[C:C + Tq], vn_big[C:C + Tq], o_big[C:C + Tq], lse_big[C * Tq:(C + H) * Tq].view(H, Tq)
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
    um.ops.varlen_kvcache_attention_fp8_forward(q, kc, vc, cu, 40, sl, kd, vd, bt, kn, vn, scale=D ** -0.5, causal=True, num_splits=num_splits,
                                                out=out, lse=lse)
    torch.cuda.synchronize()
    assert um.last_kernel().startswith(PREFIX)
    for a, b in ((kc, kc0), (vc, vc0)):
        assert (_bytes(a)[:GUARD] == _bytes(b)[:GUARD]).all() and (_bytes(a)[-GUARD:] == _bytes(b)[-GUARD:]).all()
    assert torch.equal(q_big, q0) and torch.equal(kn_big, kn0) and torch.equal(vn_big, vn0)
    assert (o_big[:C] == 7.0).all() and (o_big[C + Tq:] == 7.0).all()
    assert (lse_big[:C * Tq] == 7.0).all() and (lse_big[(C + H) * Tq:] == 7.0).all()
    assert torch.isfinite(out).all() and not torch.isnan(lse).any() and not torch.isposinf(lse).any()
    if cu_kind == "good":  # defined results: the pools equal the reference's append, the values its attention
        refs = _reference(q, kc0, vc0, cu, 40, sl, bt, kd, vd, kn, vn, causal=True, min_live=0.0)
        assert (_bytes(kc) == refs[3]).all() and (_bytes(vc) == refs[4]).all()
        _check(refs, cu, 40, vd, out, lse, "fa_fwd16_paged_varlen_fp8<bf16,128,causal,pv16>")


# ------------------------------------------------------------------------------------------------ layouts and shape
@pytest.mark.parametrize("static", ["bshd", "bhsd"])
def test_static_cache_mixed_batch(static):
    lq, H, Hkv, D, Smax = [1, 200, 0, 4, 33], 8, 2, 128, 300
    g = torch.Generator(device="cuda").manual_seed(5)
    q = torch.randn(sum(lq), H, D, device="cuda", dtype=torch.bfloat16, generator=g)
    kc, vc = tf._static(static, len(lq), Smax, Hkv, D, g)  # bhsd: HF StaticCache's [B, S_max, H_kv, D] view, byte strides
    kd, vd = _descales(len(lq), Hkv, seed=5)
    cu, sl = _i32(_cu(lq)), _i32([17, 300, 129, 0, 250])
    for causal in (False, True):
        refs = _reference(q, kc, vc, cu, 200, sl, None, kd, vd, causal=causal)
        o, lse, kernel = _run(q, kc, vc, cu, 200, sl, None, kd, vd, causal=causal)
        _check(refs, cu, 200, vd, o, lse, kernel)


def test_uncovered_rows_are_not_written():
    um = _umfa()
    lq, pad = [3, 50, 1], 6  # max_seqlen_q = 20 caps the 50-token sequence: its rows 20 .. 49 and the 6 pad rows belong to nobody
    q, kc, vc, bt, _, _ = _setup(lq, 8, 2, 64, 16, 8, torch.float16, seed=23, pad=pad)
    kd, vd = _descales(len(lq), 2, seed=23)
    Tq = q.shape[0]
    out = torch.full((Tq, 8, 64), 7.0, device="cuda", dtype=torch.float32)
    lse = torch.full((8, Tq), 7.0, device="cuda", dtype=torch.float32)
    cu, sl = _i32(_cu(lq)), _i32([100, 90, 128])
    for n in (1, 2):
        um.ops.varlen_kvcache_attention_fp8_forward(q, kc, vc, cu, 20, sl, kd, vd, bt, scale=0.125, num_splits=n, out=out, lse=lse)
        torch.cuda.synchronize()
        cov = torch.tensor(vref.covered(_cu(lq), Tq, 20), device="cuda")
        assert cov.sum().item() == 3 + 20 + 1
        assert (out[~cov] == 7.0).all() and (lse[:, ~cov] == 7.0).all()
        refs = _reference(q, kc, vc, cu, 20, sl, bt, kd, vd, min_live=0.0)
        _check(refs, cu, 20, vd, out, lse, "fa_fwd16_paged_varlen_fp8<fp16,64>", dt="fp16")


def test_strided_q_from_a_fused_projection():
    um = _umfa()
    lq, H, Hkv, D = [1, 70, 4, 9], 8, 2, 128
    _, kc, vc, bt, _, _ = _setup(lq, H, Hkv, D, 16, 8, torch.bfloat16, seed=24, share=False)
    kd, vd = _descales(len(lq), Hkv, seed=24)
    g = torch.Generator(device="cuda").manual_seed(25)
    qkv = torch.randn(sum(lq), (H + 2 * Hkv) * D, device="cuda", dtype=torch.bfloat16, generator=g)
    q = qkv[:, :H * D].view(sum(lq), H, D)
    k = qkv[:, H * D:(H + Hkv) * D].view(sum(lq), Hkv, D)
    v = qkv[:, (H + Hkv) * D:].view(sum(lq), Hkv, D)
    assert not q.is_contiguous() and q.stride(0) == (H + 2 * Hkv) * D
    cu, sl = _i32(_cu(lq)), _i32([17, 30, 0, 100])
    kc0, vc0 = kc.clone(), vc.clone()
    refs = _reference(q, kc0, vc0, cu, 70, sl, bt, kd, vd, k, v, causal=True)
    o, lse = um.varlen_kvcache_attention(q, kc, vc, cu, 70, sl, block_table=bt, k=k, v=v, causal=True, return_softmax_lse=True,
                                         k_descale=kd, v_descale=vd)
    torch.cuda.synchronize()
    assert o.dtype == torch.bfloat16 and o.shape == q.shape and o.is_contiguous() and lse.shape == (H, sum(lq))
    assert um.last_kernel().startswith(PREFIX)
    _check(refs, cu, 70, vd, o, lse, um.last_kernel(), out_dt=torch.bfloat16)
    o2, lse2, _ = _run(q.contiguous(), kc0, vc0, cu, 70, sl, bt, kd, vd, k.contiguous(), v.contiguous(), causal=True, out_dtype=torch.bfloat16)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)  # the strides, not a copy
    assert (_bytes(kc) == _bytes(kc0)).all() and (_bytes(vc) == _bytes(vc0)).all()


def test_both_forms_in_one_launch():
    um = _umfa()
    H, Hkv, D, ps, mp = 8, 2, 128, 16, 20
    for lq in ([1, 1, 1], [300, 129], [1, 300, 4, 9, 0, 128]):
        q, kc, vc, bt, _, _ = _setup(lq, H, Hkv, D, ps, mp, torch.bfloat16, seed=len(lq))
        kd, vd = _descales(len(lq), Hkv, seed=len(lq))
        for n in (1, 3):
            _, _, kernel = _run(q, kc, vc, _i32(_cu(lq)), max(lq), _i32([300] * len(lq)), bt, kd, vd, causal=True, num_splits=n)
            assert um.ops.varlen_kvcache_item_counts() == tv._items(lq, H // Hkv, Hkv), (lq, n)
            assert kernel == "fa_fwd16_paged_varlen_fp8<bf16,128,causal,pv16" + (",split>" if n > 1 else ">")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("mix", ["decode", "mixed"])
def test_forced_and_automatic_splits(dt, mix):
    """1, 2, 5 and 30 forced parts and the library's own choice; 30 parts over sequences of 64 / 9 / 0 keys are mostly empty"""
    H, Hkv, D, ps, mp = 32, 8, 128, 64, 40
    lq = [1, 1, 2, 1] if mix == "decode" else [1, 150, 0, 2, 40]
    slv = [2500, 1111, 64, 0] if mix == "decode" else [2500, 1111, 9, 777, 2560]
    q, kc, vc, bt, _, _ = _setup(lq, H, Hkv, D, ps, mp, DT[dt], seed=15)
    kd, vd = _descales(len(lq), Hkv, seed=15)
    cu, sl = _i32(_cu(lq)), _i32(slv)
    refs = _reference(q, kc, vc, cu, max(lq), sl, bt, kd, vd, causal=True)
    for n in (1, 2, 5, 30, 0):
        o, lse, kernel = _run(q, kc, vc, cu, max(lq), sl, bt, kd, vd, causal=True, num_splits=n)
        if n:
            assert (n > 1) == ("split" in kernel), kernel
        _check(refs, cu, max(lq), vd, o, lse, kernel, dt=dt)
        o2, lse2, _ = _run(q, kc, vc, cu, max(lq), sl, bt, kd, vd, causal=True, num_splits=n)
        assert torch.equal(o, o2) and torch.equal(lse, lse2)  # the fold takes the parts in order: bitwise repeatable


# ------------------------------------------------------------------------------------------------ fused rotary
# (dtype, head_dim, rotary_dim, interleaved, causal, fp32 tables, cache, num_splits, pad rows)
ROPE_GRID = [("bf16", 128, 128, False, True, True, "paged", 0, 0), ("fp16", 64, 64, True, True, False, "paged", 0, 0),
             ("bf16", 64, 32, True, False, True, "paged", 0, 3), ("fp16", 128, 16, False, True, False, "paged", 2, 0),
             ("bf16", 128, 32, False, False, False, "bshd", 2, 3), ("fp16", 128, 64, True, False, True, "bhsd", 0, 0)]
ROPE_LQ, ROPE_SL = [1, 35, 2, 0], [47, 14, 0, 30]  # decode, a 128-row prefill chunk, speculative decode, an idle sequence; capacity 96


@pytest.mark.parametrize("dt,D,rd,inter,causal,f32,cache,splits,pad", ROPE_GRID)
def test_fused_rotary_equals_the_plain_call_on_rotated_operands(dt, D, rd, inter, causal, f32, cache, splits, pad):
    """O, LSE and both pools, bit for bit: the fused call against the plain fp8 packed call on q / k rotated by ops.rope_rotate at the
    packed rows' positions (every query row of a non-causal call at L0_b) and rounded to the operand type"""
    um = _umfa()
    H, Hkv, ps, mp, lq = 8, 2, 16, 6, ROPE_LQ
    seed = 200 + ROPE_GRID.index((dt, D, rd, inter, causal, f32, cache, splits, pad))
    q, kc, vc, bt, kn, vn = _setup(lq, H, Hkv, D, ps, mp, DT[dt], seed, new=True, share=False, pad=pad)
    if cache != "paged":
        kc, vc = tf._static(cache, len(lq), ps * mp, Hkv, D, torch.Generator(device="cuda").manual_seed(seed))
        bt = None
    kd, vd = _descales(len(lq), Hkv, seed)
    cos, sin = tables(104, rd, torch.float32 if f32 else DT[dt], seed, pad=8 if pad else 0)
    cu, sl = _i32(_cu(lq)), _i32(ROPE_SL)
    k1, v1 = kc.clone(), vc.clone()
    o1, lse1, kern1 = _run(q, k1, v1, cu, max(lq), sl, bt, kd, vd, kn, vn, causal=causal, num_splits=splits, out_dtype=DT[dt],
                           rotary_cos=cos, rotary_sin=sin, rotary_interleaved=inter)
    assert um.ops.varlen_kvcache_item_counts() == (2 * Hkv, 2 * Hkv), "decode-form and 128-row items in one launch"
    c, s = cu.cpu().numpy(), sl.cpu().numpy()
    pq, cov = rr.packed_positions(c, q.shape[0], max(lq), s, ps * mp, causal)
    pk, _ = rr.packed_positions(c, q.shape[0], max(lq), s, ps * mp, True)
    covt = torch.tensor(cov, device="cuda")
    rq = torch.where(covt[:, None, None], rotate_by_ops(um, q, pq, cos, sin, inter), q)
    rk = torch.where(covt[:, None, None], rotate_by_ops(um, kn, pk, cos, sin, inter), kn)
    k2, v2 = kc.clone(), vc.clone()
    o2, lse2, kern2 = _run(rq, k2, v2, cu, max(lq), sl, bt, kd, vd, rk, vn, causal=causal, num_splits=splits, out_dtype=DT[dt])
    assert kern1 == kern2 and ("split" in kern1) == (splits > 1)
    assert torch.equal(o1[covt].view(torch.int16), o2[covt].view(torch.int16))
    assert torch.equal(lse1[:, covt].view(torch.int32), lse2[:, covt].view(torch.int32))
    assert (_bytes(k1) == _bytes(k2)).all() and (_bytes(v1) == _bytes(v2)).all()
    assert not (_bytes(k1) == _bytes(kc)).all()  # something was appended
    refs = _reference(rq, kc, vc, cu, max(lq), sl, bt, kd, vd, rk, vn, causal=causal)  # and the values are the reference's
    _check(refs, cu, max(lq), vd, o1, lse1, kern1, dt=dt, out_dt=DT[dt])


# ------------------------------------------------------------------------------------------------ graph replay
def test_graph_replay_follows_cu_lengths_table_and_descales():
    um = _umfa()
    H, Hkv, D, ps, mp, Tq, max_q = 8, 2, 128, 16, 16, 120, 100
    heavy, light = [100, 18, 1, 1], [1, 1, 2, 1]  # prefill-heavy, then decode-heavy at the same T_q, B and max_seqlen_q
    q, kc, vc, bt, kn, vn = _setup(heavy, H, Hkv, D, ps, mp, torch.bfloat16, seed=18, new=True, share=False)
    kd, vd = _descales(len(heavy), Hkv, seed=18)
    cu, sl = _i32(_cu(heavy)), _i32([40, 100, 7, 0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def step():
        return um.varlen_kvcache_attention(q, kc, vc, cu, max_q, sl, block_table=bt, k=kn, v=vn, causal=True, num_splits=3,
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
        sl.add_(29)
        if it >= 1:
            cu.copy_(_i32(_cu(light)))
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
        assert um.last_kernel().startswith(PREFIX)
        cov = torch.tensor(vref.covered(cu.cpu().numpy(), Tq, max_q), device="cuda")
        assert torch.equal(got[0][cov], want[0][cov]) and torch.equal(got[1][:, cov], want[1][:, cov]), it
        assert (_bytes(kr) == _bytes(kc)).all() and (_bytes(vr) == _bytes(vc)).all(), it
        refs = _reference(q, kc0, vc0, cu, max_q, sl, bt, kd, vd, kn, vn, causal=True, min_live=0.0)
        _check(refs, cu, max_q, vd, got[0], got[1], um.last_kernel(), out_dt=torch.bfloat16)
        assert (_bytes(kr) == refs[3]).all()
        assert int(cov.sum()) == (Tq if it == 0 else 5)


# ------------------------------------------------------------------------------------------------ plumbing
def test_opcheck_custom_ops():
    _umfa()
    lq = [2, 40, 1]
    q, kc, vc, bt, kn, vn = _setup(lq, 8, 2, 64, 16, 4, torch.bfloat16, seed=19, new=True, share=False)
    kd, vd = _descales(len(lq), 2, seed=19)
    cos, sin = tables(80, 32, torch.float32, 19)
    cu, sl = _i32(_cu(lq)), _i32([5, 20, 33])
    k8, v8 = kc.view(torch.uint8), vc.view(torch.uint8)  # the ops take the caches' bytes (torch's schema check has no float8 kernels)
    torch.library.opcheck(torch.ops.umfa.varlen_kvcache_fp8_forward.default, (q, k8, v8, cu, 40, sl, kd, vd, bt, True, 0.125, 0))
    torch.library.opcheck(torch.ops.umfa.varlen_kvcache_fp8_forward_append.default, (q, k8, v8, kn, vn, cu, 40, sl, kd, vd, bt, True, 0.125, 2))
    torch.library.opcheck(torch.ops.umfa.varlen_kvcache_fp8_rope_forward_append.default,
                          (q, k8, v8, kn, vn, cu, 40, sl, kd, vd, cos, sin, True, bt, True, 0.125, 2))


@pytest.mark.parametrize("rotary", [False, True])
def test_compile_fullgraph_single_node(rotary):
    um = _umfa()
    lq = [1, 35, 2]
    q, kc, vc, bt, kn, vn = _setup(lq, 8, 2, 128, 16, 8, torch.float16, seed=20, new=True, share=False)
    kd, vd = _descales(len(lq), 2, seed=20)
    cos, sin = tables(128, 64, torch.float32, 20)
    cu, sl = _i32(_cu(lq)), _i32([30, 64, 1])
    rope = dict(rotary_cos=cos, rotary_sin=sin) if rotary else {}
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    def f(q, kc, vc, kn, vn):
        return um.varlen_kvcache_attention(q, kc, vc, cu, 35, sl, block_table=bt, k=kn, v=vn, causal=True, k_descale=kd, v_descale=vd, **rope)

    kc0, kc_e, vc_e = kc.clone(), kc.clone(), vc.clone()
    torch._dynamo.reset()
    oc = torch.compile(f, fullgraph=True, backend=backend)(q, kc, vc, kn, vn)
    oe = f(q, kc_e, vc_e, kn, vn)
    torch.cuda.synchronize()
    assert len(graphs) == 1
    calls = [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function" and "umfa" in str(n.target)]
    assert calls == ["umfa.varlen_kvcache_fp8_rope_forward_append" if rotary else "umfa.varlen_kvcache_fp8_forward_append"], calls
    assert torch.equal(oc, oe)
    assert (_bytes(kc) == _bytes(kc_e)).all() and (_bytes(vc) == _bytes(vc_e)).all()  # the compiled call appended in place too
    assert not (_bytes(kc) == _bytes(kc0)).all()


def test_refusals_and_no_backward():
    um = _umfa()
    lq = [1, 20, 3]
    q, kc, vc, bt, kn, vn = _setup(lq, 8, 2, 128, 16, 4, torch.bfloat16, seed=21, new=True, share=False)
    kd, vd = _descales(len(lq), 2, seed=21)
    cu, sl = _i32(_cu(lq)), _i32([10, 20, 30])
    kc0, vc0 = kc.clone(), vc.clone()
    call = lambda k_, v_, **kw: um.varlen_kvcache_attention(q, k_, v_, cu, 20, sl, block_table=bt, k=kn, v=vn, **kw)  # noqa: E731
    both = dict(k_descale=kd, v_descale=vd)
    for kw in (dict(), dict(k_descale=kd), dict(v_descale=vd), dict(k_descale=1.0), dict(v_descale=0.5)):
        with pytest.raises(ValueError):  # fp8 caches are served only when BOTH descales are given
            call(kc, vc, **kw)
    k16, v16 = kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    for kw in (dict(k_descale=kd), dict(v_descale=1.0), both):
        with pytest.raises(ValueError):  # descales with a 16-bit cache
            call(k16, v16, **kw)
    raw = kc.view(torch.uint8)
    for k_, v_ in ((raw.view(torch.float8_e4m3fnuz), raw.view(torch.float8_e4m3fnuz)), (raw.view(torch.float8_e5m2), raw.view(torch.float8_e5m2)),
                   (raw, raw), (kc, v16), (k16, vc), (kc, vc.view(torch.uint8).view(torch.float8_e5m2))):  # other 8-bit formats; mixed K / V
        with pytest.raises(ValueError):
            call(k_, v_, **both)
    for bad in (kd.double(), kd.cpu(), _dev([1.0, 2.0, 3.0]), _dev(np.ones((4, 2))), _dev(np.ones((3, 2, 1))), kd.to(torch.bfloat16), "1.0"):
        with pytest.raises(ValueError):  # descales of the wrong dtype / device / shape ([B, H_kv] = [3, 2] here)
            call(kc, vc, k_descale=bad, v_descale=vd)
        with pytest.raises(ValueError):
            call(kc, vc, k_descale=kd, v_descale=bad)
    with pytest.raises(ValueError):  # a token stride that is not a multiple of 16 bytes
        pool = torch.zeros(kc.shape[0], 16, 2, 136, device="cuda", dtype=torch.uint8).view(F8)
        call(pool[..., :128], pool[..., :128], **both)
    with pytest.raises(ValueError):  # page_size not a multiple of 16
        call(kc[:, :8].contiguous(), vc[:, :8].contiguous(), **both)
    for kw in (dict(window_size=(8, 0)), dict(softcap=30.0), dict(rotary_cos=torch.zeros(1)), dict(seqused_k=sl)):
        with pytest.raises(ValueError):  # no window on this entry; malformed tables
            call(kc, vc, **both, **kw)
    with pytest.raises(ValueError):  # rotary needs new tokens
        cos, sin = tables(64, 64, torch.float32, 21)
        um.varlen_kvcache_attention(q, kc, vc, cu, 20, sl, block_table=bt, rotary_cos=cos, rotary_sin=sin, **both)
    with pytest.raises(ValueError):  # the ops entry refuses the same formats: there is no fall-back
        um.ops.varlen_kvcache_attention_fp8_forward(q, k16, v16, cu, 20, sl, kd, vd, bt, scale=0.1)
    torch.cuda.synchronize()
    assert (_bytes(kc) == _bytes(kc0)).all() and (_bytes(vc) == _bytes(vc0)).all()  # nothing was appended by a refused call
    for kd_, vd_ in ((kd, vd), (0.5, 2.0), (kd[0], vd[:, :1]), (kd.new_tensor(0.5), 1)):  # [B, H_kv], floats, [H_kv] / [B, 1], 0-d
        o = call(kc.clone(), vc.clone(), k_descale=kd_, v_descale=vd_)
        torch.cuda.synchronize()
        assert o.shape == q.shape and o.dtype == q.dtype and um.last_kernel().startswith("fa_fwd16_paged_varlen_fp8<bf16,128")
    o = um.varlen_kvcache_attention(q.clone().requires_grad_(True), kc.clone(), vc.clone(), cu, 20, sl, block_table=bt, k=kn, v=vn, **both)
    with pytest.raises(RuntimeError):  # inference only: no backward
        o.float().sum().backward()
