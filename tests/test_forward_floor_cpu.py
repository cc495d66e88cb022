"""The forward format floor of the KV-cache, banded and dropout forwards without a GPU (the references' forward(kind=...),
tolerances.check_forward(floor=, regime=), tests/forward_floor_ref.py).

- Each reference's floor is oracle.flash_format_floor on an equal-length dense case (bottom-right causal through zero-padded Q rows, as
  the packed forward's tests do), and kind=None returns the values it returned before, bit for bit.
- An fp64 emulation of the paged kernels' arithmetic (128-key steps, per-tile running max, the decode form's quarters, split parts) is
  ACCEPTED by the bounds at the shapes tests/test_gpu_forward_floor.py runs, for both input types and head dims, over 5 seeds: 16-bit and
  fp8 caches in the decode form, the 128-row form and its split cases, the static view's shape, the append across a page boundary and the
  table with holes; the packed batch (each sequence as its own call); the band at every window, causal and not; the dropout forward on
  a spread of rows of each shape.  The bounds hold for a kernel that does nothing worse than the format asks.  (Page sizes and views change
  no arithmetic: the emulation runs the 128-row lengths of all three page sizes on a static cache.)  test_zz_report prints the clean
  emulation's rms ratio to the floor per fp8 / one-each form: profiles/fwd_floor/summary.md quotes it beside the kernels' ratios.
- The same emulation is REJECTED with one planted defect each: P in bf16 under fp16, P truncated, split partial O in fp16, fold weights
  in fp16, the last key of a ragged page dropped, the neighbouring KV head's v_descale, dropout's keep applied after the rounding of P
  with 1 / (1 - p) folded into P, and the floor's error x 1.15 everywhere (by the rms bound alone).  Each rejection is matched to the
  bound that has to make it: the floor's for the defects the ceiling lets through (partial O, fold weights, keep after the rounding).
"""
import numpy as np
import pytest

import dropout_ref
import forward_floor_ref as ffr
import paged_fp8_ref
import paged_ref
import tolerances as tol
import varlen_paged_ref
import varlen_window_ref
from oracle import oracle as orc

SEEDS = 5


def _rnd(rng, shape, dt):
    """N(0, 1) values of the input type, as fp64"""
    return orc.round_to(rng.standard_normal(shape), dt)


def _oracle_in(x, dt):
    """[.., D] fp64 values of the type -> what the oracle takes (bf16 as uint16 bits)"""
    x = np.ascontiguousarray(x, np.float32)
    return x.astype(np.float16) if dt == "fp16" else orc.f32_to_bf16_bits(x).reshape(x.shape)


# ------------------------------------------------------------------------------------------- floors against oracle.flash_format_floor
def _dense_case(dt, B, Sq, L, H, Hkv, D, seed):
    rng = np.random.default_rng(seed)
    return _rnd(rng, (B, Sq, H, D), dt), _rnd(rng, (B, L, Hkv, D), dt), _rnd(rng, (B, L, Hkv, D), dt)


def _dense_floor(q, k, v, dt, kind, causal):
    """oracle.flash_format_floor of [B, S, H, D] inputs, grouped heads expanded; bottom-right causal as top-left causal on Q padded in
    front with L - Sq zero rows"""
    B, Sq, H, D = q.shape
    L, g = k.shape[1], H // k.shape[2]
    pad = L - Sq if causal else 0
    qd = np.concatenate([np.zeros((B, pad, H, D)), q], 1).transpose(0, 2, 1, 3)
    kd, vd = (np.repeat(t, g, axis=2).transpose(0, 2, 1, 3) for t in (k, v))
    o = orc.flash_format_floor(_oracle_in(qd, dt), _oracle_in(kd, dt), _oracle_in(vd, dt), np.arange(pad, pad + Sq), kind, causal=causal)
    return o.transpose(0, 2, 1, 3)  # [B, Sq, H, D] fp32


@pytest.mark.parametrize("dt,kind", [("fp16", "fp16"), ("bf16", "fp16"), ("bf16", "bf16")])
@pytest.mark.parametrize("causal", [False, True])
def test_paged_floors_are_the_dense_floor(dt, kind, causal):
    B, Sq, L, H, Hkv, D = 2, 9, 77, 4, 2, 64
    q, k, v = _dense_case(dt, B, Sq, L, H, Hkv, D, seed=1)
    want = _dense_floor(q, k, v, dt, kind, causal)
    sl = np.full(B, L)
    o = paged_ref.forward(q, k, v, sl, None, causal=causal, kind=kind)[0]
    np.testing.assert_allclose(o, want, rtol=2e-6, atol=1e-7)  # (the oracle's floor is returned in fp32)
    ex = paged_ref.forward(q, k, v, sl, None, causal=causal)[0]
    e = tol.errors(o, ex)[0]
    assert 0.05 * tol.ULP_AT_ONE[kind] < e < tol.ULP_AT_ONE[kind], e  # at the format's level: not the exact values, inside the ceiling
    # packed queries over the same cache, one sequence per batch entry
    cu = np.arange(B + 1) * Sq
    o2 = varlen_paged_ref.forward(q.reshape(B * Sq, H, D), k, v, cu, Sq, sl, None, causal=causal, kind=kind)[0]
    assert np.array_equal(o2.reshape(B, Sq, H, D), o)
    # the banded reference with a window that bounds nothing (L_q < L_k: bottom-right)
    o3 = varlen_window_ref.forward(q.reshape(B * Sq, H, D), k.reshape(B * L, Hkv, D), v.reshape(B * L, Hkv, D), cu, np.arange(B + 1) * L,
                                   causal, (-1, -1), kind=kind)[0]
    np.testing.assert_allclose(o3.reshape(B, Sq, H, D), want, rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("kind", ["fp16", "bf16"])
def test_fp8_floor_is_the_dense_floor_on_the_dequantised_post_append_bytes(kind):
    B, Sq, L, H, Hkv, D, S_new = 2, 3, 40, 4, 2, 64, 3
    rng = np.random.default_rng(2)
    q = _rnd(rng, (B, Sq, H, D), "bf16")
    k8, v8 = (paged_fp8_ref.quantise(rng.standard_normal((B, L + S_new, Hkv, D)) * 4, 1.0) for _ in range(2))
    kn, vn = _rnd(rng, (B, S_new, Hkv, D), "bf16"), _rnd(rng, (B, S_new, Hkv, D), "bf16")
    kd, vd = rng.uniform(0.05, 0.3, (B, Hkv)).astype(np.float32), rng.uniform(0.05, 0.3, (B, Hkv)).astype(np.float32)
    sl = np.full(B, L)
    o, _, k8n, v8n = paged_fp8_ref.forward(q, k8, v8, sl, kd, vd, None, kn, vn, True, kind=kind)
    assert not np.array_equal(k8n, k8)
    kdq = paged_fp8_ref.dequantise(k8n, kd.astype(np.float64)[:, None, :, None])
    vdq = paged_fp8_ref.dequantise(v8n, vd.astype(np.float64)[:, None, :, None])
    # (dequantised values are e4m3 x fp32: exact in fp64, not in a 16-bit type -- the dense floor is run in fp64 here)
    want = paged_ref.forward(q, kdq, vdq, sl + S_new, None, causal=True, kind=kind)[0]
    np.testing.assert_allclose(o, want, rtol=1e-12, atol=1e-14)
    ex = paged_fp8_ref.forward(q, k8, v8, sl, kd, vd, None, kn, vn, True)[0]
    assert 0.05 * tol.ULP_AT_ONE[kind] < tol.errors(o, ex)[0] < tol.ULP_AT_ONE[kind]


@pytest.mark.parametrize("dt,kind", [("fp16", "fp16"), ("bf16", "fp16"), ("bf16", "bf16")])
@pytest.mark.parametrize("causal", [False, True])
def test_dropout_floor_with_everything_kept_is_the_dense_floor(dt, kind, causal):
    B, H, S, D = 1, 2, 70, 64
    q, k, v = (t.transpose(0, 2, 1, 3) for t in _dense_case(dt, B, S, S, H, H, D, seed=3))
    keep = np.ones((B, H, S, S), bool)
    o, lse = dropout_ref.forward(q, k, v, keep, 0.0, scale=D ** -0.5, causal=causal, kind=kind)
    want = orc.flash_format_floor(_oracle_in(q, dt), _oracle_in(k, dt), _oracle_in(v, dt), np.arange(S), kind, causal=causal)
    np.testing.assert_allclose(o, want, rtol=2e-6, atol=1e-7)
    assert np.array_equal(lse, dropout_ref.forward(q, k, v, keep, 0.0, scale=D ** -0.5, causal=causal)[1])


def test_dropout_floor_rounds_keep_o_p_in_the_numerator_only():
    B, H, Sq, Skv, D, p = 1, 2, 33, 90, 64, 0.5
    rng = np.random.default_rng(4)
    q, k, v = _rnd(rng, (B, H, Sq, D), "fp16"), _rnd(rng, (B, H, Skv, D), "fp16"), _rnd(rng, (B, H, Skv, D), "fp16")
    keep = dropout_ref.keep_mask(B, H, Sq, Skv, p, 7, 9)
    o = dropout_ref.forward(q, k, v, keep, p, scale=D ** -0.5, kind="fp16")[0]
    s = np.einsum("bhid,bhjd->bhij", q, k) * D ** -0.5
    e = np.exp(s - s.max(-1, keepdims=True))
    want = dropout_ref.keep_scale(p) * np.einsum("bhij,bhjd->bhid", orc.round_to(e, "fp16") * keep, v) / e.sum(-1, keepdims=True)
    np.testing.assert_allclose(o, want, rtol=1e-12, atol=1e-14)


def test_kind_none_is_unchanged():
    """the exact paths do the arithmetic they did before the argument existed, restated here operation by operation"""
    B, Sq, L, H, Hkv, D = 2, 5, 37, 4, 2, 64
    q, k, v = _dense_case("bf16", B, Sq, L, H, Hkv, D, seed=5)
    sl = np.array([L, 20])
    got = paged_ref.forward(q, k, v, sl, None, causal=True)[0]
    g = H // Hkv
    for b in range(B):
        Lk = int(sl[b])
        vis = np.arange(Lk)[None, :] <= np.arange(Sq)[:, None] + (Lk - Sq)
        for h in range(H):
            s = np.where(vis, q[b, :, h] @ k[b, :Lk, h // g].T * D ** -0.5, -np.inf)
            p = np.where(vis, np.exp(s - s.max(1)[:, None]), 0.0)
            assert np.array_equal(got[b, :, h], (p @ v[b, :Lk, h // g]) / p.sum(1)[:, None])
    cu = np.arange(B + 1) * Sq
    assert np.array_equal(varlen_paged_ref.forward(q.reshape(-1, H, D), k, v, cu, Sq, sl, None, causal=True)[0].reshape(q.shape), got)
    assert np.array_equal(varlen_paged_ref.forward(q.reshape(-1, H, D), k, v, cu, Sq, sl, None, causal=True, kind=None)[0].reshape(q.shape), got)
    kp = np.concatenate([k[0, :L], k[1, :20]])
    vp = np.concatenate([v[0, :L], v[1, :20]])
    w = varlen_window_ref.forward(q.reshape(-1, H, D), kp, vp, cu, [0, L, L + 20], True, (-1, -1))[0]
    assert np.array_equal(w.reshape(q.shape), got)
    # dropout: O = s ((P o keep) V) with the normalised P
    qd, kd, vd = (t.transpose(0, 2, 1, 3) for t in _dense_case("fp16", 1, 40, 40, 2, 2, 64, seed=6))
    keep = dropout_ref.keep_mask(1, 2, 40, 40, 0.1, 1, 2)
    s = np.einsum("bhid,bhjd->bhij", qd, kd) * 0.125
    e = np.exp(s - s.max(-1, keepdims=True))
    want = dropout_ref.keep_scale(0.1) * np.einsum("bhij,bhjd->bhid", e / e.sum(-1, keepdims=True) * keep, vd)
    assert np.array_equal(dropout_ref.forward(qd, kd, vd, keep, 0.1, scale=0.125)[0], want)


# ------------------------------------------------------------------------------------------- check_forward(floor=, regime=)
def test_floor_argument_is_additive_and_bounds_zero_floor_rows():
    rng = np.random.default_rng(8)
    ref = rng.standard_normal((1, 1, 80, 64))
    floor = ref + 1e-4 * rng.standard_normal(ref.shape)
    floor[:, :, :10] = ref[:, :, :10]  # rows whose floor error is exactly zero
    tol.check_forward(floor, ref, "fp16", "fa_fwd16_paged<fp16,64>", floor=floor)
    got = floor.copy()
    got[:, :, :10] += 0.5 * tol.BWD_EPS * np.abs(ref).max()  # fp32 noise on them: inside the absolute allowance
    tol.check_forward(got, ref, "fp16", "fa_fwd16_paged<fp16,64>", floor=floor)
    only = slice(0, 10)
    tol.check_forward(got[:, :, only], ref[:, :, only], "fp16", "fa_fwd16_paged<fp16,64>", floor=floor[:, :, only], min_elems_for_rms=1)
    with pytest.raises(AssertionError, match="vs format floor"):
        tol.check_forward(ref[:, :, only] + 1e-5, ref[:, :, only], "fp16", "fa_fwd16_paged<fp16,64>", floor=floor[:, :, only])
    # regime: a name, or (max, rms); the pair keeps the exact rms multiple
    bad = ref + 1.10 * (floor - ref)
    with pytest.raises(AssertionError, match="rms vs format floor"):
        tol.check_forward(bad, ref, "fp16", "k", floor=floor, regime=("stale", "exact"))
    tol.check_forward(bad, ref, "fp16", "k", floor=floor, regime="stale")
    assert ffr.form_regime(32, False) == ("stale", "exact") and ffr.form_regime(33, False) == "exact" and ffr.form_regime(128, True)[0] == "stale"


# ------------------------------------------------------------------------------------------- the emulation is accepted
def _static_case(dt, B, Sq, Hkv, g, D, lens, seed):
    rng = np.random.default_rng(seed)
    Smax = max(max(lens), 1)
    return _rnd(rng, (B, Sq, Hkv * g, D), dt), _rnd(rng, (B, Smax, Hkv, D), dt), _rnd(rng, (B, Smax, Hkv, D), dt)


def _paged_pool(q, kc, vc, lens, causal, got):
    """(got, want, floor, nkeys) rows of a static-cache case"""
    B, Sq, H, D = q.shape
    want = paged_ref.forward(q, kc, vc, lens, None, causal=causal)[0]
    floor = paged_ref.forward(q, kc, vc, lens, None, causal=causal, kind=ffr.KIND)[0]
    nk = np.repeat(ffr.paged_nkeys(Sq, lens, kc.shape, causal=causal)[:, :, None], H, axis=2)
    return got.reshape(-1, D), want.reshape(-1, D), floor.reshape(-1, D), nk.reshape(-1)


def _accept_paged(dt, D, B, Hkv, g, Sq, lens, causal, nsplit, tag):
    worst = [0.0, 0.0]
    for seed in range(SEEDS):
        q, kc, vc = _static_case(dt, B, Sq, Hkv, g, D, lens, seed)
        got = ffr.emulate_paged(q, kc, vc, lens, causal, nsplit)
        mx, rms = ffr.check_pool(*_paged_pool(q, kc, vc, lens, causal, got), dt, "emulated", f"{tag} seed {seed}",
                                 ffr.form_regime(g * Sq, nsplit > 1))
        worst = [max(worst[0], mx), max(worst[1], rms)]
    return worst


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("g,Sq,causal,nsplit", ffr.DECODE)
def test_emulated_decode_form_is_accepted(dt, D, g, Sq, causal, nsplit):
    _accept_paged(dt, D, 8, 2, g, Sq, ffr.DECODE_LENS, causal, nsplit, "decode")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("page", ffr.ROWS128_PAGES)
@pytest.mark.parametrize("g,Sq", ffr.ROWS128)
def test_emulated_128_row_form_is_accepted(dt, D, causal, page, g, Sq):
    _accept_paged(dt, D, 4, 2, g, Sq, ffr.rows128_lens(page), causal, 1, "128-row")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("nsplit,L", ffr.ROWS128_SPLIT)
@pytest.mark.parametrize("g,Sq", ffr.ROWS128)
def test_emulated_128_row_split_is_accepted(dt, D, nsplit, L, g, Sq):
    _accept_paged(dt, D, 2, 2, g, Sq, [L, L - 37], True, nsplit, "128-row split")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("nsplit", [1, 3])
def test_emulated_packed_queries_are_accepted(dt, D, nsplit):
    """(one part: the unsplit kernel, whose 128-row items take the exact max multiple; three: the split one)  each sequence of the packed batch as its own static-cache call; decode-form and 128-row items pooled separately"""
    g, Hkv = ffr.PACKED_G, ffr.PACKED_HKV
    for seed in range(SEEDS):
        pools = {True: [], False: []}
        for n, (lq, L) in enumerate(zip(ffr.PACKED_LQ, ffr.PACKED_CACHE)):
            if lq == 0:
                continue
            q, kc, vc = _static_case(dt, 1, lq, Hkv, g, D, [L], 100 * seed + n)
            got = ffr.emulate_paged(q, kc, vc, [L], True, nsplit)
            pools[g * lq <= 32].append(_paged_pool(q, kc, vc, [L], True, got))
        for dec, items in pools.items():
            rows = [np.concatenate(x) for x in zip(*items)]
            ffr.check_pool(*rows, dt, "emulated", f"packed decode={dec} seed {seed}", ffr.form_regime(32 if dec else 128, nsplit > 1))


def _descales(rng, B, Hkv):
    """test_gpu_paged_fp8._descales: neighbouring heads differ by 2^+-6, no powers of two"""
    base = rng.uniform(0.7, 1.4, (B, Hkv))
    e = np.where((np.arange(Hkv)[None, :] + np.arange(B)[:, None]) % 2 == 0, 2.0 ** -3, 2.0 ** 3)
    return (base * e).astype(np.float32), (base[::-1, ::-1] / e).astype(np.float32)


def _hole_table(B, max_pages):
    """the GPU case's table: page 1 of every sequence one past the pool, page 3 of sequence 2 negative"""
    bt = np.arange(B * max_pages, dtype=np.int64).reshape(B, max_pages)
    bt[:, 1] = B * max_pages
    bt[2, 3] = -1
    return bt


def _kv_case(dt, D, B, Hkv, g, Sq, lens, seed, fp8=False, S_new=0, hole=False):
    """(q, K cache, V cache, block_table, k_new, v_new, k_descale, v_descale): a static cache, or 16-key pages behind _hole_table; 16-bit
    values of the type, or e4m3 bytes (N(0, 1) x 4 rounded, as the GPU tests draw them) with _descales"""
    rng = np.random.default_rng(seed)
    q = _rnd(rng, (B, Sq, Hkv * g, D), dt)
    max_pages = -(-(max(lens) + S_new) // 16)
    shape = (B * max_pages, 16, Hkv, D) if hole else (B, max(max(lens) + S_new, 1), Hkv, D)
    if fp8:
        kc, vc = (paged_fp8_ref.quantise(rng.standard_normal(shape) * 4, 1.0) for _ in range(2))
    else:
        kc, vc = _rnd(rng, shape, dt), _rnd(rng, shape, dt)
    kn, vn = (_rnd(rng, (B, S_new, Hkv, D), dt), _rnd(rng, (B, S_new, Hkv, D), dt)) if S_new else (None, None)
    kd, vd = _descales(rng, B, Hkv) if fp8 else (None, None)
    return q, kc, vc, _hole_table(B, max_pages) if hole else None, kn, vn, kd, vd


def _kv_emulate(case, lens, causal, nsplit, defect=None):
    """(got, want, floor, nkeys) rows of a case (fp8: divided by the group's v_descale): the references run the append themselves, the
    emulation sees the caches they return under the advanced lengths"""
    q, kc, vc, bt, kn, vn, kd, vd = case
    B, Sq, H, D = q.shape
    S_new = 0 if kn is None else kn.shape[1]
    if kd is None:
        want, _, kca, vca = paged_ref.forward(q, kc, vc, lens, bt, kn, vn, causal)
        floor = paged_ref.forward(q, kc, vc, lens, bt, kn, vn, causal, kind=ffr.KIND)[0]
        div = 1.0
    else:
        want, _, k8a, v8a = paged_fp8_ref.forward(q, kc, vc, lens, kd, vd, bt, kn, vn, causal)
        floor = paged_fp8_ref.forward(q, kc, vc, lens, kd, vd, bt, kn, vn, causal, kind=ffr.KIND)[0]
        per = kc.shape[0] // B  # pool entries per sequence (its own pages, or its one static row): each decodes under its sequence's scales
        vuse = np.roll(vd, 1, axis=1) if defect == "v_descale" else vd  # the neighbouring KV head's scale
        kca = paged_fp8_ref.dequantise(k8a, np.repeat(kd.astype(np.float64), per, axis=0)[:, None, :, None])
        vca = paged_fp8_ref.dequantise(v8a, np.repeat(vuse.astype(np.float64), per, axis=0)[:, None, :, None])
        div = np.repeat(vd.astype(np.float64), H // vd.shape[1], axis=1)[:, None, :, None]
    cap = kc.shape[1] * (1 if bt is None else bt.shape[1])
    after = [Lk for _, Lk in paged_ref.lengths(lens, S_new, cap)]
    got = ffr.emulate_paged(q, kca, vca, after, causal, nsplit, block_table=bt, defect=None if defect == "v_descale" else defect, page=16)
    nk = np.repeat(ffr.paged_nkeys(Sq, lens, kc.shape, bt, S_new, causal)[:, :, None], H, axis=2)
    return tuple((t / div).reshape(-1, D) for t in (got, want, floor)) + (nk.reshape(-1),)


RATIOS = {}  # tag -> [min rms ratio, max rms ratio] of the clean emulation (printed by test_zz_report for profiles/fwd_floor/summary.md)


def _accept_kv(dt, D, B, Hkv, g, Sq, lens, causal, nsplit, tag, **kw):
    for seed in range(SEEDS):
        got, want, floor, nk = _kv_emulate(_kv_case(dt, D, B, Hkv, g, Sq, lens, seed, **kw), lens, causal, nsplit)
        S_new = kw.get("S_new", 0)
        ffr.check_pool(got, want, floor, nk, dt, "emulated", f"{tag} seed {seed}", ffr.form_regime(g * Sq, nsplit > 1))
        sel = nk >= 2
        r = tol.errors(got[sel], want[sel])[1] / tol.errors(floor[sel], want[sel])[1]
        lo, hi = RATIOS.get(tag, (r, r))
        RATIOS[tag] = (min(lo, r), max(hi, r))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("g,Sq,causal,nsplit", ffr.DECODE)
def test_emulated_fp8_decode_form_is_accepted(dt, D, g, Sq, causal, nsplit):
    _accept_kv(dt, D, 8, 2, g, Sq, ffr.DECODE_LENS, causal, nsplit, f"fp8 decode{' split' if nsplit > 1 else ''}", fp8=True)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("g,Sq", ffr.ROWS128)
def test_emulated_fp8_128_row_form_is_accepted(dt, D, causal, g, Sq):
    _accept_kv(dt, D, 4, 2, g, Sq, ffr.rows128_lens(16), causal, 1, "fp8 128-row", fp8=True)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("nsplit,L", ffr.ROWS128_SPLIT)
@pytest.mark.parametrize("g,Sq", ffr.ROWS128)
def test_emulated_fp8_128_row_split_is_accepted(dt, D, nsplit, L, g, Sq):
    _accept_kv(dt, D, 2, 2, g, Sq, [L, L - 37], True, nsplit, f"fp8 128-row split{nsplit} L{L}", fp8=True)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "kv8"])
def test_emulated_one_each_cases_are_accepted(dt, D, fp8):
    """the static view's shape (a view changes no arithmetic), the append across a page boundary, the table with holes"""
    if not fp8:
        _accept_kv(dt, D, 3, 2, 4, 4, [17, 300, 129], True, 1, "static")
    _accept_kv(dt, D, 4, 2, 8, 3, ffr.APPEND_LENS, True, 1, "fp8 append" if fp8 else "append", fp8=fp8, S_new=3)
    _accept_kv(dt, D, 4, 2, 8, 1, ffr.HOLE_LENS, False, 1, "fp8 hole" if fp8 else "hole", fp8=fp8, hole=True)


DROP_SHAPES = [(64, 256, 256, 64, False, 0.1), (48, 130, 1000, 128, False, 0.5), (80, 1000, 257, 64, True, 0.9)]  # (rows kept, Sq, Skv, D, causal, p)


def _drop_case(dt, nrows, Sq, Skv, D, causal, p, seed):
    """a spread of `nrows` query rows of the GPU shape (the keep mask at their own coordinates)"""
    rng = np.random.default_rng(seed)
    rows = np.unique(np.linspace(1 if causal else 0, Sq - 1, nrows).astype(np.int64))
    q, k, v = _rnd(rng, (rows.size, D), dt), _rnd(rng, (Skv, D), dt), _rnd(rng, (Skv, D), dt)
    keep = dropout_ref.keep_bits(rows[:, None], np.arange(Skv)[None, :], 0, 11 + seed, 5, dropout_ref.threshold(p))
    vis = np.arange(Skv)[None, :] <= rows[:, None] if causal else np.ones((rows.size, Skv), bool)
    S = np.where(vis, q @ k.T * D ** -0.5, -np.inf)
    e = np.exp(S - S.max(1, keepdims=True))
    s = dropout_ref.keep_scale(p)
    want = s * ((e * keep) @ v) / e.sum(1, keepdims=True)
    floor = s * (orc.round_to(e * keep, ffr.KIND) @ v) / e.sum(1, keepdims=True)
    return q, k, v, vis, keep, s, want, floor


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("nrows,Sq,Skv,D,causal,p", DROP_SHAPES)
def test_emulated_dropout_forward_is_accepted(dt, nrows, Sq, Skv, D, causal, p):
    for seed in range(SEEDS):
        q, k, v, vis, keep, s, want, floor = _drop_case(dt, nrows, Sq, Skv, D, causal, p, seed)
        got = ffr.emulate(q, k, v, vis, scale=D ** -0.5, ks4=False, keep=keep, keep_s=s)
        tol.check_forward(got[None, None], want[None, None], ffr.KIND, "emulated", tag=f"dropout seed {seed}", floor=floor[None, None], regime="exact")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("window", ffr.WINDOWS)
def test_emulated_band_is_accepted(dt, D, causal, window):
    """the banded kernel is the 128-row form, one head's rows of one sequence per block, on the band's visibility: the GPU test's lengths,
    windows and heads"""
    H, Hkv = 4, 2
    cq, ck = (np.concatenate([[0], np.cumsum(x)]) for x in (ffr.BAND_LENS_Q, ffr.BAND_LENS_K))
    for seed in range(SEEDS):
        rng = np.random.default_rng(seed)
        q, k, v = _rnd(rng, (cq[-1], H, D), dt), _rnd(rng, (ck[-1], Hkv, D), dt), _rnd(rng, (ck[-1], Hkv, D), dt)
        want = varlen_window_ref.forward(q, k, v, cq, ck, causal, window)[0]
        floor = varlen_window_ref.forward(q, k, v, cq, ck, causal, window, kind=ffr.KIND)[0]
        got, nk = np.zeros_like(want), np.zeros(cq[-1], np.int64)
        for q0, Lq, k0, Lk in varlen_window_ref.seqs(cq, ck):
            vis = varlen_window_ref.visible(Lq, Lk, causal, window)
            nk[q0:q0 + Lq] = vis.sum(1)
            for h in range(H):
                for r0 in range(0, Lq, 128):
                    got[q0 + r0:q0 + min(r0 + 128, Lq), h] = ffr.emulate(q[q0 + r0:q0 + min(r0 + 128, Lq), h], k[k0:k0 + Lk, h // 2],
                                                                         v[k0:k0 + Lk, h // 2], vis[r0:r0 + 128], scale=D ** -0.5, ks4=False)
        one_key_only = nk.max() <= 1
        assert one_key_only == (window[0] == 0 and (causal or window[1] == 0))
        ffr.check_pool(got.reshape(-1, D), want.reshape(-1, D), floor.reshape(-1, D), np.repeat(nk, H), dt, "emulated",
                       f"band {window} seed {seed}", "exact", min_elems=0 if one_key_only else 4096)


# ------------------------------------------------------------------------------------------- planted defects are rejected
FLOOR, CEIL = "vs format floor", "format ceiling"  # which bound has to do the rejecting


@pytest.mark.parametrize("defect,g,Sq,lens,nsplit,match", [
    ("p_bf16", 8, 1, ffr.DECODE_LENS, 1, CEIL),  # (eight times the error: already over the ceiling)
    ("p_bf16", 1, 200, [150, 21, 640], 1, CEIL),
    ("p_trunc", 8, 1, [21, 127, 128, 129, 333, 640], 3, "format ceiling, rms|" + FLOOR),  # (the rms ceiling from 4096 elements, else a floor bound)
    ("p_trunc", 8, 16, [150, 21, 640], 1, "format ceiling, rms|" + FLOOR),
    ("part_o_fp16", 8, 1, ffr.DECODE_LENS, 3, "rms " + FLOOR),  # (inside the ceiling: the floor's rms bound alone)
    ("part_o_fp16", 1, 200, [1300], 3, "rms " + FLOOR),
    ("fold_w_fp16", 8, 1, [333, 640, 1300, 2500], 3, "rms " + FLOOR),  # (every sequence longer than one step: each is folded)
    ("fold_w_fp16", 8, 16, [1300], 3, "rms " + FLOOR),
    ("ragged_key", 8, 1, [21, 127, 128, 129, 333, 640], 1, CEIL),  # (a whole key's weight missing)
    ("ragged_key", 1, 200, [150, 21, 640], 1, CEIL),
])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_planted_defects_are_rejected(defect, g, Sq, lens, nsplit, match, dt):
    D, causal = 64, Sq > 1
    q, kc, vc = _static_case(dt, len(lens), Sq, 2, g, D, lens, seed=17)
    regime = ffr.form_regime(g * Sq, nsplit > 1)
    clean = ffr.emulate_paged(q, kc, vc, lens, causal, nsplit)
    ffr.check_pool(*_paged_pool(q, kc, vc, lens, causal, clean), dt, "emulated", "clean", regime)
    bad = ffr.emulate_paged(q, kc, vc, lens, causal, nsplit, defect=defect, page=16)
    with pytest.raises(AssertionError, match=match):
        ffr.check_pool(*_paged_pool(q, kc, vc, lens, causal, bad), dt, "emulated", defect, regime)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_the_neighbouring_heads_v_descale_is_rejected(dt):
    lens = [21, 127, 128, 129, 333, 640]
    case = _kv_case(dt, 64, len(lens), 2, 8, 1, lens, 3, fp8=True)
    ffr.check_pool(*_kv_emulate(case, lens, False, 1), dt, "emulated", "clean", ffr.form_regime(8, False))
    with pytest.raises(AssertionError, match=CEIL):  # (off by 2^+-6)
        ffr.check_pool(*_kv_emulate(case, lens, False, 1, defect="v_descale"), dt, "emulated", "v_descale", ffr.form_regime(8, False))


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("nrows,Sq,Skv,D,causal,p", [DROP_SHAPES[0], DROP_SHAPES[2][:5] + (0.1,), DROP_SHAPES[2][:5] + (0.7,)])
def test_keep_after_the_rounding_is_rejected(dt, nrows, Sq, Skv, D, causal, p):
    """what the defect costs is the row's largest P: 1.0 is exact, 1 / (1 - p) is not (p = 0.1, 0.7; with p = 0.5 or 0.9 the factor is 2 or
    10, both fp16 values, and the two orders round alike), so it shows where a row's largest P carries weight: a few hundred keys or fewer
    (emulated rms ratio 1.09 ... 1.66 against 0.85 ... 0.94 clean; at 1000 keys it drowns: 1.05 ... 1.06)"""
    q, k, v, vis, keep, s, want, floor = _drop_case(dt, nrows, Sq, Skv, D, causal, p, seed=23)
    bad = ffr.emulate(q, k, v, vis, scale=D ** -0.5, ks4=False, keep=keep, keep_s=s, defect="keep_after")
    with pytest.raises(AssertionError, match=FLOOR):  # (inside the ceiling: the floor's bounds alone, max or rms)
        tol.check_forward(bad[None, None], want[None, None], ffr.KIND, "emulated", tag="keep_after", floor=floor[None, None], regime="exact")


@pytest.mark.parametrize("g,Sq,nsplit", [(8, 1, 1), (8, 1, 3), (1, 200, 1)])
def test_a_kernel_15_percent_worse_everywhere_fails_on_rms_only(g, Sq, nsplit, monkeypatch):
    lens = ffr.DECODE_LENS
    q, kc, vc = _static_case("fp16", len(lens), Sq, 2, g, 64, lens, seed=29)
    regime = ffr.form_regime(g * Sq, nsplit > 1)
    _, want, floor, nk = _paged_pool(q, kc, vc, lens, Sq > 1, np.zeros_like(q))
    bad = want + 1.15 * (floor - want)
    with pytest.raises(AssertionError, match="rms vs format floor"):
        ffr.check_pool(bad, want, floor, nk, "fp16", "emulated", "x1.15", regime)
    monkeypatch.setitem(tol.FLOOR_MULT, "exact", (1.15, 1.2))
    ffr.check_pool(bad, want, floor, nk, "fp16", "emulated", "x1.15 at 1.2", regime)


def test_zz_report():
    """the clean emulation's rms ratio to the floor per fp8 / one-each form, for the record (run with -s)"""
    for tag, (lo, hi) in sorted(RATIOS.items()):
        print(f"emulated rms ratio {tag}: {lo:.3f} ... {hi:.3f}")
