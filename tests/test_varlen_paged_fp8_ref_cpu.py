"""The fp64 reference of packed queries over an fp8 KV cache (tests/varlen_paged_fp8_ref.py), pinned three ways with no GPU: to
paged_fp8_ref.forward when every L_q is equal, to varlen_paged_ref.forward on the dequantised cache at descale 1, and its append bytes
bitwise to paged_fp8_ref.quantise."""
import numpy as np
import pytest

import paged_fp8_ref
import varlen_paged_fp8_ref as ref
import varlen_paged_ref


def _case(lq, H, Hkv, D, ps, max_pages, seed, new, static=False):
    rng = np.random.default_rng(seed)
    B, Tq = len(lq), int(sum(lq))
    q = rng.standard_normal((Tq, H, D))
    if static:
        shape, bt = (B, ps * max_pages, Hkv, D), None
    else:
        shape = (B * max_pages + 2, ps, Hkv, D)
        bt = (rng.permutation(B * max_pages) + 1).reshape(B, max_pages).astype(np.int32)
    finite = np.array([b for b in range(256) if b & 0x7f != 0x7f], np.uint8)  # every byte but the two NaNs
    k8, v8 = finite[rng.integers(0, len(finite), shape)], finite[rng.integers(0, len(finite), shape)]
    kn = rng.standard_normal((Tq, Hkv, D)).astype(np.float32) * 3 if new else None
    vn = rng.standard_normal((Tq, Hkv, D)).astype(np.float32) * 3 if new else None
    kd = rng.uniform(0.05, 2.0, (B, Hkv)).astype(np.float32)
    vd = rng.uniform(0.05, 2.0, (B, Hkv)).astype(np.float32)
    cu = np.concatenate([[0], np.cumsum(lq)]).astype(np.int64)
    return q, k8, v8, bt, kn, vn, kd, vd, cu


@pytest.mark.parametrize("Sq,new", [(1, False), (4, True), (40, True)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("static", [False, True])
def test_equal_lengths_equal_the_dense_fp8_reference(Sq, new, causal, static):
    B, H, Hkv, D = 3, 4, 2, 16
    q, k8, v8, bt, kn, vn, kd, vd, cu = _case([Sq] * B, H, Hkv, D, 16, 4, seed=Sq, new=new, static=static)
    sl = np.array([0, 21, 60])  # the last one appends past the capacity of 64 when Sq = 40
    o, lse, k8n, v8n = ref.forward(q, k8, v8, cu, Sq, sl, kd, vd, bt, kn, vn, causal)
    r = lambda a: None if a is None else a.reshape(B, Sq, *a.shape[1:])  # noqa: E731
    o2, lse2, k8d, v8d = paged_fp8_ref.forward(r(q), k8, v8, sl, kd, vd, bt, r(kn), r(vn), causal)
    np.testing.assert_allclose(o.reshape(B, Sq, H, D), o2, rtol=0, atol=1e-12)
    live = np.isfinite(lse2)
    assert (np.isfinite(lse.reshape(H, B, Sq).transpose(1, 0, 2)) == live).all()
    np.testing.assert_allclose(lse.reshape(H, B, Sq).transpose(1, 0, 2)[live], lse2[live], rtol=0, atol=1e-12)
    assert (k8n == k8d).all() and (v8n == v8d).all()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("new", [False, True])
def test_descale_one_equals_the_16_bit_reference_on_the_dequantised_cache(causal, new):
    lq, H, Hkv, D = [0, 1, 5, 33, 2], 4, 2, 16
    q, k8, v8, bt, kn, vn, _, _, cu = _case(lq, H, Hkv, D, 16, 4, seed=7, new=new)
    sl = np.array([3, 0, 17, 30, 64])
    o, lse, k8n, v8n = ref.forward(q, k8, v8, cu, max(lq), sl, 1.0, 1.0, bt, kn, vn, causal)
    dq = lambda a: None if a is None else ref.dequantise(ref.quantise(a, 1.0))  # noqa: E731
    o2, lse2, kc2, vc2 = varlen_paged_ref.forward(q, ref.dequantise(k8), ref.dequantise(v8), cu, max(lq), sl, bt, dq(kn), dq(vn), causal)
    np.testing.assert_allclose(o, o2, rtol=0, atol=1e-12)
    live = np.isfinite(lse2)
    assert live.mean() > 0.5 and (np.isfinite(lse) == live).all()
    np.testing.assert_allclose(lse[live], lse2[live], rtol=0, atol=1e-12)
    assert (ref.dequantise(k8n) == kc2).all() and (ref.dequantise(v8n) == vc2).all()


def test_kind_passes_through_to_the_format_floor():
    lq = [2, 40]
    q, k8, v8, bt, _, _, kd, vd, cu = _case(lq, 4, 2, 16, 16, 4, seed=9, new=False)
    sl = np.array([50, 64])
    exact = ref.forward(q, k8, v8, cu, 40, sl, kd, vd, bt, causal=True)[0]
    floor = ref.forward(q, k8, v8, cu, 40, sl, kd, vd, bt, causal=True, kind="fp16")[0]
    # P rounded to fp16 once, in the numerator only: |floor - exact| <= 2^-11 sum(p |v|) / l <= 2^-11 max |V|, and not zero
    err = np.abs(floor - exact).max()
    assert 0 < err <= 2.0 ** -11 * 448 * float(vd.max())


@pytest.mark.parametrize("static", [False, True])
def test_append_bytes_are_the_quantisers(static):
    lq, H, Hkv, D, ps, mp = [5, 0, 1, 40, 3], 4, 2, 16, 16, 3
    q, k8, v8, bt, kn, vn, kd, vd, cu = _case(lq, H, Hkv, D, ps, mp, seed=11, new=True, static=static)
    kn[0, 0, :4] = [1e4, -1e4, 0.0, -0.0]  # beyond +-448 descale: saturates; both zeros
    sl = np.array([14, 7, 47, 3, 46])  # page crossings; the last one runs past the capacity of 48: one row dropped
    k8n, v8n = ref.append(k8, v8, kn, vn, cu, 40, sl, kd, vd, bt)
    touched = np.zeros(k8.shape[:2], bool)
    for b, (q0, Lq) in enumerate(varlen_paged_ref.ranges(cu, sum(lq), 40)):
        for i in range(Lq):
            pos = sl[b] + i
            if pos >= ps * mp:
                continue
            pg, row = (b, pos) if static else (bt[b, pos // ps], pos % ps)
            touched[pg, row] = True
            assert (k8n[pg, row] == paged_fp8_ref.quantise(kn[q0 + i], kd[b][:, None])).all()
            assert (v8n[pg, row] == paged_fp8_ref.quantise(vn[q0 + i], vd[b][:, None])).all()
    assert touched.sum() == sum(lq) - 1
    assert (k8n[~touched] == k8[~touched]).all() and (v8n[~touched] == v8[~touched]).all()
    assert k8n[(0, 14) if static else (bt[0, 0], 14)][0, :4].tolist() == [0x7e, 0xfe, 0x00, 0x80]  # +-448, +0, -0
