"""The 16-bit backward's gradient metric without a GPU (oracle.flash_backward_format_floor, tolerances.check_backward).

- The floor's `exact` gradients are the C oracle's backward (oracle.sdpa_backward) to fp64 summation noise, at Sq != Skv both
  ways, causal both ways, Sq < 32, and grouped heads against the expanded call.
- check_backward accepts the floor itself and rejects emulated kernels with one planted defect each: P rounded to bf16 under
  fp16 operands, dS rounded twice, the last ragged 32-key tile dropped, D from the neighbouring row, a grouped head missing
  from dK, the floor's error x 1.15 everywhere (caught by the rms bound alone: at 1.5 x it passes).
- sample_rows looks at every 128-row block of the grid, ragged tails included.
"""
import numpy as np
import pytest

from oracle import oracle as orc
import tolerances as tol


def _inputs(kind, B, H, Sq, Skv, D, seed, Hkv=None):
    rng = np.random.default_rng(seed)
    Hkv = Hkv or H
    f = [rng.standard_normal(s).astype(np.float32) for s in ((B, H, Sq, D), (B, Hkv, Skv, D), (B, Hkv, Skv, D), (B, H, Sq, D))]
    if kind == "fp16":
        return [a.astype(np.float16) for a in f]
    return [orc.f32_to_bf16_bits(a).reshape(a.shape) for a in f]


def _f64(a):
    return orc.to_f32(a).astype(np.float64)


def _fwd(q, k, v, causal, group=1):
    if group > 1:
        k, v = (np.ascontiguousarray(np.repeat(t, group, axis=1)) for t in (k, v))
    return orc.sdpa_forward(q, k, v, causal=causal, return_lse=True)


def emulate(dout, q, k, v, o, lse, kind, *, causal, scale, group=1, defect=None):
    """a 16-bit backward written out in fp64 with the kernel's two roundings -- and, on request, one planted defect"""
    Q, K, V, dO = (_f64(a) for a in (q, k, v, dout))
    K, V = (np.repeat(t, group, axis=1) for t in (K, V))
    O = np.asarray(o, np.float64)
    Sq, Skv = Q.shape[2], K.shape[2]
    s = np.einsum("bhid,bhjd->bhij", Q, K) * scale
    if causal:
        s = np.where(np.arange(Skv)[None, :] <= np.arange(Sq)[:, None], s, -np.inf)
    p = np.exp(s - np.asarray(lse, np.float64).reshape(s.shape[:3])[..., None])
    if defect == "tail_tile":
        p[..., 32 * ((Skv - 1) // 32):] = 0.0
    dvec = (dO * O).sum(-1)
    if defect == "d_neighbour":
        dvec = np.roll(dvec, 1, axis=2)
    dp = np.einsum("bhid,bhjd->bhij", dO, V)
    ds = p * (dp - dvec[..., None])
    pr = orc.round_to(p, "bf16" if defect == "p_bf16" else kind)
    dsr = orc.round_to(ds, kind)
    if defect == "ds_twice":
        dsr = orc.round_to(pr * orc.round_to(dp - dvec[..., None], kind), kind)
    dq = scale * np.einsum("bhij,bhjd->bhid", dsr, K)
    dk = scale * np.einsum("bhij,bhid->bhjd", dsr, Q)
    dv = np.einsum("bhij,bhid->bhjd", pr, dO)
    if group > 1:
        B, H = Q.shape[:2]
        dk = dk.reshape(B, H // group, group, Skv, -1)
        if defect == "gqa_member":
            dk = dk.copy()
            dk[:, :, group - 1] = 0.0
        dk = dk.sum(2)
        dv = dv.reshape(B, H // group, group, Skv, -1).sum(2)
    return dq, dk, dv


CASES = [  # kind, B, H, Sq, Skv, D, causal
    ("bf16", 2, 3, 77, 45, 64, False),
    ("fp16", 2, 3, 45, 77, 64, False),
    ("bf16", 1, 2, 40, 100, 128, True),   # causal, Sq < Skv: keys >= 40 seen by nobody
    ("fp16", 1, 2, 100, 40, 128, True),   # causal, Sq > Skv
    ("bf16", 2, 2, 7, 64, 64, False),     # Sq < 32
    ("fp16", 1, 2, 31, 33, 256, True),
]


@pytest.mark.parametrize("kind,B,H,Sq,Skv,D,causal", CASES)
def test_exact_matches_the_c_oracle(kind, B, H, Sq, Skv, D, causal):
    q, k, v, do = _inputs(kind, B, H, Sq, Skv, D, seed=Sq * 7 + Skv)
    o, lse = _fwd(q, k, v, causal)
    rdq, rdk, rdv, _ = orc.sdpa_backward(do, q, k, v, o, lse, causal=causal)
    fl = orc.flash_backward_format_floor(do, q, k, v, o, lse, kind, scale=D ** -0.5, causal=causal)
    for a, r in zip(fl["exact"], (rdq, rdk, rdv)):
        assert np.abs(a - r).max() <= 1e-6 * np.abs(r).max()
    if causal and Sq < Skv:
        assert fl["dead"][1][:, :, Sq:].all() and not fl["dead"][1][:, :, :Sq].any()
        assert (fl["exact"][1][:, :, Sq:] == 0).all() and (fl["floor"][2][:, :, Sq:] == 0).all()
    # the floor sits at the format's level: well inside the ceiling, clearly above fp32 noise
    for a, f in zip(fl["exact"], fl["floor"]):
        e = tol.errors(f, a)[0]
        assert 1e-5 < e < 0.25 * tol.BWD_CEILING[kind], e


@pytest.mark.parametrize("causal", [False, True])
def test_exact_grouped_heads_match_the_expanded_oracle(causal):
    B, Hq, Hkv, Sq, Skv, D = 2, 6, 2, 50, 70, 64
    q, k, v, do = _inputs("bf16", B, Hq, Sq, Skv, D, seed=3, Hkv=Hkv)
    g = Hq // Hkv
    ke, ve = (np.ascontiguousarray(np.repeat(t, g, axis=1)) for t in (k, v))
    o, lse = orc.sdpa_forward(q, ke, ve, causal=causal, return_lse=True)
    rdq, rdk, rdv, _ = orc.sdpa_backward(do, q, ke, ve, o, lse, causal=causal)
    rdk, rdv = (t.astype(np.float64).reshape(B, Hkv, g, Skv, D).sum(2) for t in (rdk, rdv))
    fl = orc.flash_backward_format_floor(do, q, k, v, o, lse, "bf16", scale=D ** -0.5, causal=causal, kv_group=g)
    for a, r in zip(fl["exact"], (rdq, rdk, rdv)):
        assert a.shape == r.shape
        assert np.abs(a - r).max() <= 1e-6 * np.abs(r).max()


def test_subsets_are_the_full_gradients_on_those_rows_and_keys():
    kind, B, H, Sq, Skv, D = "fp16", 2, 3, 300, 260, 64
    q, k, v, do = _inputs(kind, B, H, Sq, Skv, D, seed=5)
    o, lse = _fwd(q, k, v, True)
    full = orc.flash_backward_format_floor(do, q, k, v, o, lse, kind, scale=D ** -0.5, causal=True)
    rows, keys = tol.sample_rows(Sq, B, H, seed=1), tol.sample_rows(Skv, B, H, seed=2)
    sub = orc.flash_backward_format_floor(do, q, k, v, o, lse, kind, scale=D ** -0.5, causal=True, rows=rows, keys=keys, budget=5000)
    for n in ("exact", "floor", "abs"):
        for i, idx in enumerate((rows, keys, keys)):
            np.testing.assert_allclose(sub[n][i], tol.gather_rows(full[n][i], idx), rtol=1e-12, atol=1e-12)


def _case(kind="fp16", B=2, H=2, Sq=96, Skv=83, D=64, causal=False, group=1, seed=11):
    q, k, v, do = _inputs(kind, B, H, Sq, Skv, D, seed=seed, Hkv=H // group)
    o, lse = _fwd(q, k, v, causal, group)
    fl = orc.flash_backward_format_floor(do, q, k, v, o, lse, kind, scale=D ** -0.5, causal=causal, kv_group=group)
    return (do, q, k, v, o, lse), fl


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True])
def test_floor_and_its_emulation_pass(kind, causal):
    args, fl = _case(kind, causal=causal)
    tol.check_backward(fl["floor"], fl, kind, tag="floor")
    got = emulate(*args, kind, causal=causal, scale=64 ** -0.5)
    for a, f in zip(got, fl["floor"]):
        np.testing.assert_allclose(a, f, rtol=1e-9, atol=1e-12)
    tol.check_backward(got, fl, kind, tag="emulated")
    # 16-bit gradients: the floor rounded once more
    tol.check_backward([orc.round_to(g, kind) for g in got], fl, kind, tag="emulated, 16-bit", grad_dt=kind)


@pytest.mark.parametrize("defect,kind,causal,group", [
    ("p_bf16", "fp16", False, 1),
    ("ds_twice", "bf16", False, 1),
    ("ds_twice", "fp16", True, 1),
    ("tail_tile", "bf16", False, 1),
    ("tail_tile", "fp16", True, 1),
    ("d_neighbour", "bf16", True, 1),
    ("d_neighbour", "fp16", False, 1),
    ("gqa_member", "bf16", False, 3),
])
def test_planted_defects_are_rejected(defect, kind, causal, group):
    args, fl = _case(kind, H=6 if group > 1 else 2, causal=causal, group=group)
    tol.check_backward(emulate(*args, kind, causal=causal, scale=64 ** -0.5, group=group), fl, kind, tag="clean")
    bad = emulate(*args, kind, causal=causal, scale=64 ** -0.5, group=group, defect=defect)
    with pytest.raises(AssertionError):
        tol.check_backward(bad, fl, kind, tag=defect)


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_a_kernel_15_percent_worse_everywhere_fails_on_rms_only(kind, monkeypatch):
    args, fl = _case(kind, Sq=160, Skv=150)
    bad = [e + 1.15 * (f - e) for e, f in zip(fl["exact"], fl["floor"])]
    with pytest.raises(AssertionError, match="rms vs format floor"):
        tol.check_backward(bad, fl, kind, tag="x1.15")
    monkeypatch.setattr(tol, "BWD_FLOOR_MULT", (1.5, 1.5))
    tol.check_backward(bad, fl, kind, tag="x1.15 at 1.5")


def test_dead_keys_must_be_exact_zeros():
    args, fl = _case("bf16", Sq=40, Skv=100, causal=True)
    got = [g.copy() for g in fl["floor"]]
    got[2][0, 1, 70, 5] = 1e-30
    with pytest.raises(AssertionError, match="exactly zero"):
        tol.check_backward(got, fl, "bf16")


def test_a_cancelling_gradient_is_held_element_by_element():
    """Skv = 1: P = 1, dS = dP - D cancels; the ratio has no meaning, the absolute bound still rejects a real error"""
    args, fl = _case("fp16", Sq=64, Skv=1)
    rec = tol.check_backward(fl["floor"], fl, "fp16")
    assert rec["dq"]["near_zero"] and not rec["dv"]["near_zero"]
    got = list(fl["floor"])
    got[0] = got[0] + 0.01 * fl["abs"][0].max()
    with pytest.raises(AssertionError, match="element bound"):
        tol.check_backward(got, fl, "fp16")


@pytest.mark.parametrize("n", [1, 7, 127, 128, 129, 255, 256, 1000, 1920, 32768])
def test_sampler_covers_every_block(n):
    B, H = 2, 3
    idx = tol.sample_rows(n, B, H, seed=4)
    assert idx.shape[:2] == (B, H) and idx.min() >= 0 and idx.max() < n
    nblk = (n + 127) // 128
    for b in range(B):
        for h in range(H):
            r = idx[b, h]
            assert (np.diff(r) > 0).all()
            assert set(range(nblk)) <= set((r // 128).tolist())
            for j in range(nblk):
                assert j * 128 in r and min(j * 128 + 127, n - 1) in r  # both edges of every block, the ragged tail's too
    if n > 2 * nblk + 16:  # interior rows differ between slabs
        assert not all(np.array_equal(idx[0, 0], idx[b, h]) for b in range(B) for h in range(H) if (b, h) != (0, 0))
