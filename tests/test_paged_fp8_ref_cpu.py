"""The fp8 KV-cache reference (tests/paged_fp8_ref.py) pinned on the CPU: its e4m3fn decode table against torch.float8_e4m3fn, every finite
value exact in fp16 and bf16 (what lets the kernel expand K8 / V8 to its 16-bit operand types without rounding), and its quantiser
against torch's (x.float() / d).clamp(-448, 448).to(float8_e4m3fn) bit for bit, saturation included."""
import numpy as np
import pytest
import torch

import paged_fp8_ref as ref
import paged_ref


def test_decode_table_is_torch_e4m3fn():
    t = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    nan = np.isnan(ref.E4M3FN)
    assert (np.flatnonzero(nan) == [0x7F, 0xFF]).all() and (np.isnan(t) == nan).all()
    assert (t[~nan] == ref.E4M3FN[~nan]).all()
    assert (np.signbit(t) == np.signbit(ref.E4M3FN))[~nan].all()  # -0 at 0x80
    fin = ref.E4M3FN[~nan]
    assert len(fin) == 254 and fin.max() == 448 and np.abs(fin[fin != 0]).min() == 2.0 ** -9


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_every_finite_value_is_exact_in_the_operand_types(dt):
    fin = torch.tensor(ref.E4M3FN[~np.isnan(ref.E4M3FN)], dtype=torch.float64)
    assert torch.equal(fin.to(dt).double(), fin)


def _torch_quantise(x, d):
    return (x.float() / d).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("descale", [1.0, 2.0 ** -6, 2.0 ** 5, 0.0371, 3.3, 1e-3])
def test_quantiser_matches_torch_bitwise(dt, descale):
    g = torch.Generator().manual_seed(int(descale * 1e4) % 1000)
    x = torch.randn(4096, generator=g) * torch.tensor([0.01, 1.0, 30.0, 1000.0]).repeat(1024)  # far beyond +-448 descale too
    x = torch.cat([x, torch.tensor([0.0, -0.0, 448.0 * descale, -448.0 * descale, 1e4, -1e4, 2.0 ** -10 * descale, 3 * 2.0 ** -11 * descale])]).to(dt)
    d = torch.tensor(descale, dtype=torch.float32)
    got = ref.quantise(x.float().numpy(), np.float32(descale))
    want = _torch_quantise(x, d)
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    assert not np.isnan(ref.E4M3FN[got]).any()  # saturates, never NaN
    big = np.abs(x.float().numpy() / np.float32(descale)) >= 448
    assert big.any() and (np.abs(ref.E4M3FN[got[big]]) == 448).all()


def test_quantiser_ties_go_to_even():
    mids = (ref.E4M3FN[:126] + ref.E4M3FN[1:127]) / 2  # exact in fp32
    got = ref.quantise(mids.astype(np.float32), np.float32(1.0))
    assert (got % 2 == 0).all()
    assert (got == _torch_quantise(torch.tensor(mids, dtype=torch.float32), torch.tensor(1.0))).all()


def test_per_head_descales_broadcast_like_torch():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 4, 16, generator=g).to(torch.bfloat16)
    d = torch.tensor([[0.5, 0.01, 2.0, 1.0], [0.3, 8.0, 0.125, 0.07]])
    got = ref.quantise(x.float().numpy(), d.numpy()[:, None, :, None])
    assert (got == _torch_quantise(x, d[:, None, :, None])).all()


def test_forward_is_the_16bit_reference_on_dequantised_caches():
    rng = np.random.default_rng(5)
    B, Sq, H, Hkv, D, ps, mp = 3, 2, 4, 2, 16, 16, 3
    q = rng.standard_normal((B, Sq, H, D))
    k8 = rng.integers(0, 256, (B * mp + 1, ps, Hkv, D)).astype(np.uint8)
    v8 = rng.integers(0, 256, (B * mp + 1, ps, Hkv, D)).astype(np.uint8)
    k8[(k8 & 0x7F) == 0x7F] = 0x10  # no NaN bytes
    v8[(v8 & 0x7F) == 0x7F] = 0x10
    bt = rng.permutation(B * mp).reshape(B, mp).astype(np.int32)
    kn, vn = rng.standard_normal((B, 2, Hkv, D)), rng.standard_normal((B, 2, Hkv, D))
    sl = np.array([0, 17, 46], np.int32)
    kd = np.array([0.25, 0.5], np.float32)  # per head only: one dequantised pool serves every sequence
    vd = np.float32(2.0)
    o, lse, k8n, v8n = ref.forward(q, k8, v8, sl, kd, vd, bt, kn, vn, causal=True, scale=0.2)
    kq = ref.quantise(kn, kd[None, None, :, None])
    vq = ref.quantise(vn, vd)
    o2, lse2, kc2, vc2 = paged_ref.forward(q, ref.dequantise(k8, kd[None, None, :, None]), ref.dequantise(v8, vd), sl, bt,
                                           ref.dequantise(kq, kd[None, None, :, None]), ref.dequantise(vq, vd), causal=True, scale=0.2)
    np.testing.assert_allclose(o, o2, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lse, lse2, rtol=1e-12, atol=1e-12)
    assert (ref.dequantise(k8n, kd[None, None, :, None]) == kc2).all() and (ref.dequantise(v8n, vd) == vc2).all()
    assert (k8n != k8).any()
