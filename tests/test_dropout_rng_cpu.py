"""Attention dropout on the CPU: the Philox4x32-10 known answers, csrc/fa_dropout.h compiled for the host against the numpy
restatement (tests/dropout_ref.py), the custom ops under FakeTensorMode and the routing option."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dropout_ref as ref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "universal-metal-flash-attention_amd" / "csrc"

KNOWN = [  # Random123 known answers of philox4x32_10
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_restatement_known_answers(ctr, key, want):
    got = tuple(int(x) for x in ref.philox4x32_10(*ctr, *key))
    assert got == want


def test_threshold_and_scale():
    assert ref.threshold(2.0 ** -32) == 1
    assert ref.threshold(0.5) == 1 << 31
    assert ref.threshold(1 - 2.0 ** -32) == 0xFFFFFFFF
    assert ref.keep_scale(0.5) == 2.0
    assert abs(ref.keep_scale(0.1) - 1 / 0.9) < 1e-6


_SHIM = r"""
#include <stdint.h>
#include "fa_dropout.h"
extern "C" {
void philox(const uint32_t* c, const uint32_t* k, uint32_t* out) {
    umfa::DropWords w = umfa::philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
    for (int i = 0; i < 4; ++i) out[i] = w.w[i];
}
uint32_t threshold(double p) { return umfa::drop_threshold(p); }
float scale(uint32_t t) { return umfa::drop_scale(t); }
// keep bits at n coordinates
void keep(int64_t n, const uint32_t* i, const uint32_t* j, const uint32_t* bh, uint64_t seed, uint64_t offset, uint32_t thresh, uint8_t* out) {
    for (int64_t x = 0; x < n; ++x) out[x] = (umfa::drop_keep4(j[x] >> 2, i[x], bh[x], seed, offset, thresh) >> (j[x] & 3)) & 1u;
}
}
"""


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("fa_dropout_host")
    src = d / "shim.cpp"
    src.write_text(_SHIM)
    so = d / "libshim.so"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", f"-I{CSRC}", str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.threshold.restype = ctypes.c_uint32
    lib.threshold.argtypes = [ctypes.c_double]
    lib.scale.restype = ctypes.c_float
    lib.scale.argtypes = [ctypes.c_uint32]
    lib.keep.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    return lib


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_header_known_answers(host_lib, ctr, key, want):
    c = (ctypes.c_uint32 * 4)(*ctr)
    k = (ctypes.c_uint32 * 2)(*key)
    out = (ctypes.c_uint32 * 4)()
    host_lib.philox(c, k, out)
    assert tuple(out) == want


@pytest.mark.parametrize("p", [2.0 ** -32, 0.1, 0.5, 0.9, 1 - 2.0 ** -32])
def test_header_threshold_matches(host_lib, p):
    t = host_lib.threshold(p)
    assert t == ref.threshold(p)
    assert np.float32(host_lib.scale(t)) == np.float32(ref.keep_scale(p))


@pytest.mark.parametrize("p", [2.0 ** -32, 0.5, 1 - 2.0 ** -32, 0.1])
@pytest.mark.parametrize("seed,offset", [(0, 0), (0x0123456789ABCDEF, 0), (-7, 0xFFFFFFFF12345678), (2 ** 40 + 3, 97)])
def test_header_keep_matches_restatement(host_lib, p, seed, offset):
    rng = np.random.default_rng(abs(seed) % 1000 + int(p * 1000))
    n = 20000
    i = np.concatenate([rng.integers(0, 1 << 16, n // 2), rng.integers(1 << 16, 1 << 31, n // 2)]).astype(np.uint32)
    j = np.concatenate([rng.integers(0, 64, n // 4), rng.integers(1 << 16, 1 << 30, n // 4), rng.integers(0, 1 << 32, n // 2, dtype=np.uint64)]).astype(np.uint32)
    bh = np.concatenate([rng.integers(0, 96, n // 2), rng.integers(1 << 20, 1 << 32, n // 2, dtype=np.uint64)]).astype(np.uint32)
    out = np.zeros(n, np.uint8)
    t = ref.threshold(p)
    s64, o64 = seed & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFFFFFFFFFF
    host_lib.keep(n, i.ctypes.data, j.ctypes.data, bh.ctypes.data, s64, o64, t, out.ctypes.data)
    want = ref.keep_bits(i, j, bh, seed, offset, t)
    assert np.array_equal(out.astype(bool), want)
    if p == 2.0 ** -32:
        assert out.mean() > 0.999
    if p == 1 - 2.0 ** -32:
        assert out.mean() < 0.001


def test_custom_ops_trace_as_single_nodes():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.proxy_tensor import make_fx

    import umfa_torch  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        q = torch.empty(2, 4, 256, 64, device="cuda", dtype=torch.bfloat16)
        rs = torch.empty(2, device="cuda", dtype=torch.int64)
        gm = make_fx(lambda a, b, c, r: torch.ops.umfa.sdpa_forward_dropout(a, b, c, True, 0.125, 0.1, r), tracing_mode="fake")(q, q, q, rs)
        targets = [n.target for n in gm.graph.nodes if n.op == "call_function"]
        assert torch.ops.umfa.sdpa_forward_dropout.default in targets, targets
        out, lse = torch.ops.umfa.sdpa_forward_dropout(q, q, q, False, 0.125, 0.1, rs)
        assert out.shape == q.shape and out.dtype == q.dtype and lse.shape == (2 * 4 * 256,) and lse.dtype == torch.float32
        gb = make_fx(lambda d, a, b, c, o, l, r: torch.ops.umfa.sdpa_backward_dropout(d, a, b, c, o, l, False, 0.125, 0.1, r),
                     tracing_mode="fake")(q, q, q, q, q, lse, rs)
        targets = [n.target for n in gb.graph.nodes if n.op == "call_function"]
        assert torch.ops.umfa.sdpa_backward_dropout.default in targets, targets


def test_op_supports_follows_the_option(monkeypatch):
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode

    import umfa_torch
    from umfa_torch import dropout as drop
    with FakeTensorMode():
        q = torch.empty(2, 4, 256, 128, device="cuda", dtype=torch.bfloat16)
        q32 = torch.empty(2, 4, 256, 128, device="cuda", dtype=torch.float32)
        q256 = torch.empty(2, 4, 256, 256, device="cuda", dtype=torch.bfloat16)
        m = torch.empty(256, 256, device="cuda", dtype=torch.bool)
        monkeypatch.setattr(drop, "routing_enabled", lambda: False)
        assert not umfa_torch.library.op_supports(q, q, q, None, 0.1, True)
        monkeypatch.setattr(drop, "routing_enabled", lambda: True)
        assert umfa_torch.library.op_supports(q, q, q, None, 0.1, True)
        assert umfa_torch.library.op_supports(q, q, q, None, 0.1, False, True)
        assert not umfa_torch.library.op_supports(q, q, q, m, 0.1, True)
        assert not umfa_torch.library.op_supports(q32, q32, q32, None, 0.1, True)
        assert not umfa_torch.library.op_supports(q256, q256, q256, None, 0.1, True)
        assert not umfa_torch.library.op_supports(q, q, q, None, 1.0, True)
        assert umfa_torch.library.op_supports(q, q, q, None, 0.0, True)  # no dropout: the existing op, unchanged


def test_dropout_attention_scope_errors():
    import torch

    import umfa_torch
    q = torch.empty(1, 2, 8, 64, dtype=torch.bfloat16)  # host tensors: out of scope
    with pytest.raises(ValueError):
        umfa_torch.dropout_attention(q, q, q, 0.1)
