"""In-stream launches of the HIP kernels on torch-ROCm tensors (zero-copy).

Counterpart of the reference's try_instream_flash_attention + mps_utils::encode_attention_on_torch_stream
(metal_sdpa_backend.cpp:1308-1446, mps_utils.mm:115-247): raw device pointers, byte offsets folded into
the pointers, BHSD element strides, launched on torch's CURRENT stream -- no host synchronisation.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from umfa._ffi import (MFA_MASK_SCALAR_BF16, MFA_MASK_SCALAR_BYTE, MFA_MASK_SCALAR_FP16, MFA_MASK_SCALAR_FP32,
                       MFA_MASK_TYPE_ADDITIVE, MFA_MASK_TYPE_BOOL, MFA_MASK_TYPE_NONE, MFA_PRECISION_BF16,
                       MFA_PRECISION_FP16, MFA_PRECISION_FP32, MFAError, _check_error, _lib, mfa_context_t)

_PREC = {torch.float16: MFA_PRECISION_FP16, torch.bfloat16: MFA_PRECISION_BF16, torch.float32: MFA_PRECISION_FP32}
_PREC_NAME = {torch.float16: b"fp16", torch.bfloat16: b"bf16", torch.float32: b"fp32"}

_ctx = None


def context():
    """Process-wide context handle (created on first use; metal_sdpa_backend.cpp:936-955)."""
    global _ctx
    if _ctx is None:
        if not torch.cuda.is_available():
            raise RuntimeError("umfa_torch needs a ROCm device: there is no CPU fallback")
        h = mfa_context_t()
        _check_error(_lib.mfa_create_context(ctypes.byref(h)))
        _ctx = h
    return _ctx


def last_kernel() -> str:
    return _lib.umfa_last_kernel_name(context()).decode()


def release_scratch(stream=None, all_streams: bool = False) -> None:
    """Free the library's pooled device scratch of `stream` (default: torch's current stream) or of every stream
    (umfa_release_scratch): only when no graph captured with it will be replayed again."""
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    _check_error(_lib.umfa_release_scratch(context(), ctypes.c_void_p(st), 1 if all_streams else 0))


# launcher switches (include/umfa_abi.h umfa_set_option / umfa_get_option).  The LIBRARY holds the state (seeded once from the
# environment: UMFA_FORCE_W64, UMFA_W64_TAU, ...); this module only reads and writes it.
_OPTION_NAMES = ("softmax_reference", "softmax_tau", "w64_tau", "force_w64", "no_w64", "w64_grid", "w64_skew", "no_mask_flags", "bwd_exact",
                 "bwd_dq", "bwd_persist", "bwd_separate_delta", "no_split", "force_split", "no_dma", "bn64", "pv_fp16", "bwd_ds_store", "no_w64_mask", "ksplit", "no_pipe", "no_w64_mask_lazy", "no_w64_bias", "no_w64_f32_mask", "f32_mask_ratio", "mask_pass_ratio", "no_w64_ragged_mask", "no_mask_realign",
                 "cast_two_pass", "bwd_ds_lab", "cast_u", "quant_block_wg", "cast_wait_us", "cbal", "cbal_delta", "decode_ks", "sync_chunks", "sync_chunked_calls", "mirror_cache_hits", "no_bwd_mask", "sdpa_dropout")


def get_option(name: str) -> str:
    """The live value of a launcher switch as text."""
    buf = ctypes.create_string_buffer(64)
    _check_error(_lib.umfa_get_option(context(), name.encode(), buf, 64))
    return buf.value.decode()


def pv_fp16_status() -> int:
    """Round 4's status word of the fp16 P V product (1 = a V value left fp16's range).  Always 0 since round 5: V goes into the product as
    V * 2^-e, one power of two per (batch, head) slab chosen on the device, so the condition no longer exists.  Kept for round-4 callers."""
    return int(get_option("pv_fp16_status"))


def set_option(name: str, value) -> None:
    """Context-wide launcher switch, e.g. set_option("softmax_reference", "exact") -- see umfa_set_option in the header."""
    _check_error(_lib.umfa_set_option(context(), name.encode(), str(value).encode()))


class options:
    """with umfa_torch.options(softmax_reference="exact", force_w64=1): ...  -- sets the switches and puts the values the
    library held before back on exit.  Names are validated before anything is applied."""

    def __init__(self, **kw):
        unknown = [k for k in kw if k not in _OPTION_NAMES]
        if unknown:
            raise KeyError(f"unknown launcher switch(es) {unknown}; known: {_OPTION_NAMES}")
        self.kw = kw
        self.prev = {}

    def __enter__(self):
        prev = {k: get_option(k) for k in self.kw}  # everything read before anything is written
        if "w64_tau" in self.kw or "softmax_tau" in self.kw:  # w64_tau also moves the reference policy
            prev.setdefault("softmax_reference", get_option("softmax_reference"))
        for k, v in self.kw.items():
            set_option(k, v)
        self.prev = prev
        return self

    def __exit__(self, *exc):
        ref = self.prev.pop("softmax_reference", None)
        for k, v in self.prev.items():
            set_option("softmax_tau" if k == "w64_tau" else k, v)
        if ref is not None:
            set_option("softmax_reference", ref)
        return False


def _i64(vals):
    return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


def _mask_args(mask: Optional[torch.Tensor]):
    if mask is None:
        return None, None, None, 0, MFA_MASK_TYPE_NONE, MFA_MASK_SCALAR_BYTE
    if mask.dtype == torch.bool:
        mt, ms = MFA_MASK_TYPE_BOOL, MFA_MASK_SCALAR_BYTE
    elif mask.dtype == torch.float32:
        mt, ms = MFA_MASK_TYPE_ADDITIVE, MFA_MASK_SCALAR_FP32
    elif mask.dtype == torch.float16:
        mt, ms = MFA_MASK_TYPE_ADDITIVE, MFA_MASK_SCALAR_FP16
    elif mask.dtype == torch.bfloat16:
        mt, ms = MFA_MASK_TYPE_ADDITIVE, MFA_MASK_SCALAR_BF16
    else:
        raise TypeError(f"unsupported mask dtype {mask.dtype}")
    if mask.dim() > 4:
        raise ValueError("attention masks of more than 4 dims are not supported")
    return (ctypes.c_void_p(mask.data_ptr()), _i64(mask.shape), _i64(mask.stride()), mask.dim(), mt, ms)


def _quant_mode(name: str) -> int:
    """"tensor" -> 0, "blockwise" -> 2 (the reference's two modes, MFABridge+Quantized.swift:268-272), "blockwise_fp8pv" -> 3:
    UMFA_QUANT_BLOCKWISE_FP8PV, the MI355X fast mode (block-wise int8 Q K^T, fp8 e4m3 P and V on the 2x-rate MFMA)."""
    n = name.lower()
    return 3 if "fp8" in n else 2 if n.startswith("block") else 0


def attention_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, scale: Optional[float] = None,
                      causal: bool = False, mask: Optional[torch.Tensor] = None, out_dtype=None,
                      return_lse: bool = False, intermediate_dtype=None, out: Optional[torch.Tensor] = None,
                      window=None):
    """q [B,H,Sq,D], k/v [B,H,Skv,D] device tensors (any BHSD strides with a contiguous last dim).

    window=(left, right): sliding-window attention without a mask tensor -- key j attends to row i iff
    i - left <= j <= i + right (add causal=True for a look-back-only window); key tiles outside the band are never
    touched, so the cost follows the band, not Skv.  Exclusive with `mask`.

    out_dtype: torch.float32 (the C-ABI contract) or q.dtype (fused cast-back epilogue).
    Asynchronous on torch's current stream.
    """
    assert q.is_cuda and k.is_cuda and v.is_cuda, "device tensors required"
    B, H, Sq, D = q.shape
    Skv = k.shape[2]
    if scale is None:
        scale = D ** -0.5
    out_dtype = out_dtype or q.dtype
    for t in (q, k, v):
        if t.stride(-1) != 1:
            raise ValueError("last dimension must be contiguous")
    if out is None:
        out = torch.empty((B, H, Sq, D), dtype=out_dtype, device=q.device)
    lse = torch.empty((B * H * Sq,), dtype=torch.float32, device=q.device) if return_lse else None
    if window is not None:
        if mask is not None:
            raise ValueError("window and mask are exclusive")
        mptr, mshape, mstr, mnd, mt, ms = None, _i64((int(window[0]), int(window[1]))), None, 0, 3, MFA_MASK_SCALAR_BYTE
    else:
        mptr, mshape, mstr, mnd, mt, ms = _mask_args(mask)
    inter = _PREC[intermediate_dtype or q.dtype]
    stream = torch.cuda.current_stream(q.device).cuda_stream
    _check_error(_lib.umfa_attention_forward_stream(
        context(), ctypes.c_void_p(stream),
        ctypes.c_void_p(q.data_ptr()), _i64(q.stride()), ctypes.c_void_p(k.data_ptr()), _i64(k.stride()),
        ctypes.c_void_p(v.data_ptr()), _i64(v.stride()), ctypes.c_void_p(out.data_ptr()), _PREC[out.dtype],
        ctypes.c_void_p(lse.data_ptr()) if lse is not None else None,
        mptr, mshape, mstr, mnd, mt, ms, B, Sq, Skv, H, D, float(scale), bool(causal), _PREC[q.dtype], inter))
    return (out, lse) if return_lse else out


def attention_encode(q, k, v, out32, *, scale=None, causal=False, mask=None, stream=None):
    """The reference's exact in-stream entry (mfa_attention_encode_mtl): fp32 dense output, precisions as
    strings, byte offsets (0 here: data_ptr() already includes the storage offset)."""
    B, H, Sq, D = q.shape
    Skv = k.shape[2]
    if scale is None:
        scale = D ** -0.5
    mptr, mshape, mstr, mnd, mt, ms = _mask_args(mask)
    s = stream if stream is not None else torch.cuda.current_stream(q.device).cuda_stream
    _check_error(_lib.mfa_attention_encode_mtl(
        context(), ctypes.c_void_p(s),
        ctypes.c_void_p(q.data_ptr()), 0, _i64(q.stride()), ctypes.c_void_p(k.data_ptr()), 0, _i64(k.stride()),
        ctypes.c_void_p(v.data_ptr()), 0, _i64(v.stride()), ctypes.c_void_p(out32.data_ptr()), 0,
        mptr, 0, mshape, mstr, mnd, mt, ms, B, Sq, Skv, H, D, float(scale), bool(causal),
        _PREC_NAME[q.dtype], _PREC_NAME[q.dtype]))
    return out32


class _DevBuf:
    """mfa_buffer_t view of a device tensor (mfa_buffer_from_mtl_buffer: borrowed raw device pointer)."""

    def __init__(self, t: Optional[torch.Tensor]):
        from umfa._ffi import mfa_buffer_t
        self.handle = mfa_buffer_t()
        if t is not None:
            _check_error(_lib.mfa_buffer_from_mtl_buffer(context(), ctypes.c_void_p(t.data_ptr()),
                                                         t.numel() * t.element_size(), ctypes.byref(self.handle)))

    def close(self):
        if self.handle:
            _lib.mfa_destroy_buffer(self.handle)
            self.handle = None


def quantized_attention_forward(q, k, v, *, scale=None, causal=False, mask=None, bits: int = 8,
                                quant_mode: str = "blockwise"):
    """Runtime-quantised SDPA on device tensors through mfa_quantized_forward_with_lse (synchronous, like the
    reference's MetalQuantizedFlashAttentionFn::forward, metal_sdpa_backend.cpp:3142-3267).
    Returns (O fp32 [B,H,Sq,D], LSE fp32 [B*H*Sq]); GPU seconds of quantiser + attention via gpu_latency()."""
    B, H, Sq, D = q.shape
    Skv = k.shape[2]
    if scale is None:
        scale = D ** -0.5
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    out = torch.empty((B, H, Sq, D), dtype=torch.float32, device=q.device)
    lse = torch.empty((B * H * Sq,), dtype=torch.float32, device=q.device)
    m32 = None
    if mask is not None:
        m32 = torch.zeros((B, H, Sq, Skv), dtype=torch.float32, device=q.device)
        m32 = m32.masked_fill(~mask, float("-inf")) if mask.dtype == torch.bool else m32 + mask.float()
        m32 = m32.contiguous()
    torch.cuda.current_stream(q.device).synchronize()  # the entry runs on the legacy default stream
    bufs = [_DevBuf(t) for t in (q, k, v, out, lse, m32)]
    try:
        _check_error(_lib.mfa_quantized_forward_with_lse(
            context(), *(b.handle for b in bufs), B, Sq, Skv, H, D, float(scale), bool(causal),
            4 if bits == 4 else 3, _quant_mode(quant_mode), _PREC[q.dtype]))
    finally:
        for b in bufs:
            b.close()
    return out, lse


def quantized_attention_forward_stream(q, k, v, *, scale=None, causal=False, mask=None, bits: int = 8,
                                       quant_mode: str = "blockwise", return_lse: bool = False, out=None, lse=None):
    """quantized_attention_forward without the host round trips: umfa_quantized_forward_stream on torch's current
    stream (asynchronous).  Same numbers as the blocking entry.  out / lse: caller-provided fp32 [B,H,Sq,D] / [B*H*Sq]
    (no allocation on the launch path, like attention_forward's out=)."""
    B, H, Sq, D = q.shape
    Skv = k.shape[2]
    if scale is None:
        scale = D ** -0.5
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    if out is None:
        out = torch.empty((B, H, Sq, D), dtype=torch.float32, device=q.device)
    if lse is None:
        lse = torch.empty((B * H * Sq,), dtype=torch.float32, device=q.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and lse.dtype == torch.float32 and lse.numel() == B * H * Sq
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
    tail = (B, Sq, Skv, H, D, float(scale), bool(causal), 4 if bits == 4 else 3, _quant_mode(quant_mode), _PREC[q.dtype])
    if mask is not None and hasattr(_lib, "umfa_quantized_forward_masked_stream"):
        # the mask as the caller has it -- any <= 4-D broadcastable bool / float tensor, read in place with its strides -- instead of the dense
        # fp32 [B, H, Sq, Skv] expansion of the reference's quantised entry (4.3 GB at config 4; a bool [1, 1, S, S] mask is 64 MB)
        mptr, mshape, mstr, mnd, mt, ms = _mask_args(mask)
        _check_error(_lib.umfa_quantized_forward_masked_stream(context(), stream, vp(q), vp(k), vp(v), vp(out), vp(lse), mptr, mshape, mstr, mnd, mt, ms, *tail))
        return (out, lse) if return_lse else out
    m32 = None
    if mask is not None:  # (a library without the masked entry: UMFA_LIBRARY pointing at an older build)
        if mask.dtype == torch.float32 and tuple(mask.shape) == (B, H, Sq, Skv) and mask.is_contiguous():
            m32 = mask
        else:
            m32 = torch.zeros((B, H, Sq, Skv), dtype=torch.float32, device=q.device)
            m32 = (m32.masked_fill(~mask, float("-inf")) if mask.dtype == torch.bool else m32 + mask.float()).contiguous()
    _check_error(_lib.umfa_quantized_forward_stream(context(), stream, vp(q), vp(k), vp(v), vp(out), vp(lse), vp(m32), *tail))
    return (out, lse) if return_lse else out


def quantized_attention_backward_stream(dout, q, k, v, o32, lse, *, scale=None, causal=False, bits: int = 8,
                                        quant_mode: str = "blockwise"):
    """Backward of quantized_attention_forward_stream, in-stream (umfa_quantized_backward_stream): contiguous BHSD device
    tensors, O fp32 and LSE from the quantised forward.  Returns (dq, dk, dv, status): fp32 gradients and a device
    uint32 that round 4 set when an operand left fp16's range on the 16-bit MFMA engine; every operand enters that engine as
    a power-of-two multiple now (exponents chosen on the device), so it stays 0."""
    B, H, Sq, D = q.shape
    Skv = k.shape[2]
    if scale is None:
        scale = D ** -0.5
    for t in (dout, q, k, v, o32, lse):
        assert t.is_cuda and t.is_contiguous()
    assert o32.dtype == torch.float32 and lse.dtype == torch.float32 and dout.dtype == q.dtype
    dq = torch.empty((B, H, Sq, D), dtype=torch.float32, device=q.device)
    dk = torch.empty((B, H, Skv, D), dtype=torch.float32, device=q.device)
    dv = torch.empty_like(dk)
    status = torch.zeros(1, dtype=torch.int32, device=q.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _check_error(_lib.umfa_quantized_backward_stream(
        context(), ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream), vp(q), vp(k), vp(v), vp(o32), vp(dout),
        vp(lse), vp(dq), vp(dk), vp(dv), vp(status), B, Sq, Skv, H, D, float(scale), bool(causal), 4 if bits == 4 else 3,
        _quant_mode(quant_mode), _PREC[q.dtype]))
    return dq, dk, dv, status


def attention_backward_gqa(dout, q, k, v, o, lse, *, scale: float, causal: bool = False):
    """dQ [B,Hq,Sq,D], dK, dV [B,Hkv,Skv,D] of grouped-query attention with K / V read IN PLACE (no repeat_interleave
    copies): umfa_attention_backward_gqa_stream, in-stream, gradients in q.dtype.  Returns None when the 16-bit MFMA
    backward cannot serve the call (fp32 operands, head_dim other than 64 / 128 / 256): the caller then expands K / V."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    for t in (dout, q, k, v, o, lse):
        assert t.is_cuda and t.is_contiguous()
    if q.dtype == torch.float32 or D not in (64, 128, 256) or Hq % Hkv:
        return None
    assert o.dtype in (torch.float32, q.dtype) and lse.dtype == torch.float32 and dout.dtype == q.dtype
    dq = torch.empty_like(q)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    dvec = torch.empty((B * Hq * Sq,), dtype=torch.float32, device=q.device)
    rc = _lib.umfa_attention_backward_gqa_stream(
        context(), ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream),
        *(ctypes.c_void_p(t.data_ptr()) for t in (dout, q, k, v, o, lse, dq, dk, dv, dvec)),
        B, Sq, Skv, Hq, Hkv, D, float(scale), bool(causal), _PREC[q.dtype], True, o.dtype != torch.float32)
    if rc == 1:
        return None
    _check_error(rc)
    return dq, dk, dv


def gpu_latency() -> float:
    return float(_lib.mfa_get_gpu_latency(context()))


def attention_backward(dout, q, k, v, o32, lse, *, scale: float, causal: bool = False, grads_in_input_type: bool = True,
                       intermediate_dtype=None, keep_fp32: bool = False, mask: Optional[torch.Tensor] = None, window=None):
    """dQ, dK, dV of the SDPA in-stream (umfa_attention_backward_stream): contiguous BHSD device tensors, O fp32 and LSE
    from the forward; asynchronous on torch's current stream.  Gradients come back in q.dtype straight from the kernels
    when the 16-bit MFMA backward serves the call, else fp32 tensors cast afterwards (same values the blocking ABI gives).

    mask / window: the forward call's mask (any strides, as attention_forward takes it) or sliding window (left, right)
    -- umfa_attention_backward_masked_stream; head_dim <= 256.  With neither, the unmasked call."""
    B, H, Sq, D = q.shape
    Skv = k.shape[2]
    for t in (dout, q, k, v, o32, lse):
        assert t.is_cuda and t.is_contiguous()
    assert o32.dtype in (torch.float32, q.dtype) and lse.dtype == torch.float32 and dout.dtype == q.dtype
    o_typed = o32.dtype != torch.float32  # O in the operand type (what the forward returned) instead of an fp32 copy
    inter = _PREC[intermediate_dtype or q.dtype]
    dvec = torch.empty((B * H * Sq,), dtype=torch.float32, device=q.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)

    if window is not None:
        if mask is not None:
            raise ValueError("window and mask are exclusive")
        margs = (None, _i64((int(window[0]), int(window[1]))), None, 0, 3, MFA_MASK_SCALAR_BYTE)
    elif mask is not None:
        margs = _mask_args(mask)
    else:
        margs = None

    def call(gdt, typed):
        dq = torch.empty((B, H, Sq, D), dtype=gdt, device=q.device)
        dk = torch.empty((B, H, Skv, D), dtype=gdt, device=q.device)
        dv = torch.empty_like(dk)
        ptrs = (ctypes.c_void_p(t.data_ptr()) for t in (dout, q, k, v, o32, lse, dq, dk, dv, dvec))
        if margs is None:
            rc = _lib.umfa_attention_backward_stream(context(), stream, *ptrs, B, Sq, Skv, H, D, float(scale), bool(causal),
                                                     _PREC[q.dtype], inter, typed, o_typed)
        else:
            rc = _lib.umfa_attention_backward_masked_stream(context(), stream, *ptrs, B, Sq, Skv, H, D, float(scale), bool(causal),
                                                            _PREC[q.dtype], inter, typed, o_typed, *margs)
        return rc, dq, dk, dv

    if grads_in_input_type and not keep_fp32 and q.dtype != torch.float32:
        rc, dq, dk, dv = call(q.dtype, True)
        if rc == 0:
            return dq, dk, dv
    rc, dq, dk, dv = call(torch.float32, False)
    _check_error(rc)
    if keep_fp32:  # the caller post-processes the gradients in fp32 (RoPE inverse rotation)
        return dq, dk, dv
    return dq.to(q.dtype), dk.to(q.dtype), dv.to(q.dtype)


def attention_forward_dropout(q, k, v, dropout_p: float, rng_state: torch.Tensor, *, scale: float, causal: bool = False, out_dtype=None):
    """O and the undropped LSE [B*H*Sq] of the SDPA with attention dropout (umfa_attention_forward_dropout_stream): q [B,H,Sq,D], k / v
    [B,H,Skv,D] fp16 / bf16 device tensors with contiguous rows, rng_state a device int64[2] = {seed, offset}.  Asynchronous on torch's
    current stream."""
    B, H, Sq, D = q.shape
    Skv = k.shape[2]
    out = torch.empty((B, H, Sq, D), dtype=out_dtype or q.dtype, device=q.device)
    lse = torch.empty((B * H * Sq,), dtype=torch.float32, device=q.device)
    stream = torch.cuda.current_stream(q.device).cuda_stream
    _check_error(_lib.umfa_attention_forward_dropout_stream(
        context(), ctypes.c_void_p(stream), ctypes.c_void_p(q.data_ptr()), _i64(q.stride()), ctypes.c_void_p(k.data_ptr()), _i64(k.stride()),
        ctypes.c_void_p(v.data_ptr()), _i64(v.stride()), ctypes.c_void_p(out.data_ptr()), _PREC[out.dtype], ctypes.c_void_p(lse.data_ptr()),
        B, Sq, Skv, H, D, float(scale), bool(causal), _PREC[q.dtype], _PREC[q.dtype], float(dropout_p), ctypes.c_void_p(rng_state.data_ptr())))
    return out, lse


def attention_backward_dropout(dout, q, k, v, out, lse, dropout_p: float, rng_state: torch.Tensor, *, scale: float, causal: bool = False,
                               grads_in_input_type: bool = True):
    """dQ, dK, dV of attention_forward_dropout (umfa_attention_backward_dropout_stream): contiguous BHSD device tensors, `out` the dropped
    O the forward returned (operand type or fp32), `lse` its LSE, the forward's dropout_p and rng_state."""
    B, H, Sq, D = q.shape
    Skv = k.shape[2]
    for t in (dout, q, k, v, out, lse):
        assert t.is_cuda and t.is_contiguous()
    gdt = q.dtype if grads_in_input_type else torch.float32
    dq = torch.empty((B, H, Sq, D), dtype=gdt, device=q.device)
    dk = torch.empty((B, H, Skv, D), dtype=gdt, device=q.device)
    dv = torch.empty_like(dk)
    dvec = torch.empty((B * H * Sq,), dtype=torch.float32, device=q.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
    ptrs = (ctypes.c_void_p(t.data_ptr()) for t in (dout, q, k, v, out, lse, dq, dk, dv, dvec))
    _check_error(_lib.umfa_attention_backward_dropout_stream(
        context(), stream, *ptrs, B, Sq, Skv, H, D, float(scale), bool(causal), _PREC[q.dtype], _PREC[q.dtype], bool(grads_in_input_type),
        out.dtype != torch.float32, float(dropout_p), ctypes.c_void_p(rng_state.data_ptr())))
    return dq, dk, dv


def dropout_keep_mask(B: int, H: int, Sq: int, Skv: int, dropout_p: float, rng_state: torch.Tensor) -> torch.Tensor:
    """The keep mask the dropout kernels apply, as a uint8 [B, H, Sq, Skv] tensor of 0 / 1 (umfa_dropout_keep_mask_stream)."""
    keep = torch.empty((B, H, Sq, Skv), dtype=torch.uint8, device=rng_state.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(rng_state.device).cuda_stream)
    _check_error(_lib.umfa_dropout_keep_mask_stream(context(), stream, ctypes.c_void_p(keep.data_ptr()), B, H, Sq, Skv, float(dropout_p),
                                                    ctypes.c_void_p(rng_state.data_ptr())))
    return keep


def bench_int8(steps: int = 20, warmup: int = 3):
    """int8 block-quantised forward vs the bf16 forward on the same tensors (quantiser pre-pass included),
    for the FLUX shape and BASELINE config 4 (B1 H16 S8192 D128).  GPU time from the library's hipEvents."""
    res = {}
    for name, (B, H, S, D) in {"flux_B1_H24_S4096_D128": (1, 24, 4096, 128), "cfg4_B1_H16_S8192_D128": (1, 16, 8192, 128)}.items():
        torch.manual_seed(0)
        q, k, v = (torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16) for _ in range(3))
        out = torch.empty(B, H, S, D, device="cuda", dtype=torch.float32)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        for _ in range(warmup):
            attention_forward(q, k, v, out=out)
        for a, b in ev:
            a.record()
            attention_forward(q, k, v, out=out)
            b.record()
        torch.cuda.synchronize()
        bf = sorted(a.elapsed_time(b) for a, b in ev)
        t8 = []
        for i in range(warmup + steps):
            quantized_attention_forward(q, k, v)
            if i >= warmup:
                t8.append(gpu_latency() * 1e3)
        t8.sort()
        flops = 4.0 * B * H * S * S * D
        res[name] = {"bf16_ms": round(bf[len(bf) // 2], 4), "int8_ms_incl_quantiser": round(t8[len(t8) // 2], 4),
                     "speedup": round(bf[len(bf) // 2] / t8[len(t8) // 2], 3),
                     "int8_TOPs": round(flops / (t8[len(t8) // 2] * 1e-3) / 1e12, 1), "fp32_out": True}
        del q, k, v, out
    return res


def rope_rotate(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *, negate_sin: bool = False) -> torch.Tensor:
    """Interleaved-pair rotary rotation in-stream (mfa_rope_rotate_encode_mtl, MFABridge.swift:2286-2375).
    x [B,H,S,D] with a contiguous last dim; cos/sin fp32 [S,D] (shared) or [B,S,D], pair-duplicated.
    Returns a dense [B,H,S,D] tensor of x's dtype.  negate_sin=True is the inverse rotation (backward of Q/K)."""
    B, H, S, D = x.shape
    assert x.is_cuda and x.stride(-1) == 1 and cos.dtype == torch.float32 and sin.dtype == torch.float32
    cos, sin = cos.contiguous(), sin.contiguous()
    tb = S * D if cos.dim() == 3 else 0
    out = torch.empty((B, H, S, D), dtype=x.dtype, device=x.device)
    lib = _lib
    lib.mfa_rope_rotate_encode_mtl.restype = ctypes.c_int
    lib.mfa_rope_rotate_encode_mtl.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                               ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_int64, ctypes.c_int64, ctypes.c_bool, ctypes.c_uint32,
                                               ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p]
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _check_error(lib.mfa_rope_rotate_encode_mtl(context(), ctypes.c_void_p(stream), ctypes.c_void_p(x.data_ptr()), 0,
                                                x.stride(0), x.stride(1), x.stride(2), ctypes.c_void_p(out.data_ptr()), 0,
                                                ctypes.c_void_p(cos.data_ptr()), 0, ctypes.c_void_p(sin.data_ptr()), 0,
                                                tb, bool(negate_sin), B, H, S, D, _PREC_NAME[x.dtype]))
    return out


def rope_attention_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *,
                           scale: Optional[float] = None, causal: bool = False, out_dtype=None,
                           return_lse: bool = False):
    """softmax(rope(q) rope(k)^T * scale) v in ONE in-stream call (umfa_rope_attention_forward_stream): K is rotated
    once into the stream's workspace, Q inside the attention kernel behind its fragment load.  Bit-identical to
    rope_rotate(q), rope_rotate(k), attention_forward (the reference's sequence, metal_sdpa_backend.cpp:1472-1641).
    q, k, v [B,H,S,D] (same S), contiguous last dim; cos / sin fp32 [S,D] or [B,S,D], pair-duplicated."""
    assert q.is_cuda and k.is_cuda and v.is_cuda, "device tensors required"
    B, H, Sq, D = q.shape
    Skv = k.shape[2]
    for t in (q, k, v):
        if t.stride(-1) != 1:
            raise ValueError("last dimension must be contiguous")
    if cos.dtype != torch.float32 or sin.dtype != torch.float32 or cos.shape != sin.shape or cos.shape[-2:] != (Sq, D):
        raise ValueError("cos / sin must be fp32 [S, D] or [B, S, D]")
    cos, sin = cos.contiguous(), sin.contiguous()
    tb = Sq * D if cos.dim() == 3 else 0
    if scale is None:
        scale = D ** -0.5
    out = torch.empty((B, H, Sq, D), dtype=out_dtype or q.dtype, device=q.device)
    lse = torch.empty((B * H * Sq,), dtype=torch.float32, device=q.device) if return_lse else None
    stream = torch.cuda.current_stream(q.device).cuda_stream
    _check_error(_lib.umfa_rope_attention_forward_stream(
        context(), ctypes.c_void_p(stream),
        ctypes.c_void_p(q.data_ptr()), _i64(q.stride()), ctypes.c_void_p(k.data_ptr()), _i64(k.stride()),
        ctypes.c_void_p(v.data_ptr()), _i64(v.stride()), ctypes.c_void_p(out.data_ptr()), _PREC[out.dtype],
        ctypes.c_void_p(lse.data_ptr()) if lse is not None else None,
        ctypes.c_void_p(cos.data_ptr()), ctypes.c_void_p(sin.data_ptr()), tb, B, Sq, Skv, H, D, float(scale),
        bool(causal), _PREC[q.dtype], _PREC[q.dtype]))
    return (out, lse) if return_lse else out


def hadamard_rotate(t: torch.Tensor, block_size: int) -> torch.Tensor:
    """In-place group-wise Hadamard rotation of a contiguous fp32 / fp16 tensor (reference: hadamard_rotate_inplace,
    metal_sdpa_backend.cpp:3400-3418).  Applying it twice is the identity."""
    assert t.is_cuda and t.is_contiguous() and t.dtype in (torch.float32, torch.float16)
    if t.numel() % block_size:
        raise RuntimeError("Tensor size not divisible by block_size")
    _lib.mfa_hadamard_rotate.restype = ctypes.c_int32
    _lib.mfa_hadamard_rotate.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    context()
    torch.cuda.current_stream(t.device).synchronize()
    buf = _DevBuf(t)
    try:
        _check_error(_lib.mfa_hadamard_rotate(buf.handle, block_size, t.numel() // block_size))
    finally:
        buf.close()
    return t


def varlen_attention_forward(q, k, v, cu_seq_q, cu_seq_k, max_q: int, max_k: int, *, scale: float, causal: bool = False, out_dtype=None,
                             out: Optional[torch.Tensor] = None, window: Optional[Tuple[int, int]] = None):
    """O [T_q, H, D] and LSE [H, T_q] (fp32, natural log) of packed variable-length attention (umfa_varlen_attention_forward_stream):
    q [T_q, H, D], k / v [T_k, H_kv, D] fp16 / bf16 device tensors with a contiguous head_dim (token / head strides multiples of 8),
    cu_seq_q / cu_seq_k device int32 [N + 1].  Causal is bottom-right per sequence.  `out`: a caller-allocated dense [T_q, H, D] view
    to write into.  `window`: (left, right), flash-attention's window_size (umfa_varlen_attention_forward_window_stream; -1 unbounded).
    Asynchronous on torch's current stream; the offsets are never read back."""
    Tq, H, D = q.shape
    Tk, Hkv = k.shape[0], k.shape[1]
    N = cu_seq_q.numel() - 1
    if out is None:
        out = torch.empty((Tq, H, D), dtype=out_dtype or q.dtype, device=q.device)
    lse = torch.empty((H, Tq), dtype=torch.float32, device=q.device)
    stream = torch.cuda.current_stream(q.device).cuda_stream
    args = (context(), ctypes.c_void_p(stream), ctypes.c_void_p(q.data_ptr()), _i64(q.stride()[:2]), ctypes.c_void_p(k.data_ptr()),
            _i64(k.stride()[:2]), ctypes.c_void_p(v.data_ptr()), _i64(v.stride()[:2]), ctypes.c_void_p(cu_seq_q.data_ptr()),
            ctypes.c_void_p(cu_seq_k.data_ptr()), N, Tq, Tk, int(max_q), int(max_k), H, Hkv, D, float(scale), bool(causal), _PREC[q.dtype],
            ctypes.c_void_p(out.data_ptr()), _PREC[out.dtype], ctypes.c_void_p(lse.data_ptr()))
    if window is None:
        _check_error(_lib.umfa_varlen_attention_forward_stream(*args))
    else:
        _check_error(_lib.umfa_varlen_attention_forward_window_stream(*args, int(window[0]), int(window[1])))
    return out, lse


def varlen_attention_backward(dout, q, k, v, out, lse, cu_seq_q, cu_seq_k, max_q: int, max_k: int, *, scale: float, causal: bool = False,
                              grads_in_input_type: bool = True, window: Optional[Tuple[int, int]] = None):
    """dQ [T_q, H, D], dK / dV [T_k, H_kv, D] of varlen_attention_forward (umfa_varlen_attention_backward_stream): dout and out dense
    [T_q, H, D] (out in the operand type or fp32), lse the forward's [H, T_q]; q / k / v and `window` as the forward takes them."""
    Tq, H, D = q.shape
    Tk, Hkv = k.shape[0], k.shape[1]
    N = cu_seq_q.numel() - 1
    for t in (dout, out, lse):
        assert t.is_cuda and t.is_contiguous()
    gdt = q.dtype if grads_in_input_type else torch.float32
    dq = torch.empty((Tq, H, D), dtype=gdt, device=q.device)
    dk = torch.empty((Tk, Hkv, D), dtype=gdt, device=q.device)
    dv = torch.empty_like(dk)
    stream = ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream)
    args = (context(), stream, ctypes.c_void_p(dout.data_ptr()), ctypes.c_void_p(q.data_ptr()), _i64(q.stride()[:2]),
            ctypes.c_void_p(k.data_ptr()), _i64(k.stride()[:2]), ctypes.c_void_p(v.data_ptr()), _i64(v.stride()[:2]),
            ctypes.c_void_p(out.data_ptr()), out.dtype != torch.float32, ctypes.c_void_p(lse.data_ptr()), ctypes.c_void_p(cu_seq_q.data_ptr()),
            ctypes.c_void_p(cu_seq_k.data_ptr()), N, Tq, Tk, int(max_q), int(max_k), H, Hkv, D, float(scale), bool(causal), _PREC[q.dtype],
            ctypes.c_void_p(dq.data_ptr()), ctypes.c_void_p(dk.data_ptr()), ctypes.c_void_p(dv.data_ptr()), bool(grads_in_input_type))
    if window is None:
        _check_error(_lib.umfa_varlen_attention_backward_stream(*args))
    else:
        _check_error(_lib.umfa_varlen_attention_backward_window_stream(*args, int(window[0]), int(window[1])))
    return dq, dk, dv


def _rope_args(name, q, cos, sin, interleaved):
    """the rotary tail of the *_rope_forward_stream entries: (cos, sin, table precision, row stride, seqlen_ro, rotary_dim, interleaved)"""
    if not isinstance(cos, torch.Tensor) or not isinstance(sin, torch.Tensor) or cos.dim() != 2 or cos.shape != sin.shape \
            or cos.dtype != sin.dtype or cos.device != q.device or sin.device != q.device or cos.dtype not in (torch.float32, q.dtype):
        raise ValueError(f"{name}: rotary_cos / rotary_sin must be equal-shaped [seqlen_ro, rotary_dim / 2] tensors on q's device, fp32 or q's dtype")
    if cos.shape[0] == 0 or cos.stride() != sin.stride() or (cos.shape[1] > 1 and cos.stride(1) != 1) \
            or (cos.stride(0) * cos.element_size()) % 16 or cos.data_ptr() % 16 or sin.data_ptr() % 16:
        raise ValueError(f"{name}: the rotary tables need seqlen_ro > 0, a unit column stride, equal strides and 16-byte aligned rows")
    return (ctypes.c_void_p(cos.data_ptr()), ctypes.c_void_p(sin.data_ptr()), _PREC[cos.dtype], int(cos.stride(0)), int(cos.shape[0]),
            2 * int(cos.shape[1]), bool(interleaved))


def _out_buffers(name, q, o_shape, lse_shape, out_dtype, out, lse):
    """(out, lse) of a KV-cache call: fresh tensors, or the caller's -- dense, 16-byte aligned, of the right shape, dtype and device"""
    if out is None:
        out = torch.empty(o_shape, dtype=out_dtype or q.dtype, device=q.device)
    elif tuple(out.shape) != tuple(o_shape) or out.dtype not in (q.dtype, torch.float32) or out.device != q.device or not out.is_contiguous() \
            or out.data_ptr() % 16:
        raise ValueError(f"{name}: out must be a dense, 16-byte aligned {tuple(o_shape)} tensor in q's dtype or fp32 on q's device")
    if lse is None:
        lse = torch.empty(lse_shape, dtype=torch.float32, device=q.device)
    elif tuple(lse.shape) != tuple(lse_shape) or lse.dtype != torch.float32 or lse.device != q.device or not lse.is_contiguous():
        raise ValueError(f"{name}: lse must be a dense fp32 {tuple(lse_shape)} tensor on q's device")
    return out, lse


def _kvcache_forward(entry, extra, q, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new, scale, causal, num_splits, out_dtype,
                     out=None, lse=None):
    """the call the KV-cache entries share; extra: the arguments behind num_splits (the fp8 entry's descales, the rotary entry's tail);
    out / lse: the caller's buffers (_out_buffers)"""
    B, Sq, H, D = q.shape
    if B > 1 and (cache_seqlens.stride(0) != 1 or (block_table is not None and block_table.stride(1) != 1)):
        raise ValueError("kvcache_attention_forward: cache_seqlens and the rows of block_table must be contiguous")
    num_pages, page_size, Hkv = k_cache.shape[0], k_cache.shape[1], k_cache.shape[2]
    if block_table is not None:
        max_pages, bt_stride, bt = block_table.shape[1], block_table.stride(0), ctypes.c_void_p(block_table.data_ptr())
    else:
        max_pages, bt_stride, bt = 1, 0, None
    Snew = 0 if k_new is None else k_new.shape[1]
    out, lse = _out_buffers("kvcache_attention_forward", q, (B, Sq, H, D), (B, H, Sq), out_dtype, out, lse)
    stream = torch.cuda.current_stream(q.device).cuda_stream
    new = [None, None, None, None]
    if Snew:
        new = [ctypes.c_void_p(k_new.data_ptr()), _i64(k_new.stride()[:3]), ctypes.c_void_p(v_new.data_ptr()), _i64(v_new.stride()[:3])]
    _check_error(entry(
        context(), ctypes.c_void_p(stream), ctypes.c_void_p(q.data_ptr()), _i64(q.stride()[:3]), ctypes.c_void_p(k_cache.data_ptr()),
        _i64(k_cache.stride()[:3]), ctypes.c_void_p(v_cache.data_ptr()), _i64(v_cache.stride()[:3]), *new, bt, int(bt_stride),
        ctypes.c_void_p(cache_seqlens.data_ptr()), B, Sq, Snew, H, Hkv, D, int(page_size), int(num_pages), int(max_pages), float(scale),
        bool(causal), _PREC[q.dtype], ctypes.c_void_p(out.data_ptr()), _PREC[out.dtype], ctypes.c_void_p(lse.data_ptr()), int(num_splits),
        *extra))
    return out, lse


def kvcache_attention_forward(q, k_cache, v_cache, cache_seqlens, block_table=None, k_new=None, v_new=None, *, scale: float,
                              causal: bool = False, num_splits: int = 0, out_dtype=None):
    """O [B, Sq, H, D] and LSE [B, H, Sq] (fp32, natural log) of attention over a paged or static KV cache
    (umfa_kvcache_attention_forward_stream), appending k_new / v_new [B, S_new, H_kv, D] into the cache in place first.
    q [B, Sq, H, D]; paged: k_cache / v_cache [num_pages, page_size, H_kv, D] with block_table device int32 [B, max_pages]; static
    (block_table None): k_cache / v_cache [B, S_max, H_kv, D] -- HF's [B, H_kv, S_max, D] as its .transpose(1, 2) view, no copy.
    cache_seqlens device int32 [B].  fp16 / bf16 with a contiguous head_dim and strides that are multiples of 8 elements.  Asynchronous
    on torch's current stream; cache_seqlens and block_table are never read back."""
    return _kvcache_forward(_lib.umfa_kvcache_attention_forward_stream, (), q, k_cache, v_cache, cache_seqlens, block_table, k_new, v_new,
                            scale, causal, num_splits, out_dtype)


def _descale_arg(d, B, Hkv, name):
    """(pointer, (batch, head) element strides) of a device fp32 descale that broadcasts to [B, H_kv]; nothing is read or copied"""
    if not isinstance(d, torch.Tensor) or d.dtype != torch.float32 or not d.is_cuda or d.dim() > 2:
        raise ValueError(f"kvcache_attention_fp8_forward: {name} must be a device fp32 tensor that broadcasts to [batch, num_kv_heads]")
    try:
        e = d.expand(B, Hkv)
    except RuntimeError:
        raise ValueError(f"kvcache_attention_fp8_forward: {name} {tuple(d.shape)} does not broadcast to [{B}, {Hkv}]") from None
    return ctypes.c_void_p(e.data_ptr()), _i64(e.stride())


def kvcache_attention_fp8_forward(q, k_cache, v_cache, cache_seqlens, k_descale, v_descale, block_table=None, k_new=None, v_new=None, *,
                                  scale: float, causal: bool = False, num_splits: int = 0, out_dtype=None):
    """kvcache_attention_forward over an fp8 cache (umfa_kvcache_attention_fp8_forward_stream): k_cache / v_cache torch.float8_e4m3fn in
    the same layouts, q / k_new / v_new fp16 or bf16.  k_descale / v_descale: device fp32, a scalar, [H_kv], [B, 1] or [B, H_kv]; a cache
    byte stands for e4m3fn(byte) * descale[b, h_kv], and k_new / v_new are stored as e4m3fn(clamp(x / descale, -448, 448)).  Cache strides
    multiples of 16 with a contiguous head_dim.  The descales are never read back."""
    if k_cache.dtype != torch.float8_e4m3fn or v_cache.dtype != torch.float8_e4m3fn:
        raise ValueError(f"kvcache_attention_fp8_forward: k_cache and v_cache must both be torch.float8_e4m3fn (got {k_cache.dtype}, {v_cache.dtype})")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"kvcache_attention_fp8_forward: q must be fp16 or bf16 (got {q.dtype})")
    B, Hkv = q.shape[0], k_cache.shape[2]
    extra = (*_descale_arg(k_descale, B, Hkv, "k_descale"), *_descale_arg(v_descale, B, Hkv, "v_descale"))
    return _kvcache_forward(_lib.umfa_kvcache_attention_fp8_forward_stream, extra, q, k_cache, v_cache, cache_seqlens, block_table, k_new,
                            v_new, scale, causal, num_splits, out_dtype)


def kvcache_attention_rope_forward(q, k_cache, v_cache, cache_seqlens, rotary_cos, rotary_sin, block_table=None, k_new=None, v_new=None, *,
                                   scale: float, causal: bool = False, num_splits: int = 0, rotary_interleaved: bool = False,
                                   k_descale=None, v_descale=None, out_dtype=None, out=None, lse=None):
    """kvcache_attention_forward (16-bit caches) or kvcache_attention_fp8_forward (float8_e4m3fn caches with k_descale / v_descale) with
    the rotary embedding of q and k_new fused into the append launch (umfa_kvcache_attention_rope_forward_stream): k_new is rotated at
    positions cache_seqlens[b] + t on its way into the cache, q at cache_seqlens[b] + i (causal) or cache_seqlens[b] (not) into a
    workspace image the attention reads; v_new is appended as it is.  rotary_cos / rotary_sin device [seqlen_ro, rotary_dim / 2], fp32
    or q's dtype, unit column stride, 16-byte aligned rows; rotary_dim a multiple of 16 in [16, D].  New tokens are required.  Bit for
    bit the plain call on rotated, rounded q and k_new.  Positions are never read back.  out / lse: optional dense buffers
    [B, Sq, H, D] / fp32 [B, H, Sq] to write into."""
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    if fp8 != (v_cache.dtype == torch.float8_e4m3fn) or q.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("kvcache_attention_rope_forward: q must be fp16 / bf16 and the caches both 16-bit or both float8_e4m3fn")
    if k_new is None or v_new is None or k_new.shape[1] == 0:
        raise ValueError("kvcache_attention_rope_forward: rotary needs new tokens (k_new / v_new)")
    if fp8:
        B, Hkv = q.shape[0], k_cache.shape[2]
        desc = (*_descale_arg(k_descale, B, Hkv, "k_descale"), *_descale_arg(v_descale, B, Hkv, "v_descale"))
    elif k_descale is not None or v_descale is not None:
        raise ValueError("kvcache_attention_rope_forward: k_descale / v_descale go with float8_e4m3fn caches only")
    else:
        desc = (None, None, None, None)
    extra = (bool(fp8), *desc, *_rope_args("kvcache_attention_rope_forward", q, rotary_cos, rotary_sin, rotary_interleaved))
    return _kvcache_forward(_lib.umfa_kvcache_attention_rope_forward_stream, extra, q, k_cache, v_cache, cache_seqlens, block_table, k_new,
                            v_new, scale, causal, num_splits, out_dtype, out, lse)


def kvcache_attention_window_forward(q, k_cache, v_cache, cache_seqlens, block_table=None, k_new=None, v_new=None, *, scale: float,
                                     causal: bool = False, window=(-1, -1), num_splits: int = 0, rotary_cos=None, rotary_sin=None,
                                     rotary_interleaved: bool = False, out_dtype=None, out=None, lse=None, cache_fp8: bool = False):
    """kvcache_attention_forward with a sliding window (umfa_kvcache_attention_window_forward_stream): window = (left, right),
    flash-attention's window_size -- with off = L_k - Sq, query token i sees keys i + off - left .. i + off + right of the L_k the plain
    call covers; -1 is unbounded, causal sets right = 0.  16-bit caches (cache_fp8 is the entry's flag and is refused).  With rotary_cos
    / rotary_sin the rotary embedding is fused into the append launch as in kvcache_attention_rope_forward (new tokens required).  The
    entry normalises the window; one that bounds nothing runs the unwindowed kernels, bit for bit."""
    left, right = (int(x) for x in window)
    if (rotary_cos is None) != (rotary_sin is None):
        raise ValueError("kvcache_attention_window_forward: rotary_cos and rotary_sin must be given together")
    if rotary_cos is not None:
        if k_new is None or v_new is None or k_new.shape[1] == 0:
            raise ValueError("kvcache_attention_window_forward: rotary needs new tokens (k_new / v_new)")
        rope = _rope_args("kvcache_attention_window_forward", q, rotary_cos, rotary_sin, rotary_interleaved)
    else:
        rope = (None, None, _PREC[q.dtype], 0, 0, 0, False)
    extra = (bool(cache_fp8), None, None, None, None, *rope, left, right)
    return _kvcache_forward(_lib.umfa_kvcache_attention_window_forward_stream, extra, q, k_cache, v_cache, cache_seqlens, block_table, k_new,
                            v_new, scale, causal, num_splits, out_dtype, out, lse)


def _varlen_kvcache_forward(name, entry, extra, q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, k_new, v_new, scale,
                            causal, num_splits, out_dtype, out=None, lse=None):
    """the call the packed KV-cache entries share; name: the public wrapper (for messages); extra: the arguments behind num_splits (the
    rotary entry's tail, the fp8 entry's descales and rotary tail); out / lse: the caller's buffers (_out_buffers)"""
    Tq, H, D = q.shape
    B = cu_seqlens_q.numel() - 1
    if cu_seqlens_q.dim() != 1 or B < 1 or cache_seqlens.shape != (B,) or cu_seqlens_q.stride(0) != 1 or (B > 1 and cache_seqlens.stride(0) != 1) \
            or (block_table is not None and (block_table.shape[0] != B or block_table.stride(1) != 1)):
        raise ValueError(f"{name}: cu_seqlens_q [B + 1], cache_seqlens [B] and the rows of block_table [B, .] must be contiguous")
    num_pages, page_size, Hkv = k_cache.shape[0], k_cache.shape[1], k_cache.shape[2]
    if block_table is not None:
        max_pages, bt_stride, bt = block_table.shape[1], block_table.stride(0), ctypes.c_void_p(block_table.data_ptr())
    else:
        max_pages, bt_stride, bt = 1, 0, None
    has_new = k_new is not None
    out, lse = _out_buffers(name, q, (Tq, H, D), (H, Tq), out_dtype, out, lse)
    stream = torch.cuda.current_stream(q.device).cuda_stream
    new = [None, None, None, None]
    if has_new:
        if k_new.shape != (Tq, Hkv, D) or v_new.shape != (Tq, Hkv, D):
            raise ValueError(f"{name}: k_new / v_new must be [T_q, H_kv, D] = {(Tq, Hkv, D)}")
        new = [ctypes.c_void_p(k_new.data_ptr()), _i64(k_new.stride()[:2]), ctypes.c_void_p(v_new.data_ptr()), _i64(v_new.stride()[:2])]
    _check_error(entry(
        context(), ctypes.c_void_p(stream), ctypes.c_void_p(q.data_ptr()), _i64(q.stride()[:2]), ctypes.c_void_p(k_cache.data_ptr()),
        _i64(k_cache.stride()[:3]), ctypes.c_void_p(v_cache.data_ptr()), _i64(v_cache.stride()[:3]), *new, bt, int(bt_stride),
        ctypes.c_void_p(cache_seqlens.data_ptr()), Tq, B, int(max_seqlen_q), ctypes.c_void_p(cu_seqlens_q.data_ptr()), bool(has_new), H, Hkv, D,
        int(page_size), int(num_pages), int(max_pages), float(scale), bool(causal), _PREC[q.dtype], ctypes.c_void_p(out.data_ptr()),
        _PREC[out.dtype], ctypes.c_void_p(lse.data_ptr()), int(num_splits), *extra))
    return out, lse


def varlen_kvcache_attention_forward(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q: int, cache_seqlens, block_table=None, k_new=None,
                                     v_new=None, *, scale: float, causal: bool = False, num_splits: int = 0, out_dtype=None):
    """O [T_q, H, D] and LSE [H, T_q] (fp32, natural log) of packed variable-length queries over a paged or static KV cache
    (umfa_varlen_kvcache_attention_forward_stream), appending k_new / v_new [T_q, H_kv, D] (packed by the same cu_seqlens_q) into the
    cache in place first.  q [T_q, H, D] with a contiguous head_dim and token / head strides that are multiples of 8 elements;
    cu_seqlens_q device int32 [B + 1]; max_seqlen_q a host int; the caches, block_table and cache_seqlens as kvcache_attention_forward
    takes them.  Asynchronous on torch's current stream; cu_seqlens_q, cache_seqlens and block_table are never read back."""
    return _varlen_kvcache_forward("varlen_kvcache_attention_forward", _lib.umfa_varlen_kvcache_attention_forward_stream, (), q, k_cache,
                                   v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, k_new, v_new, scale, causal, num_splits,
                                   out_dtype)


def varlen_kvcache_attention_rope_forward(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q: int, cache_seqlens, rotary_cos, rotary_sin,
                                          block_table=None, k_new=None, v_new=None, *, scale: float, causal: bool = False,
                                          num_splits: int = 0, rotary_interleaved: bool = False, out_dtype=None, out=None, lse=None):
    """varlen_kvcache_attention_forward with the rotary embedding of q and k_new fused into the packed append launch
    (umfa_varlen_kvcache_attention_rope_forward_stream): packed row t of sequence b is rotated at cache_seqlens[b] + (t - cu[b]) (the
    queries of a non-causal call all at cache_seqlens[b]).  Tables and rules as kvcache_attention_rope_forward; 16-bit caches.  out / lse:
    optional dense buffers [T_q, H, D] / fp32 [H, T_q] to write into (rows no sequence covers stay as they were)."""
    name = "varlen_kvcache_attention_rope_forward"
    if k_new is None or v_new is None:
        raise ValueError(f"{name}: rotary needs new tokens (k_new / v_new)")
    rope = _rope_args(name, q, rotary_cos, rotary_sin, rotary_interleaved)
    return _varlen_kvcache_forward(name, _lib.umfa_varlen_kvcache_attention_rope_forward_stream, rope, q, k_cache, v_cache, cu_seqlens_q,
                                   max_seqlen_q, cache_seqlens, block_table, k_new, v_new, scale, causal, num_splits, out_dtype, out, lse)


def varlen_kvcache_attention_fp8_forward(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q: int, cache_seqlens, k_descale, v_descale,
                                         block_table=None, k_new=None, v_new=None, *, scale: float, causal: bool = False, num_splits: int = 0,
                                         rotary_cos=None, rotary_sin=None, rotary_interleaved: bool = False, out_dtype=None, out=None,
                                         lse=None):
    """varlen_kvcache_attention_forward over an fp8 cache (umfa_varlen_kvcache_attention_fp8_forward_stream): k_cache / v_cache
    torch.float8_e4m3fn in the same layouts (strides multiples of 16 bytes), q / k_new / v_new fp16 or bf16 and packed by cu_seqlens_q.
    k_descale / v_descale: device fp32, a scalar, [H_kv], [B, 1] or [B, H_kv] with B the sequences; a cache byte stands for
    e4m3fn(byte) * descale[b, h_kv], and packed row t of sequence b is stored as e4m3fn(clamp(x / descale[b, h_kv], -448, 448)).  With
    rotary_cos / rotary_sin (new tokens required) the rotary embedding is fused into the quantising append launch as in
    varlen_kvcache_attention_rope_forward: the rotated key is rounded to q's dtype, then quantised.  The descales are never read back.
    out / lse: optional dense buffers [T_q, H, D] / fp32 [H, T_q] to write into (rows no sequence covers stay as they were)."""
    name = "varlen_kvcache_attention_fp8_forward"
    if k_cache.dtype != torch.float8_e4m3fn or v_cache.dtype != torch.float8_e4m3fn:
        raise ValueError(f"{name}: k_cache and v_cache must both be torch.float8_e4m3fn (got {k_cache.dtype}, {v_cache.dtype})")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"{name}: q must be fp16 or bf16 (got {q.dtype})")
    if (rotary_cos is None) != (rotary_sin is None):
        raise ValueError(f"{name}: rotary_cos and rotary_sin must be given together")
    if rotary_cos is not None:
        if k_new is None or v_new is None:
            raise ValueError(f"{name}: rotary needs new tokens (k_new / v_new)")
        rope = _rope_args(name, q, rotary_cos, rotary_sin, rotary_interleaved)
    else:
        rope = (None, None, _PREC[q.dtype], 0, 0, 0, False)
    B, Hkv = cu_seqlens_q.numel() - 1, k_cache.shape[2]
    extra = (*_descale_arg(k_descale, B, Hkv, "k_descale"), *_descale_arg(v_descale, B, Hkv, "v_descale"), *rope)
    return _varlen_kvcache_forward(name, _lib.umfa_varlen_kvcache_attention_fp8_forward_stream, extra, q, k_cache, v_cache, cu_seqlens_q,
                                   max_seqlen_q, cache_seqlens, block_table, k_new, v_new, scale, causal, num_splits, out_dtype, out, lse)


def varlen_kvcache_attention_window_forward(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q: int, cache_seqlens, block_table=None, k_new=None,
                                            v_new=None, *, scale: float, causal: bool = False, window=(-1, -1), num_splits: int = 0,
                                            rotary_cos=None, rotary_sin=None, rotary_interleaved: bool = False, out_dtype=None, out=None,
                                            lse=None):
    """varlen_kvcache_attention_forward with a sliding window (umfa_varlen_kvcache_attention_window_forward_stream): window = (left,
    right), flash-attention's window_size -- with off_b = L_k,b - L_q,b, query token i of sequence b sees keys i + off_b - left ..
    i + off_b + right of the L_k,b the packed call covers; -1 is unbounded, causal sets right = 0.  16-bit caches.  With rotary_cos /
    rotary_sin the rotary embedding is fused into the packed append launch as in varlen_kvcache_attention_rope_forward (new tokens
    required).  The entry normalises the window; one that bounds nothing runs the unwindowed packed kernels, bit for bit.  out / lse:
    optional dense buffers [T_q, H, D] / fp32 [H, T_q] to write into (rows no sequence covers stay as they were)."""
    name = "varlen_kvcache_attention_window_forward"
    left, right = (int(x) for x in window)
    if (rotary_cos is None) != (rotary_sin is None):
        raise ValueError(f"{name}: rotary_cos and rotary_sin must be given together")
    if rotary_cos is not None:
        if k_new is None or v_new is None:
            raise ValueError(f"{name}: rotary needs new tokens (k_new / v_new)")
        rope = _rope_args(name, q, rotary_cos, rotary_sin, rotary_interleaved)
    else:
        rope = (None, None, _PREC[q.dtype], 0, 0, 0, False)
    return _varlen_kvcache_forward(name, _lib.umfa_varlen_kvcache_attention_window_forward_stream, (*rope, left, right), q, k_cache, v_cache,
                                   cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, k_new, v_new, scale, causal, num_splits, out_dtype,
                                   out, lse)


def varlen_kvcache_item_counts(device=None):
    """(decode-form items, 128-row items) the last varlen_kvcache_attention_forward (16-bit or fp8) on torch's current stream ran, counted by the
    kernel (umfa_varlen_kvcache_item_counts).  Debug: synchronises the stream."""
    stream = torch.cuda.current_stream(device).cuda_stream
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    _check_error(_lib.umfa_varlen_kvcache_item_counts(context(), ctypes.c_void_p(stream), ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value
