"""Packed variable-length queries over a paged or static KV cache, on the 16-bit MFMA kernels: the `umfa::varlen_kvcache_forward`
custom op (and its appending form `umfa::varlen_kvcache_forward_append`, which declares the in-place write of k_cache / v_cache so that
torch.compile orders it), both with fake implementations, and `varlen_kvcache_attention`, the call an inference server with
continuous batching and chunked prefill makes (flash-attention's flash_attn_varlen_func(..., block_table=...)).

Layout: q [T_q, H, D], packed; cu_seqlens_q device int32 [B + 1] (sequence b owns rows cu[b] .. cu[b+1] - 1); max_seqlen_q a host int.
k_cache / v_cache, block_table and cache_seqlens as `kvcache_attention` takes them (paged [num_pages, page_size, H_kv, D] with
block_table int32 [B, max_pages_per_seq], or static [B, S_max, H_kv, D] with block_table None).  k / v [T_q, H_kv, D], packed by the
same cu_seqlens_q, are written into the cache at cache_seqlens[b] .. before the attention, which then covers cache_seqlens[b] + L_q,b
keys; cache_seqlens itself is not advanced.  Causal is bottom-right aligned per sequence.  One launch serves prefill chunks (128-row work
items) and decode / speculative sequences (the decode form) together; work follows the rows that exist.  cu_seqlens_q, cache_seqlens and
the table stay on the device: no call synchronises, and a captured graph follows their contents on replay.  Lengths, cu values and table
entries outside their ranges are clamped / masked on the device.

Rotary embedding: with rotary_cos / rotary_sin the packed append launch also rotates k on its way into the cache
and q into a workspace image, at positions read from cache_seqlens and cu_seqlens_q on the device
(`umfa::varlen_kvcache_rope_forward_append`); such a call launches as many kernels as the same call without rotary.

fp8 caches: k_cache / v_cache may both be torch.float8_e4m3fn when BOTH k_descale and v_descale are given -- a
float, or a device fp32 tensor that broadcasts to [B, H_kv] with B the sequences: a cache byte stands for e4m3fn(byte) * descale[b, h_kv],
the packed k / v are quantised on the way in, q and O stay 16-bit.  The `umfa::varlen_kvcache_fp8_forward` /
`umfa::varlen_kvcache_fp8_forward_append` / `umfa::varlen_kvcache_fp8_rope_forward_append` ops serve them; the descales stay on the
device like the lengths.  fp8 caches with a descale missing, and descales with a 16-bit cache, raise ValueError.

Scope: fp16 / bf16 device tensors (fp8 caches as above), head_dim 64 / 128, forward only (a backward through these ops raises).  Anything else raises
ValueError: there is no fall-back.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from .kvcache import KVCACHE_HEAD_DIMS, _DTYPES, _check_rotary, _descale, _strides_ok


def _packed_view(t: torch.Tensor) -> torch.Tensor:
    """t itself when the kernels can read it (contiguous head_dim, token / head strides multiples of 8, 16-byte aligned), else a copy"""
    return t if _strides_ok(t) else t.contiguous()


@torch.library.custom_op("umfa::varlen_kvcache_forward", mutates_args=(), device_types="cuda")
def varlen_kvcache_forward(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cu_seqlens_q: torch.Tensor, max_seqlen_q: int,
                           cache_seqlens: torch.Tensor, block_table: Optional[torch.Tensor], causal: bool, scale: float,
                           num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """O [T_q, H, D] (q's dtype) and the fp32 log-sum-exp [H, T_q] (umfa_varlen_kvcache_attention_forward_stream)."""
    return ops.varlen_kvcache_attention_forward(_packed_view(q), k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q), cache_seqlens, block_table,
                                                scale=float(scale), causal=bool(causal), num_splits=int(num_splits))


@varlen_kvcache_forward.register_fake
def _(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, causal, scale, num_splits):
    Tq, H, D = q.shape
    return q.new_empty((Tq, H, D)), q.new_empty((H, Tq), dtype=torch.float32)


@torch.library.custom_op("umfa::varlen_kvcache_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def varlen_kvcache_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                  cu_seqlens_q: torch.Tensor, max_seqlen_q: int, cache_seqlens: torch.Tensor,
                                  block_table: Optional[torch.Tensor], causal: bool, scale: float,
                                  num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """varlen_kvcache_forward after writing k / v [T_q, H_kv, D] into k_cache / v_cache in place at cache_seqlens[b] .."""
    return ops.varlen_kvcache_attention_forward(_packed_view(q), k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q), cache_seqlens, block_table,
                                                _packed_view(k), _packed_view(v), scale=float(scale), causal=bool(causal),
                                                num_splits=int(num_splits))


@varlen_kvcache_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, causal, scale, num_splits):
    Tq, H, D = q.shape
    return q.new_empty((Tq, H, D)), q.new_empty((H, Tq), dtype=torch.float32)


@torch.library.custom_op("umfa::varlen_kvcache_rope_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def varlen_kvcache_rope_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                       cu_seqlens_q: torch.Tensor, max_seqlen_q: int, cache_seqlens: torch.Tensor, rotary_cos: torch.Tensor,
                                       rotary_sin: torch.Tensor, rotary_interleaved: bool, block_table: Optional[torch.Tensor], causal: bool,
                                       scale: float, num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """varlen_kvcache_forward_append with the rotary embedding fused into the packed append launch
    (umfa_varlen_kvcache_attention_rope_forward_stream): row t of sequence b is rotated at cache_seqlens[b] + (t - cu[b])."""
    return ops.varlen_kvcache_attention_rope_forward(_packed_view(q), k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q), cache_seqlens,
                                                     rotary_cos, rotary_sin, block_table, _packed_view(k), _packed_view(v), scale=float(scale),
                                                     causal=bool(causal), num_splits=int(num_splits),
                                                     rotary_interleaved=bool(rotary_interleaved))


@varlen_kvcache_rope_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cu_seqlens_q, max_seqlen_q, cache_seqlens, rotary_cos, rotary_sin, rotary_interleaved, block_table, causal,
      scale, num_splits):
    Tq, H, D = q.shape
    return q.new_empty((Tq, H, D)), q.new_empty((H, Tq), dtype=torch.float32)


def _fp8(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.float8_e4m3fn)


@torch.library.custom_op("umfa::varlen_kvcache_fp8_forward", mutates_args=(), device_types="cuda")
def varlen_kvcache_fp8_forward(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cu_seqlens_q: torch.Tensor, max_seqlen_q: int,
                               cache_seqlens: torch.Tensor, k_descale: torch.Tensor, v_descale: torch.Tensor,
                               block_table: Optional[torch.Tensor], causal: bool, scale: float,
                               num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """varlen_kvcache_forward over float8_e4m3fn caches with device fp32 descales (umfa_varlen_kvcache_attention_fp8_forward_stream).
    k_cache / v_cache are the caches' BYTES, their .view(torch.uint8), for kvcache_fp8_forward's reason: torch's own op checks have no
    float8 kernels to run on."""
    return ops.varlen_kvcache_attention_fp8_forward(_packed_view(q), _fp8(k_cache), _fp8(v_cache), cu_seqlens_q, int(max_seqlen_q),
                                                    cache_seqlens, k_descale, v_descale, block_table, scale=float(scale), causal=bool(causal),
                                                    num_splits=int(num_splits))


@varlen_kvcache_fp8_forward.register_fake
def _(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, k_descale, v_descale, block_table, causal, scale, num_splits):
    Tq, H, D = q.shape
    return q.new_empty((Tq, H, D)), q.new_empty((H, Tq), dtype=torch.float32)


@torch.library.custom_op("umfa::varlen_kvcache_fp8_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def varlen_kvcache_fp8_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                      cu_seqlens_q: torch.Tensor, max_seqlen_q: int, cache_seqlens: torch.Tensor, k_descale: torch.Tensor,
                                      v_descale: torch.Tensor, block_table: Optional[torch.Tensor], causal: bool, scale: float,
                                      num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """varlen_kvcache_fp8_forward after quantising the packed k / v [T_q, H_kv, D] (q's dtype) into k_cache / v_cache (uint8 views,
    written in place) at cache_seqlens[b] .."""
    return ops.varlen_kvcache_attention_fp8_forward(_packed_view(q), _fp8(k_cache), _fp8(v_cache), cu_seqlens_q, int(max_seqlen_q),
                                                    cache_seqlens, k_descale, v_descale, block_table, _packed_view(k), _packed_view(v),
                                                    scale=float(scale), causal=bool(causal), num_splits=int(num_splits))


@varlen_kvcache_fp8_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cu_seqlens_q, max_seqlen_q, cache_seqlens, k_descale, v_descale, block_table, causal, scale, num_splits):
    Tq, H, D = q.shape
    return q.new_empty((Tq, H, D)), q.new_empty((H, Tq), dtype=torch.float32)


@torch.library.custom_op("umfa::varlen_kvcache_fp8_rope_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def varlen_kvcache_fp8_rope_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                           cu_seqlens_q: torch.Tensor, max_seqlen_q: int, cache_seqlens: torch.Tensor,
                                           k_descale: torch.Tensor, v_descale: torch.Tensor, rotary_cos: torch.Tensor,
                                           rotary_sin: torch.Tensor, rotary_interleaved: bool, block_table: Optional[torch.Tensor],
                                           causal: bool, scale: float, num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """varlen_kvcache_fp8_forward_append (k_cache / v_cache the caches' uint8 views) with the rotary embedding fused into the packed
    quantising append launch: row t of sequence b is rotated at cache_seqlens[b] + (t - cu[b]), the rotated k is rounded to q's dtype,
    then quantised."""
    return ops.varlen_kvcache_attention_fp8_forward(_packed_view(q), _fp8(k_cache), _fp8(v_cache), cu_seqlens_q, int(max_seqlen_q),
                                                    cache_seqlens, k_descale, v_descale, block_table, _packed_view(k), _packed_view(v),
                                                    scale=float(scale), causal=bool(causal), num_splits=int(num_splits),
                                                    rotary_cos=rotary_cos, rotary_sin=rotary_sin, rotary_interleaved=bool(rotary_interleaved))


@varlen_kvcache_fp8_rope_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cu_seqlens_q, max_seqlen_q, cache_seqlens, k_descale, v_descale, rotary_cos, rotary_sin, rotary_interleaved,
      block_table, causal, scale, num_splits):
    Tq, H, D = q.shape
    return q.new_empty((Tq, H, D)), q.new_empty((H, Tq), dtype=torch.float32)


# flash_attn_varlen_func / flash_attn_with_kvcache arguments this entry accepts only at their defaults
_UNSUPPORTED = {"cache_batch_idx": None, "cache_leftpad": None, "window_size": (-1, -1),
                "softcap": 0.0, "alibi_slopes": None, "seqused_k": None, "dropout_p": 0.0}


def _check(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, k, v, fp8=False):
    def bad(msg):
        raise ValueError(f"varlen_kvcache_attention: {msg}")

    if not isinstance(q, torch.Tensor) or q.dim() != 3 or not q.is_cuda or q.dtype not in _DTYPES:
        bad(f"q must be a packed 3-D [T_q, H, D] fp16 / bf16 device tensor (got {getattr(q, 'shape', q)}, {getattr(q, 'dtype', None)})")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or not t.is_cuda or t.dtype not in ((torch.float8_e4m3fn,) if fp8 else _DTYPES):
            bad(f"{name} must be a 4-D fp16 / bf16 device tensor, or the caches both float8_e4m3fn with k_descale and v_descale both "
                f"given (got {getattr(t, 'shape', t)}, {getattr(t, 'dtype', None)})")
    if k_cache.dtype != v_cache.dtype or (not fp8 and k_cache.dtype != q.dtype) or k_cache.shape != v_cache.shape \
            or k_cache.device != q.device or v_cache.device != q.device:
        bad("k_cache and v_cache must match each other in shape, dtype and device, and q in dtype (unless they are float8_e4m3fn) and device")
    Tq, H, D = q.shape
    Hkv = k_cache.shape[2]
    if D not in KVCACHE_HEAD_DIMS or k_cache.shape[3] != D:
        bad(f"head_dim must be 64 or 128 and equal in q and the cache (got {D}, {k_cache.shape[3]})")
    if Hkv == 0 or H % Hkv:
        bad(f"num_heads ({H}) must be a multiple of the cache's num_kv_heads ({Hkv})")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if not _strides_ok(t) or t.stride(1) < D:
            bad(f"{name} needs a contiguous head_dim, page / token / head strides that are multiples of 16 bytes and a 16-byte aligned base")
    if not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2 \
            or cu_seqlens_q.device != q.device:
        bad("cu_seqlens_q must be a device int32 [batch + 1] tensor")
    if cu_seqlens_q.stride(0) != 1:
        bad(f"cu_seqlens_q must be contiguous (got stride {cu_seqlens_q.stride(0)})")
    B = cu_seqlens_q.numel() - 1
    if isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int) or max_seqlen_q < 0 or max_seqlen_q > Tq:
        bad(f"max_seqlen_q must be a host int in [0, T_q = {Tq}] (got {max_seqlen_q!r})")
    if block_table is not None:
        if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B \
                or block_table.device != q.device or block_table.stride(1) != 1 or (B > 1 and block_table.stride(0) < block_table.shape[1]):
            bad("block_table must be a device int32 [batch, max_pages_per_seq] tensor with unit column stride and rows that do not overlap")
        if k_cache.shape[1] % 16:
            bad(f"a paged cache's page_size must be a multiple of 16 (got {k_cache.shape[1]})")
    elif k_cache.shape[0] < B:
        bad(f"a static cache needs one row per sequence ({k_cache.shape[0]} rows for batch {B})")
    if (k is None) != (v is None):
        bad("k and v must be given together")
    if k is not None:
        for name, t in (("k", k), ("v", v)):
            if not isinstance(t, torch.Tensor) or t.shape != (Tq, Hkv, D) or t.dtype != q.dtype or t.device != q.device:
                bad(f"{name} must be [T_q, num_kv_heads, head_dim] = {(Tq, Hkv, D)} in q's dtype on q's device, packed by cu_seqlens_q "
                    f"(got {tuple(getattr(t, 'shape', ()))})")
    if not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dtype != torch.int32 or cache_seqlens.shape != (B,) \
            or cache_seqlens.device != q.device:
        bad("cache_seqlens must be a device int32 [batch] tensor")
    # the kernels read cache_seqlens[b] at element b: an expanded (stride 0) or strided view would hand every sequence a wrong length
    if B > 1 and cache_seqlens.stride(0) != 1:
        bad(f"cache_seqlens must be contiguous (got stride {cache_seqlens.stride(0)}): pass cache_seqlens.contiguous()")


def varlen_kvcache_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cu_seqlens_q: torch.Tensor, max_seqlen_q: int,
                             cache_seqlens: torch.Tensor, block_table: Optional[torch.Tensor] = None, k: Optional[torch.Tensor] = None,
                             v: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None, causal: bool = False,
                             num_splits: int = 0, return_softmax_lse: bool = False, rotary_cos: Optional[torch.Tensor] = None,
                             rotary_sin: Optional[torch.Tensor] = None, rotary_interleaved: bool = False, k_descale=None, v_descale=None,
                             **unsupported):
    """softmax(q k^T scale [bottom-right causal]) v for packed queries q [T_q, H, D] (sequence b = rows cu_seqlens_q[b] ..
    cu_seqlens_q[b+1] - 1) over each sequence's cached keys, after appending the packed k / v [T_q, H_kv, D] into the cache in place.
    Returns O [T_q, H, D] in q's dtype, or (O, LSE [H, T_q] fp32) with return_softmax_lse.  Rows no sequence covers are left unwritten.
    rotary_cos / rotary_sin: device tables [seqlen_ro, rotary_dim / 2], fp32 or q's dtype, rotary_dim a
    multiple of 16 in [16, D]; with them row t of sequence b is rotated at cache_seqlens[b] + (t - cu_seqlens_q[b]) -- k on its way into
    the cache, q into a workspace image (every query row of a non-causal call at cache_seqlens[b]) -- inside the append launch, bit for
    bit the call on rotated q / k.  rotary_interleaved: pairs (2i, 2i + 1) instead of (i, i + rotary_dim / 2); ignored without tables.
    k / v are required; a position at or past seqlen_ro takes the last table row.
    k_cache / v_cache both torch.float8_e4m3fn: k_descale and v_descale must BOTH be given -- a float, or a device
    fp32 tensor that broadcasts to [B, H_kv] (B sequences) -- and give the value of a byte, e4m3fn(byte) * descale[b, h_kv]; k / v are
    quantised into the cache (with rotary: rotated, rounded to q's dtype, then quantised).  With a 16-bit cache they must stay None.
    cache_batch_idx / cache_leftpad / window_size / softcap / alibi_slopes / seqused_k / dropout_p are accepted at their defaults only.
    Raises ValueError outside the kernels' scope (see the module docstring)."""
    for name, val in unsupported.items():
        if name not in _UNSUPPORTED:
            raise TypeError(f"varlen_kvcache_attention() got an unexpected keyword argument '{name}'")
        default = _UNSUPPORTED[name]
        same = val is None if default is None else (tuple(val) == default if name == "window_size" else val == default)
        if not same:
            raise ValueError(f"varlen_kvcache_attention: {name} is not supported (only its default, {default!r}, is accepted)")
    fp8 = any(isinstance(t, torch.Tensor) and t.dtype == torch.float8_e4m3fn for t in (k_cache, v_cache))
    if not fp8 and (k_descale is not None or v_descale is not None):
        raise ValueError("varlen_kvcache_attention: k_descale / v_descale go with float8_e4m3fn caches only")
    # (fp8 caches are served only when both descales are given: with one missing the caches are refused like any other dtype)
    fp8 = fp8 and k_descale is not None and v_descale is not None
    _check(q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, k, v, fp8)
    sm = float(softmax_scale) if softmax_scale is not None else float(q.shape[-1]) ** -0.5
    if not sm > 0.0:
        raise ValueError(f"varlen_kvcache_attention: softmax_scale must be positive (got {softmax_scale})")
    rotary = _check_rotary("varlen_kvcache_attention", q, k, k is not None, rotary_cos, rotary_sin)
    if fp8:
        B, Hkv = cu_seqlens_q.numel() - 1, k_cache.shape[2]
        kd, vd = (_descale(d, q, Hkv, n, B, "varlen_kvcache_attention") for d, n in ((k_descale, "k_descale"), (v_descale, "v_descale")))
        k_cache, v_cache = k_cache.view(torch.uint8), v_cache.view(torch.uint8)  # (the ops take the bytes: varlen_kvcache_fp8_forward)
        if rotary:
            out, lse = torch.ops.umfa.varlen_kvcache_fp8_rope_forward_append(q, k_cache, v_cache, k, v, cu_seqlens_q, int(max_seqlen_q),
                                                                             cache_seqlens, kd, vd, rotary_cos, rotary_sin,
                                                                             bool(rotary_interleaved), block_table, bool(causal), sm,
                                                                             int(num_splits))
        elif k is not None:
            out, lse = torch.ops.umfa.varlen_kvcache_fp8_forward_append(q, k_cache, v_cache, k, v, cu_seqlens_q, int(max_seqlen_q),
                                                                        cache_seqlens, kd, vd, block_table, bool(causal), sm, int(num_splits))
        else:
            out, lse = torch.ops.umfa.varlen_kvcache_fp8_forward(q, k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q), cache_seqlens, kd, vd,
                                                                 block_table, bool(causal), sm, int(num_splits))
        return (out, lse) if return_softmax_lse else out
    if rotary:
        out, lse = torch.ops.umfa.varlen_kvcache_rope_forward_append(q, k_cache, v_cache, k, v, cu_seqlens_q, int(max_seqlen_q), cache_seqlens,
                                                                     rotary_cos, rotary_sin, bool(rotary_interleaved), block_table,
                                                                     bool(causal), sm, int(num_splits))
    elif k is not None:
        out, lse = torch.ops.umfa.varlen_kvcache_forward_append(q, k_cache, v_cache, k, v, cu_seqlens_q, int(max_seqlen_q), cache_seqlens,
                                                                block_table, bool(causal), sm, int(num_splits))
    else:
        out, lse = torch.ops.umfa.varlen_kvcache_forward(q, k_cache, v_cache, cu_seqlens_q, int(max_seqlen_q), cache_seqlens, block_table,
                                                         bool(causal), sm, int(num_splits))
    return (out, lse) if return_softmax_lse else out
