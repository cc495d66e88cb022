"""Attention over a paged or static KV cache for inference, on the 16-bit MFMA kernels: the `umfa::kvcache_forward` custom op (and its
appending form `umfa::kvcache_forward_append`, which declares the in-place write of k_cache / v_cache so that torch.compile orders it),
both with fake implementations, and `kvcache_attention`, with the arguments of flash-attention's flash_attn_with_kvcache.

Layout: q [B, Sq, H, D].  Paged cache: k_cache / v_cache [num_pages, page_size, H_kv, D] with block_table int32 [B, max_pages_per_seq]
(page_size a multiple of 16).  Static cache (block_table None): k_cache / v_cache [B, S_max, H_kv, D], or HF's [B, H_kv, S_max, D] passed
as its .transpose(1, 2) view -- no copy either way.  cache_seqlens int32 [B] stays on the device: no call synchronises, and a captured
graph follows its contents and the block table's on replay.  k / v [B, S_new, H_kv, D] are written into the cache at cache_seqlens[b] ..
before the attention, which then covers cache_seqlens[b] + S_new keys; cache_seqlens itself is not advanced.  Causal is bottom-right
aligned per sequence.  Lengths and table entries outside the cache are clamped / masked on the device.

fp8 caches: k_cache / v_cache may both be torch.float8_e4m3fn (OCP e4m3fn, gfx950's fp8) with k_descale /
v_descale, device fp32 tensors that broadcast to [B, H_kv] (a Python float becomes a one-element device tensor): a cache byte stands for
e4m3fn(byte) * descale[b, h_kv], k / v are quantised on the way in, q and O stay 16-bit.  The `umfa::kvcache_fp8_forward` /
`umfa::kvcache_fp8_forward_append` ops serve them.  The descales stay on the device like the lengths.

Rotary embedding: with rotary_cos / rotary_sin the append launch also rotates k on its way into the cache and q
into a workspace image, at positions read from cache_seqlens on the device; the `umfa::kvcache_rope_forward_append` /
`umfa::kvcache_fp8_rope_forward_append` ops serve those calls, which launch as many kernels as the same call without rotary.

Scope: fp16 / bf16 device tensors (fp8 caches as above), head_dim 64 / 128, forward only (a backward through these ops raises).  Anything
else raises ValueError: there is no fall-back.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops

KVCACHE_HEAD_DIMS = (64, 128)
_DTYPES = (torch.float16, torch.bfloat16)


def _strides_ok(t: torch.Tensor) -> bool:
    s = t.stride()
    # (being traced by torch.compile there is no address to look at: the op checks it when it runs)
    aligned = torch.compiler.is_compiling() or t.data_ptr() % 16 == 0
    gran = 16 // t.element_size()  # 16-byte granules: 8 elements of a 16-bit tensor, 16 of an fp8 one
    return s[-1] == 1 and all(x % gran == 0 and x >= 0 for x in s[:-1]) and aligned


def _kernel_view(t: torch.Tensor) -> torch.Tensor:
    """t itself when the kernels can read it (contiguous head_dim, other strides multiples of 8, 16-byte aligned), else a copy"""
    return t if _strides_ok(t) and t.stride(1) >= t.shape[-1] else t.contiguous()


@torch.library.custom_op("umfa::kvcache_forward", mutates_args=(), device_types="cuda")
def kvcache_forward(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_seqlens: torch.Tensor,
                    block_table: Optional[torch.Tensor], causal: bool, scale: float, num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """O [B, Sq, H, D] (q's dtype) and the fp32 log-sum-exp [B, H, Sq] (umfa_kvcache_attention_forward_stream)."""
    return ops.kvcache_attention_forward(_kernel_view(q), k_cache, v_cache, cache_seqlens, block_table, scale=float(scale),
                                         causal=bool(causal), num_splits=int(num_splits))


@kvcache_forward.register_fake
def _(q, k_cache, v_cache, cache_seqlens, block_table, causal, scale, num_splits):
    B, Sq, H, D = q.shape
    return q.new_empty((B, Sq, H, D)), q.new_empty((B, H, Sq), dtype=torch.float32)


@torch.library.custom_op("umfa::kvcache_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def kvcache_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                           cache_seqlens: torch.Tensor, block_table: Optional[torch.Tensor], causal: bool, scale: float,
                           num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """kvcache_forward after writing k / v [B, S_new, H_kv, D] into k_cache / v_cache in place at cache_seqlens[b] .."""
    return ops.kvcache_attention_forward(_kernel_view(q), k_cache, v_cache, cache_seqlens, block_table, _kernel_view(k), _kernel_view(v),
                                         scale=float(scale), causal=bool(causal), num_splits=int(num_splits))


@kvcache_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cache_seqlens, block_table, causal, scale, num_splits):
    B, Sq, H, D = q.shape
    return q.new_empty((B, Sq, H, D)), q.new_empty((B, H, Sq), dtype=torch.float32)


@torch.library.custom_op("umfa::kvcache_fp8_forward", mutates_args=(), device_types="cuda")
def kvcache_fp8_forward(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, cache_seqlens: torch.Tensor,
                        k_descale: torch.Tensor, v_descale: torch.Tensor, block_table: Optional[torch.Tensor], causal: bool, scale: float,
                        num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """kvcache_forward over float8_e4m3fn caches with device fp32 descales (umfa_kvcache_attention_fp8_forward_stream).  k_cache /
    v_cache are the caches' BYTES, their .view(torch.uint8): torch's own op checks (opcheck's schema test, which compares arguments
    before and after a call) have no float8 kernels to run on."""
    return ops.kvcache_attention_fp8_forward(_kernel_view(q), k_cache.view(torch.float8_e4m3fn), v_cache.view(torch.float8_e4m3fn),
                                             cache_seqlens, k_descale, v_descale, block_table, scale=float(scale), causal=bool(causal), num_splits=int(num_splits))


@kvcache_fp8_forward.register_fake
def _(q, k_cache, v_cache, cache_seqlens, k_descale, v_descale, block_table, causal, scale, num_splits):
    B, Sq, H, D = q.shape
    return q.new_empty((B, Sq, H, D)), q.new_empty((B, H, Sq), dtype=torch.float32)


@torch.library.custom_op("umfa::kvcache_fp8_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def kvcache_fp8_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                               cache_seqlens: torch.Tensor, k_descale: torch.Tensor, v_descale: torch.Tensor,
                               block_table: Optional[torch.Tensor], causal: bool, scale: float,
                               num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """kvcache_fp8_forward after quantising k / v [B, S_new, H_kv, D] (q's dtype) into k_cache / v_cache (uint8 views, written in place)
    at cache_seqlens[b] .."""
    return ops.kvcache_attention_fp8_forward(_kernel_view(q), k_cache.view(torch.float8_e4m3fn), v_cache.view(torch.float8_e4m3fn),
                                             cache_seqlens, k_descale, v_descale, block_table, _kernel_view(k), _kernel_view(v), scale=float(scale), causal=bool(causal),
                                             num_splits=int(num_splits))


@kvcache_fp8_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cache_seqlens, k_descale, v_descale, block_table, causal, scale, num_splits):
    B, Sq, H, D = q.shape
    return q.new_empty((B, Sq, H, D)), q.new_empty((B, H, Sq), dtype=torch.float32)


@torch.library.custom_op("umfa::kvcache_rope_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def kvcache_rope_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                cache_seqlens: torch.Tensor, rotary_cos: torch.Tensor, rotary_sin: torch.Tensor, rotary_interleaved: bool,
                                block_table: Optional[torch.Tensor], causal: bool, scale: float,
                                num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """kvcache_forward_append with the rotary embedding fused into the append launch (umfa_kvcache_attention_rope_forward_stream): k is
    rotated at cache_seqlens[b] + t on its way into k_cache, q at cache_seqlens[b] + i (causal) or cache_seqlens[b] (not)."""
    return ops.kvcache_attention_rope_forward(_kernel_view(q), k_cache, v_cache, cache_seqlens, rotary_cos, rotary_sin, block_table,
                                              _kernel_view(k), _kernel_view(v), scale=float(scale), causal=bool(causal),
                                              num_splits=int(num_splits), rotary_interleaved=bool(rotary_interleaved))


@kvcache_rope_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cache_seqlens, rotary_cos, rotary_sin, rotary_interleaved, block_table, causal, scale, num_splits):
    B, Sq, H, D = q.shape
    return q.new_empty((B, Sq, H, D)), q.new_empty((B, H, Sq), dtype=torch.float32)


@torch.library.custom_op("umfa::kvcache_fp8_rope_forward_append", mutates_args=("k_cache", "v_cache"), device_types="cuda")
def kvcache_fp8_rope_forward_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                                    cache_seqlens: torch.Tensor, k_descale: torch.Tensor, v_descale: torch.Tensor, rotary_cos: torch.Tensor,
                                    rotary_sin: torch.Tensor, rotary_interleaved: bool, block_table: Optional[torch.Tensor], causal: bool,
                                    scale: float, num_splits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """kvcache_fp8_forward_append (k_cache / v_cache the caches' uint8 views) with the rotary embedding fused into the quantising append
    launch: the rotated k is rounded to q's dtype, then quantised."""
    return ops.kvcache_attention_rope_forward(_kernel_view(q), k_cache.view(torch.float8_e4m3fn), v_cache.view(torch.float8_e4m3fn),
                                              cache_seqlens, rotary_cos, rotary_sin, block_table, _kernel_view(k), _kernel_view(v),
                                              scale=float(scale), causal=bool(causal), num_splits=int(num_splits),
                                              rotary_interleaved=bool(rotary_interleaved), k_descale=k_descale, v_descale=v_descale)


@kvcache_fp8_rope_forward_append.register_fake
def _(q, k_cache, v_cache, k, v, cache_seqlens, k_descale, v_descale, rotary_cos, rotary_sin, rotary_interleaved, block_table, causal, scale,
      num_splits):
    B, Sq, H, D = q.shape
    return q.new_empty((B, Sq, H, D)), q.new_empty((B, H, Sq), dtype=torch.float32)


# flash_attn_with_kvcache arguments this entry accepts only at their defaults
_UNSUPPORTED = {"cache_batch_idx": None, "cache_leftpad": None, "window_size": (-1, -1),
                "softcap": 0.0, "alibi_slopes": None}


def _check(q, k_cache, v_cache, k, v, cache_seqlens, block_table, fp8=False, fn="kvcache_attention"):
    def bad(msg):
        raise ValueError(f"{fn}: {msg}")

    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        ok = (torch.float8_e4m3fn,) if fp8 and name != "q" else _DTYPES
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or not t.is_cuda or t.dtype not in ok:
            bad(f"{name} must be a 4-D fp16 / bf16 device tensor, or the caches both float8_e4m3fn (got {getattr(t, 'shape', t)}, "
                f"{getattr(t, 'dtype', None)})")
    if k_cache.dtype != v_cache.dtype or (not fp8 and k_cache.dtype != q.dtype) or k_cache.shape != v_cache.shape:
        bad("k_cache and v_cache must match each other in shape and dtype, and q in dtype unless they are float8_e4m3fn")
    B, Sq, H, D = q.shape
    Hkv = k_cache.shape[2]
    if D not in KVCACHE_HEAD_DIMS or k_cache.shape[3] != D:
        bad(f"head_dim must be 64 or 128 and equal in q and the cache (got {D}, {k_cache.shape[3]})")
    if Hkv == 0 or H % Hkv:
        bad(f"num_heads ({H}) must be a multiple of the cache's num_kv_heads ({Hkv})")
    for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if not _strides_ok(t) or t.stride(1) < D:
            bad(f"{name} needs a contiguous head_dim, page / token / head strides that are multiples of 16 bytes and a 16-byte aligned base")
    if block_table is not None:
        if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B or not block_table.is_cuda \
                or block_table.stride(1) != 1 or (B > 1 and block_table.stride(0) < block_table.shape[1]):
            bad("block_table must be a device int32 [batch, max_pages_per_seq] tensor with unit column stride and rows that do not overlap")
        if k_cache.shape[1] % 16:
            bad(f"a paged cache's page_size must be a multiple of 16 (got {k_cache.shape[1]})")
    elif k_cache.shape[0] < B:
        bad(f"a static cache needs one row per sequence ({k_cache.shape[0]} rows for batch {B})")
    if (k is None) != (v is None):
        bad("k and v must be given together")
    if k is not None:
        if k.dim() != 4 or k.shape != v.shape or k.shape[0] != B or k.shape[2] != Hkv or k.shape[3] != D or k.dtype != q.dtype \
                or v.dtype != q.dtype or not k.is_cuda or not v.is_cuda:
            bad(f"k / v must be [batch, S_new, num_kv_heads, head_dim] in q's dtype (got {tuple(k.shape)}, {tuple(v.shape)})")
    if cache_seqlens.dtype != torch.int32 or cache_seqlens.shape != (B,) or not cache_seqlens.is_cuda:
        bad("cache_seqlens must be an int, or a device int32 [batch] tensor")
    # the kernels read cache_seqlens[b] at element b: an expanded (stride 0) or strided view would hand every sequence a wrong length
    if B > 1 and cache_seqlens.stride(0) != 1:
        bad(f"cache_seqlens must be contiguous (got stride {cache_seqlens.stride(0)}): pass cache_seqlens.contiguous()")


def _check_rotary(fn, q, k, new_tokens, rotary_cos, rotary_sin):
    """the rotary tables of kvcache_attention / varlen_kvcache_attention: True when the call is a rotary one"""
    def bad(msg):
        raise ValueError(f"{fn}: {msg}")

    if rotary_cos is None and rotary_sin is None:
        return False
    if rotary_cos is None or rotary_sin is None:
        bad("rotary_cos and rotary_sin must be given together")
    for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or not isinstance(q, torch.Tensor) or t.device != q.device or not t.is_cuda:
            bad(f"{name} must be a 2-D [seqlen_ro, rotary_dim / 2] tensor on q's device (got {tuple(getattr(t, 'shape', ()))}, "
                f"{getattr(t, 'device', None)})")
    if rotary_cos.shape != rotary_sin.shape or rotary_cos.dtype != rotary_sin.dtype:
        bad(f"rotary_cos and rotary_sin must match in shape and dtype (got {tuple(rotary_cos.shape)} {rotary_cos.dtype}, "
            f"{tuple(rotary_sin.shape)} {rotary_sin.dtype})")
    if rotary_cos.dtype not in (torch.float32, q.dtype):
        bad(f"the rotary tables must be fp32 or q's dtype {q.dtype} (got {rotary_cos.dtype})")
    if not new_tokens:
        bad("rotary_cos / rotary_sin need new tokens k / v (flash-attention's rule): there is nothing to rotate into the cache")
    seqlen_ro, rotary_dim = rotary_cos.shape[0], 2 * rotary_cos.shape[1]
    if rotary_dim < 16 or rotary_dim > q.shape[-1] or rotary_dim % 16:
        bad(f"rotary_dim = 2 * rotary_cos.shape[1] must be a multiple of 16 in [16, head_dim = {q.shape[-1]}] (got {rotary_dim})")
    if seqlen_ro == 0:
        bad("the rotary tables hold no position (seqlen_ro = 0)")
    for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
        aligned = torch.compiler.is_compiling() or t.data_ptr() % 16 == 0
        if t.stride(1) != 1 or (t.stride(0) * t.element_size()) % 16 or t.stride(0) < t.shape[1] or not aligned:
            bad(f"{name} needs a unit column stride and 16-byte aligned rows (got strides {t.stride()}): pass {name}.contiguous()")
    if rotary_cos.stride() != rotary_sin.stride():
        bad("rotary_cos and rotary_sin must have equal strides")
    return True


def _descale(d, q, Hkv, name, B=None, fn="kvcache_attention"):
    """a descale argument as the device fp32 tensor the op takes: None = 1.0, a Python number becomes a one-element tensor (a fill on
    the device, no synchronisation), a tensor must be device fp32 and broadcast to [B, H_kv] (B: q's batch, or the packed call's
    sequence count)"""
    B = q.shape[0] if B is None else B
    if d is None or (isinstance(d, (int, float)) and not isinstance(d, bool)):
        return torch.full((1,), 1.0 if d is None else float(d), dtype=torch.float32, device=q.device)
    if not isinstance(d, torch.Tensor) or d.dtype != torch.float32 or d.device != q.device or d.dim() > 2:
        raise ValueError(f"{fn}: {name} must be a float or an fp32 tensor on q's device that broadcasts to [batch, num_kv_heads]")
    try:
        torch.broadcast_shapes(tuple(d.shape), (B, Hkv))
    except RuntimeError:
        raise ValueError(f"{fn}: {name} {tuple(d.shape)} does not broadcast to [{B}, {Hkv}]") from None
    if d.dim() == 2 and (d.shape[0] > B or d.shape[1] > Hkv):
        raise ValueError(f"{fn}: {name} {tuple(d.shape)} does not broadcast to [{B}, {Hkv}]")
    return d


def kvcache_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: Optional[torch.Tensor] = None,
                      v: Optional[torch.Tensor] = None, cache_seqlens=None, block_table: Optional[torch.Tensor] = None,
                      softmax_scale: Optional[float] = None, causal: bool = False, num_splits: int = 0,
                      return_softmax_lse: bool = False, k_descale=None, v_descale=None, rotary_cos: Optional[torch.Tensor] = None,
                      rotary_sin: Optional[torch.Tensor] = None, rotary_interleaved: bool = False, **unsupported):
    """flash_attn_with_kvcache on the MFMA kernels: softmax(q k^T scale [bottom-right causal]) v over each sequence's cached keys,
    after appending k / v into the cache in place.  Returns O [B, Sq, H, D] in q's dtype, or (O, LSE [B, H, Sq] fp32) with
    return_softmax_lse.  cache_seqlens: an int (broadcast to every sequence) or a device int32 [B]; None = the whole capacity.
    k_cache / v_cache both torch.float8_e4m3fn: k_descale / v_descale (a float, or a device fp32 tensor that broadcasts to [B, H_kv];
    default 1.0) give the value of a byte, e4m3fn(byte) * descale[b, h_kv], and k / v are quantised into the cache; with a 16-bit cache
    they must stay None.
    rotary_cos / rotary_sin: device tables [seqlen_ro, rotary_dim / 2], fp32 or q's dtype, rotary_dim a
    multiple of 16 in [16, D]; with them k is rotated at positions cache_seqlens[b] + t on its way into the cache and q at
    cache_seqlens[b] + i (causal) or cache_seqlens[b] (not causal), inside the append launch -- bit for bit the call on rotated q / k.
    rotary_interleaved: pairs (2i, 2i + 1) instead of (i, i + rotary_dim / 2); ignored without tables.  k / v are required; a position
    at or past seqlen_ro takes the last table row.
    cache_batch_idx / cache_leftpad / window_size / softcap / alibi_slopes are accepted at their defaults only.
    A sliding window over the cache is a function of its own, kvcache_window_attention.
    Raises ValueError outside the kernels' scope (see the module docstring)."""
    for name, val in unsupported.items():
        if name not in _UNSUPPORTED:
            raise TypeError(f"kvcache_attention() got an unexpected keyword argument '{name}'")
        default = _UNSUPPORTED[name]
        same = val is None if default is None else (tuple(val) == default if name == "window_size" else val == default)
        if not same:
            raise ValueError(f"kvcache_attention: {name} is not supported (only its default, {default!r}, is accepted)")
    if isinstance(q, torch.Tensor) and q.dim() == 4:
        B = q.shape[0]
        cap = k_cache.shape[1] * (block_table.shape[1] if isinstance(block_table, torch.Tensor) and block_table.dim() == 2 else 1)
        if cache_seqlens is None:
            cache_seqlens = cap
        if isinstance(cache_seqlens, int):
            cache_seqlens = torch.full((B,), cache_seqlens, dtype=torch.int32, device=q.device)
    if not isinstance(cache_seqlens, torch.Tensor):
        raise ValueError("kvcache_attention: cache_seqlens must be an int, or a device int32 [batch] tensor")
    fp8 = any(isinstance(t, torch.Tensor) and t.dtype == torch.float8_e4m3fn for t in (k_cache, v_cache))
    if not fp8 and (k_descale is not None or v_descale is not None):
        raise ValueError("kvcache_attention: k_descale / v_descale go with float8_e4m3fn caches only")
    _check(q, k_cache, v_cache, k, v, cache_seqlens, block_table, fp8)
    rotary = _check_rotary("kvcache_attention", q, k, k is not None and k.shape[1] > 0, rotary_cos, rotary_sin)
    sm = float(softmax_scale) if softmax_scale is not None else float(q.shape[-1]) ** -0.5
    if fp8:
        kd, vd = (_descale(d, q, k_cache.shape[2], n) for d, n in ((k_descale, "k_descale"), (v_descale, "v_descale")))
        k_cache, v_cache = k_cache.view(torch.uint8), v_cache.view(torch.uint8)  # (the ops take the bytes: kvcache_fp8_forward)
        if rotary:
            out, lse = torch.ops.umfa.kvcache_fp8_rope_forward_append(q, k_cache, v_cache, k, v, cache_seqlens, kd, vd, rotary_cos, rotary_sin,
                                                                      bool(rotary_interleaved), block_table, bool(causal), sm, int(num_splits))
        elif k is not None and k.shape[1] > 0:
            out, lse = torch.ops.umfa.kvcache_fp8_forward_append(q, k_cache, v_cache, k, v, cache_seqlens, kd, vd, block_table, bool(causal),
                                                                 sm, int(num_splits))
        else:
            out, lse = torch.ops.umfa.kvcache_fp8_forward(q, k_cache, v_cache, cache_seqlens, kd, vd, block_table, bool(causal), sm,
                                                          int(num_splits))
        return (out, lse) if return_softmax_lse else out
    if rotary:
        out, lse = torch.ops.umfa.kvcache_rope_forward_append(q, k_cache, v_cache, k, v, cache_seqlens, rotary_cos, rotary_sin,
                                                              bool(rotary_interleaved), block_table, bool(causal), sm, int(num_splits))
    elif k is not None and k.shape[1] > 0:
        out, lse = torch.ops.umfa.kvcache_forward_append(q, k_cache, v_cache, k, v, cache_seqlens, block_table, bool(causal), sm,
                                                         int(num_splits))
    else:
        out, lse = torch.ops.umfa.kvcache_forward(q, k_cache, v_cache, cache_seqlens, block_table, bool(causal), sm, int(num_splits))
    return (out, lse) if return_softmax_lse else out
