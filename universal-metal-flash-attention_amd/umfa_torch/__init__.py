"""umfa_torch -- PyTorch-ROCm binding of the MI355X flash-attention kernels (in-stream, zero-copy)."""
from .ops import (attention_encode, attention_forward, bench_int8, context, gpu_latency, hadamard_rotate, last_kernel, options, release_scratch, set_option, get_option, pv_fp16_status,
                  quantized_attention_forward, quantized_attention_forward_stream, quantized_attention_backward_stream, attention_backward, rope_rotate,
                  rope_attention_forward)
from . import dropout, kvcache, kvcache_window, library, parallel, varlen, varlen_kvcache, varlen_kvcache_window
from .dropout import dropout_attention
from .varlen import varlen_attention
from .kvcache import kvcache_attention
from .kvcache_window import kvcache_window_attention
from .varlen_kvcache import varlen_kvcache_attention
from .varlen_kvcache_window import varlen_kvcache_window_attention
from .sdpa import (QUANT_BLOCK_WISE, QUANT_INT4, QUANT_INT8, QUANT_NONE, QUANT_TENSOR_WISE, get_dispatch_stats,
                   get_quantization_mode, register_backend, reset_dispatch_stats, rope_scaled_dot_product_attention,
                   scaled_dot_product_attention, sliding_window_attention,
                   set_quantization_mode, unregister_backend, use_umfa_sdpa)

__all__ = ["dropout", "dropout_attention", "kvcache", "kvcache_attention", "kvcache_window", "kvcache_window_attention", "library", "parallel", "varlen", "varlen_attention", "varlen_kvcache", "varlen_kvcache_attention", "varlen_kvcache_window", "varlen_kvcache_window_attention", "rope_rotate", "rope_attention_forward", "hadamard_rotate", "attention_forward", "attention_encode", "quantized_attention_forward", "quantized_attention_forward_stream", "quantized_attention_backward_stream", "attention_backward", "bench_int8", "context",
           "gpu_latency", "last_kernel", "set_option", "get_option", "pv_fp16_status", "options", "release_scratch", "scaled_dot_product_attention", "sliding_window_attention", "rope_scaled_dot_product_attention", "register_backend", "unregister_backend",
           "use_umfa_sdpa", "set_quantization_mode", "get_quantization_mode", "get_dispatch_stats",
           "reset_dispatch_stats", "QUANT_NONE", "QUANT_INT8", "QUANT_INT4", "QUANT_TENSOR_WISE", "QUANT_BLOCK_WISE"]
