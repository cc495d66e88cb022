"""Build contract of the rotary pre-pass of the KV-cache calls (no GPU): the Makefile builds fa_paged_rope.hip into the library and lists
its header; the unit compiles for gfx950 and holds the full kernel set -- {bf16, fp16} operands x {fp32, operand-type} tables x
{[B, S, ..] operands over a 16-bit cache, over an fp8 cache, packed operands} -- every kernel free of scratch and spills; umfa_abi.h
declares both entries and the built library exports them."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "universal-metal-flash-attention_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TYPES = {"bf16": "DF16b", "fp16": "DF16_"}
ENTRIES = ("umfa_kvcache_attention_rope_forward_stream", "umfa_varlen_kvcache_attention_rope_forward_stream")
ROPE_ARGS = ("rotary_cos", "rotary_sin", "rotary_table_precision", "rotary_row_stride", "seqlen_ro", "rotary_dim", "rotary_interleaved")


def _flags():
    mk = (CSRC / "Makefile").read_text()
    assert re.search(r"^SRCS :=.*\bfa_paged_rope\.hip\b", mk, re.M)
    assert re.search(r"^SRCS :=.*\bruntime_paged\.hip\b.*\bruntime_paged_varlen\.hip\b", mk, re.M)
    assert re.search(r"^HDRS :=.*\bfa_paged_rope\.h\b", mk, re.M)
    m = re.search(r"^build/fa_paged_rope\.o: EXTRA \+= (.*)$", mk, re.M)  # a streaming kernel: the default flags unless a line says otherwise
    return m.group(1).split() if m else []


def _kernels(text):
    res = {}
    for blk in re.findall(r"^\s+- \.agpr_count:.*?(?=^\s+- \.agpr_count:|\Z)", text, re.M | re.S):
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
        res[name] = {k: int(re.search(rf"^\s+\.{k}:\s+(\d+)", blk, re.M).group(1))
                     for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")}
    return res


def test_kernel_set(tmp_path):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not found")
    out = tmp_path / "fa_paged_rope.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
                           *_flags(), "--cuda-device-only", "-S", str(CSRC / "fa_paged_rope.hip"), "-o", str(out)], cwd=CSRC)
    ks = _kernels(out.read_text())
    for name, r in ks.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)  # no LDS either
    want = {f"_ZN4umfa20fa_paged_rope_kernelI{t}{tt}Li{m}EEEvNS_15PagedRopeParamsE"
            for t in TYPES.values() for tt in ("f", t) for m in "012"}
    assert want <= set(ks), (sorted(want - set(ks)), sorted(ks))
    assert len(ks) == len(want) == 12


def test_existing_units_do_not_include_the_new_header():
    """the attention kernels are untouched: only the new unit and the two runtime units see fa_paged_rope.h"""
    users = sorted(p.name for p in CSRC.iterdir() if p.suffix in (".hip", ".h", ".inc") and '"fa_paged_rope.h"' in p.read_text())
    assert users == ["fa_paged_rope.hip", "runtime_paged.hip", "runtime_paged_varlen.hip"]


def test_header_declares_and_library_exports_the_entries():
    text = (ROOT / "include" / "umfa_abi.h").read_text()
    for entry in ENTRIES:
        m = re.search(entry + r"\s*\(([^;]*)\);", text)
        assert m, f"{entry} is not declared in umfa_abi.h"
        for arg in ROPE_ARGS + ("block_table", "cache_seqlens", "num_splits"):
            assert re.search(rf"\b{arg}\b", m.group(1)), (entry, arg)
    dense = re.search(ENTRIES[0] + r"\s*\(([^;]*)\);", text).group(1)
    for arg in ("cache_fp8", "k_descale", "v_descale", "seqlen_new"):
        assert re.search(rf"\b{arg}\b", dense), arg
    packed = re.search(ENTRIES[1] + r"\s*\(([^;]*)\);", text).group(1)
    assert "cu_seqlens_q" in packed and "has_new" in packed and "k_descale" not in packed
    so = ROOT / "universal-metal-flash-attention_amd" / "lib" / "libMFAFFI.so"
    assert so.exists(), "build() has not produced libMFAFFI.so"
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    names = {line.split()[-1] for line in subprocess.check_output([nm, "-D", "--defined-only", str(so)], text=True).splitlines() if line.strip()}
    assert set(ENTRIES) <= names
