"""Build contract of the packed-query fp8 KV-cache kernels (no GPU): fa_fwd_16_paged_varlen_fp8.hip compiles for gfx950 with its
Makefile flags and holds exactly the kernel set built -- the forward for {bf16, fp16} x {64, 128} x {causal, not} x {fp32, operand-type
output, split partials}, the packed quantising append per operand type and the packed fp8 rotary pre-pass for {bf16, fp16} x {fp32,
operand-type table} -- every kernel free of scratch and spills; umfa_abi.h declares the entry and the built library exports it."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "universal-metal-flash-attention_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TYPES = {"bf16": "DF16b", "fp16": "DF16_"}
ENTRY = "umfa_varlen_kvcache_attention_fp8_forward_stream"


def _flags():
    mk = (CSRC / "Makefile").read_text()
    assert re.search(r"^SRCS :=.*\bfa_fwd_16_paged_varlen_fp8\.hip\b.*\bruntime_paged_varlen\.hip\b", mk, re.M)
    assert re.search(r"^HDRS :=.*\bfa_paged_varlen_fp8\.h\b", mk, re.M)
    m = re.search(r"^build/fa_fwd_16_paged_varlen_fp8\.o: EXTRA \+= (.*)$", mk, re.M)
    assert m, "the packed-query fp8 source has no flag line"
    paged = re.search(r"^build/fa_fwd_16_paged_fp8\.o: EXTRA \+= (.*)$", mk, re.M)
    assert paged and m.group(1) == paged.group(1), "the flags are the paged units'"
    return m.group(1).split()


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
    out = tmp_path / "fa_fwd_16_paged_varlen_fp8.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
                           *_flags(), "--cuda-device-only", "-S", str(CSRC / "fa_fwd_16_paged_varlen_fp8.hip"), "-o", str(out)], cwd=CSRC)
    ks = _kernels(out.read_text())
    for name, r in ks.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, (name, r)  # (the forward's LDS is dynamic: 128 KiB at D 128, 64 KiB at D 64)
    P = "NS_20PagedVarlenFp8ParamsE"
    want = {f"_ZN4umfa32fa_fwd16_paged_varlen_fp8_kernelI{t}Lb{c}ELi{d}E{o}EEv{P}"
            for t in TYPES.values() for c in "01" for d in ("64", "128") for o in ("f", t, "v")}
    assert len(want) == 24
    want |= {f"_ZN4umfa33fa_paged_varlen_fp8_append_kernelI{t}EEv{P}" for t in TYPES.values()}
    want |= {f"_ZN4umfa31fa_paged_varlen_fp8_rope_kernelI{t}{tt}EEvNS_24PagedVarlenFp8RopeParamsE" for t in TYPES.values() for tt in ("f", t)}
    assert want == set(ks), (sorted(want - set(ks)), sorted(set(ks) - want))
    assert len(ks) == 30


def test_header_declares_and_library_exports_the_entry():
    text = (ROOT / "include" / "umfa_abi.h").read_text()
    m = re.search(ENTRY + r"\s*\(([^;]*)\);", text)
    assert m, f"{ENTRY} is not declared in umfa_abi.h"
    args = [a.split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
    # umfa_varlen_kvcache_attention_forward_stream's arguments, then the fp8 entry's four descale arguments, then the rotary arguments
    plain = re.search(r"umfa_varlen_kvcache_attention_forward_stream\s*\(([^;]*)\);", text).group(1)
    plain = [a.split()[-1].lstrip("*") for a in plain.replace("\n", " ").split(",")]
    assert args == plain + ["k_descale", "k_descale_strides", "v_descale", "v_descale_strides", "rotary_cos", "rotary_sin",
                            "rotary_table_precision", "rotary_row_stride", "seqlen_ro", "rotary_dim", "rotary_interleaved"], args
    assert "seqlen_new" not in m.group(1) and "cache_fp8" not in m.group(1)
    so = ROOT / "universal-metal-flash-attention_amd" / "lib" / "libMFAFFI.so"
    assert so.exists(), "build() has not produced libMFAFFI.so"
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    names = {line.split()[-1] for line in subprocess.check_output([nm, "-D", "--defined-only", str(so)], text=True).splitlines() if line.strip()}
    assert ENTRY in names
    assert not any("paged_varlen_fp8" in n and not n.startswith("umfa_") for n in names)  # (no launcher or host stub leaks out)
