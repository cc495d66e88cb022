"""Build contract of the packed-query KV-cache kernels (no GPU): fa_fwd_16_paged_varlen.hip compiles for gfx950 with its Makefile flags
and holds the full kernel set -- the forward for {bf16, fp16} x {64, 128} x {causal, not} x {fp32, operand-type output, split partials},
the split-KV fold per output type, the packed append and the item-list pre-pass -- every kernel free of scratch and spills; umfa_abi.h
declares the entry and the built library exports it."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "universal-metal-flash-attention_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TYPES = {"bf16": "DF16b", "fp16": "DF16_"}
ENTRY = "umfa_varlen_kvcache_attention_forward_stream"


def _flags():
    mk = (CSRC / "Makefile").read_text()
    assert re.search(r"^SRCS :=.*\bfa_fwd_16_paged_varlen\.hip\b.*\bruntime_paged_varlen\.hip\b", mk, re.M)
    assert re.search(r"^HDRS :=.*\bfa_paged_varlen\.h\b", mk, re.M)
    m = re.search(r"^build/fa_fwd_16_paged_varlen\.o: EXTRA \+= (.*)$", mk, re.M)
    assert m, "the packed-query paged source has no flag line"
    return m.group(1).split()


def _kernels(text):
    res = {}
    for blk in re.findall(r"^\s+- \.agpr_count:.*?(?=^\s+- \.agpr_count:|\Z)", text, re.M | re.S):
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
        res[name] = {k: int(re.search(rf"^\s+\.{k}:\s+(\d+)", blk, re.M).group(1))
                     for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    return res


def test_kernel_set(tmp_path):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not found")
    out = tmp_path / "fa_fwd_16_paged_varlen.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
                           *_flags(), "--cuda-device-only", "-S", str(CSRC / "fa_fwd_16_paged_varlen.hip"), "-o", str(out)], cwd=CSRC)
    ks = _kernels(out.read_text())
    for name, r in ks.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
    P = "NS_17PagedVarlenParamsE"
    want = {f"_ZN4umfa28fa_fwd16_paged_varlen_kernelI{t}Lb{c}ELi{d}E{o}EEv{P}"
            for t in TYPES.values() for c in "01" for d in ("64", "128") for o in ("f", t, "v")}
    want |= {f"_ZN4umfa27fa_paged_varlen_fold_kernelI{o}EEv{P}" for o in ("f", *TYPES.values())}
    want.add(f"_ZN4umfa29fa_paged_varlen_append_kernelE{P}")
    want.add(f"_ZN4umfa28fa_paged_varlen_items_kernelE{P}")
    assert want <= set(ks), sorted(want - set(ks))
    assert len(ks) == len(want) == 29


def test_header_declares_and_library_exports_the_entry():
    text = (ROOT / "include" / "umfa_abi.h").read_text()
    m = re.search(ENTRY + r"\s*\(([^;]*)\);", text)
    assert m, f"{ENTRY} is not declared in umfa_abi.h"
    for arg in ("total_q", "batch", "max_seqlen_q", "cu_seqlens_q", "has_new", "block_table", "cache_seqlens", "num_splits"):
        assert re.search(rf"\b{arg}\b", m.group(1)), arg
    assert "seqlen_new" not in m.group(1)
    so = ROOT / "universal-metal-flash-attention_amd" / "lib" / "libMFAFFI.so"
    assert so.exists(), "build() has not produced libMFAFFI.so"
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    names = {line.split()[-1] for line in subprocess.check_output([nm, "-D", "--defined-only", str(so)], text=True).splitlines() if line.strip()}
    assert ENTRY in names
