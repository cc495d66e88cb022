"""Build contract of the KV-cache kernels (no GPU): fa_fwd_16_paged.hip compiles for gfx950 with its Makefile flags and holds the full
kernel set -- the forward for {bf16, fp16} x {64, 128} x {causal, not} x {fp32, operand-type output, split partials}, the split-KV fold
per output type, the append -- every kernel free of scratch and spills."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "universal-metal-flash-attention_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TYPES = {"bf16": "DF16b", "fp16": "DF16_"}


def _flags():
    mk = (CSRC / "Makefile").read_text()
    assert re.search(r"^SRCS :=.*\bfa_fwd_16_paged\.hip\b.*\bruntime_paged\.hip\b", mk, re.M)
    assert re.search(r"^HDRS :=.*\bfa_paged\.h\b", mk, re.M)
    m = re.search(r"^build/fa_fwd_16_paged\.o: EXTRA \+= (.*)$", mk, re.M)
    assert m, "the paged source has no flag line"
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
    out = tmp_path / "fa_fwd_16_paged.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
                           *_flags(), "--cuda-device-only", "-S", str(CSRC / "fa_fwd_16_paged.hip"), "-o", str(out)], cwd=CSRC)
    ks = _kernels(out.read_text())
    for name, r in ks.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
    want = {f"_ZN4umfa21fa_fwd16_paged_kernelI{t}Lb{c}ELi{d}E{o}EEvNS_11PagedParamsE"
            for t in TYPES.values() for c in "01" for d in ("64", "128") for o in ("f", t, "v")}
    want |= {f"_ZN4umfa20fa_paged_fold_kernelI{o}EEvNS_11PagedParamsE" for o in ("f", *TYPES.values())}
    want.add("_ZN4umfa22fa_paged_append_kernelENS_11PagedParamsE")
    assert want <= set(ks), sorted(want - set(ks))
    assert len(ks) == len(want) == 28
