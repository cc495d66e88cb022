"""Build contract of the sliding-window packed KV-cache kernels (no GPU): fa_fwd_16_paged_varlen_window.hip is in the Makefile with the
flags of fa_fwd_16_paged.hip, compiles for gfx950 with them and holds exactly the 12 kernels -- {bf16, fp16} x {64, 128} x {fp32 out,
operand-type out, split}; the window bounds are runtime values, so there is no causal instantiation -- every kernel free of scratch and
spills.  Only the kernels' metadata is read."""
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
    assert re.search(r"^SRCS :=.*\bfa_fwd_16_paged_varlen_window\.hip\b", mk, re.M)
    assert re.search(r"^HDRS :=.*\bfa_paged_varlen_window\.h\b", mk, re.M)
    m = re.search(r"^build/fa_fwd_16_paged_varlen_window\.o: EXTRA \+= (.*)$", mk, re.M)
    assert m, "the packed window KV-cache source has no flag line"
    paged = re.search(r"^build/fa_fwd_16_paged\.o: EXTRA \+= (.*)$", mk, re.M)
    assert paged and m.group(1).split() == paged.group(1).split(), "not the paged line's flags"
    return m.group(1).split()


def _asm(src, tmp_path):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not found")
    out = tmp_path / (src + ".s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
                           *_flags(), "--cuda-device-only", "-S", str(CSRC / src), "-o", str(out)], cwd=CSRC)
    return out.read_text()


def _kernels(text):
    res = {}
    for blk in re.findall(r"^\s+- \.agpr_count:.*?(?=^\s+- \.agpr_count:|\Z)", text, re.M | re.S):
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
        res[name] = {k: int(re.search(rf"^\s+\.{k}:\s+(\d+)", blk, re.M).group(1))
                     for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count", "sgpr_count")}
    return res


def test_makefile_lines():
    assert _flags() == ["-fno-slp-vectorize", "-mllvm", "-pragma-unroll-threshold=262144"]


def test_packed_window_kernel_set(tmp_path):
    ks = _kernels(_asm("fa_fwd_16_paged_varlen_window.hip", tmp_path))
    for name, r in sorted(ks.items()):
        print(name, r)
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
    want = {f"_ZN4umfa35fa_fwd16_paged_varlen_window_kernelI{t}Li{d}E{o}EEvNS_23PagedVarlenWindowParamsE"
            for t in TYPES.values() for d in ("64", "128") for o in ("f", t, "v")}
    assert len(want) == 12 and set(ks) == want, (sorted(want - set(ks)), sorted(set(ks) - want))
