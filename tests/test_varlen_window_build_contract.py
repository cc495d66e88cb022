"""Build contract of the sliding-window varlen kernels (no GPU): fa_fwd_16_varlen_window.hip and fa_bwd_16_varlen_window.hip compile for
gfx950 with their Makefile flags and hold the full kernel set -- {fwd, dq, dkdv} x {bf16, fp16} x {64, 128}, the forward with fp32 and
operand-type outputs; the window bounds are runtime values, so there is no causal instantiation -- every kernel free of scratch and
spills."""
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
    assert re.search(r"^SRCS :=.*\bfa_fwd_16_varlen_window\.hip\b.*\bfa_bwd_16_varlen_window\.hip\b", mk, re.M)
    m = re.search(r"^build/fa_fwd_16_varlen_window\.o build/fa_bwd_16_varlen_window\.o: EXTRA \+= (.*)$", mk, re.M)
    assert m, "the window varlen sources have no flag line"
    varlen = re.search(r"^build/fa_fwd_16_varlen\.o build/fa_bwd_16_varlen\.o: EXTRA \+= (.*)$", mk, re.M)
    assert varlen and m.group(1).split() == varlen.group(1).split(), "not the varlen line's flags"
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
                     for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    return res


def _check_clean(ks):
    for name, r in ks.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)


def test_forward_kernel_set(tmp_path):
    ks = _kernels(_asm("fa_fwd_16_varlen_window.hip", tmp_path))
    _check_clean(ks)
    want = {f"_ZN4umfa29fa_fwd16_varlen_window_kernelI{t}Li{d}E{o}EEvNS_12VarlenParamsE"
            for t in TYPES.values() for d in ("64", "128") for o in ("f", t)}
    assert set(ks) == want, (sorted(want - set(ks)), sorted(set(ks) - want))


def test_backward_kernel_set(tmp_path):
    ks = _kernels(_asm("fa_bwd_16_varlen_window.hip", tmp_path))
    _check_clean(ks)
    want = {f"_ZN4umfa{n}{kind}I{t}Li{d}EEEvNS_12VarlenParamsE"
            for kind, n in (("bwd16_dq_varlen_window_kernel", 29), ("bwd16_dkdv_varlen_window_kernel", 31))
            for t in TYPES.values() for d in ("64", "128")}
    assert set(ks) == want, (sorted(want - set(ks)), sorted(set(ks) - want))
