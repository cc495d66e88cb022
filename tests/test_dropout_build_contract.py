"""Build contract of the attention-dropout kernels (no GPU): fa_fwd_16_drop.hip and fa_bwd_16_drop.hip compile for gfx950 with their
Makefile flags and hold the full kernel set -- {fwd, dq, dkdv} x {bf16, fp16} x {causal, not} x {64, 128}, the forward with fp32 and
operand-type outputs -- plus the keep-mask materialiser, every kernel free of scratch and spills."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "universal-metal-flash-attention_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _flags():
    mk = (CSRC / "Makefile").read_text()
    assert re.search(r"^SRCS :=.*\bfa_fwd_16_drop\.hip\b.*\bfa_bwd_16_drop\.hip\b.*\bruntime_dropout\.hip\b", mk, re.M)
    m = re.search(r"^build/fa_fwd_16_drop\.o build/fa_bwd_16_drop\.o: EXTRA \+= (.*)$", mk, re.M)
    assert m, "the dropout sources have no flag line"
    return m.group(1).split()


def _kernels(src, tmp_path):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not found")
    out = tmp_path / (src + ".s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
                           *_flags(), "--cuda-device-only", "-S", str(CSRC / src), "-o", str(out)], cwd=CSRC)
    text = out.read_text()
    res = {}
    for blk in re.findall(r"^\s+- \.agpr_count:.*?(?=^\s+- \.agpr_count:|\Z)", text, re.M | re.S):
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
        res[name] = {k: int(re.search(rf"^\s+\.{k}:\s+(\d+)", blk, re.M).group(1))
                     for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    return res


def _check_clean(ks):
    for name, r in ks.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)


TYPES = {"bf16": "DF16b", "fp16": "DF16_"}


def test_forward_kernel_set(tmp_path):
    ks = _kernels("fa_fwd_16_drop.hip", tmp_path)
    _check_clean(ks)
    want = set()
    for t in TYPES.values():
        for c in ("0", "1"):
            for d in ("64", "128"):
                for o in ("f", t):
                    want.add(f"_ZN4umfa20fa_fwd16_drop_kernelI{t}Lb{c}ELi{d}E{o}EEvNS_13DropFwdParamsE")
    assert want <= set(ks), sorted(want - set(ks))
    assert len([k for k in ks if "fa_fwd16_drop_kernel" in k]) == 16
    assert any("fa_dropout_keep_kernel" in k for k in ks)


def test_backward_kernel_set(tmp_path):
    ks = _kernels("fa_bwd_16_drop.hip", tmp_path)
    _check_clean(ks)
    for kind, n in (("bwd16_dq_drop_kernel", 20), ("bwd16_dkdv_drop_kernel", 22)):
        want = {f"_ZN4umfa{n}{kind}I{t}Lb{c}ELi{d}EEEvNS_13DropBwdParamsE" for t in TYPES.values() for c in "01" for d in ("64", "128")}
        assert want <= set(ks), sorted(want - set(ks))
    assert len(ks) == 16
