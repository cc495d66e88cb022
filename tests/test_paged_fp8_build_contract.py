"""Build contract of the fp8 KV-cache kernels (no GPU): fa_fwd_16_paged_fp8.hip compiles for gfx950 with its Makefile flags and holds the
full kernel set -- the forward for {bf16, fp16} x {64, 128} x {causal, not} x {fp32, operand-type output, split partials} and the
quantising append per input type -- every kernel free of scratch and spills, the expansions and the append on the packed fp8 conversion
instructions, and the 16-bit unit's kernel set untouched (the fold is shared through a host launcher)."""
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
    assert re.search(r"^SRCS :=.*\bfa_fwd_16_paged_fp8\.hip\b", mk, re.M)
    assert re.search(r"^HDRS :=.*\bfa_paged_fp8\.h\b", mk, re.M)
    m = re.search(r"^build/fa_fwd_16_paged_fp8\.o: EXTRA \+= (.*)$", mk, re.M)
    assert m, "the fp8 paged source has no flag line"
    paged = re.search(r"^build/fa_fwd_16_paged\.o: EXTRA \+= (.*)$", mk, re.M)
    assert paged and m.group(1).split() == paged.group(1).split()  # the flag line the paged unit has
    return m.group(1).split()


def _kernels(text):
    res = {}
    for blk in re.findall(r"^\s+- \.agpr_count:.*?(?=^\s+- \.agpr_count:|\Z)", text, re.M | re.S):
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M).group(1)
        res[name] = {k: int(re.search(rf"^\s+\.{k}:\s+(\d+)", blk, re.M).group(1))
                     for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")}
    return res


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail("hipcc not found")
    out = tmp_path_factory.mktemp("fp8") / "fa_fwd_16_paged_fp8.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
                           *_flags(), "--cuda-device-only", "-S", str(CSRC / "fa_fwd_16_paged_fp8.hip"), "-o", str(out)], cwd=CSRC)
    return out.read_text()


def test_kernel_set(asm):
    ks = _kernels(asm)
    for name, r in ks.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
    want = {f"_ZN4umfa25fa_fwd16_paged_fp8_kernelI{t}Lb{c}ELi{d}E{o}EEvNS_14PagedFp8ParamsE"
            for t in TYPES.values() for c in "01" for d in ("64", "128") for o in ("f", t, "v")}
    want |= {f"_ZN4umfa26fa_paged_fp8_append_kernelI{t}EEvNS_14PagedFp8ParamsE" for t in TYPES.values()}
    assert want <= set(ks), sorted(want - set(ks))
    assert len(ks) == len(want) == 26


def test_packed_fp8_conversions(asm):
    """K8 -> T and V8 -> fp16 by the packed scaled conversions, the append by the packed fp32 -> fp8 one: no byte-wise decode"""
    assert re.search(r"\bv_cvt_scalef32_pk_bf16_fp8\b", asm) and re.search(r"\bv_cvt_scalef32_pk_f16_fp8\b", asm)
    assert re.search(r"\bv_cvt_pk_fp8_f32\b", asm)


def test_ring_waits_are_counted(asm):
    """the loop waits for a stage with a counted vmcnt (8 requests per wave and step at head_dim 128, 4 at 64), so the younger stage stays
    in flight; and the stages land by LDS-DMA"""
    assert "s_waitcnt vmcnt(8)" in asm and "s_waitcnt vmcnt(4)" in asm
    assert re.search(r"buffer_load_dwordx4 v\d+, s\[\d+:\d+\], 0 offen lds", asm)


def test_the_16bit_unit_keeps_its_kernels():
    """the fp8 kernels live in their own unit: fa_fwd_16_paged.hip defines no fp8 kernel, and the fold is reached through a host launcher"""
    src = (CSRC / "fa_fwd_16_paged.hip").read_text()
    assert "fp8" not in re.sub(r"//.*", "", src)
    assert re.search(r"^hipError_t launch_paged_fold\(", src, re.M)
    assert "launch_paged_fold(" in (CSRC / "fa_fwd_16_paged_fp8.hip").read_text()
