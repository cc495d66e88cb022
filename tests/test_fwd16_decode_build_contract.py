"""Build-time contract of the decode form of the 128-row forward (fa_fwd_16_kernel.h KS = 4), checked without a GPU: fa_fwd_16.hip
(bf16 / fp16 P V) and fa_fwd_16_pv.hip (bf16 operands, fp16 P V converted in the kernel or by the cast pre-pass) compile for gfx950
with the flags of their Makefile lines, hold every decode-form instantiation -- {bf16, fp16} x head_dim {64, 128} x {fp32, operand-type O}
and bf16 x {64, 128} x {fp32, bf16 O} x pv16 {1, 2} -- and each is scratch-free and spill-free with a static LDS size that is a multiple
of 16 bytes (the dynamic tile area starts 16-byte aligned).  The compile also evaluates the epilogue's layout static_asserts: the key
quarters' exchange areas start behind the words the range check and the split-KV ticket reserve (FWD16_EPI_HDR), so an edit that puts
them back over those words fails here."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "universal-metal-flash-attention_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SOURCES = ("fa_fwd_16", "fa_fwd_16_pv")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    mk = (CSRC / "Makefile").read_text()
    assert re.search(r"^SRCS :=.*\bfa_fwd_16\.hip\b.*\bfa_fwd_16_pv\.hip\b", mk, re.M), "the library no longer builds both forward sources"
    out_dir = tmp_path_factory.mktemp("fwd16dec")
    procs = {}
    for src in SOURCES:  # the two translation units compile side by side (about two minutes each)
        extra = [f for m in re.finditer(r"^(build/\S+\.o(?: build/\S+\.o)*): EXTRA \+= (.*)$", mk, re.M) if f"build/{src}.o" in m.group(1).split()
                 for f in m.group(2).split()]  # (the Makefile's per-object flags, if it ever gives these files any)
        procs[src] = subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-w", "--cuda-device-only", "-S", *extra,
                                       str(CSRC / f"{src}.hip"), "-o", str(out_dir / f"{src}.s")], cwd=CSRC,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    texts = {}
    for src, p in procs.items():
        log, _ = p.communicate()
        assert p.returncode == 0, f"{src}.hip did not compile for gfx950:\n{log[-4000:]}"
        texts[src] = (out_dir / f"{src}.s").read_text()
    return texts


def _kernels(text):
    out = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(.*?)\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        meta = m.group(2) + m.group(4)
        get = lambda key: int(re.search(key + r":\s+(\d+)", meta).group(1))  # noqa: E731
        out[m.group(3)] = dict(lds=int(m.group(1)), scratch=get(r"\.private_segment_fixed_size"), spill=get(r"\.vgpr_spill_count"),
                               sspill=get(r"\.sgpr_spill_count"))
    return out


# fa_fwd16_kernel<T, DP, CAUSAL = false, HAS_MASK = false, OUT, DMA = true, BN = 128, PV16, KS = 4, PIPE = 0, CBAL = false>
def _decode_name(t, dp, out, pv):
    return f"_ZN4umfa15fa_fwd16_kernelI{t}Li{dp}ELb0ELb0E{out}Lb1ELi128ELi{pv}ELi4ELi0ELb0EEEvNS_9FwdParamsE"


BF, FP = "DF16b", "DF16_"
WANT = {
    "fa_fwd_16": {_decode_name(t, dp, o, 0) for t in (BF, FP) for dp in (64, 128) for o in (t, "f")},
    "fa_fwd_16_pv": {_decode_name(BF, dp, o, pv) for dp in (64, 128) for o in (BF, "f") for pv in (1, 2)},
}


@pytest.mark.parametrize("src", SOURCES)
def test_decode_form_set_is_complete_and_scratch_free(asm, src):
    ks = _kernels(asm[src])
    assert ks, f"no kernel metadata parsed from {src}.s"
    dec = {n for n in ks if re.search(r"ELi128ELi\dELi4ELi0ELb0E", n)}
    assert dec == WANT[src], (sorted(dec - WANT[src]), sorted(WANT[src] - dec))
    for name in sorted(dec):
        k = ks[name]
        assert k["scratch"] == 0 and k["spill"] == 0 and k["sspill"] == 0, (name, k)
        assert k["lds"] % 16 == 0, (name, k)  # (Guideline 17: static LDS shifts the dynamic base; keep it 16-byte aligned)


def test_epilogue_layout_is_asserted_in_the_kernel():
    """the asserts the compile above evaluates are there, and the exchange base they check is the one the epilogue uses"""
    src = (CSRC / "fa_fwd_16_kernel.h").read_text()
    assert re.search(r"constexpr int FWD16_EPI_HDR = (\d+);", src) and int(re.search(r"constexpr int FWD16_EPI_HDR = (\d+);", src).group(1)) >= 17
    assert "constexpr int EX4 = FWD16_EPI_HDR;" in src
    assert re.search(r"float\* const ex0 = \(float\*\)smem \+ \(KS == 4 \? EX4 :", src)
    assert re.search(r"static_assert\(KS != 4 \|\| \(FWD16_EPI_RED \+ NW <= FWD16_EPI_FLAG && FWD16_EPI_FLAG < FWD16_EPI_HDR && EX4 >= FWD16_EPI_HDR", src)
    assert src.count("smem + FWD16_EPI_FLAG)") == 2  # the split-KV ticket and the CBAL pair's flag
    launch = (CSRC / "fa_fwd_16_launch.h").read_text()
    assert "FWD16_EPI_HDR + fwd16_decode_exchange_words(DP)" in launch
