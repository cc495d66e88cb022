"""Build-time contract of the masked / sliding-window bf16 / fp16 backward (fa_bwd_16_mask.hip), checked without a GPU: the file
compiles for gfx950 with the flags of its own Makefile line, holds the full kernel set -- {dQ, dK dV} x {bf16, fp16} x {causal, not}
x head_dim {64, 128, 256} x {tensor mask, window} -- and every kernel is scratch-free and spill-free."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "universal-metal-flash-attention_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    mk = (CSRC / "Makefile").read_text()
    m = re.search(r"build/fa_bwd_16_mask\.o: EXTRA \+= (.*)", mk)
    assert m and "-pragma-unroll-threshold" in m.group(1) and "-fno-slp-vectorize" in m.group(1), "fa_bwd_16_mask.o lost its flags"
    out = tmp_path_factory.mktemp("bwd16m") / "fa_bwd_16_mask.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-w", "--cuda-device-only", "-S",
                           *m.group(1).split(), str(CSRC / "fa_bwd_16_mask.hip"), "-o", str(out)], cwd=CSRC)
    return out.read_text()


def _kernels(text):
    out = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        name, meta = m.group(1), m.group(2)
        get = lambda key: int(re.search(key + r":\s+(\d+)", meta).group(1))  # noqa: E731
        out[name] = dict(scratch=get(r"\.private_segment_fixed_size"), spill=get(r"\.vgpr_spill_count"))
    return out


def test_masked_kernel_set_is_complete_and_scratch_free(asm):
    ks = _kernels(asm)
    dq = [n for n in ks if "bwd16_dq_masked_kernel" in n]
    kv = [n for n in ks if "bwd16_dkdv_masked_kernel" in n]
    assert len(dq) == 24 and len(kv) == 24, sorted(ks)
    assert len(ks) == 48, sorted(ks)  # nothing else lives in this file
    for name, k in ks.items():
        assert k["scratch"] == 0 and k["spill"] == 0, (name, k)

