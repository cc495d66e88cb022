#!/usr/bin/env python3
"""Per-kernel register / scratch / LDS figures of one .hip source, from the device assembly (no GPU needed).

    python tools/kernel_resources.py fa_fwd_16_pv.hip [--filter substr] [--extra "-DFOO -fno-slp-vectorize"] [--src-dir DIR] [--dyn-lds BYTES] [--mangled]

Prints one line per kernel: vgpr, agpr, sgpr, scratch bytes, spill count, LDS bytes, waves per SIMD, MFMA count, instruction lines.
Waves per SIMD: what the 512-register file allows in blocks of 8, floor(512 / (8 ceil(vgpr / 8))), at most 8, and no more than the
256-thread workgroups whose LDS (static + --dyn-lds, the dynamic bytes of a launch) fits a CU's 160 KiB: each puts one wave on every SIMD."""
import argparse
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "universal-metal-flash-attention_amd" / "csrc"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source")
    ap.add_argument("--filter", default="")
    ap.add_argument("--extra", default="")
    ap.add_argument("--src-dir", default=str(CSRC))
    ap.add_argument("--keep", default="", help="write the assembly here")
    ap.add_argument("--reuse", action="store_true", help="with --keep: parse the file if it exists instead of compiling")
    ap.add_argument("--mangled", action="store_true", help="print the mangled kernel names (c++filt does not know every 16-bit type)")
    ap.add_argument("--dyn-lds", type=int, default=0, help="dynamic LDS bytes of a launch (added to the static figure for waves / SIMD)")
    a = ap.parse_args()
    src_dir = Path(a.src_dir)
    extra = a.extra.split()
    mk = (CSRC / "Makefile").read_text()
    m = re.search(r"^(?:build/\S+\.o )*build/%s(?: build/\S+\.o)*: EXTRA \+= (.*)" % re.escape(Path(a.source).stem + ".o"), mk, re.M)  # (a rule may name several objects)
    if m:
        extra += m.group(1).split()
    with tempfile.TemporaryDirectory() as td:
        out = Path(a.keep) if a.keep else Path(td) / "k.s"
        if not (a.keep and a.reuse and out.exists()):
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-w", "--cuda-device-only", "-S", *extra,
                                   str(src_dir / a.source), "-o", str(out)], cwd=src_dir)
        text = out.read_text()
    meta_all = text[text.index("amdhsa.kernels:"):]
    for entry in re.split(r"\n  - ", meta_all)[1:]:
        nm = re.search(r"\.name:\s+(\S+)", entry)
        if not nm:
            continue
        name = nm.group(1)
        if a.filter and a.filter not in name:
            continue

        def get(key, entry=entry):
            g = re.search(key + r":\s+(\d+)", entry)
            return int(g.group(1)) if g else -1
        k0 = text.index("\n" + name + ":")
        body = text[k0:text.index("\n.Lfunc_end", k0)]  # (the whole function: a kernel with an early exit holds more than one s_endpgm)
        dem = name if a.mangled else subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        vgpr, lds = get(r'.vgpr_count'), get(r'.group_segment_fixed_size') + a.dyn_lds
        waves = min(8, 512 // (8 * max(1, -(-vgpr // 8))))
        if lds > 0:
            waves = min(waves, 160 * 1024 // lds)
        print(f"vgpr {vgpr:4d} agpr {get(r'.agpr_count'):4d} sgpr {get(r'.sgpr_count'):4d} scratch {get(r'.private_segment_fixed_size'):5d} "
              f"spill {get(r'.vgpr_spill_count'):4d} lds {lds:6d} waves {waves:2d} mfma {body.count('v_mfma'):4d} insts {len(body.splitlines()):6d}  {dem[:170]}")


if __name__ == "__main__":
    sys.exit(main())
