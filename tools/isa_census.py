#!/usr/bin/env python3
"""Static instruction census of the conv kernels: a device-only -S compile of every csrc/conv_mfma*.hip with the
Makefile's flags, then per kernel instantiation the counts that do not depend on register naming -- MFMAs, LDS reads and
writes, global / buffer loads with and without the LDS-DMA modifier, barriers, scratch accesses.  A helper that failed
to inline, or that reloads what a hand-written copy kept in a register, moves one of them.

    tools/isa_census.py [CSRC_DIR] > census.txt      (diff two trees' outputs)
"""
import glob
import os
import re
import subprocess
import sys

FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -fno-slp-vectorize".split()
COLS = ["mfma", "ds_rd", "ds_wr", "vm_ld", "vm_ld_lds", "barrier", "scratch"]


def classify(op, rest):
    if op.startswith("v_mfma_"):
        return "mfma"
    if op.startswith(("ds_read", "ds_load")):
        return "ds_rd"
    if op.startswith(("ds_write", "ds_store")):
        return "ds_wr"
    if op.startswith(("global_load_", "buffer_load_")):
        return "vm_ld_lds" if ("_lds_" in op or re.search(r"\blds\b", rest)) else "vm_ld"
    if op == "s_barrier":
        return "barrier"
    if op.startswith("scratch_"):
        return "scratch"
    return None


def census(asm):
    out, cur = {}, None
    for ln in asm.splitlines():
        m = re.match(r"^(_Z\w*conv_mfma\w*):", ln)
        if m:
            cur = out.setdefault(m.group(1), dict.fromkeys(COLS, 0))
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
        if cur is None:
            continue
        m = re.match(r"^\s+([a-z]\w+)\s*(.*)$", ln)
        if m:
            k = classify(m.group(1), m.group(2))
            if k:
                cur[k] += 1
    return out


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "..", "ratio_guided_multimodal_fm_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    print(f"{'kernel':60s} " + " ".join(f"{c:>9s}" for c in COLS))
    for src in sorted(glob.glob(os.path.join(csrc, "conv_mfma*.hip"))):
        asm = subprocess.run([hipcc, *FLAGS, "--cuda-device-only", "-S", "-x", "hip", src, "-o", "-"], check=True,
                             capture_output=True, text=True).stdout
        rows = census(asm)
        names = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True, text=True).stdout.split("\n")
        for mn, dn in sorted(zip(rows, names), key=lambda t: t[1]):
            short = re.sub(r"\(.*$", "", re.sub(r"^void rgfm::", "", dn))
            print(f"{short:60s} " + " ".join(f"{rows[mn][c]:9d}" for c in COLS))


if __name__ == "__main__":
    sys.exit(main())
