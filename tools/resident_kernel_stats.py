"""What the compiler made of the resident kernels, without a
GPU: elp_resident.hip compiled to gfx950 assembly with the product flags, then
per kernel the instruction count (assembly lines that are instructions) and,
from the code object's metadata, spilled SGPRs / VGPRs, scratch, registers.

    python tools/resident_kernel_stats.py [--src DIR] [--out FILE.json]

--src: another checkout's easylp_amd/csrc (the parent commit's, to compare)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed"]
KERNELS = ("k_resident", "k_resident_batch", "k_resident_tree")
META = {"sgpr_spill_count": "spilled_sgprs", "vgpr_spill_count": "spilled_vgprs",
        "private_segment_fixed_size": "scratch_bytes_per_lane", "sgpr_count": "sgprs", "vgpr_count": "vgprs"}


def kernel_of(symbol):
    """k_resident_batch from _ZN3elp12_GLOBAL__N_116k_resident_batchEPK..."""
    hits = [k for k in KERNELS if re.search(r"\d+" + k + r"E", symbol)]
    return max(hits, key=len) if hits else None


def stats(asm):
    out = {}
    cur = None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = kernel_of(m.group(1))
            if cur:
                out[cur] = {"instructions": 0}
            continue
        if cur and re.match(r"^\s+\.end_amdhsa_kernel|^\.Lfunc_end", line):
            cur = None
            continue
        if cur and re.match(r"^\s+[a-z_0-9]+(\s|$)", line) and not line.lstrip().startswith("."):
            out[cur]["instructions"] += 1
    # the metadata block: one YAML record per kernel
    for rec in re.split(r"\n  - ", asm[asm.find("amdhsa.kernels:"):]):
        name = re.search(r"\.name:\s+(\S+)", rec)
        k = kernel_of(name.group(1)) if name else None
        if not k or k not in out:
            continue
        for key, label in META.items():
            v = re.search(r"\." + key + r":\s+(\d+)", rec)
            if v:
                out[k][label] = int(v.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "easylp_amd", "csrc"))
    ap.add_argument("--out")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "elp_resident.s")
        subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", "-o", s, "elp_resident.hip"], cwd=a.src, check=True)
        doc = {"flags": FLAGS, "kernels": stats(open(s).read())}
    for k, v in doc["kernels"].items():
        print(f"{k:18s} " + "  ".join(f"{n} {x}" for n, x in v.items()))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
