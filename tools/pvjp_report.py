#!/usr/bin/env python3
"""Register table of the parameter-gradient kernels, from the code-object
metadata of the cross-compiled library (host-only; no GPU needed).

    python tools/pvjp_report.py [libmpcqp.so]

One line per `*_pvjp` kernel: instructions, VGPRs, SGPRs, waves per SIMD
(floor(512 / VGPRs rounded up to 8), at most 8), private segment (scratch) and LDS bytes.
"""
import sys
import tempfile

import codeobj


def rows(lib):
    with tempfile.TemporaryDirectory() as wd:
        for co in codeobj.code_objects(lib, wd):
            for name, md in sorted(codeobj.metadata(co).items()):
                if "pvjp" not in name:
                    continue
                ins, _ = codeobj.instructions(co, name)
                vg = md["vgpr_count"]
                waves = min(8, 512 // max(8, -(-vg // 8) * 8))
                yield (name, len(ins), vg, md["sgpr_count"], waves, md["private_segment_fixed_size"],
                       md["group_segment_fixed_size"], md["vgpr_spill_count"], md["sgpr_spill_count"])


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else codeobj.library_path()
    print("insns  VGPR  SGPR waves scratch   LDS vspill sspill  kernel")
    for r in rows(lib):
        print("%5d %5d %5d %5d %7d %5d %6d %6d  %s" % (r[1:] + r[:1]))


if __name__ == "__main__":
    main()
