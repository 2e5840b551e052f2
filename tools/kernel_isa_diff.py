#!/usr/bin/env python3
"""Compare two builds of the library's device code kernel by kernel (not file by file: kernels may move between translation units).

    for u in msda_api ffn_mfma rows_api cls_mfma conv_mfma conv_wgrad lin256_mfma attn_mfma; do
        hipcc <flags of richsem_amd/_build.py> --cuda-device-only -S -o DIR/$u.s richsem_amd/csrc/$u.hip
    done                                   # once per commit, into DIR_A and DIR_B
    python tools/kernel_isa_diff.py DIR_A DIR_B

Per kernel symbol: the instruction text and .vgpr_count / .sgpr_count / .private_segment_fixed_size / .group_segment_fixed_size of the
code object's metadata.  What depends on the position in a file is normalised: the compilation unit's id in the names of
internal-linkage symbols, the function index in basic-block labels.  Exit status 1 if any kernel differs or exists on one side only.
"""
import glob
import os
import re
import sys

FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def normalise(text):
    text = re.sub(r"\.(intern|static)\.[0-9a-f]{8,}", "", text)      # the compilation unit's id
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", text)
    return re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+(_\d+)?", lambda m: ".L%s%s" % (m.group(1), m.group(2) or ""), text)


def kernels(directory):
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        text = normalise(open(path).read())
        meta = {}
        for block in text.split("  - .agpr_count:")[1:]:
            name = re.search(r"^\s+\.name:\s+(\S+)", block, re.M).group(1)
            meta[name] = tuple(re.search(r"^\s+%s:\s+(\S+)" % re.escape(f), block, re.M).group(1) for f in FIELDS)
        for name, fields in meta.items():
            m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.M | re.S)
            body = "\n".join(l.split(";")[0].rstrip() for l in m.group(1).splitlines() if l.strip() and not l.lstrip().startswith(";"))
            assert name not in out, name
            out[name] = (os.path.basename(path), fields, body)
    return out


def main(dir_a, dir_b):
    a, b = kernels(dir_a), kernels(dir_b)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("only in %s: %s" % (dir_a if name in a else dir_b, name))
        elif a[name][1] != b[name][1]:
            print("resources differ: %s %s -> %s" % (name, a[name][1], b[name][1]))
        elif a[name][2] != b[name][2]:
            print("instructions differ: %s" % name)
        else:
            continue
        bad += 1
    moved = sorted(n for n in set(a) & set(b) if a[n][0] != b[n][0])
    files = sorted(set(v[0] for v in b.values()))
    print("%d kernels in %s, %d in %s; %d differ; %d moved between files" % (len(a), dir_a, len(b), dir_b, bad, len(moved)))
    for f in files:
        print("  %s: %d kernels, %d instruction lines" % (f, sum(1 for v in b.values() if v[0] == f),
                                                         sum(v[2].count("\n") + 1 for v in b.values() if v[0] == f)))
    for n in moved:
        print("  moved %s -> %s: %s" % (a[n][0], b[n][0], n))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
