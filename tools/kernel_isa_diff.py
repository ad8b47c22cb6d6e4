#!/usr/bin/env python3
"""Compare two device assembly files (hipcc --cuda-device-only -S) function by function.

    python tools/kernel_isa_diff.py before.s after.s

Per function symbol: the instruction stream (comments, .loc / .file / .cfi lines and blank lines dropped,
the per-function ordinal in local labels normalised) and, for kernels, the .amdhsa_* resource lines.  The
__hip_cuid_* object at the end of the file is ignored.  Prints how many functions there are, how many are
identical, and the name and line counts of each one that differs.  Exit status 1 if any differs.
"""
import re
import sys

SKIP = re.compile(r"\.(loc|file|cfi_\w+)\b")
LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp)\d+")


def functions(path):
    """{symbol: (code lines, .amdhsa_* lines)} of one assembly file"""
    out, name, code, res, in_desc = {}, None, None, None, False
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].strip()
        if not line or SKIP.match(line):
            continue
        m = re.match(r"\.type\s+([^,\s]+),@function", line)
        if m:
            name, code, res = m.group(1), [], []
            continue
        if name is None:
            continue
        if line.startswith(".size") and line.split()[1].rstrip(",") == name:
            if not name.startswith("__hip_cuid_"):
                out[name] = (code, res)
            name = None
        elif line.startswith(".amdhsa_kernel"):
            in_desc = True
        elif line.startswith(".end_amdhsa_kernel"):
            in_desc = False
        elif in_desc:
            res.append(line)
        else:
            code.append(LOCAL.sub(lambda x: ".L" + x.group(1), line))
    return out


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = functions(argv[1]), functions(argv[2])
    names = sorted(set(a) | set(b))
    kernels = sum(1 for n in names if (a.get(n) or b.get(n))[1])
    differ = []
    for n in names:
        if n not in a or n not in b:
            differ.append("%s: only in %s" % (n, argv[1] if n in a else argv[2]))
        elif a[n] != b[n]:
            what = [w for w, i in (("code", 0), ("amdhsa", 1)) if a[n][i] != b[n][i]]
            differ.append("%s: %s differs (%d / %d code lines)" % (n, " + ".join(what), len(a[n][0]), len(b[n][0])))
    print("functions: %d (%d kernels)   identical: %d   differing: %d" % (len(names), kernels, len(names) - len(differ), len(differ)))
    for d in differ:
        print("  " + d)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
