#!/usr/bin/env python3
"""Compare the device functions of two builds of the HIP sources, from their assembly listings.

    hipcc <build.py's flags> -S --offload-device-only unit.hip -o unit.s          # once per unit and build
    python scripts/kernel_asm_diff.py OLD NEW                                     # two .s files, or two directories of them

Every device function is keyed by its mangled name, whichever listing of a side holds it, so a kernel that moved to another
translation unit is compared with itself; a function with internal linkage may have one copy per unit, all alike.  Compared are the instruction text between a function's label and its `.Lfunc_end`
(comments and blank lines dropped, the function index of `.LBB<n>_<m>` labels normalised) and, for a kernel, its
`.amdhsa_kernel ... .end_amdhsa_kernel` descriptor (registers, LDS, private_segment_fixed_size).  One line per function; the exit
status is 1 if anything differs, is missing or is new.
"""
import glob
import os
import re
import sys

_FUNC = re.compile(r"^\s*\.type\s+([\w$.]+),@function")
_LBB = re.compile(r"\.LBB\d+_(\d+)")


def _listings(path):
    return sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]


def functions(path):
    """{mangled name: (unit, body lines, descriptor lines or None)} of every device function under `path`."""
    out = {}
    for listing in _listings(path):
        unit = os.path.basename(listing)
        name, body, desc, in_desc = None, [], None, False
        with open(listing) as fh:
            for raw in fh:
                line = raw.split(";", 1)[0].rstrip()
                text = line.strip()
                if not text:
                    continue
                if name is None:
                    m = _FUNC.match(line)
                    if m:
                        name, body, desc = m.group(1), [], None
                    continue
                if text == name + ":":
                    continue
                if text.startswith(".Lfunc_end"):
                    if name not in out:
                        out[name] = (unit, body, desc)
                    elif desc is None and out[name][1:] == (body, None):          # an internal-linkage function, one copy per unit
                        out[name] = (out[name][0] + "+" + unit, body, None)
                    else:
                        raise SystemExit("%s: %s is defined twice, differently (also in %s)" % (listing, name, out[name][0]))
                    name = None
                elif text.startswith(".amdhsa_kernel "):
                    in_desc, desc = True, []
                elif text == ".end_amdhsa_kernel":
                    in_desc = False
                elif in_desc:
                    desc.append(text)
                else:
                    body.append(_LBB.sub(r".LBB_\1", text))
    return out


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    old, new = functions(argv[1]), functions(argv[2])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in new:
            verdict, where = "MISSING", old[name][0]
        elif name not in old:
            verdict, where = "NEW", new[name][0]
        else:
            (uo, bo, do), (un, bn, dn) = old[name], new[name]
            where = uo if uo == un else "%s -> %s" % (uo, un)
            verdict = "identical" if bo == bn and do == dn else "DIFFERS (%s)" % ", ".join(
                w for w, d in (("text", bo != bn), ("descriptor", do != dn)) if d)
        bad += verdict != "identical"
        kind = "kernel" if (new.get(name) or old[name])[2] is not None else "function"
        lines = len((new.get(name) or old[name])[1])
        print("%-9s %-18s %6d lines  %-40s %s" % (kind, verdict, lines, where, name))
    kernels = sum(1 for v in new.values() if v[2] is not None)
    print("%d functions (%d kernels) in the new build, %d in the old; %d not identical" % (len(new), kernels, len(old), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
