#!/usr/bin/env python3
"""Compare two device assembly listings symbol by symbol.

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S -o OLD.s device/engine.hip   (at the old commit)
    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S -o NEW.s device/engine.hip   (at the new one)
    tools/device_asm_diff.py OLD.s NEW.s

A change that only moves source text must leave every function's instructions as they were. The compiler
numbers functions in the order it emits them, and that number appears in local labels (.LBB<n>_<m>,
.Lfunc_end<n>), so those numbers are masked, and assembler comments are dropped. A type that moves to another
namespace changes the mangled name of every function taking it, so functions are keyed by their demangled
name with the namespace qualifiers stripped (llvm-cxxfilt or c++filt), and inside a body every symbol of the
listing is written as its key. Prints every symbol whose
text differs (or that one side lacks) with its instruction count and, for kernels, the registers and
scratch bytes of both sides. Exit status 1 if any symbol differs, else 0.
"""
import re
import shutil
import subprocess
import sys

TYPE = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
END = re.compile(r"^\.Lfunc_end\d+:")
LOCAL = re.compile(r"\.L(BB|func_begin|func_end|JTI|CPI)\d+")
FIGURES = ("next_free_vgpr", "accum_offset", "private_segment_fixed_size")
FIGURE = re.compile(r"^\.amdhsa_(%s)\s+(\S+)" % "|".join(FIGURES))


MANGLED = re.compile(r"\b_Z\w+")
QUALIFIER = re.compile(r"(?:\(anonymous namespace\)|[A-Za-z_]\w*)::")


def keys(names):
    """{symbol: demangled name without namespace qualifiers}; the symbol itself where it does not demangle"""
    tool = shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin") \
        or shutil.which("c++filt")
    if not tool:
        sys.exit("device_asm_diff.py needs llvm-cxxfilt or c++filt")
    names = list(names)
    plain = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return {n: QUALIFIER.sub("", d) for n, d in zip(names, plain.split("\n"))}


def symbols(path):
    """{key: (normalized lines, instruction count, {figure: value})} of one listing"""
    raw = raw_symbols(path)
    key = keys(raw)
    if len(set(key.values())) != len(key):
        sys.exit("%s: two symbols with one key" % path)
    return {key[n]: ([MANGLED.sub(lambda k: key.get(k.group(0), k.group(0)), l) for l in lines], instr, fig)
            for n, (lines, instr, fig) in raw.items()}


def raw_symbols(path):
    out = {}
    name, body, descriptor = None, None, False
    for raw in open(path, errors="replace"):
        m = TYPE.match(raw)
        if m:
            name, body, descriptor = m.group(1), None, False
            continue
        if name is None:
            continue
        if body is None:
            if raw.startswith(name + ":"):
                body = {"lines": [], "instr": 0, "fig": {}}
            continue
        if END.match(raw):
            out[name] = (body["lines"], body["instr"], body["fig"])
            name = None
            continue
        line = LOCAL.sub(lambda k: ".L" + k.group(1) + "#", raw.split(";", 1)[0]).strip()
        if not line:
            continue
        body["lines"].append(line)
        if line.startswith(".amdhsa_kernel"):
            descriptor = True
        f = FIGURE.match(line)
        if f:
            body["fig"][f.group(1)] = f.group(2)
        elif not descriptor and not line.startswith(".") and not line.endswith(":"):
            body["instr"] += 1
    return out


def describe(entry):
    if entry is None:
        return "absent"
    _, instr, fig = entry
    return "%d instructions, %s" % (instr, ", ".join("%s %s" % (k, fig.get(k, "-")) for k in FIGURES))


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    old, new = symbols(argv[1]), symbols(argv[2])
    names = sorted(set(old) | set(new))
    differing = [n for n in names if n not in old or n not in new or old[n][0] != new[n][0]]
    for n in differing:
        print(n)
        print("    old: " + describe(old.get(n)))
        print("    new: " + describe(new.get(n)))
    kernels = sum(1 for n in names if n in new and new[n][2])
    scratch = [n for n in names if n in new and new[n][2].get("private_segment_fixed_size", "0") != "0"]
    print("%d symbols (%d kernels in NEW), %d differing; %d kernels of NEW use scratch" %
          (len(names), kernels, len(differing), len(scratch)))
    for n in scratch:
        print("    scratch: %s %s bytes" % (n, new[n][2]["private_segment_fixed_size"]))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
