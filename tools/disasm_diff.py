"""Compare the device code of two builds of ctc_amd/csrc function by function (no GPU needed).

    python tools/disasm_diff.py [--rename FROM=TO]... OLD.o NEW.o
    python tools/disasm_diff.py [--rename FROM=TO]... OLD_OBJDIR NEW_OBJDIR

OLD / NEW: two hipcc -c objects of the same source, or two directories of them (e.g. ctc_amd/lib/obj, obj_diag, obj_fault
of two checkouts: every *.o of either directory is compared with the one of the same name).  The gfx950 code object is
unbundled from each, disassembled with llvm-objdump, and every function's instructions are compared with branch targets,
encodings and the fill between functions (zeros, trailing s_nop 0) left out.  --rename FROM=TO (repeatable) replaces
the substring FROM by TO in the function names of the OLD object (mangled, as `llvm-objdump --syms` prints them) before
the names are matched: for a kernel that was renamed, or that gained or lost a template argument, between the two
builds.  Exit status 1 if any function (or object) is missing, added or differs."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"


def disassemble(obj, tmp):
    base = os.path.join(tmp, "%d_%s" % (len(os.listdir(tmp)), os.path.basename(obj)))
    # (llvm-objcopy without an output file would rewrite `obj` in place)
    subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section=.hip_fatbin=%s.fatbin" % base, obj, base + ".copy"])
    subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--input=%s.fatbin" % base,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s.co" % base, "--unbundle"])
    syms = subprocess.check_output([LLVM + "/llvm-objdump", "--syms", base + ".co"], text=True)
    funcs = {l.split()[-1] for l in syms.splitlines() if re.search(r"\sF\s+\.text\s", l)}
    return funcs, subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr",
                                           base + ".co"], text=True)


def functions(funcs, text, renames=()):
    """name -> instructions; a label that is no function symbol (the numbered loop labels of inline assembly) stays
    inside the function around it"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(\S+)>:$", line.strip())
        if m:
            if m.group(1) in funcs:
                name = m.group(1)
                for old, new in renames:
                    name = name.replace(old, new)
                cur = out.setdefault(name, [])
            continue
        ins = re.sub(r"//.*$", "", re.sub(r"<[^>]*>", "<>", line)).strip()
        ins = re.sub(r"^(s_c?branch\S*)\s+\S+$", r"\1 <>", ins)       # (a target printed as a bare label)
        if cur is not None and ins and ins != "...":
            cur.append(ins)
    for body in out.values():                                        # the s_nop fill behind a function's last instruction
        while body and body[-1] == "s_nop 0":                        # (its length depends on what follows in .text)
            body.pop()
    return out


def compare(old, new, renames=()):
    """-> number of functions of the two objects that are missing, added or differ"""
    with tempfile.TemporaryDirectory() as tmp:
        a, b = functions(*disassemble(old, tmp), renames), functions(*disassemble(new, tmp))
    missing, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    print("%s: %d functions, %s: %d functions; %d missing, %d added, %d differ" % (
        old, len(a), new, len(b), len(missing), len(added), len(differ)))
    for k in missing:
        print("  missing:", k)
    for k in added:
        print("  added:", k)
    for k in differ:
        print("  differs:", k, len(a[k]), len(b[k]))
    return len(missing) + len(added) + len(differ)


def main(old, new, renames=()):
    if not os.path.isdir(old):
        return 1 if compare(old, new, renames) else 0
    names = [sorted(f for f in os.listdir(d) if f.endswith(".o")) for d in (old, new)]
    bad = 0
    for f in sorted(set(names[0]) | set(names[1])):
        if f in names[0] and f in names[1]:
            bad += compare(os.path.join(old, f), os.path.join(new, f), renames)
        else:
            print("%s: only in %s" % (f, old if f in names[0] else new))
            bad += 1
    print("%d objects compared, %d differences" % (len(set(names[0]) & set(names[1])), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rename", action="append", default=[], metavar="FROM=TO")
    ap.add_argument("old")
    ap.add_argument("new")
    args = ap.parse_args()
    if any("=" not in r for r in args.rename):
        ap.error("--rename takes FROM=TO")
    sys.exit(main(args.old, args.new, [tuple(r.split("=", 1)) for r in args.rename]))
