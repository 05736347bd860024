"""Compare the device code of two builds of ctc_amd/csrc/noblank.hip function by function (no GPU needed).

    python tools/r16_disasm_diff.py OLD.o NEW.o

OLD.o / NEW.o: hipcc -c objects of noblank.hip (e.g. ctc_amd/lib/obj/noblank.o of two checkouts).  The gfx950 code object
is unbundled from each, disassembled with llvm-objdump, and every function's instructions are compared with branch
targets, encodings and the zero fill between functions left out.  fp32 instantiations of noblank_r16_kernel that gained
the element-type template argument (`...EfEEvNS...`) are matched with their old names.  Exit status 1 if any function of
OLD.o is missing from NEW.o or differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"


def disassemble(obj, tmp):
    base = os.path.join(tmp, os.path.basename(obj) + str(abs(hash(obj))))
    subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section=.hip_fatbin=%s.fatbin" % base, obj])
    subprocess.check_call([LLVM + "/clang-offload-bundler", "--type=o", "--input=%s.fatbin" % base,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s.co" % base, "--unbundle"])
    return subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr",
                                    base + ".co"], text=True)


def functions(text):
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^<(\S+)>:$", line.strip())
        if m:
            cur = out.setdefault(m.group(1).replace("EfEEvNS", "EEEvNS"), [])
            continue
        ins = re.sub(r"//.*$", "", re.sub(r"<[^>]*>", "<>", line)).strip()
        if cur is not None and ins and ins != "...":
            cur.append(ins)
    return out


def main(old, new):
    with tempfile.TemporaryDirectory() as tmp:
        a, b = functions(disassemble(old, tmp)), functions(disassemble(new, tmp))
    missing = sorted(k for k in a if k not in b)
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    r16 = [k for k in a if "noblank_r16_kernel" in k]
    print("%d functions in %s, %d in %s (%d new)" % (len(a), old, len(b), new, len(set(b) - set(a))))
    print("noblank_r16_kernel instantiations of %s: %d, identical in %s: %d" % (
        old, len(r16), new, sum(1 for k in r16 if k in b and a[k] == b[k])))
    for k in missing:
        print("missing:", k)
    for k in differ:
        print("differs:", k, len(a[k]), len(b[k]))
    return 1 if missing or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
