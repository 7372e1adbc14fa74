#!/usr/bin/env python3
"""Compare the gfx950 instruction text of two builds of libnbody_hip.so, kernel by kernel (no GPU needed).

Disassembles every code object embedded in each library (llvm-objdump -d --no-show-raw-insn), strips addresses, branch-target
offsets, symbol comments and the s_nop padding behind a function's last instruction (it belongs to whatever the linker placed
next, not to the function), and for every kernel symbol present in both reports whether its instruction text is identical.  Used to
show that a change which adds kernels left the existing ones as they were.

    python tools/compare_kernel_isa.py OLD.so NEW.so [-v] [--rename OLD_TEXT=NEW_TEXT ...]

Prints one summary line; exit status 1 if any common kernel differs (-v lists them, and the symbols found in one build only).
--rename replaces OLD_TEXT in the old build's symbols first: a type that was renamed changes the mangled name of every kernel that
takes it (--rename 7knn_rec=8pair_rec), and without this such kernels would be listed as gone and new instead of being compared."""
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
ELF_AMDGPU = b"\x7fELF\x02\x01\x01\x40"


def kernels(lib_path):
    """{symbol: tuple of instruction lines} for every function in the library's gfx950 code objects."""
    raw = open(lib_path, "rb").read()
    out, pos, k = {}, 0, 0
    with tempfile.TemporaryDirectory() as d:
        while True:
            pos = raw.find(ELF_AMDGPU, pos)
            if pos < 0:
                break
            path = os.path.join(d, f"co{k}.elf")
            open(path, "wb").write(raw[pos:])
            text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--mcpu=gfx950", path], capture_output=True,
                                  text=True).stdout
            cur = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = m.group(1)
                    out[cur] = []
                    continue
                if cur is None or not line.strip() or line.startswith("Disassembly"):
                    continue
                ins = re.sub(r"\s*//.*$", "", line).strip()          # address / encoding comment
                ins = re.sub(r"\s*<[^>]*>$", "", ins)                # branch target label
                if ins and ins != "...":
                    out[cur].append(ins)
            pos += len(ELF_AMDGPU)
            k += 1
    for v in out.values():  # alignment padding up to the next function or the end of the section
        while v and v[-1] == "s_nop 0":
            v.pop()
    return {n: tuple(v) for n, v in out.items() if v}


def compare(old_path, new_path, renames=()):
    a, b = kernels(old_path), kernels(new_path)
    for old, new in renames:
        a = {n.replace(old, new): v for n, v in a.items()}
    common = sorted(set(a) & set(b))
    differ = [n for n in common if a[n] != b[n]]
    return common, differ, sorted(set(a) - set(b)), sorted(set(b) - set(a))


def main():
    if len(sys.argv) < 3:
        print(__doc__)
        return 2
    renames = [tuple(sys.argv[i + 1].split("=", 1)) for i, arg in enumerate(sys.argv[:-1]) if arg == "--rename"]
    common, differ, gone, added = compare(sys.argv[1], sys.argv[2], renames)
    print(f"{len(common)} kernels in both builds: {len(common) - len(differ)} identical, {len(differ)} differ; "
          f"{len(gone)} only in the old build, {len(added)} only in the new")
    if "-v" in sys.argv:
        for tag, names in (("differs", differ), ("old only", gone), ("new only", added)):
            for n in names:
                print(f"  {tag}: {n}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
