#!/usr/bin/env python3
"""Compare the gfx950 device code of two object files or shared libraries, kernel by kernel.  CPU only (no GPU, no HIP runtime).

    tools/codeobj_diff.py A.o B.o [--arch gfx950] [--show N]

For each input: `llvm-objdump --offloading` unbundles the code object(s) (one per object file, several per library), `llvm-readelf -sW`
lists the kernels (a FUNC symbol with a `.kd` descriptor beside it), `llvm-objdump -d` disassembles them.  Compared per kernel name:

  instruction stream   the disassembly without addresses and encodings, and without the literals of the pc-relative address sequences
                       (s_getpc_b64 + s_add_u32 / s_addc_u32): those hold the distance to a global and move with the layout
  kernel descriptor    the 64 bytes of NAME.kd without kernel_code_entry_byte_offset (bytes 16..23: the distance to the code)
  metadata             the kernel's entry of the NT_AMDGPU_METADATA note (arguments, LDS, registers, spills)

and prints one line each: equal, differs, only-in-A or only-in-B.  A refactor of host code should give `equal` for every kernel present
in both; exit status 1 if anything differs or is missing on one side.  The tool compares; it does not look for particular instructions.
"""
import argparse
import difflib
import glob
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def tool(name, *args):
    exe = os.path.join(LLVM, name)
    return subprocess.run([exe if os.path.exists(exe) else name, *args], check=True, capture_output=True, text=True).stdout


def sections(elf):
    """[(address, file offset, size)] of the ELF64 little-endian image `elf`."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    out = []
    for i in range(shnum):
        addr, off, size = struct.unpack_from("<QQQ", elf, shoff + i * shentsize + 0x10)
        typ, = struct.unpack_from("<I", elf, shoff + i * shentsize + 4)
        if typ != 8 and addr:                       # not SHT_NOBITS, and loaded
            out.append((addr, off, size))
    return out


def kernels_of(path):
    """{kernel name: (instruction lines, descriptor bytes, metadata text)} of one extracted code object."""
    elf = open(path, "rb").read()
    secs = sections(elf)
    func, kd = {}, {}
    for ln in tool("llvm-readelf", "-sW", "--symbols", path).splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] == "FUNC":
            func[f[7]] = int(f[1], 16)
        elif len(f) == 8 and f[3] == "OBJECT" and f[7].endswith(".kd"):
            kd[f[7][:-3]] = int(f[1], 16)
    # disassembly, split at the `<symbol>:` headers
    code, cur = {}, None
    for ln in tool("llvm-objdump", "-d", path).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = code.setdefault(m.group(1), [])
        elif cur is not None and ln.startswith("\t") and ln.strip() != "...":      # "...": zero padding behind the section's last kernel
            cur.append(ln.split("//")[0].strip())
    for lines in code.values():
        while lines and lines[-1] in ("s_nop 0", "s_code_end"):   # alignment fill behind a kernel's end (it depends on what follows)
            lines.pop()
        for i, ins in enumerate(lines):             # literals of the pc-relative sequences
            if ins.startswith("s_getpc_b64"):
                for j in range(i + 1, min(i + 5, len(lines))):
                    if re.match(r"s_addc?_u32 ", lines[j]):
                        lines[j] = re.sub(r", (0x[0-9a-f]+|-?\d+)$", ", <pcrel>", lines[j])
    # metadata: the entries of amdhsa.kernels
    meta, entry = {}, None
    for ln in tool("llvm-readelf", "--notes", path).splitlines():
        if ln.startswith("  - "):
            entry = [ln]
        elif entry is not None and ln.startswith("    "):
            entry.append(ln)
            m = re.match(r"^    \.name:\s+(\S+)", ln)
            if m:
                meta[m.group(1)] = entry
        else:
            entry = None
    out = {}
    for name in func:
        if name not in kd:
            continue                                # a device function, not a kernel
        desc = b""
        for addr, off, size in secs:
            if addr <= kd[name] < addr + size:
                raw = elf[off + kd[name] - addr: off + kd[name] - addr + 64]
                desc = raw[:16] + raw[24:]
        out[name] = (code.get(name, []), desc, "\n".join(meta.get(name, [])))
    return out


def load(path, arch, tmp):
    """All kernels of an object file or library (every bundled code object for `arch`)."""
    work = os.path.join(tmp, str(len(os.listdir(tmp))))
    os.mkdir(work)
    copy = shutil.copy(path, work)
    tool("llvm-objdump", "--offloading", copy)
    parts = sorted(glob.glob(copy + ".*" + arch))
    if not parts:
        sys.exit(f"{path}: no {arch} code object inside")
    out = {}
    for p in parts:
        for name, v in kernels_of(p).items():
            n, k = name, 2
            while n in out:                         # the same kernel name in two translation units of a library
                n, k = f"{name}#{k}", k + 1
            out[n] = v
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--show", type=int, default=0, help="print up to N differing instruction lines per kernel")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        A, B = load(args.a, args.arch, tmp), load(args.b, args.arch, tmp)
    names = sorted(set(A) | set(B))
    try:
        pretty = dict(zip(names, tool("llvm-cxxfilt", *[n.split("#")[0] for n in names]).splitlines())) if names else {}
    except (OSError, subprocess.CalledProcessError):
        pretty = {}
    count = {"equal": 0, "differs": 0, "only-in-A": 0, "only-in-B": 0}
    for n in names:
        if n not in A or n not in B:
            verdict, detail = ("only-in-A" if n in A else "only-in-B"), ""
        else:
            (ca, da, ma), (cb, db, mb) = A[n], B[n]
            verdict = "equal" if (ca, da, ma) == (cb, db, mb) else "differs"
            detail = f"  [code {'equal' if ca == cb else 'differs'}, descriptor {'equal' if da == db else 'differs'}, metadata {'equal' if ma == mb else 'differs'}]"
        count[verdict] += 1
        print(f"{verdict:10s} {pretty.get(n, n)}{detail}")
        if verdict == "differs" and args.show:
            d = [ln for ln in difflib.unified_diff(A[n][0], B[n][0], "A", "B", lineterm="", n=0) if not ln.startswith("@@")]
            print("\n".join("    " + ln for ln in d[:args.show]))
    print(f"{len(names)} kernels: " + ", ".join(f"{v} {k}" for k, v in count.items()))
    return 0 if count["equal"] == len(names) else 1


if __name__ == "__main__":
    sys.exit(main())
