"""Compare the machine code of every kernel between two builds of the library, kernel by kernel.

  python tools/isa_diff.py BEFORE_BUILD_DIR AFTER_BUILD_DIR

Each directory is a factorizer_amd/csrc/build of a build (the .o files).  The gfx950 code object of every object is unbundled and
disassembled with the recipe of tools/pk_opsel_audit.py (llvm-objcopy, clang-offload-bundler, llvm-objdump); each kernel's
instruction stream (addresses and branch-target offsets stripped) is compared by mangled name.  Prints the kernels that exist in
both builds with different instructions, the ones that vanished and the count of new ones; exits 1 if a kernel of the first build
is missing from or differs in the second.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
HEAD = re.compile(r"^[0-9a-f]+ <(\S+)>:$")
ADDR = re.compile(r"^\s*[0-9a-f]+:\s*")
OFFS = re.compile(r"\s*//.*$|<[^>]*>")


def kernels(obj):
    out = {}
    with tempfile.TemporaryDirectory() as td:
        fb, co = os.path.join(td, "fb.bin"), os.path.join(td, "co.elf")
        if subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj], capture_output=True).returncode:
            return out
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
        txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                             text=True).stdout
    cur = None
    for ln in txt.splitlines():
        m = HEAD.match(ln)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur is not None and ln.strip() and ln.strip() != "...":   # ("...": objdump's elision of the zero padding after a kernel)
            out[cur].append(OFFS.sub("", ADDR.sub("", ln)).strip())
    return out


def collect(d):
    allk = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".o"):
            for k, ins in kernels(os.path.join(d, f)).items():
                allk[(f, k)] = ins
    return allk


def main(before, after):
    a, b = collect(before), collect(after)
    bnames = {k for (_, k) in b}
    bmap = {k: v for (_, k), v in b.items()}
    missing = [k for (_, k) in a if k not in bnames]
    differ = [k for (_, k), ins in a.items() if k in bmap and bmap[k] != ins]
    new = bnames - {k for (_, k) in a}
    n_ins = sum(len(v) for v in a.values())
    print(f"before: {len(a)} kernels ({n_ins} instructions); after: {len(b)} kernels")
    print(f"identical: {len(a) - len(missing) - len(differ)}  differ: {len(differ)}  missing: {len(missing)}  new: {len(new)}")
    for k in differ[:20]:
        print("DIFFERS", k)
    for k in missing[:20]:
        print("MISSING", k)
    return 1 if (missing or differ) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
