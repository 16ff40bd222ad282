#!/usr/bin/env python3
"""Compare the gfx950 device code that two source trees produce for one translation unit, kernel by kernel.  No GPU needed.

  tools/devcode_diff.py <tree_a> <tree_b> <unit> [extra hipcc flags...]
  tools/devcode_diff.py ../parent . ltr_scorer.hip -DLTR_F16X2=1 -DLTR_STAMPS

For each tree: compile csrc/<unit> with that tree's ltr_mi355x/build.py FLAGS plus the extras, take the .hip_fatbin section out
of the result, unbundle the gfx950 code object, disassemble it, split the text by symbol and drop the branch-target comments
(the only place an address appears).  Prints how many kernels were compared, whether both trees define the same symbols and the
name of every kernel whose instructions differ; the exit status is 1 on any difference.  This is the check behind a refactor
that claims to leave the device code alone.
"""
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

PKG = "nn-with-pytorch-personalized-losses_amd"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def llvm_tool(name):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for d in (os.path.join(rocm, "lib", "llvm", "bin"), os.path.join(rocm, "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name) or sys.exit(f"{name} not found under {rocm}")


def build_flags(tree):
    spec = importlib.util.spec_from_file_location("_build", os.path.join(tree, PKG, "ltr_mi355x", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.FLAGS)


def disassemble(tree, unit, extra, work):
    """{symbol: [instruction lines]} of the gfx950 code object of one translation unit."""
    lib, fat, co = (os.path.join(work, n) for n in ("unit.so", "unit.hipfb", "unit.co"))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.run([hipcc] + build_flags(tree) + extra + [os.path.join(tree, PKG, "csrc", unit), "-o", lib], check=True)
    subprocess.run([llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    subprocess.run([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                    f"--input={fat}", f"--output={co}"], check=True)
    text = subprocess.run([llvm_tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                          check=True, capture_output=True, text=True).stdout
    kernels, body = {}, None
    for line in text.splitlines():
        head = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if head:
            body = kernels.setdefault(head.group(1), [])
        elif body is not None and line.strip():
            body.append(re.sub(r"\s*//.*$", "", line).strip())
    return kernels


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    tree_a, tree_b, unit, extra = os.path.abspath(argv[0]), os.path.abspath(argv[1]), argv[2], argv[3:]
    with tempfile.TemporaryDirectory() as wa, tempfile.TemporaryDirectory() as wb:
        a, b = disassemble(tree_a, unit, extra, wa), disassemble(tree_b, unit, extra, wb)
    same_symbols = a.keys() == b.keys()
    common = sorted(a.keys() & b.keys())
    differing = [k for k in common if a[k] != b[k]]
    print(f"{unit} {' '.join(extra) or '(default flags)'}: {len(common)} kernels compared, "
          f"symbol sets {'equal' if same_symbols else 'DIFFER'}, {len(differing)} differ")
    for k in sorted(a.keys() - b.keys()):
        print(f"  only in {tree_a}: {k}")
    for k in sorted(b.keys() - a.keys()):
        print(f"  only in {tree_b}: {k}")
    for k in differing:
        print(f"  differs: {k} ({len(a[k])} vs {len(b[k])} instructions)")
    return 0 if same_symbols and not differing else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
