"""Kernel-by-kernel comparison of two device-only assembly builds of engine.hip (a host-only change must leave every kernel as it was).

Build each side with the flags of probes/kstats.sh:
  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -mllvm -amdgpu-mfma-vgpr-form -ffp-contract=on -fno-honor-nans \\
        texocr_amd/csrc/engine.hip -o before.s
then: python probes/asm_diff.py before.s after.s
Two builds of the same tree differ in the __hip_cuid_* symbol and, when templates are instantiated in another order, in the order of the
functions and the numbers of their local labels: so every function is cut out on its own and its labels are renumbered before comparing
(and the padding in front of a label's comment, which depends on the number's width, is dropped).
Prints the functions present on one side only and those whose text differs; exit status 1 if any body differs."""
import re
import shutil
import subprocess
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            name, body = m.group(1), []
        if name is None:
            continue
        body.append(re.sub(r"[ \t]+;", " ;", re.sub(r"(BB|\.Lfunc_end|\.Ltmp)\d+", r"\1", line)))
        if "; -- End function" in line:
            out[name], name = "".join(body), None
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("/opt/rocm/llvm/bin/llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return list(names)
    return subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")[:len(names)]


def main(a, b):
    fa, fb = functions(a), functions(b)
    kernels = lambda f: sum(".amdhsa_kernel " in body for body in f.values())
    print(f"{a}: {len(fa)} functions, {kernels(fa)} kernels; {b}: {len(fb)} functions, {kernels(fb)} kernels")
    for label, names in (("only in " + a, sorted(set(fa) - set(fb))), ("only in " + b, sorted(set(fb) - set(fa))),
                         ("DIFFERENT", sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k]))):
        for n in demangle(names):
            print(f"{label}: {n}")
    same = sum(fa[k] == fb[k] for k in set(fa) & set(fb))
    print(f"identical: {same} of {len(set(fa) & set(fb))} common functions")
    return 0 if same == len(set(fa) & set(fb)) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
