"""Kernel-by-kernel comparison of two device-only assembly builds of engine.hip (a host-only change must leave every kernel as it was).

Build each side with the flags of probes/kstats.sh:
  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -mllvm -amdgpu-mfma-vgpr-form -ffp-contract=on -fno-honor-nans \\
        texocr_amd/csrc/engine.hip -o before.s
then: python probes/asm_diff.py before.s after.s
Two builds of the same tree differ in the __hip_cuid_* symbol and, when templates are instantiated in another order, in the order of the
functions and the numbers of their local labels: so every function is cut out on its own and its labels are renumbered before comparing
(and the padding in front of a label's comment, which depends on the number's width, is dropped).
Prints the functions present on one side only and those whose text differs; exit status 1 if any body differs.

A kernel template that gained a parameter has another mangled name on the second side although its old instantiations are meant to be the
old kernels: --rename REGEX REPL rewrites the second side's text first (re.sub), so that such a kernel meets its predecessor, and --diff
prints the lines in which a DIFFERENT pair differs.  For attn_mq_kernel / attn_probs_kernel after they gained `RAGGED` and `lens`:
  python probes/asm_diff.py before.s after.s --diff --rename '(attn_(?:mq|probs)_kernelI\w*?)Lb0E(EEv\w*?PKhi)PKi' '\1\2'
(a new trailing kernel argument shows as a larger .amdhsa_kernarg_size and nothing else)."""
import difflib
import re
import shutil
import subprocess
import sys


def functions(path, rename=None):
    out, name, body = {}, None, []
    text = open(path).read()
    if rename:
        text = re.sub(rename[0], rename[1], text)
    for line in text.splitlines(keepends=True):
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


def main(a, b, rename=None, show=False):
    fa, fb = functions(a), functions(b, rename)
    kernels = lambda f: sum(".amdhsa_kernel " in body for body in f.values())
    print(f"{a}: {len(fa)} functions, {kernels(fa)} kernels; {b}: {len(fb)} functions, {kernels(fb)} kernels")
    for label, names in (("only in " + a, sorted(set(fa) - set(fb))), ("only in " + b, sorted(set(fb) - set(fa))),
                         ("DIFFERENT", sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k]))):
        for n, raw in zip(demangle(names), names):
            print(f"{label}: {n}")
            if show and label == "DIFFERENT":
                for line in difflib.unified_diff(fa[raw].splitlines(), fb[raw].splitlines(), lineterm="", n=0):
                    if not line.startswith(("---", "+++", "@@")):
                        print("    " + line)
    same = sum(fa[k] == fb[k] for k in set(fa) & set(fb))
    print(f"identical: {same} of {len(set(fa) & set(fb))} common functions")
    return 0 if same == len(set(fa) & set(fb)) else 1


if __name__ == "__main__":
    argv = sys.argv[1:]
    rename = None
    if "--rename" in argv:
        i = argv.index("--rename")
        rename = (argv[i + 1], argv[i + 2])
        del argv[i:i + 3]
    show = "--diff" in argv
    argv = [x for x in argv if x != "--diff"]
    sys.exit(main(argv[0], argv[1], rename, show))
