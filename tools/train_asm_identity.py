#!/usr/bin/env python3
"""Compare the trainer kernels' gfx950 device assembly of two builds, kernel by kernel (no GPU needed):
    hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only -o parent.s alphazero_gym_amd/csrc/dispatch_train.hip     (in a checkout of the parent)
    hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only -o change.s alphazero_gym_amd/csrc/dispatch_train.hip     (in this tree)
    python tools/train_asm_identity.py parent.s change.s
A kernel's text runs from its label to its .Lfunc_end, the kernel descriptor (.amdhsa_ block: registers, LDS, kernarg size) included.
Before the comparison comments are dropped, basic-block labels are renumbered in order of appearance (their numbers count the
functions of the file), the kernel's own mangled name is replaced by KERNEL (a template instantiation is named differently from a
plain function) and the `.text` / `.section .text.<name>,...,comdat` line that follows a kernel is dropped (an instantiation lives
in a comdat section).  Of a templated kernel the instantiation without LayerNorm (<false>) is taken.  Exit status 1 if any differs."""
import difflib
import re
import sys

KERNELS = ("train_forward_kernel", "train_backward_kernel", "train_backward_deferred_kernel", "train_loss_kernel", "train_gather_kernel",
           "train_loss_sum_kernel")


def functions(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                out[cur].append(line.rstrip())
    return out


def body(lines, name):
    labels, res = {}, []
    for ln in lines:
        ln = re.sub(r";.*$", "", ln).rstrip()
        if not ln.strip() or ln.strip() == ".text" or ln.strip().startswith(".section"):
            continue
        ln = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), ln)
        res.append(ln.replace(name, "KERNEL"))
    return res


def pick(funcs, base):
    names = [k for k in funcs if re.match(r"_Z\d+" + base + r"(?![a-z_])", k) and "ILb1E" not in k]
    return names[0] if names else None


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for base in KERNELS:
        ka, kb = pick(a, base), pick(b, base)
        if ka is None or kb is None:
            print(f"{base:32s} {'absent from the first file' if ka is None else 'absent from the second file'}")
            continue
        na, nb = body(a[ka], ka), body(b[kb], kb)
        insts = sum(1 for ln in na if ln.startswith("\t") and not ln.strip().startswith("."))
        same = na == nb
        bad += not same
        print(f"{base:32s} lines {len(na):5d} / {len(nb):5d}  instructions {insts:5d}  {'identical' if same else 'DIFFERENT'}")
        if not same:
            for i, ln in enumerate(difflib.unified_diff(na, nb, lineterm="", n=0)):
                if i < 60:
                    print("    " + ln)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
