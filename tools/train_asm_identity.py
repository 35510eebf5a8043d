#!/usr/bin/env python3
"""Compare the kernels' gfx950 device assembly of two builds of one translation unit, kernel by kernel (no GPU needed); written for the
trainer's units, it takes any two .s files:
    hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only -o parent.s alphazero_gym_amd/csrc/dispatch_train.hip     (in a checkout of the parent)
    hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only -o change.s alphazero_gym_amd/csrc/dispatch_train.hip     (in this tree)
    python tools/train_asm_identity.py parent.s change.s
(likewise dispatch_train_wide.hip, engine_selfplay.hip, ...).  Every kernel of either file -- every symbol with an .amdhsa_kernel block -- is compared with
the kernel of the same mangled name in the other; a kernel that only one file has is a difference.  A kernel's text runs from its
label to its .Lfunc_end, the kernel descriptor (.amdhsa_ block: registers, LDS, kernarg size) included.
Before the comparison comments are dropped, basic-block labels are renumbered in order of appearance (their numbers count the
functions of the file) and the `.text` / `.section .text.<name>,...,comdat` line that follows a kernel is dropped (an instantiation
lives in a comdat section).  With --renamed OLD=NEW (mangled names, repeatable) a kernel that was renamed is compared with its
successor, the kernel's own name replaced by KERNEL on both sides.  With --added-ok a kernel that only the second file has is
listed as added and is not a difference (a change that adds kernels beside the ones it must leave alone); the last line counts
them, and with --added=N the run also fails unless exactly N kernels were added (a new instantiation that was not meant shows).
Exit status 1 on any difference."""
import difflib
import re
import sys

def functions(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^([A-Za-z_]\w*):", line)   # (mangled names, and the extern "C" kernels' plain ones)
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
        res.append(ln.replace(name, "KERNEL") if name else ln)
    return res


def kernels(path):
    return [m.group(1) for m in (re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line) for line in open(path)) if m]


def main():
    args, renamed, added_ok, want_added, added = [], {}, False, None, 0
    for arg in sys.argv[1:]:
        if arg == "--added-ok":
            added_ok = True
        elif arg.startswith("--added="):
            added_ok, want_added = True, int(arg[len("--added="):])
        elif arg.startswith("--renamed="):
            old, new = arg[len("--renamed="):].split("=")
            renamed[old] = new
        elif arg != "--renamed":
            args.append(arg)
    a, b = functions(args[0]), functions(args[1])
    ka, kb = kernels(args[0]), kernels(args[1])
    bad = 0
    for name in ka:
        other = renamed.get(name, name)
        if other not in kb:
            bad += 1
            print(f"{name}\n    absent from the second file: DIFFERENT")
            continue
        # (the KERNEL substitution only where the names differ)
        na, nb = body(a[name], name if other != name else None), body(b[other], other if other != name else None)
        insts = sum(1 for ln in na if ln.startswith("\t") and not ln.strip().startswith("."))
        same = na == nb
        bad += not same
        print(f"{name}\n    lines {len(na):5d} / {len(nb):5d}  instructions {insts:5d}  {'identical' if same else 'DIFFERENT'}")
        if not same:
            for i, ln in enumerate(difflib.unified_diff(na, nb, lineterm="", n=0)):
                if i < 60:
                    print("    " + ln)
    for name in kb:
        if name not in ka and name not in renamed.values():
            if added_ok:
                added += 1
                print(f"{name}\n    absent from the first file: added")
                continue
            bad += 1
            print(f"{name}\n    absent from the first file: DIFFERENT")
    if want_added is not None and added != want_added:
        bad += 1
        print(f"{added} kernels added where {want_added} were expected: DIFFERENT")
    print(f"{len(ka)} / {len(kb)} kernels, {bad} different" + (f", {added} added" if added_ok else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
