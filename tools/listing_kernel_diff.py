#!/usr/bin/env python3
"""Compare chosen kernels of two device listings (hipcc --save-temps: *-hip-amdgcn-amd-amdhsa-gfx950.s) whose SYMBOLS differ.

    python tools/listing_kernel_diff.py parent.s result.s 'attention_mfma_kernel<false, 64' 'attention_cls_kernel<'

tools/listing_diff.py keys every kernel by its mangled symbol, so a template that gains a defaulted parameter shows up as "only in
first / only in second" although no instruction moved.  This tool pairs kernels by their DEMANGLED names instead: a kernel of the
second listing is the partner of one of the first when its name is equal after the template arguments the first does not have --
trailing defaulted ones -- are taken off (`f<false, 64>` pairs with `f<false, 64, false>`; `f<false, 64, true>` has no partner
and is listed as new).  Of each pair it compares the code, the kernel descriptor (.amdhsa_ block) and the metadata entry with the
kernel's own symbol replaced by a placeholder and function-local label numbers dropped, and prints a unified diff where they differ.
Every argument is a substring a demangled name must contain to be looked at (none: all kernels).
Exit status 0: every selected pair identical; 1: a pair differs or a selected kernel of the first listing has no partner.
"""
import difflib
import re
import shutil
import subprocess
import sys

import listing_diff as LD


def demangle(symbols):
    out = subprocess.run([shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "c++filt"], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout
    return dict(zip(symbols, out.splitlines()))


def template_args(name):
    """'void f<a, g<b, c>, d>(int)' -> ('void f', ['a', 'g<b, c>', 'd']) for the FIRST template argument list"""
    lt = name.index("<")
    depth, args, cur = 0, [], ""
    for i in range(lt, len(name)):
        ch = name[i]
        if ch in "<(":
            depth += 1
            if depth == 1:
                continue
        elif ch in ">)":
            depth -= 1
            if depth == 0:
                args.append(cur.strip())
                return name[:lt], args
        if ch == "," and depth == 1:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    raise ValueError(name)


SYMBOL_COMMENT = re.compile(r" ?; %\S+")       # a label's comment: the IR block's name (a counter, or the symbol of an inlined function)
LOOP_COMMENT = re.compile(r"\bBB\d+_")          # "Child Loop BB17_22": the function's number in a loop comment
DEFAULTS = ("false", "")          # what a trailing argument the parent does not have may be: an off switch, an empty pack


def blocks(path):
    kernels, _, _, entries = LD.parse(path)
    names = demangle(list(kernels))
    out = {}
    for sym, text in kernels.items():
        body = [l.replace(sym, "<kernel>") for l in text + entries.get(sym, [])]
        out[names[sym]] = [l for l in body if ".symbol:" not in l and ".name:" not in l and "; -- Begin function" not in l]
    return out


def partner(name, candidates):
    if "<" not in name:
        return name if name in candidates else None
    base, args = template_args(name)
    for c in candidates:
        if "<" not in c:
            continue
        cb, ca = template_args(c)
        if cb == base and ca[:len(args)] == args and all(a in DEFAULTS for a in ca[len(args):]):
            return c
    return None


def main(a, b, picks):
    ka, kb = blocks(a), blocks(b)
    rc, paired = 0, set()
    for name in sorted(ka):
        if picks and not any(p in name for p in picks):
            continue
        p = partner(name, kb)
        if p is None:
            print("NO PARTNER  " + name)
            rc = 1
            continue
        paired.add(p)
        ta, tb = ([LOOP_COMMENT.sub("BB_", SYMBOL_COMMENT.sub("", l)) for l in k] for k in (ka[name], kb[p]))
        if ta == tb:
            print("identical   %s  (%d lines)\n         == %s" % (name, len(ta), p))
        else:
            rc = 1
            print("DIFFERENT   %s\n         != %s" % (name, p))
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(ta, tb, "first", "second", lineterm="", n=2))
    for name in sorted(kb):
        if name not in paired and (not picks or any(p in name for p in picks)):
            print("new         " + name)
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
