#!/usr/bin/env python3
"""Per-kernel comparison of two gfx950 assembly files of the same source at two commits.

    hipcc <the Makefile's flags> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage x.hip -o x.s 2> x.remarks
    tools/compare_kernel_isa.py before/x.s after/x.s [--rename 'regex=replacement' ...] [--remarks after/x.remarks]

Per kernel the text from its label to its end and its .amdhsa_kernel descriptor (registers, LDS, scratch) are compared after
stripping `;` comments and blank lines and renumbering `.L` local labels in order of appearance; the kernel's own mangled
name is replaced by a placeholder, so a kernel whose NAME changed (a template parameter or an argument type added) still
compares by its code.  --rename maps demangled names of the first file onto the second's.  sha1 = first 12 hex digits of
the normalised text.  With --remarks, the resource usage of the kernels that only the second file has is printed."""
import argparse
import hashlib
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def kernels(path):
    """{mangled name: normalised text of its code and descriptor}"""
    lines = open(path).read().splitlines()
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    res = {}
    for name in names:
        body, on = [], False
        for l in lines:
            if l.startswith(name + ":"):
                on = True
            if on:
                body.append(l)
                if l.strip().startswith(".Lfunc_end") or l.strip().startswith(".size\t" + name):
                    break
        desc, on = [], False
        for l in lines:
            if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$", l):
                on = True
            if on:
                desc.append(l)
                if l.strip() == ".end_amdhsa_kernel":
                    break
        text, labels = [], {}
        for l in body + desc:
            l = l.split(";")[0].rstrip()
            if not l.strip():
                continue
            l = l.replace(name, "<kernel>")
            l = re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), l)
            text.append(l)
        res[name] = "\n".join(text)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("--remarks")
    a = ap.parse_args()
    kb, ka = kernels(a.before), kernels(a.after)
    db, da = demangle(list(kb)), demangle(list(ka))
    renamed = {}
    for m, d in db.items():
        for r in a.rename:
            pat, rep = r.split("=", 1)
            d = re.sub(pat, rep, d)
        renamed[d] = m
    after_by_name = {d: m for m, d in da.items()}
    differ = 0
    for d in sorted(set(renamed) | set(after_by_name)):
        mb, ma = renamed.get(d), after_by_name.get(d)
        if mb and ma:
            same = kb[mb] == ka[ma]
            differ += not same
            sha = hashlib.sha1(ka[ma].encode()).hexdigest()[:12]
            was = "" if db[mb] == d else f"  [was {db[mb]}]"
            print(f"  {'identical' if same else 'DIFFERENT'}    {d}  ({ka[ma].count(chr(10)) + 1} lines, sha1 {sha}){was}")
        elif ma:
            print(f"  new          {d}")
        else:
            print(f"  parent only  {d}")
    if a.remarks:
        text = open(a.remarks).read()
        for d in sorted(set(after_by_name) - set(renamed)):
            m = re.search(r"Function Name: " + re.escape(after_by_name[d]) + r"\b(.*?)LDS Size \[bytes/block\]: (\d+)", text, re.S)
            if m:
                f = dict(re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", m.group(1)))
                print(f"  usage        {d}: " + " ".join(f"{k.replace(' ', '')}={v}" for k, v in f.items()) + f" LDS={m.group(2)}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
