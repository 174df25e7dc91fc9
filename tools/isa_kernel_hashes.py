#!/usr/bin/env python3
"""Compare the device assembly of one translation unit before and after a change, file by file and kernel by kernel.

usage: tools/isa_kernel_hashes.py <parent.s> <new.s> [-v]
  both from  hipcc <the Makefile's CXXFLAGS> <the file's FLAGS_*> --cuda-device-only -S file.hip -o file.s

What is compared is the text without what cannot matter to the machine code: comment lines and trailing comments, .file / .ident / __hip_cuid_* lines, and the
numbering of local labels (.LBB<function>_<block>, .Lfunc_end<function>), which shifts when a change adds a kernel in front of the others.  A kernel's text is
its body up to .Lfunc_end plus its .amdhsa_kernel descriptor (registers, LDS, kernarg size).  A template parameter appended to k_mlp_small_mfma at its default
(a trailing Lb0E in the mangled name) is taken out of the new names, so that an instantiation is compared with the one it was before the parameter existed.
Prints the two file hashes, the counts, every kernel that differs or is new, and with -v the hash of every identical kernel."""
import hashlib
import re
import sys

APPENDED_DEFAULT = re.compile(r"(k_mlp_small_mfmaI(?:Li\d+E){4}(?:Lb[01]E){5})Lb0E(EEv)")


def clean(path):
    out = []
    for ln in open(path):
        t = ln.rstrip("\n")
        st = t.strip()
        if not st or st.startswith(";") or st.startswith(".file") or st.startswith(".ident") or "__hip_cuid" in st:
            continue
        t = APPENDED_DEFAULT.sub(r"\1\2", t)
        t = re.sub(r"\.LBB\d+_", ".LBB_", t)
        t = re.sub(r"\.Lfunc_(end|begin)\d+", r".Lfunc_\1", t)
        out.append(re.sub(r"\s*;.*$", "", t))
    return out


def sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def kernels(lines):
    desc, cur = {}, None
    for t in lines:
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", t)
        if m:
            cur = m.group(1)
            desc[cur] = []
        if cur is not None:
            desc[cur].append(t)
            if t.strip() == ".end_amdhsa_kernel":
                cur = None
    res, cur, buf = {}, None, []
    for t in lines:
        m = re.match(r"^(_Z\w+):", t)
        if m and cur is None:
            cur, buf = m.group(1), [t]
            continue
        if cur is not None:
            buf.append(t)
            if t.startswith(".Lfunc_end"):
                res[cur] = sha(buf + desc.get(cur, []))
                cur = None
    return res


if __name__ == "__main__":
    la, lb = clean(sys.argv[1]), clean(sys.argv[2])
    print("file", sha(la), sha(lb), "lines", len(la), len(lb))
    ka, kb = kernels(la), kernels(lb)
    same = [k for k in ka if kb.get(k) == ka[k]]
    diff = [k for k in ka if k in kb and kb[k] != ka[k]]
    print("kernels: parent", len(ka), "new", len(kb), "identical", len(same), "different", len(diff), "only in new", len([k for k in kb if k not in ka]),
          "only in parent", len([k for k in ka if k not in kb]))
    for k in diff:
        print("DIFFERENT", k, ka[k], kb[k])
    for k in ka:
        if k not in kb:
            print("GONE", k)
    for k in kb:
        if k not in ka:
            print("NEW", k, kb[k])
    if "-v" in sys.argv:
        for k in sorted(same):
            print("SAME", k, ka[k])
    sys.exit(1 if diff or any(k not in kb for k in ka) else 0)
