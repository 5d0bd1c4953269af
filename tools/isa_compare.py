#!/usr/bin/env python3
"""isa_compare.py OLD_CSRC NEW_CSRC -- did a change to csrc/ change any device code?  Needs hipcc, no GPU.

Every .hip of both trees is compiled for the device only with its own Makefile's flags (hipcc $(CXXFLAGS) --offload-device-only
-S), the lines naming the per-compile __hip_cuid_ symbol are dropped, the per-file numbering of local labels is taken out (in the
loop comments too) and the text is cut per symbol: a function's instruction
stream (label .. .Lfunc_end, with its .amdhsa_kernel block) and its entry in the .amdgpu_metadata note.  What is left over (LDS
and constant symbols, file-scope directives) is compared as one more piece per file.  Prints every kernel that differs; exit
status 1 if any does or if the sets of symbols differ."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LOCAL = re.compile(r"(\.L(?:BB|func_end|func_begin|tmp|JTI)|\bBB)\d+")   # local labels, and the loop comments naming them, carry the function's index in its file


def make_var(mk, name):
    return re.search(rf"^{name}\s*\??=\s*(.*)$", mk, re.M).group(1).strip()


def device_asm(csrc, hip, out):
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = make_var(mk, "CXXFLAGS").replace("$(ARCH)", make_var(mk, "ARCH")).split()
    r = subprocess.run([make_var(mk, "HIPCC"), *flags, "--offload-device-only", "-S", hip, "-o", out], cwd=csrc,
                       capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{csrc}/{hip}: {r.stderr[-2000:]}")
    # (the comment column after a label moves with the number of digits taken out of it)
    return [re.sub(r"[ \t]+;", " ;", LOCAL.sub(lambda m: m.group(1), l)) for l in open(out) if "__hip_cuid_" not in l]


def pieces(lines, hip):
    """{symbol: text} of one file: code (+ .amdhsa block) and metadata entry per function, the rest under '<file scope>'."""
    out, rest, cur, i = {}, [], None, 0
    while i < len(lines):
        l = lines[i]
        m = re.match(r"([A-Za-z_$][\w$.]*):", l)
        if cur is None and m and not l.startswith(".L") and i and "@function" in "".join(lines[max(0, i - 4):i]):
            cur = m.group(1)
            out[cur] = []
        (rest if cur is None else out[cur]).append(l)
        if cur and l.startswith(".Lfunc_end"):
            j = i + 1                                      # a kernel's descriptor follows its code
            while j < len(lines) and not re.match(r"\s*\.(amdhsa_kernel|type|globl|protected|amdgpu_metadata)\b", lines[j]):
                j += 1
            if j < len(lines) and ".amdhsa_kernel" in lines[j]:
                while ".end_amdhsa_kernel" not in lines[i]:
                    i += 1
                    out[cur].append(lines[i])
            cur = None
        i += 1
    text = "".join(rest)
    meta = re.search(r"amdhsa\.kernels:\n(.*?)(?=^amdhsa\.|\Z)", text, re.M | re.S)
    for entry in re.split(r"(?m)^  - ", meta.group(1))[1:] if meta else []:
        out[re.search(r"\.name:\s*(\S+)", entry).group(1)].append(entry)
    out[f"<file scope of {hip}>"] = [text.replace(meta.group(1), "") if meta else text]
    return {k: "".join(v) for k, v in out.items()}


def main(old, new):
    hips = sorted(f for f in os.listdir(old) if f.endswith(".hip") and os.path.exists(os.path.join(new, f)))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        jobs = [(t, h, pool.submit(device_asm, d, h, os.path.join(tmp, f"{t}_{h}.s"))) for h in hips for t, d in (("a", old), ("b", new))]
        asm = {(t, h): pieces(j.result(), h) for t, h, j in jobs}
    differ, kernels = [], 0
    for h in hips:
        a, b = asm["a", h], asm["b", h]
        kernels += sum(".amdhsa_kernel" in v for v in b.values())
        differ += [f"{h}: {k}: only in {'old' if k in a else 'new'}" for k in sorted(a.keys() ^ b.keys())]
        differ += [f"{h}: {k}: differs" for k in sorted(a.keys() & b.keys()) if a[k] != b[k]]
    print("\n".join(differ + [f"isa_compare: {len(hips)} files, {kernels} kernels, {len(differ)} differing symbols"]))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
