#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of libfpc.so.

    python profiles/compare_code_objects.py PARENT/libfpc.so RESULT/libfpc.so > profiles/<name>.txt

For a host-only change the device code must not move.  Each library's code object is extracted with
`llvm-objdump --offloading`; the report gives the sha256 of both, and, where they are not byte-identical, shows that
only the symbol table differs -- its order, and the name of the one symbol that carries a hash of the source:
  - the set of symbols is identical (but for that name);
  - every function symbol's machine code (the bytes its disassembly is made from) is identical;
  - every kernel's metadata from `llvm-readelf --notes` (registers, spills, LDS, scratch, arguments) is identical.
Exit status 0 if the device code is the same, 1 otherwise.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def extract(lib, tmp):
    d = tempfile.mkdtemp(dir=tmp)
    copy = os.path.join(d, "lib.so")
    shutil.copy(lib, copy)
    run(os.path.join(LLVM, "llvm-objdump"), "--offloading", copy, cwd=d)
    (co,) = [os.path.join(d, f) for f in os.listdir(d) if "gfx950" in f]
    return co


def sections(co):
    out = {}
    for m in re.finditer(r"^\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", run(os.path.join(LLVM, "llvm-readelf"), "-S", "-W", co), re.M):
        out[m.group(1)] = (int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16))   # address, file offset, size
    return out


def symbols(co):
    syms = {}
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[0].rstrip(":").isdigit() and f[6] != "UND":
            # (__hip_cuid_<hash> names the translation unit by a hash of its source: one per build, never the same)
            syms[re.sub(r"^__hip_cuid_[0-9a-f]+$", "__hip_cuid_<source hash>", f[7])] = (int(f[1], 16), int(f[2]), f[3])   # value, size, type
    return syms


def kernel_metadata(co):
    """The .name -> text of every kernel's entry in the AMDGPU metadata note."""
    text = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    body = text[text.index("amdhsa.kernels:"):]
    body = body[:body.index("amdhsa.target:")] if "amdhsa.target:" in body else body
    out = {}
    for entry in re.split(r"^  - ", body, flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M).group(1)
        out[name] = entry
    return out


def main(parent_lib, result_lib):
    tmp = tempfile.mkdtemp()
    same = True
    try:
        cos = [extract(parent_lib, tmp), extract(result_lib, tmp)]
        blobs = [open(c, "rb").read() for c in cos]
        shas = [hashlib.sha256(b).hexdigest() for b in blobs]
        print(f"parent code object: {len(blobs[0])} bytes, sha256 {shas[0]}")
        print(f"result code object: {len(blobs[1])} bytes, sha256 {shas[1]}")
        if shas[0] == shas[1]:
            print("byte-identical")
            return 0
        secs = [sections(c) for c in cos]
        for name in (".text", ".rodata", ".note"):
            b = [blob[s[name][1]:s[name][1] + s[name][2]] for blob, s in zip(blobs, secs)]
            eq = b[0] == b[1]
            same &= eq
            print(f"section {name}: {len(b[0])} / {len(b[1])} bytes, sha256 {hashlib.sha256(b[0]).hexdigest()} / "
                  f"{hashlib.sha256(b[1]).hexdigest()}: {'identical' if eq else 'DIFFERENT'}")
        syms = [symbols(c) for c in cos]
        only = [sorted(set(syms[0]) - set(syms[1])), sorted(set(syms[1]) - set(syms[0]))]
        same &= not only[0] and not only[1]
        print(f"symbols: {len(syms[0])} / {len(syms[1])}; only in parent {only[0]}; only in result {only[1]}")
        order = [sorted(s, key=lambda n: s[n][0]) for s in syms]
        print(f"symbol table order: {'same' if list(syms[0]) == list(syms[1]) else 'differs'}; "
              f"order by address: {'same' if order[0] == order[1] else 'differs'}")
        ncode = bad_code = 0
        for name in sorted(set(syms[0]) & set(syms[1])):
            (v0, n0, t0), (v1, n1, t1) = syms[0][name], syms[1][name]
            if t0 != "FUNC":
                continue
            ncode += 1
            t = [s[".text"] for s in secs]
            c0 = blobs[0][t[0][1] + v0 - t[0][0]:][:n0]
            c1 = blobs[1][t[1][1] + v1 - t[1][0]:][:n1]
            if c0 != c1 or n0 != n1:
                bad_code += 1
                print(f"  machine code DIFFERS: {name} ({n0} / {n1} bytes)")
        same &= bad_code == 0
        print(f"function symbols with identical machine code: {ncode - bad_code} of {ncode}")
        meta = [kernel_metadata(c) for c in cos]
        bad_meta = [n for n in sorted(set(meta[0]) | set(meta[1])) if meta[0].get(n) != meta[1].get(n)]
        same &= not bad_meta
        print(f"kernels with identical metadata (registers, spills, LDS, scratch, arguments): "
              f"{len(meta[0]) - len(bad_meta)} of {len(meta[0])}" + (f"; DIFFERENT: {bad_meta}" if bad_meta else ""))
        for key in (".sgpr_count", ".vgpr_count", ".agpr_count", ".sgpr_spill_count", ".vgpr_spill_count",
                    ".group_segment_fixed_size", ".private_segment_fixed_size"):
            tot = [sum(int(m.group(1)) for e in mm.values() for m in re.finditer(rf"{re.escape(key)}:\s+(\d+)", e)) for mm in meta]
            print(f"  sum of {key} over all kernels: {tot[0]} / {tot[1]}")
        print("RESULT: " + ("same device code; only the symbol table differs (order, source-hash name)" if same else "DEVICE CODE DIFFERS"))
        return 0 if same else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
