"""Per-kernel resources and code hashes of compiled objects, for "did the machine code change" checks.

usage: python tools/kernel_identity.py build/sampler.o build/sampler_split.o [...] > table.tsv
       python tools/kernel_identity.py --diff parent.tsv change.tsv

Each row: object, kernel (mangled), VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes, VGPR / SGPR spills,
code bytes, sha256 of the code bytes (first 16 hex digits). Read from the gfx950 code object's
metadata note and symbol table (llvm-readelf on the code object inside the offload bundle); no GPU needed.
--diff pairs kernels by name; streaming sampler kernels (sample_kernel<...>), whose template list
may differ between two trees, are paired by geometry instead: (policy, NT, NO, KSI, INJ, waves,
resident hidden k-steps, in/out layers resident).
"""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

import yaml

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
COLS = ["object", "kernel", "vgpr", "agpr", "sgpr", "lds", "scratch", "vgpr_spill", "sgpr_spill", "code_bytes", "sha"]


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def rows_of(obj, arch="gfx950"):
    # the object's .hip_fatbin section is an (uncompressed) offload bundle: magic, count, then
    # {offset, size, id length, id} per entry, offsets relative to the magic
    raw = open(obj, "rb").read()
    base = raw.find(b"__CLANG_OFFLOAD_BUNDLE__")
    if base < 0:
        raise SystemExit(f"{obj}: no offload bundle")
    n, = struct.unpack_from("<Q", raw, base + 24)
    p, blob = base + 32, None
    for _ in range(n):
        off, size, idl = struct.unpack_from("<QQQ", raw, p)
        if raw[p + 24:p + 24 + idl].decode().endswith(arch):
            blob = raw[base + off:base + off + size]
        p += 24 + idl
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "dev.co")
        open(co, "wb").write(blob)
        notes = run(f"{LLVM}/llvm-readelf", "--notes", co)
        meta = yaml.safe_load(notes[notes.index("---"):notes.rindex("...")])
        text = None
        for line in run(f"{LLVM}/llvm-readelf", "-S", "-W", co).splitlines():
            m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
            if m:
                text = (int(m.group(1), 16), int(m.group(2), 16))     # address, file offset
        syms = {}
        for line in run(f"{LLVM}/llvm-readelf", "-s", "-W", co).splitlines():
            f = line.split()
            if len(f) == 8 and f[3] == "FUNC":
                syms[f[7]] = (int(f[1], 16), int(f[2]))
    out = []
    for k in meta["amdhsa.kernels"]:
        addr, size = syms[k[".name"]]
        code = blob[text[1] + addr - text[0]:text[1] + addr - text[0] + size]
        out.append([os.path.basename(obj), k[".name"], k[".vgpr_count"], k.get(".agpr_count", 0), k[".sgpr_count"],
                    k[".group_segment_fixed_size"], k[".private_segment_fixed_size"], k.get(".vgpr_spill_count", 0),
                    k.get(".sgpr_spill_count", 0), size, hashlib.sha256(code).hexdigest()[:16]])
    return sorted(out, key=lambda r: r[1])


def stream_key(name):
    """sample_kernel<P, NT, NO, KSI, INJ, QD, SW, RK, (LK, RIO) | RES> -> its geometry."""
    m = re.match(r"_Z13sample_kernelI(\d+)(\w+?)((?:L[ib]\d+E)+)Ev", name)
    if not m:
        return None
    pol = m.group(2)[:int(m.group(1))]
    a = [int(x) for x in re.findall(r"L[ib](\d+)E", m.group(3))]
    nt, no, ksi, inj, _, sw, rk = a[:7]
    res = a[8] == 3 if len(a) == 9 else bool(a[7])      # old: LK, RIO mask; new: one bool
    return ("sample_kernel", pol, nt, no, ksi, inj, sw, rk, int(res))


def load(path):
    t = {}
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        if f[0] == "object" or len(f) != len(COLS):
            continue
        t[stream_key(f[1]) or f[1]] = f
    return t


def diff(pa, pb):
    a, b = load(pa), load(pb)
    bad = 0
    print(f"kernels: {len(a)} -> {len(b)}")
    for k in sorted(set(a) | set(b), key=str):
        if k not in a or k not in b:
            print(f"ONLY IN {'parent' if k in a else 'change'}: {k}")
            bad += 1
            continue
        ra, rb = a[k], b[k]
        res = [c for c in ("vgpr", "agpr", "sgpr", "lds", "scratch", "vgpr_spill", "sgpr_spill")
               if ra[COLS.index(c)] != rb[COLS.index(c)]]
        if res or ra[-1] != rb[-1]:
            print(f"DIFFERS {k}: " + ", ".join(f"{c} {ra[COLS.index(c)]} -> {rb[COLS.index(c)]}" for c in res) +
                  f" code {ra[-2]} B {ra[-1]} -> {rb[-2]} B {rb[-1]}" + (f"  (was in {ra[0]}, now {rb[0]})" if ra[0] != rb[0] else ""))
        if res:
            bad += 1
    same = sum(1 for k in a if k in b and a[k][2:] == b[k][2:])
    print(f"identical resources and code: {same} of {len(a)}")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
    print("\t".join(COLS))
    for obj in sys.argv[1:]:
        for r in rows_of(obj):
            print("\t".join(str(x) for x in r))
