"""Kernel-by-kernel comparison of the gfx950 device code of two builds of libf110qp.so.
Run:  python tools/isa_identity.py PARENT/libf110qp.so BRANCH/libf110qp.so [MORE PAIRS ...] > table.txt
Every code object of each library is extracted (llvm-objdump --offloading) and, per kernel symbol,
its code bytes, the registers, spills, scratch and static LDS of its metadata and a hash of its
instruction text (llvm-objdump -d, addresses and encodings dropped) are printed, parent and branch
side by side. Exit status 1 if the kernel names differ or any kernel differs in any column."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
META = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size"]
HEAD = ["bytes", "vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds", "sha1[:12]"]


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def kernels(lib):
    """{kernel name: (code bytes, the META figures ..., hash of the instruction text)}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        run(f"{LLVM}/llvm-objdump", "--offloading", "lib.so", cwd=tmp)
        for co in sorted(f for f in os.listdir(tmp) if "gfx950" in f):
            co = os.path.join(tmp, co)
            meta, ent = {}, None
            for line in run(f"{LLVM}/llvm-readelf", "--notes", co).split("\n"):
                if line.startswith("  - .agpr_count"):
                    ent = {}
                m = re.match(r"\s+(?:- )?\.(\w+):\s*(\S+)$", line)
                if m and ent is not None and (m.group(1) in META or m.group(1) == "name"):
                    if m.group(1) == "name":
                        meta[m.group(2)] = ent
                    else:
                        ent[m.group(1)] = int(m.group(2))
            size = {}
            for line in run(f"{LLVM}/llvm-readelf", "-sW", co).split("\n"):
                f = line.split()
                if len(f) == 8 and f[3] == "FUNC":
                    size[f[7]] = int(f[2])
            name, text = None, {}
            for line in run(f"{LLVM}/llvm-objdump", "-d", co).split("\n"):
                m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
                if m:
                    name = m.group(1)
                    text[name] = []
                elif name and line.startswith("\t"):
                    text[name].append(line.split("//")[0].strip())
            for k, ent in meta.items():
                h = hashlib.sha1("\n".join(text[k]).encode()).hexdigest()[:12]
                assert k not in out, k
                out[k] = tuple([size[k]] + [ent[f] for f in META] + [h])
    return out


bad = 0
pairs = sys.argv[1:]
for parent, branch in zip(pairs[0::2], pairs[1::2]):
    kp, kb = kernels(parent), kernels(branch)
    print(f"# parent {parent}\n# branch {branch}")
    print(f"# {len(kp)} kernels in the parent, {len(kb)} in the branch; names equal: {sorted(kp) == sorted(kb)}")
    print("# kernel | " + " ".join(HEAD) + " (parent) | the same (branch) | verdict")
    same = 0
    for k in sorted(set(kp) | set(kb)):
        a, b = kp.get(k), kb.get(k)
        ok = a is not None and a == b
        same += ok
        fmt = lambda t: " ".join(str(x) for x in t) if t else "missing"
        print(f"{k} | {fmt(a)} | {fmt(b)} | {'identical' if ok else 'DIFFERENT'}")
    print(f"# identical: {same} of {len(set(kp) | set(kb))}\n")
    bad += same != len(set(kp) | set(kb))
sys.exit(1 if bad else 0)
