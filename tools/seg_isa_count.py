"""Instruction counts of a segmented lane kernel's pass loop, from the compiler's assembly.
Run:  hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -If110-mpc_amd/csrc -DF110QP_SEG_SCR=0 \
            -S --cuda-device-only f110-mpc_amd/csrc/lane_seg_inst.hip -o seg.s
      python tools/seg_isa_count.py seg.s [TEMPLATE_ARGS ...]
TEMPLATE_ARGS: the mangled template arguments that pick the kernels (default: the four Q = 5 ones and
the Q = 0 S = 4 kernels; `lane_seg_kernel_qILi4ELb1EfLi5E` is C2's twin kernel). Per kernel: the
registers, spills and scratch of its metadata, then every basic block of the pass loop (the kernel's
depth-1 loop) with more than 40 instructions: its instruction count and the count per class. In the
Q = 5 kernels the largest block is the backward sweep with the segment ends, the next two are the two
copies of the forward sweep: the larger one the single-flip copy, the smaller one the PDAS copy."""
import collections
import re
import sys

path = sys.argv[1]
picks = sys.argv[2:] or ["EfLi5E", "EdLi5E", "ILi4ELb1ELb1EdLb0ELb1ELb1EfLi0E", "ILi4ELb1ELb1EdLb0ELb0ELb1EfLi0E"]

CLASSES = [
    ("fp64 fma/fmac", r"v_fmac?_f64"), ("fp64 mul", r"v_mul_f64"), ("fp64 add", r"v_add_f64"),
    ("fp64 rcp", r"v_rcp_f64"), ("fp64 cmp", r"v_cmpx?_\w+_f64"), ("cndmask", r"v_cndmask"),
    ("dpp move", r"v_mov_b32_dpp"), ("accvgpr", r"v_accvgpr"), ("v_mov", r"v_mov_b"),
    ("other VALU", r"v_"), ("ds", r"ds_"), ("waitcnt", r"s_waitcnt"), ("SALU", r"s_"),
]


def classify(op):
    for name, pat in CLASSES:
        if re.match(pat, op):
            return name
    return "other"


lines = open(path).read().split("\n")
# the code-object metadata (amdhsa.kernels): one entry per kernel, opened by its .agpr_count line
META, ent = {}, None
for l in lines:
    if l.startswith("  - .agpr_count"):
        ent = {}
    m = re.match(r"\s+(?:- )?\.(agpr_count|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|name):\s*(\S+)", l)
    if m and ent is not None:
        if m.group(1) == "name":
            META[m.group(2)] = ent
        else:
            ent[m.group(1)] = int(m.group(2))
starts = [i for i, l in enumerate(lines) if re.match(r"_ZN6f110qp\d+lane_seg_kernel\w+:", l)]
for s in starts:
    name = lines[s].split(":")[0]
    if not any(p in name for p in picks):
        continue
    e = next(i for i in range(s, len(lines)) if "-- End function" in lines[i])
    meta = META.get(name, {})
    body = lines[s + 1:e + 1]
    total = sum(1 for l in body if re.match(r"\t[a-z]", l) and not l.startswith("\t."))
    print(name)
    print("  instructions", total, " ".join(f"{k}={v}" for k, v in meta.items()))
    # basic blocks: split at labels and after branches
    blocks, cur, in_loop = [], [], False
    for l in body:
        is_label = l.startswith(".LBB")
        is_inst = bool(re.match(r"\t[a-z]", l)) and not l.startswith("\t.")
        if is_label:
            if cur:
                blocks.append((in_loop, cur))
            cur = []
            in_loop = "Depth=1" in l
        elif is_inst:
            op = l.split()[0]
            cur.append(op)
            if op.startswith("s_cbranch") or op.startswith("s_branch"):
                blocks.append((in_loop, cur))
                cur = []
    if cur:
        blocks.append((in_loop, cur))
    loop_total = 0
    for in_loop, ops in blocks:
        if not in_loop:
            continue
        loop_total += len(ops)
        if len(ops) > 40:
            c = collections.Counter(classify(o) for o in ops)
            print(f"  loop block {len(ops):5d}: " + ", ".join(f"{k} {c[k]}" for k, _ in CLASSES if c[k]))
    print("  pass loop, all blocks:", loop_total)
