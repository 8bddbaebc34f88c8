"""Scalar-register spill traffic of one kernel in a hipcc -S listing, per basic block (sibling of tools/isa_mix.py).

    tools/regcheck.sh                                  # -> /tmp/regcheck/one.s
    python tools/isa_spills.py /tmp/regcheck/one.s [kernel-name-substring] [min_spills]

A spilled SGPR lives in a lane of a VGPR: v_writelane_b32 parks it, v_readlane_b32 brings it back, both on the vector
pipe.  The table lists every block with at least `min_spills` (default 1) of them beside what places the block in the
kernel (its size and its LDS / float64 / Philox-multiply / memory instructions) and whether it is part of a loop (a
branch at most LOOP_SPAN blocks further down the listing jumps back to or above it: the kernel's long outer loops, which
hold nearly everything, are left out); the last lines are the totals and the metadata's own counts.
"""
import collections
import json
import re
import sys

LOOP_SPAN = 48


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "k_point_step"
    min_spills = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    lines = open(path).read().split("\n")
    start = max(i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(want) + r"\S*:", l))
    blocks, cur, label = [], [], "entry"
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\S+):", l)
        if m:
            blocks.append((label, cur))
            cur, label = [], m.group(1)
            continue
        t = l.split(";")[0].strip()
        if not t or t.startswith((".", "//")):
            continue
        cur.append(t)
    blocks.append((label, cur))
    index = {lab: i for i, (lab, _) in enumerate(blocks)}
    # block i is inside a loop if a later (or the same) block branches to a block at or above it
    in_loop = [False] * len(blocks)
    for i, (_, ins) in enumerate(blocks):
        for t in ins:
            if t.startswith(("s_cbranch", "s_branch")):
                tgt = index.get(t.split()[-1])
                if tgt is not None and tgt <= i and i - tgt <= LOOP_SPAN:
                    for k in range(tgt, i + 1):
                        in_loop[k] = True
    rows, tot = [], collections.Counter()
    for i, (lab, ins) in enumerate(blocks):
        c = collections.Counter({k: 0 for k in ("n", "valu", "readlane", "writelane", "lds", "f64", "mad_u64", "vmem")})
        for t in ins:
            op = t.split()[0]
            c["n"] += 1
            c["valu"] += op.startswith("v_")
            c["readlane"] += op == "v_readlane_b32"
            c["writelane"] += op == "v_writelane_b32"
            c["lds"] += op.startswith("ds_")
            c["f64"] += "_f64" in op and not op.startswith("v_cvt")
            c["mad_u64"] += op.startswith("v_mad_u64_u32")
            c["vmem"] += op.startswith(("global_", "buffer_", "flat_", "scratch_"))
        tot.update(c)
        if c["readlane"] + c["writelane"] >= min_spills:
            rows.append({"block": lab, "at": i, "loop": in_loop[i], **{k: int(v) for k, v in c.items()}})
    meta = {k: int(v) for k, v in re.findall(r"\.(sgpr_spill_count|vgpr_spill_count|sgpr_count|vgpr_count):\s+(\d+)",
                                             "\n".join(lines[start:]))[:4]}
    print(f"{'block':>12} {'loop':>4} {'instr':>6} {'valu':>5} {'rdlane':>6} {'wrlane':>6} {'lds':>4} {'f64':>4} {'mad64':>5} {'vmem':>4}")
    for r in rows:
        print(f"{r['block']:>12} {'L' if r['loop'] else '':>4} {r['n']:6d} {r['valu']:5d} {r['readlane']:6d} {r['writelane']:6d} "
              f"{r['lds']:4d} {r['f64']:4d} {r['mad_u64']:5d} {r['vmem']:4d}")
    loop_rd = sum(r["readlane"] for r in rows if r["loop"])
    loop_wr = sum(r["writelane"] for r in rows if r["loop"])
    print(f"total: {tot['n']} instructions, {tot['valu']} VALU, v_readlane {tot['readlane']} ({loop_rd} in loops), "
          f"v_writelane {tot['writelane']} ({loop_wr} in loops)")
    print("metadata:", meta)
    if len(sys.argv) > 4:
        json.dump({"kernel": want, "metadata": meta, "totals": {k: int(v) for k, v in tot.items()},
                   "readlane_in_loops": loop_rd, "writelane_in_loops": loop_wr, "blocks": rows}, open(sys.argv[4], "w"),
                  indent=1)


main()
