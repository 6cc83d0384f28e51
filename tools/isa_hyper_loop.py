"""The serial waits of the hyper MH step loop, read from AMDGPU assembly.

    hipcc --offload-arch=gfx950 -O3 ... --cuda-device-only -S csrc/gst_inst.hip \
        -DGST_SHAPE=10,3,2,76,0 -o inst.s
    python tools/isa_hyper_loop.py inst.s --kernel "gst_sweep_kernel<10, 3, 2, 76, false, 4, 2, false, false, false>"

The step loop is found as the loop of the kernel with the most ds_write_b128 (the column
publications of the elimination that is inlined in it); --loop BBn_m names another one by its header.  The compiler's
own block annotations ("in Loop: Header=BBn_m") say which blocks belong to it.  Listed, with the
line of the kernel's text (1 = the kernel's label):

    scratch   vector scratch loads (register reloads), and which of them are waited for alone
    branches  s_cbranch_* instructions: on the exec mask (a lane-divergent region) or on a
              scalar condition; those that leave the loop or close it are marked
    single    s_waitcnt vmcnt(0) / lgkmcnt(0) that follow exactly one load on that counter
              since the counter was last waited for: a round trip with nothing else in flight
    bpermute  ds_bpermute_b32 (chol_harvest's lane permutes)
    readlane  v_readlane_b32 from the SGPR-spill registers (those the kernel v_writelane's)

and the kernel's VGPR / AGPR / scratch figures.
"""
import argparse
import re
import sys

from isa_load_runs import AMDHSA, demangle

LABEL = re.compile(r"^([.\w$]+):")
INLOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
HEADER = re.compile(r"Loop Header: Depth=(\d+)")
VMEM = re.compile(r"^\s+(global_load|flat_load|buffer_load|scratch_load)_\w+")
LGKM = re.compile(r"^\s+(ds_read|ds_bpermute|s_load|s_buffer_load|s_memtime)\w*")
FMA = re.compile(r"^\s+v_(fma|fmac)_f64")
PUB = re.compile(r"^\s+ds_write_b128")
CNT = {"vm": re.compile(r"vmcnt\((\d+)\)"), "lgkm": re.compile(r"lgkmcnt\((\d+)\)")}


def kernels(path):
    """{kernel label: [its lines]} and {kernel label: {.amdhsa figure: value}}."""
    text, res, cur, name = {}, {}, None, None
    for s in open(path):
        m = LABEL.match(s)
        if m and not m.group(1).startswith((".L", "__")):
            cur = text.setdefault(m.group(1), [])
        elif m and m.group(1).startswith(".Lfunc_end"):
            cur = None
        if s.startswith("\t.amdhsa_kernel "):
            name = s.split()[1]
        a = AMDHSA.match(s)
        if a and name:
            res.setdefault(name, {})[a.group(1)] = int(a.group(2))
        if cur is not None:
            cur.append(s.rstrip("\n"))
    return text, res


def blocks(lines):
    """[(first line index, label or None, header of the innermost loop it is in or None)]."""
    out = []
    for i, s in enumerate(lines):
        m = LABEL.match(s)
        bb = re.match(r"^; %bb\.\d+:", s)
        if not (m or bb):
            continue
        lab = m.group(1) if m else None
        # the annotation sits on the label's line or the comment lines right under it
        loop, j = None, i
        while j < len(lines) and (j == i or lines[j].lstrip().startswith(";")):
            h = HEADER.search(lines[j])
            n = INLOOP.search(lines[j])
            if h and lab and "Parent" not in lines[j]:
                loop = lab.lstrip(".L")
                break
            if n and "Parent" not in lines[j]:
                loop = n.group(1)
            j += 1
        out.append((i, lab, loop))
    return out


def loop_lines(lines, bl, header):
    """Line indices of the blocks of loop `header` (its inner loops' blocks excluded)."""
    idx = []
    for k, (i, lab, loop) in enumerate(bl):
        end = bl[k + 1][0] if k + 1 < len(bl) else len(lines)
        if loop == header:
            idx.extend(range(i, end))
    return idx


def report(lines, header, out):
    bl = blocks(lines)
    idx = loop_lines(lines, bl, header)
    inside = {lab for i, lab, loop in bl if loop == header and lab}
    spill = {m.group(1) for s in lines for m in [re.match(r"^\s+v_writelane_b32 (v\d+),", s)] if m}
    pend = {"vm": 0, "lgkm": 0}       # loads issued since the counter's last wait
    last = {"vm": None, "lgkm": None}
    rows = {"scratch": [], "branches": [], "single": [], "bpermute": [], "readlane": []}
    prev = None
    for i in idx:
        if prev is not None and i != prev + 1:   # a block from elsewhere lies between
            pend = {"vm": 0, "lgkm": 0}
        prev = i
        s = lines[i]
        op = s.split()[0] if s.split() else ""
        if VMEM.match(s):
            pend["vm"] += 1
            last["vm"] = i
            if op.startswith("scratch_load"):
                rows["scratch"].append([i, s.strip().split(";")[0].strip(), False])
        elif LGKM.match(s):
            pend["lgkm"] += 1
            last["lgkm"] = i
            if op == "ds_bpermute_b32":
                rows["bpermute"].append(i)
        elif op == "s_waitcnt":
            arg = s.split(";")[0]
            bare = re.fullmatch(r"\s*s_waitcnt\s+(0x[0-9a-f]+|\d+)\s*", arg)
            for c, rx in CNT.items():
                m = rx.search(arg)
                if not (m or bare):
                    continue
                if (bare or int(m.group(1)) == 0) and pend[c] == 1:
                    ld = lines[last[c]].strip().split(";")[0].strip()
                    rows["single"].append((i, c, i - last[c] - 1, ld))
                    for r in rows["scratch"]:
                        if r[0] == last[c]:
                            r[2] = True
                pend[c] = 0
        elif op.startswith("s_cbranch"):
            tgt = s.split()[1]
            kind = "exec" if "exec" in op else "scalar"
            where = "closes the loop" if tgt.lstrip(".L") == header else \
                ("inside" if tgt in inside else "leaves the loop")
            rows["branches"].append((i, op, tgt, kind, where))
        elif op == "v_readlane_b32":
            src = s.split()[2].rstrip(",")
            if src in spill:
                rows["readlane"].append(i)
    w = out.write
    w(f"  step loop {header}: {len(idx)} lines, "
      f"{sum(1 for i in idx if FMA.match(lines[i]))} fp64 FMAs\n")
    w(f"  vector scratch loads: {len(rows['scratch'])}, "
      f"{sum(r[2] for r in rows['scratch'])} waited for alone\n")
    for i, t, alone in rows["scratch"]:
        w(f"    {i + 1:6d}  {t}{'   <- waited for alone' if alone else ''}\n")
    ex = [b for b in rows["branches"] if b[3] == "exec"]
    w(f"  branches: {len(rows['branches'])}, {len(ex)} on the exec mask "
      f"({sum(1 for b in ex if b[4] == 'inside')} of them inside the loop)\n")
    for i, op, tgt, kind, where in rows["branches"]:
        w(f"    {i + 1:6d}  {op:18s} {tgt:12s} {where}\n")
    w(f"  waits for a single load: {len(rows['single'])}\n")
    for i, c, gap, ld in rows["single"]:
        w(f"    {i + 1:6d}  {c}cnt(0), {gap} instructions after  {ld}\n")
    bp = rows["bpermute"]
    w(f"  ds_bpermute_b32: {len(bp)}" + (f" (lines {bp[0] + 1} .. {bp[-1] + 1})" if bp else "") + "\n")
    w(f"  v_readlane_b32 from spill registers ({', '.join(sorted(spill, key=lambda v: int(v[1:])))}): "
      f"{len(rows['readlane'])}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="", help="kernels whose demangled name contains this")
    ap.add_argument("--loop", default="", help="loop header (BBn_m); default: the most ds_write_b128")
    a = ap.parse_args()
    text, res = kernels(a.asm)
    names = demangle(list(text))
    for k, lines in text.items():
        nm = names[k].split("(")[0]
        if k not in res or a.kernel not in nm:
            continue
        r = res[k]
        tot = r.get("next_free_vgpr", 0)
        acc = r.get("accum_offset", tot)
        print(f"{nm}\n  VGPR {min(tot, acc)} AGPR {max(tot - acc, 0)} scratch "
              f"{r.get('private_segment_fixed_size', 0)} B")
        header = a.loop
        if not header:
            bl = blocks(lines)
            heads = {loop for _, _, loop in bl if loop}
            header = max(heads, key=lambda h: sum(1 for i in loop_lines(lines, bl, h)
                                                  if PUB.match(lines[i])), default="")
        if header:
            report(lines, header, sys.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
