"""Which VMEM loads of a kernel are waited for one by one?  Reads AMDGPU assembly.

    hipcc --offload-arch=gfx950 -O3 ... --cuda-device-only -S csrc/gst_inst.hip \
        -DGST_SHAPE=10,3,2,76,0 -o inst.s
    python tools/isa_load_runs.py inst.s [--min-loads N] [--kernel SUBSTRING]

Per kernel and basic block (a label up to the next label) it prints

    loads   VMEM loads in the block (global_load / flat_load / buffer_load)
    single  how many of them are followed by `s_waitcnt vmcnt(0)` with no other VMEM load
            in between: each such load is a memory round trip of its own
    ahead   loads issued before the block's first wait on the vector-memory counter
    x4      128-bit global loads (the low-rank Gram's flagged rows)
    flat    flat loads (a generic pointer: these also wait on the LDS counter)
    vdiv    v_div_* instructions (an IEEE division sequence)

and the kernel's registers and scratch from its .amdhsa directives.  Blocks with fewer than
--min-loads loads (default 2) are counted in the kernel's totals only.
"""
import argparse
import re
import shutil
import subprocess
import sys

LOAD = re.compile(r"^\s+(global_load|flat_load|buffer_load)_\w+")
WAIT = re.compile(r"^\s+s_waitcnt\b(.*)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
LABEL = re.compile(r"^([.\w$]+):")
AMDHSA = re.compile(r"^\s+\.amdhsa_(next_free_vgpr|accum_offset|private_segment_fixed_size)\s+(\d+)")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or \
        shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout
    got = out.splitlines()
    return dict(zip(names, got)) if len(got) == len(names) else {n: n for n in names}


class Block:
    def __init__(self, name):
        self.name = name
        self.loads = self.single = self.x4 = self.flat = self.vdiv = 0
        self.ahead = None          # loads before the first vmcnt wait (None: no wait yet)
        self.pending = False       # a load with no other load or vmcnt(0) wait after it yet

    def line(self, s):
        if LOAD.match(s):
            self.loads += 1
            self.pending = True
            op = s.split()[0]
            self.x4 += op == "global_load_dwordx4"
            self.flat += op.startswith("flat_load")
            return
        if s.lstrip().startswith("v_div_"):
            self.vdiv += 1
            return
        w = WAIT.match(s)
        if w:
            # `s_waitcnt vmcnt(N) ...`; a bare immediate (`s_waitcnt 0`) waits on every counter
            m = VMCNT.search(w.group(1))
            bare = re.fullmatch(r"\s*(0x[0-9a-f]+|\d+)\s*", w.group(1).split(";")[0])
            n = int(m.group(1)) if m else (0 if bare else None)
            if n is None:
                return
            if self.ahead is None:
                self.ahead = self.loads
            if n == 0 and self.pending:
                self.single += 1
                self.pending = False

    def first_wait(self):
        return self.loads if self.ahead is None else self.ahead


def parse(path):
    """[(kernel, {vgpr, agpr, scratch}, [Block])] of every kernel of the file."""
    kernels, cur, blocks, res = [], None, [], {}
    byname = {}
    for s in open(path):
        m = LABEL.match(s)
        if m:
            lab = m.group(1)
            if lab.startswith(".Lfunc_end"):
                if cur:
                    kernels.append((cur, blocks))
                cur, blocks = None, []
            elif lab.startswith(".L"):
                if cur:
                    blocks.append(Block(lab))
            elif not lab.startswith("__"):
                cur, blocks = lab, [Block("(entry)")]
            continue
        if s.startswith("\t.amdhsa_kernel "):
            res = byname.setdefault(s.split()[1], {})
            continue
        a = AMDHSA.match(s)
        if a:
            res[a.group(1)] = int(a.group(2))
            continue
        if cur and blocks:
            blocks[-1].line(s)
    out = []
    for name, bl in kernels:
        r = byname.get(name)
        if r is None:          # a device function, not a kernel
            continue
        tot = r.get("next_free_vgpr", 0)
        acc = r.get("accum_offset", tot)
        out.append((name, dict(vgpr=min(tot, acc), agpr=max(tot - acc, 0),
                               scratch=r.get("private_segment_fixed_size", 0)), bl))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm", nargs="+")
    ap.add_argument("--min-loads", type=int, default=2)
    ap.add_argument("--kernel", default="", help="only kernels whose demangled name contains this")
    a = ap.parse_args()
    for path in a.asm:
        ks = parse(path)
        names = demangle([k[0] for k in ks])
        print(f"== {path}")
        for name, r, blocks in ks:
            nm = names[name].split("(")[0]
            if a.kernel not in nm:
                continue
            loads = sum(b.loads for b in blocks)
            single = sum(b.single for b in blocks)
            print(f"{nm}\n  VGPR {r['vgpr']} AGPR {r['agpr']} scratch {r['scratch']} B; "
                  f"{len(blocks)} blocks, {loads} loads, {single} waited for singly")
            print(f"  {'block':<14s} {'loads':>5s} {'single':>6s} {'ahead':>5s} {'x4':>4s} "
                  f"{'flat':>4s} {'vdiv':>4s}")
            for b in blocks:
                if b.loads >= a.min_loads:
                    print(f"  {b.name:<14s} {b.loads:5d} {b.single:6d} {b.first_wait():5d} "
                          f"{b.x4:4d} {b.flat:4d} {b.vdiv:4d}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
