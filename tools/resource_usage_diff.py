#!/usr/bin/env python
"""Compare the kernels' resource usage of two builds.

Build each tree with GST_EXTRA_CFLAGS="-Rpass-analysis=kernel-resource-usage", keep the
compiler's stderr, and give the two logs:

    python tools/resource_usage_diff.py parent.log new.log [--json out.json]

Kernels are keyed by their mangled name.  The sweep kernel's instances that keep the posterior
sums (template parameter ACC, the last bool of gst_sweep_kernel<...>) and lg_accum are listed
with their deltas; every other kernel must be identical, else the exit status is 1.
"""
from __future__ import annotations

import json
import re
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
          "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1)
        if body.startswith("Function Name:"):
            cur = out.setdefault(body.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in body:
            k, v = body.rsplit(":", 1)
            if k.strip() in FIELDS:
                cur[k.strip()] = int(v)
    return out


def accumulating(name):
    """The kernels that read the accumulator descriptor."""
    if "lg_accum" in name or "set_accum_kernel" in name:
        return True
    m = re.search(r"gst_sweep_kernelI((?:L[ib]\d+E)+)E", name)
    return bool(m) and m.group(1).endswith("Lb1E") and len(re.findall(r"L[ib]\d+E", m.group(1))) == 10


def main(argv):
    a, b = parse(argv[1]), parse(argv[2])
    changed, acc_rows = [], []
    for name in sorted(set(a) | set(b)):
        ra, rb = a.get(name), b.get(name)
        if accumulating(name):
            if ra != rb:
                acc_rows.append({"kernel": name, "parent": ra, "new": rb})
        elif ra != rb:
            changed.append({"kernel": name, "parent": ra, "new": rb})
    nacc = sum(accumulating(n) for n in b)
    print(f"{len(b)} kernels, {nacc} accumulating; other kernels changed: {len(changed)}; "
          f"accumulating kernels changed: {len(acc_rows)}")
    for row in changed:
        print("CHANGED", row["kernel"], row["parent"], "->", row["new"])
    for row in acc_rows:
        pa, nw = row["parent"] or {}, row["new"] or {}
        d = {k: (pa.get(k), nw.get(k)) for k in FIELDS if pa.get(k) != nw.get(k)}
        print("acc", row["kernel"], d)
    if "--json" in argv:
        with open(argv[argv.index("--json") + 1], "w") as f:
            json.dump({"kernels": len(b), "accumulating": nacc, "other_changed": changed,
                       "accumulating_changed": acc_rows}, f, indent=1)
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
