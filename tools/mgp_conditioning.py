"""Conditioning of the multi-process reference fixtures (tests/golden/mgp_ref_*.npz): the share
of the recorded hyper-likelihood points at which the reference's own fp64 value lies within
1e-10 (relative) of the long-double value oracle.gibbs_oracle.lnlike_marginal_extended.  A
fixture is committed only when that share is at least 90%: the long-double arbitration of the
GPU likelihood tests may then decide at most the remaining tenth.

    python tools/mgp_conditioning.py [fixture names]
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_io import MGP_NAMES as NAMES, load_ref, sweep_state  # noqa: E402
from oracle.gibbs_oracle import ChainState, lnlike_marginal_extended  # noqa: E402

RTOL = 1e-10


def share(name):
    ref = load_ref(name)
    t = ref["tape"]
    S = int(ref["niter"])
    ok = n = 0
    worst = 0.0
    for i in range(S):
        s = sweep_state(ref, i)
        st = ChainState(b=s["b"], z=s["z"], alpha=s["alpha"], pout=s["pout"], theta=s["theta"],
                        nu=s["nu"])
        for x, want in zip(t["hyper_lnl_x"][i], t["hyper_lnl"][i]):
            if not np.isfinite(want):
                continue
            ext = lnlike_marginal_extended(ref["pta"], st, x)
            r = abs(want - ext) / max(abs(ext), 1e-300)
            worst = max(worst, r)
            ok += r <= RTOL
            n += 1
    return ok / n, n, worst, float(np.nanmax(t["b_cond"]))


def main():
    bad = 0
    for name in sys.argv[1:] or NAMES:
        sh, n, worst, cond = share(name)
        print(f"{name}: {100 * sh:.1f}% of {n} points within {RTOL:g}, worst {worst:.2e}, "
              f"max cond(Sigma) at a b draw {cond:.2e}")
        bad += sh < 0.9
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
