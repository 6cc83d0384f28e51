"""Are two libgst builds' simulated datasets bitwise identical?  (tools/ab_bitwise.py for the
simulator, csrc/gst_sim.hpp.)

    python tools/sim_ab.py LIB_A LIB_B

Each library runs simulate_batch in its own process (GST_LIB): 16 datasets at 333 epochs, once
with Student-t and once with Gaussian white noise.
"""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
def worker(out):
    sys.path.insert(0, ROOT)
    from gibbs_student_t_amd.simulate import simulate_batch
    rng = np.random.default_rng(11)
    n = 333
    toas = np.sort(rng.uniform(0, 10 * 365.25 * 86400.0, n))
    M = np.stack([np.ones(n), toas / toas[-1], (toas / toas[-1]) ** 2], axis=1)
    res = {}
    for tag, kw in (("t", dict(dof=4.0)), ("g", dict(dof=None))):
        r = simulate_batch(toas, M, 16, seed=77, theta=0.08, log10_A=np.linspace(-15, -13, 16),
                           gamma=np.linspace(1, 6, 16), components=30, **kw)
        res.update({f"{tag}_{k}": v for k, v in r.items()})
    np.savez(out, **res)
if sys.argv[1] == "--worker":
    worker(sys.argv[2]); sys.exit(0)
with tempfile.TemporaryDirectory() as td:
    outs = []
    for lib in sys.argv[1:3]:
        o = os.path.join(td, os.path.basename(lib) + ".npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", o],
                       env=dict(os.environ, GST_LIB=os.path.abspath(lib)), check=True)
        outs.append(np.load(o))
    bad = [k for k in outs[0].files if not np.array_equal(outs[0][k], outs[1][k])]
    print("simulate:", "bitwise identical" if not bad else "DIFFER in " + ", ".join(bad), flush=True)
    sys.exit(1 if bad else 0)
