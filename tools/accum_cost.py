"""What the on-device posterior sums (gst_set_accum) cost, against recording the same arrays.

    python tools/accum_cost.py [--sweeps 200] [--out profiles/accum_cost.json]

Config 2 of bench.py (2048 chains of J1713+0747, the persistent kernel, two chains per SIMD)
and a J1643-sized synthetic pulsar (12,870 TOAs, tools/j1643_rate.py) on the large path, each
timed with device events after a warm-up launch:

    off         no accumulators, no records
    accum       all six accumulators set, no records
    accum_toa   sums + thresholds (K = 2) + band: the six, pout_gt at two thresholds and
                resid_sum / resid_sq (gst_set_accum_toa; skipped on a library without it)
    accum_block20 / accum_block60
                the six plus the block second moment of b (gst_set_accum_block) over the
                columns [0, 20) (a dm_gp-sized block) and [0, 60) (the whole Fourier block):
                2 * 8 * K (K + 1) / 2 more bytes per chain-sweep; skipped on a library
                without the entry point
    rec_every10 z / alpha / pout / b recorded every 10th sweep on the device
    rec_full    ... every sweep (the large-path run cut to the sweeps whose records fit)

GST_LIB=<another build's libgst.so> times that build with the same driver (a parent build for
comparison; --large-repeats 3 gives the large-path rows a spread to compare against;
--rows off accum ... times only those rows).

Records are timed on the device only: the copy to the host that Gibbs.sample adds is not in
these numbers.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

REC_KEYS = ("b", "z", "alpha", "pout")


TOA_THR = (0.5, 0.9)     # the accum_toa row's K = 2 thresholds


def has_toa(ns):
    """The library under test has gst_set_accum_toa (a parent build given by GST_LIB may not)"""
    return hasattr(ns.lib, "gst_set_accum_toa")


BLOCKS = {"accum_block20": (0, 20), "accum_block60": (0, 60)}
ROWS = ("off", "accum", "accum_toa") + tuple(BLOCKS) + ("rec_every10", "rec_full")


def has_block(ns):
    return hasattr(ns.lib, "gst_set_accum_block")


def timed(ns, S, *, accum=False, toa=False, block=None, record_every=0, seed=1, warm=8):
    """ms per sweep of one S-sweep launch (device events), after a warm-up launch."""
    import torch
    ns.sweep(warm, seed=seed)
    acc = rec = None
    if accum and toa:
        from gibbs_student_t_amd.native import ACCUM_KEYS, ACCUM_TOA_KEYS
        acc = ns.alloc_accum(ACCUM_KEYS + ACCUM_TOA_KEYS, pout_thresholds=TOA_THR)
        ns.set_accum(acc, from_sweep=warm, pout_thresholds=TOA_THR)
    elif accum and block:
        from gibbs_student_t_amd.native import ACCUM_KEYS
        acc = ns.alloc_accum(ACCUM_KEYS + ("b_outer",), b_block=block)
        ns.set_accum(acc, from_sweep=warm, b_block=block)
    elif accum:
        acc = ns.alloc_accum()
        ns.set_accum(acc, from_sweep=warm)
    if record_every:
        rec = ns.alloc_records((S + record_every - 1) // record_every, REC_KEYS)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ns.sweep(S, records=rec, record_every=max(record_every, 1), seed=seed, sweep0=warm)
    e1.record()
    e1.synchronize()
    if accum:
        ns.clear_accum()
        assert int(acc["count"].min()) == S == int(acc["count"].max())
    return e0.elapsed_time(e1) / S


def measure(make, S, S_full, repeats=3, rows=ROWS):
    out = {}
    for label, kw, sweeps in (("off", {}, S), ("accum", dict(accum=True), S),
                              ("accum_toa", dict(accum=True, toa=True), S),
                              *((k, dict(accum=True, block=v), S) for k, v in BLOCKS.items()),
                              ("rec_every10", dict(record_every=10), S),
                              ("rec_full", dict(record_every=1), S_full)):
        if label not in rows:
            continue
        ms = []
        for _ in range(repeats):
            ns = make()
            if (kw.get("toa") and not has_toa(ns)) or (kw.get("block") and not has_block(ns)):
                ns.close()
                break
            ms.append(timed(ns, sweeps, **kw))
            ns.close()
        if ms:
            out[label] = {"sweeps": sweeps, "ms_per_sweep": sorted(ms),
                          "median_ms_per_sweep": float(np.median(ms))}
    for label in ROWS[1:]:
        if label in out and "off" in out:
            out[label]["over_off"] = \
                out[label]["median_ms_per_sweep"] / out["off"]["median_ms_per_sweep"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--large-chains", type=int, default=1024)
    ap.add_argument("--large-full-sweeps", type=int, default=20,
                    help="sweeps of the large path's full-record run (316 KB per chain-sweep)")
    ap.add_argument("--large-repeats", type=int, default=1,
                    help="repeats of each large-path row (3: a spread to compare builds against)")
    ap.add_argument("--rows", nargs="+", default=list(ROWS), choices=ROWS,
                    help="the rows to time (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_cost.json"))
    a = ap.parse_args()
    import bench
    from gibbs_student_t_amd.native import NativeSampler
    from gibbs_student_t_amd.run_sims import MODELS
    from j1643_rate import j1643_like

    wl = bench.workload(2, 0, 1, None)

    def config2():
        ns = NativeSampler(wl["ptas"], wl["cfgs"], 0)
        ns.alloc(wl["C"], dataset=wl["ds"])
        ns.set_state(**wl["init"])
        return ns

    pta = j1643_like()
    C = a.large_chains
    lo = np.array([p.pmin for p in pta.params])
    hi = np.array([p.pmax for p in pta.params])
    x0 = np.random.default_rng(3).uniform(lo, hi, size=(C, len(lo)))

    def j1643():
        ns = NativeSampler(pta, MODELS["vvh17"], 0, path="large")
        ns.alloc(C)
        ns.set_state(x=x0, z=np.ones((C, ns.n)), alpha=np.full((C, ns.n), 1e10),
                     theta=np.full(C, 0.05), nu=np.full(C, 4.0))
        return ns

    res = {"sweeps": a.sweeps,
           "config2": dict(chains=wl["C"], n=int(wl["ptas"][0].n), path="persistent",
                           **measure(config2, a.sweeps, a.sweeps, rows=a.rows)),
           "j1643_like": dict(chains=C, n=int(pta.n), path="large",
                              **measure(j1643, a.sweeps, a.large_full_sweeps,
                                        repeats=a.large_repeats, rows=a.rows))}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
