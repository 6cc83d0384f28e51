"""What the GPU tests share.  Importing this module is the device gate: without torch or a HIP
device the import raises pytest's skip, which skips the importing test module at collection."""
from __future__ import annotations

import numpy as np
import pytest
import scipy.stats

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from gibbs_student_t_amd import _abi  # noqa: E402
from gibbs_student_t_amd.native import (ACCUM_KEYS, STATE_KEYS, NativeSampler,  # noqa: E402
                                        pack_tape)
from golden_io import load_ref  # noqa: E402
from support import SAME_START_P, batch_start_state, prior_box  # noqa: E402

SENTINEL = -7.25        # what the accumulator scaffold writes where no TOA is
PER_TOA_SUMS = ("z_sum", "pout_sum", "alpha_sum", "resid_sum", "resid_sq", "pout_gt")
ACCUM_SEED, ACCUM_SWEEP0 = 11, 3


def open_sampler(ref, C, path="auto", waves=None, dataset=None, skip_if_no_instance=False,
                 **debug):
    """NativeSampler of a fixture (a dict with "pta" and "kw", or a list of them: a dataset
    batch) with C chains allocated.  The debug flags, if any, are set before the chains are
    allocated, the waves after."""
    refs = ref if isinstance(ref, (list, tuple)) else None
    try:
        if refs is None:
            ns = NativeSampler(ref["pta"], ref["kw"], 0, path=path)
        else:
            ns = NativeSampler([r["pta"] for r in refs], [r["kw"] for r in refs], 0, path=path)
    except _abi.GstNativeError as e:
        # the persistent kernel's instances (gst_shapes.h) do not cover this model: its
        # parity runs on the large path only (test_general_white_noise_path_choice pins which)
        if skip_if_no_instance and path == "persistent" \
                and "no persistent-kernel instance" in str(e):
            pytest.skip("beyond the persistent kernel's shapes (large path only)")
        raise
    assert path == "auto" or ns.path == path
    if debug:
        ns.set_debug(**debug)
    ns.alloc(C, dataset=dataset)
    if waves is not None:
        ns.set_waves(waves)
    return ns


def upload_tape(ns, rows):
    """Packed tape rows [C, S, stride] as the device tensor ``sweep(tape=)`` takes"""
    return torch.as_tensor(rows).to(ns.tdev).contiguous()


def replay(ns, ref, S, keys=None):
    """S sweeps of chain 0 (C == 1) on the reference's tape from the state already set;
    the records as numpy arrays [S, ...]."""
    rows = pack_tape(ref["tape"], np.arange(S), ns.n, ns.m, ns.stride)
    rec = ns.alloc_records(S) if keys is None else ns.alloc_records(S, keys=keys)
    ns.sweep(S, records=rec, tape=upload_tape(ns, rows[None]))
    return {k: v.cpu().numpy()[0] for k, v in rec.items()}


def run_sweeps(ns, S, **sweep_kw):
    """S recorded sweeps from the state already set, then the sampler is closed: the final
    state and the records, as numpy arrays."""
    rec = ns.alloc_records(S)
    ns.sweep(S, records=rec, **sweep_kw)
    out = ns.get_state()
    recs = {k: v.cpu().numpy() for k, v in rec.items()}
    ns.close()
    return out, recs


def launch_records(ns, S, **sweep_kw):
    """One launch of S recorded sweeps from the state already set, then the sampler is closed:
    the records and a copy of the final state, as device tensors."""
    rec = ns.alloc_records(S)
    ns.sweep(S, records=rec, **sweep_kw)
    state = {k: v.clone() for k, v in ns.state.items()}
    ns.close()
    return rec, state


def single_sweep_differences(ns, rec, long_state, S, seed, sweep0):
    """S one-sweep launches from the state already set against one launch of S sweeps (its
    records and final state); closes the sampler.  The first (sweep, array) pairs that differ
    bitwise: the state entering sweep s must be record s of the long launch."""
    bad = []
    for s in range(S):
        bad += [(s, k) for k in STATE_KEYS if not torch.equal(ns.state[k], rec[k][:, s])]
        if bad:
            break
        ns.sweep(1, seed=seed, sweep0=sweep0 + s)
    if not bad:
        bad += [(S, k) for k in STATE_KEYS + ("status",)
                if not torch.equal(ns.state[k], long_state[k])]
    ns.close()
    return bad


def same_start_ks_failures(ns, pta, ref, C=4096, label=None):
    """The same-start law check against a ``samestart_*.npz`` run of the reference: its C0 starts
    plus fresh prior draws (C chains, all iid from the same start law) through ``ns`` (not yet
    allocated; closed here) from gibbs.py:29-51's latents; every sampled parameter, theta and
    nu at five sweeps and each chain's mean over the second half of the run against the
    reference's by two-sample KS.  Returns the series with p <= SAME_START_P; with ``label``
    every p-value is printed."""
    x0r, thin = ref["x0"], int(ref["thin"])
    R = ref["x"].shape[1]
    lo, hi = prior_box(pta)
    x0 = np.concatenate([x0r, np.random.default_rng(17).uniform(lo, hi,
                                                                 size=(C - len(x0r), len(lo)))])
    ns.alloc(C)
    ns.set_state(x=x0, z=np.ones((C, pta.n)), alpha=np.ones((C, pta.n)),
                 theta=np.full(C, 0.01), nu=np.full(C, 4.0))
    rec = ns.alloc_records(R, keys=("x", "theta", "nu"))
    ns.sweep(R * thin, records=rec, record_every=thin, seed=2024)
    assert np.all((ns.get_state()["status"] & _abi.STATUS_ERRORS) == 0)
    got = {k: v.cpu().numpy() for k, v in rec.items()}
    ns.close()
    names = [str(s) for s in ref["names"]]
    assert names == pta.param_names
    series = [(nm, got["x"][..., j], ref["x"][..., j]) for j, nm in enumerate(names)]
    series += [("theta", got["theta"], ref["theta"]), ("nu", got["nu"], ref["nu"])]
    points = sorted({1, R // 10, R // 4, R // 2, R - 1})
    assert len(points) == 5
    half = R // 2
    bad = []
    for nm, g, r in series:
        tests = [(f"{nm}@{t * thin}", g[:, t], r[:, t]) for t in points]
        tests.append((f"{nm} window mean", g[:, half:].mean(axis=1), r[:, half:].mean(axis=1)))
        for what, u, v in tests:
            p = scipy.stats.ks_2samp(u, v).pvalue
            if label:
                print(f"{label} {what}: p={p:.3g}")
            if p <= SAME_START_P:
                bad.append(f"{what}: p={p:.1e} gpu {u.mean():.4g} ref {v.mean():.4g}")
    return bad


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def builds():
    """build -> (chains, waves): one chain per SIMD (wpb 1 / OCC 1, C <= CUs), two waves per
    chain, and the two-chains-per-SIMD build (C > 4 x CUs picks OCC = 2 and the progress
    counter)"""
    return {"occ1": (96, 1), "pair": (96, 2), "occ2": (4 * ncu() + 64, 1)}


# ---- the posterior-sum scaffold of test_gpu_accum.py and test_gpu_accum_toa.py --------------------
def accum_sampler(names, per, path="auto", waves=None, poison=False):
    """The fixtures' sweep-0 states tiled over ``per`` chains each (x spread over the prior):
    the sampler, the fixtures and each chain's dataset."""
    refs = [load_ref(n) for n in names]
    ds_of = np.repeat(np.arange(len(refs)), per)
    if len(refs) == 1:
        ns = open_sampler(refs[0], per, path, waves)
    else:
        ns = open_sampler(refs, per * len(refs), path, waves, dataset=ds_of)
    if poison:
        ns.set_debug(poison=True)
    ns.set_state(**batch_start_state(refs, per, ns.n, x=lambda d: [5, d]))
    return ns, refs, ds_of


def accum_alloc(ns, n_of, keys, thr=None):
    acc = ns.alloc_accum(keys, pout_thresholds=thr if "pout_gt" in keys else None)
    for k, v in acc.items():
        if k in PER_TOA_SUMS:
            for c, n in enumerate(n_of):
                v[..., c, n:] = SENTINEL       # entries t >= n must stay untouched
    return acc


def accum_run(names, per, launches, S, *, path="auto", waves=None, poison=False, every=1,
              accum=ACCUM_KEYS, thr=None, burn=5, rec_keys=("b", "z", "alpha", "pout"),
              with_accum=True):
    """``launches`` launches of S sweeps; returns a dict: the records [C, launches * S / every,
    ...], the sums, the final state, the fixtures, each chain's dataset and n.  accum None: no
    accumulators set; with_accum False: gst_set_accum_toa alone."""
    ns, refs, ds_of = accum_sampler(names, per, path, waves, poison)
    n_of = np.array([refs[d]["pta"].n for d in ds_of])
    acc = None
    if accum is not None:
        acc = accum_alloc(ns, n_of, accum, thr)
        if with_accum:
            ns.set_accum(acc, from_sweep=ACCUM_SWEEP0 + burn, pout_thresholds=thr)
        else:
            ns.set_accum_toa(acc, pout_thresholds=thr)
    recs = []
    for i in range(launches):
        rec = ns.alloc_records((S + every - 1) // every, rec_keys)
        ns.sweep(S, records=rec, record_every=every, seed=ACCUM_SEED,
                 sweep0=ACCUM_SWEEP0 + i * S)
        recs.append({k: v.cpu().numpy() for k, v in rec.items()})
    state = ns.get_state()
    sums = None if acc is None else {k: v.cpu().numpy() for k, v in acc.items()}
    ns.close()
    return dict(rec={k: np.concatenate([r[k] for r in recs], axis=1) for k in rec_keys},
                sums=sums, state=state, refs=refs, ds_of=ds_of, n_of=n_of)
