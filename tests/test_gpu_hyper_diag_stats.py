"""The hyper MH's statistics taken from the diagonal lanes (chol_stats_diag) and the one harvest per
sweep in front of the b draw, on the three instances that differ in where the augmented row's
diagonal element sits and in whether the last slot column is partial:

  classic  (8, 2, 2, 56), dummy pad columns     RA % 8 = 0, last slot column full
  general  (8, 2, 2, 62), general white noise   RA % 8 = 6, partial
  j1713    (10, 3, 2, 76)                       RA % 8 = 4, partial

Models and states are tests/test_gpu_hyper_stats.py's.  The goldens hold what the build before
that change gave (``python tests/test_gpu_hyper_diag_stats.py`` writes both files, as
hyper_stats_vvh17.npz was written): only the last bits of lnL may move (1e-12 of the magnitude
of its cancelling terms), and every recorded draw stays bitwise.
"""
import functools
import os
import warnings

import numpy as np
import pytest

from gpu_support import builds, open_sampler
from gibbs_student_t_amd import _abi
from gibbs_student_t_amd.run_sims import MODELS
from golden_io import GOLDEN, load_dataset
from oracle.gibbs_oracle import ChainState, Oracle, OutlierModel, lnlike_marginal_extended
from support import (MIXTURE_KW as KW, cached_ref, narrowed_prior_model, prior_box, start_state,
                     states_at)

pytestmark = pytest.mark.gpu

C = 64
INSTANCES = ("classic", "general", "j1713")
LNL_GOLDEN = os.path.join(GOLDEN, "hyper_diag_lnl.npz")
SWEEPS_GOLDEN = os.path.join(GOLDEN, "hyper_diag_sweeps.npz")
REC_KEYS = ("x", "b", "theta")
SEED, SWEEPS = 77, 3


@functools.lru_cache(maxsize=None)
def _model(inst):
    """(fixture dict with pta and kw, x0)"""
    if inst == "j1713":
        ref = cached_ref("beta_fixed")
        return dict(pta=ref["pta"], kw=ref["kw"]), ref["xs"]
    pta, x0 = narrowed_prior_model(inst, 0.03, 0.03)
    return dict(pta=pta, kw=KW), x0


def _box_states(inst, n_chains, seed=41):
    """Hyper parameters anywhere in their prior box, the others at x0; a tenth of the TOAs
    flagged at alpha = 5.  Chain c is the same for every n_chains > c."""
    mdl, x0 = _model(inst)
    pta = mdl["pta"]
    n, m = pta.n, pta.get_basis()[0].shape[1]
    hind = Oracle(pta, OutlierModel(**KW)).hind
    lo, hi = prior_box(pta)
    x = np.tile(x0, (n_chains, 1))
    z = np.empty((n_chains, n))
    for c in range(n_chains):
        rng = np.random.default_rng([seed, c])
        x[c, hind] = rng.uniform(lo[hind], hi[hind])
        z[c] = rng.uniform(size=n) < 0.1
    return dict(x=x, b=np.zeros((n_chains, m)), z=z, alpha=np.where(z > 0, 5.0, 1.0),
                pout=np.zeros((n_chains, n)), theta=np.full(n_chains, 0.05),
                nu=np.full(n_chains, 4.0))


def _eval_states(inst):
    """The states of test_gpu_hyper_stats.py's eval_lnlike tests: prior-box states on the small
    instances, the reference's first 64 hyper-likelihood points on J1713+0747."""
    if inst != "j1713":
        return _box_states(inst, C)
    ref = cached_ref("beta_fixed")
    st, ss = states_at(ref, np.arange(C) // 11)
    st.update(x=ref["tape"]["hyper_lnl_x"].reshape(-1, len(ref["xs"]))[:C],
              theta=np.array([s["theta"] for s in ss]), nu=np.array([s["nu"] for s in ss]))
    return st


def _chain_state(st, c):
    return ChainState(b=st["b"][c], z=st["z"][c], alpha=st["alpha"][c], pout=st["pout"][c],
                      theta=float(st["theta"][c]), nu=float(st["nu"][c]))


def _scales(inst, st):
    """Magnitude of each state's cancelling terms (lnlike_marginal_extended)"""
    pta = _model(inst)[0]["pta"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.array([lnlike_marginal_extended(pta, _chain_state(st, c), st["x"][c],
                                                  with_scale=True)[1] for c in range(C)])


def _eval(inst, st, n_chains=C, waves=None):
    ns = open_sampler(_model(inst)[0], n_chains, "persistent", waves)
    ns.set_state(**st)
    _, h = ns.eval_lnlike()
    ns.close()
    return h


def _failure_states(inst):
    """One, four and all TOAs flagged at a negative alpha (negative noise weights), chain by
    chain in turn, alpha in turn -1 and -1e-3: Sigma stays positive definite for some and
    loses definiteness, at whichever column the flagged TOAs weigh on, for the others."""
    st = _box_states(inst, C, seed=43)
    n = st["z"].shape[1]
    for c in range(C):
        rng = np.random.default_rng([47, c])
        k = (1, 4, n)[c % 3]
        z = np.zeros(n)
        z[rng.permutation(n)[:k]] = 1.0
        st["z"][c] = z
        st["alpha"][c] = np.where(z > 0, (-1.0, -1e-3)[(c // 3) % 2], 1.0)
    return st


def _sweep_start(case, n_chains=C):
    """(fixture, start state) of the recorded runs: the instances' fixture starts (x spread over
    the prior), and the vvh17 all-outlier start whose first b draw takes the floor pass."""
    if case == "vvh17":
        pta = load_dataset()
        lo, hi = prior_box(pta)
        x = np.stack([np.random.default_rng([3, c]).uniform(lo, hi) for c in range(n_chains)])
        return dict(pta=pta, kw=MODELS["vvh17"]), dict(
            x=x, z=np.ones((n_chains, pta.n)), alpha=np.full((n_chains, pta.n), 1e10),
            theta=np.full(n_chains, 0.01), nu=np.full(n_chains, 4.0))
    if case == "j1713":
        ref = cached_ref("beta_fixed")
        st = start_state(ref, n_chains)
        lo, hi = prior_box(ref["pta"])
        st["x"] = np.stack([np.random.default_rng([21, c]).uniform(lo, hi)
                            for c in range(n_chains)])
        return dict(pta=ref["pta"], kw=ref["kw"]), st
    return _model(case)[0], _box_states(case, n_chains)


def _run(case, n_chains=C, waves=1):
    """SWEEPS recorded sweeps with the kernel's own variates: records and the final status"""
    mdl, st = _sweep_start(case, n_chains)
    ns = open_sampler(mdl, n_chains, "persistent", waves)
    ns.set_state(**st)
    rec = ns.alloc_records(SWEEPS, keys=REC_KEYS)
    ns.sweep(SWEEPS, records=rec, seed=SEED)
    out = {k: v.cpu().numpy() for k, v in rec.items()}
    fin = ns.get_state()
    ns.close()
    out["status"] = np.asarray(fin["status"], np.int64)
    for k in REC_KEYS:
        out["final_" + k] = fin[k]
    return out


@pytest.mark.parametrize("inst", INSTANCES)
def test_eval_lnlike_against_previous_build(inst):
    want = np.load(LNL_GOLDEN)
    st = _eval_states(inst)
    got = _eval(inst, st)
    lnl, scale = want[inst + "_lnl"], want[inst + "_scale"]
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(lnl))
    fin = np.isfinite(lnl)
    assert fin.all() and np.isfinite(got).all()
    err = np.abs(got - lnl) / scale
    print(f"{inst}: max |new - previous| / scale = {err.max():.3e}")
    assert np.all(err <= 1e-12), (inst, err.max(), int(err.argmax()))


@pytest.mark.parametrize("inst", INSTANCES)
def test_failure_flag_follows_the_oracle(inst):
    mdl = _model(inst)[0]
    st = _failure_states(inst)
    orc = Oracle(mdl["pta"], OutlierModel(**mdl["kw"]))
    want = np.empty(C, bool)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in range(C):
            orc.cache = None
            want[c] = np.isneginf(orc.lnlike_marginal(_chain_state(st, c), st["x"][c]))
    # both outcomes among the states, and among the states with one and with four flagged TOAs
    assert 8 <= want.sum() <= C - 8, want
    assert want[2::3].all()                     # every weight negative
    got = _eval(inst, st)
    np.testing.assert_array_equal(np.isneginf(got), want)


@pytest.mark.parametrize("inst", INSTANCES)
def test_builds_agree(inst):
    """One wave per chain, two waves per chain and two chains per SIMD: the same bits for lnL
    and for the records of 3 sweeps on the chains they share."""
    runs = {}
    for name, (n_chains, waves) in builds().items():
        ev = _box_states(inst, n_chains)
        runs[name] = (_eval(inst, ev, n_chains, waves), _run(inst, n_chains, waves))
    lnl0, rec0 = runs["occ1"]
    n0 = len(lnl0)
    assert np.isfinite(lnl0).all()
    for name in ("pair", "occ2"):
        lnl, rec = runs[name]
        np.testing.assert_array_equal(lnl[:n0], lnl0, err_msg=f"{name} lnL")
        for k, v in rec.items():
            np.testing.assert_array_equal(v[:n0], rec0[k], err_msg=f"{name} {k}")


@pytest.mark.parametrize("waves", (1, 2))
@pytest.mark.parametrize("case", INSTANCES + ("vvh17",))
def test_three_sweeps_against_previous_build(case, waves):
    """x, b, theta of 3 sweeps and the final status, bitwise: the harvest in its new place (after
    the step loop, before floor_shift and the b draw, in both floor passes) hands the b draw the
    pivots and entries the per-likelihood harvest did."""
    want = np.load(SWEEPS_GOLDEN)
    got = _run(case, C, waves)
    if case == "vvh17":                         # the floor pass is taken
        assert np.sum((want["vvh17_status"] & _abi.STATUS_FLOOR) != 0) >= C // 2
    for k, v in got.items():
        np.testing.assert_array_equal(v, want[f"{case}_{k}"], err_msg=f"{case} {k}")


if __name__ == "__main__":
    lnl, sweeps = {}, {}
    for inst_ in INSTANCES:
        st_ = _eval_states(inst_)
        lnl[inst_ + "_lnl"] = _eval(inst_, st_)
        lnl[inst_ + "_scale"] = _scales(inst_, st_)
    for case_ in INSTANCES + ("vvh17",):
        for k_, v_ in _run(case_, C, 1).items():
            sweeps[f"{case_}_{k_}"] = v_
    np.savez(LNL_GOLDEN, **lnl)
    np.savez(SWEEPS_GOLDEN, **sweeps)
