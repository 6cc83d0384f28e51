"""What the hyper MH step hands on from a factorisation: the marginal likelihood (log|Sigma| as
mantissa product + exponent sum, d^T Sigma^-1 d, the failure flag) on instances with and
without dummy pad columns, and the posterior sums that ride on the same sweeps.

Every case runs 64 chains on the persistent path; the smaller models are
tests/test_gpu_hyper_steps.py's (100 TOAs, 10 components on the (8, 2, 2, 56) instance, whose
56 hyper columns it pads with unit-prior dummies; the two-backend ECORR dataset on the general
white-noise (8, 2, 2, 62) instance) with their narrowed hyper prior, the full-size one is the
J1713+0747 fixture on (10, 3, 2, 76).  Likelihoods are held to the suite's 1e-10 relative
(tests/test_gpu_parity.py's RTOL and its long-double arbitration for ill-conditioned Sigma).
"""
import os
import sys
import warnings

import numpy as np
import pytest

from gpu_support import accum_run, open_sampler, upload_tape
from gibbs_student_t_amd import _abi
from gibbs_student_t_amd.native import pack_tape
from gibbs_student_t_amd.run_sims import MODELS
from golden_io import GOLDEN, load_dataset, load_ref, oracle_replay, sweep_state
from oracle.gibbs_oracle import ChainState, Oracle, OutlierModel
from support import (MIXTURE_KW as KW, RTOL, assert_lnl_within_reference_error,
                     assert_replay_matches, check_accum_sums, narrowed_prior_model, prior_box,
                     start_state, states_at)

pytestmark = pytest.mark.gpu

C = 64


def _states(pta, x0, rng):
    """C start states: the hyper parameters anywhere in their prior box, the others at x0; a
    tenth of the TOAs flagged as outliers with alpha = 5."""
    orc = Oracle(pta, OutlierModel(**KW))
    n, m = len(orc.r), pta.get_basis()[0].shape[1]
    lo, hi = prior_box(pta)
    hyp = np.zeros(len(x0), bool)
    hyp[orc.hind] = True
    x = np.where(hyp[None], rng.uniform(lo, hi, size=(C, len(x0))), x0[None])
    z = (rng.uniform(size=(C, n)) < 0.1).astype(np.float64)
    return orc, dict(x=x, b=np.zeros((C, m)), z=z, alpha=np.where(z > 0, 5.0, 1.0),
                     pout=np.zeros((C, n)), theta=np.full(C, 0.05), nu=np.full(C, 4.0))


def _check_lnl(pta, orc, st, got, label):
    """got[c] against the oracle's fp64 value; where they differ by more than RTOL the
    long-double value arbitrates as in tests/test_gpu_parity.py::test_lnlikelihoods."""
    for c in range(C):
        cs = ChainState(b=st["b"][c], z=st["z"][c], alpha=st["alpha"][c], pout=st["pout"][c],
                        theta=st["theta"][c], nu=st["nu"][c])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = orc.lnlike_marginal(cs, st["x"][c])
        assert np.isfinite(want) and np.isfinite(got[c]), (label, c, want, got[c])
        if abs(got[c] - want) <= RTOL * abs(want):
            continue
        assert_lnl_within_reference_error(pta, cs, st["x"][c], got[c], want, f"{label}[{c}]")


@pytest.mark.parametrize("kind", ["classic", "general"])
def test_eval_lnlike_small_instances(kind):
    """eval_only marginal likelihood of 64 states on the (8, 2, 2, 56) instance with a model
    smaller than the instance (dummy pad columns: pivot exactly 1) and on the general
    white-noise (8, 2, 2, 62) instance, against the oracle."""
    pta, x0 = narrowed_prior_model(kind, 0.03, 0.03)
    orc, st = _states(pta, x0, np.random.default_rng(41))
    ns = open_sampler(dict(pta=pta, kw=KW), C, "persistent")
    ns.set_state(**st)
    _, h = ns.eval_lnlike()
    ns.close()
    _check_lnl(pta, orc, st, h, kind)


def test_eval_lnlike_j1713():
    """The same on the J1713+0747 fixture ((10, 3, 2, 76), no pad column in the Fourier block):
    the first 64 points at which the reference evaluated its hyper likelihood."""
    ref = load_ref("beta_fixed")
    K = 11
    idx = np.arange(C) // K
    st, ss = states_at(ref, idx)
    st.update(x=ref["tape"]["hyper_lnl_x"].reshape(-1, len(ref["xs"]))[:C],
              theta=np.array([s["theta"] for s in ss]), nu=np.array([s["nu"] for s in ss]))
    ns = open_sampler(ref, C, "persistent")
    ns.set_state(**st)
    _, h = ns.eval_lnlike()
    ns.close()
    _check_lnl(ref["pta"], Oracle(ref["pta"], OutlierModel(**ref["kw"])), st, h, "j1713")


def test_failed_factor_is_minus_inf_and_flagged():
    """Sigma not positive definite (negative noise weights where z = 1): the likelihood is
    -inf (gibbs.py:320-324) and a hyper block started there sets status bit 0."""
    ref = load_ref("beta_fixed")
    s0 = sweep_state(ref, 0)
    ns = open_sampler(ref, C, "persistent")
    one = lambda v: np.tile(np.asarray(v, float), (C, 1))   # noqa: E731
    ns.set_state(x=one(ref["xs"]), b=np.zeros((C, ns.m)), z=np.ones((C, ns.n)),
                 alpha=np.full((C, ns.n), -1.0), pout=one(s0["pout"]),
                 theta=np.full(C, s0["theta"]), nu=np.full(C, s0["nu"]))
    _, h = ns.eval_lnlike()
    assert np.all(np.isneginf(h)), h
    ns.sweep(1, mask=_abi.STAGE_HYPER, seed=5)
    status = ns.get_state()["status"]
    ns.close()
    assert np.all(status & 1), status


def test_posterior_sums_of_three_sweeps():
    """ACC instance: the sums over 3 sweeps are the sequential sums of the recorded chain
    (tests/test_gpu_accum.py's check, at this module's 64 chains)."""
    out = accum_run(["beta_fixed"], C, 1, 3, path="persistent", burn=0)
    check_accum_sums(out["rec"], out["sums"], out["n_of"], 0)
    assert np.all(out["sums"]["count"] == 3)


def test_last_step_accept_and_reject_draw_b():
    """Two tape-mode replays of the fixture's first two sweeps that differ only in the last
    hyper step's acceptance variate of sweep 0: u = 1e-300 (log u = -691: accepted, the b draw
    takes the factor left in the registers) and u = 1e300 (log u = +691: rejected, step NHYPER
    refactors at x for it); 32 chains each.  Both against the oracle replaying the same tapes
    (tests/test_gpu_parity.py's tolerances), and the rejected side's b bitwise that of a launch
    with the direct update_b mask from the same x."""
    ref = load_ref("beta_fixed")
    refs = []
    for u in (1e-300, 1e300):
        r = dict(ref)
        r["tape"] = {k: np.array(v, copy=True) for k, v in ref["tape"].items()}
        r["tape"]["hyper_acc"][0][9] = u
        refs.append(r)
    ns = open_sampler(ref, C, "persistent")
    start = start_state(ref, C)
    ns.set_state(**start)
    rows = np.stack([pack_tape(refs[c >= C // 2]["tape"], [0, 1], ns.n, ns.m, ns.stride)
                     for c in range(C)])
    rec = ns.alloc_records(2)
    ns.sweep(2, records=rec, tape=upload_tape(ns, rows))
    got = {k: v.cpu().numpy() for k, v in rec.items()}
    assert np.all((ns.get_state()["status"] & _abi.STATUS_ERRORS) == 0)
    want = [oracle_replay(r, 2) for r in refs]
    # the step decides: the two sides end sweep 0 at different x
    assert not np.array_equal(want[0]["x"][1], want[1]["x"][1])
    for c in (0, C // 2 - 1, C // 2, C - 1):
        side = int(c >= C // 2)
        assert_replay_matches({k: v[c] for k, v in got.items()}, want[side], refs[side],
                              f"side {side} chain {c}")
    for k, v in got.items():                      # one tape, one chain: every copy bitwise
        np.testing.assert_array_equal(v[:C // 2], np.broadcast_to(v[0], v[:C // 2].shape), k)
        np.testing.assert_array_equal(v[C // 2:], np.broadcast_to(v[C // 2], v[C // 2:].shape), k)
    # the rejected side drew b from a refactorisation at its final x: so does a launch with
    # the direct update_b mask from that x, the start state and the same draw term
    ns.set_state(**dict(start, x=got["x"][:, 1]))
    ns.sweep(1, mask=_abi.STAGE_B | _abi.STAGE_B_FORCE,
             tape=upload_tape(ns, rows[:, :1]))
    direct = ns.get_state()["b"]
    ns.close()
    np.testing.assert_array_equal(direct[C // 2:], got["b"][C // 2:, 1])


def vvh17_floor_run():
    """64 vvh17 chains from the all-outlier start (z = 1, alpha = 1e10: Sigma beyond fp64
    resolution, so the first b draw takes the SVD-floor pass), 2 sweeps with the kernel's own
    variates: the final x, b and status.  `python tests/test_gpu_hyper_stats.py OUT.npz`
    writes them (the golden was written so by the build before the step loop's rework)."""
    pta = load_dataset()
    ns = open_sampler(dict(pta=pta, kw=MODELS["vvh17"]), C, "persistent")
    lo, hi = prior_box(pta)
    ns.set_state(x=np.random.default_rng(3).uniform(lo, hi, size=(C, len(lo))),
                 z=np.ones((C, ns.n)), alpha=np.full((C, ns.n), 1e10),
                 theta=np.full(C, 0.01), nu=np.full(C, 4.0))
    ns.sweep(2, seed=99)
    out = ns.get_state()
    ns.close()
    return dict(x=out["x"], b=out["b"], status=np.asarray(out["status"], np.int64))


def test_vvh17_floor_draw_matches_golden():
    """The floor draw (pass 1 of the hyper block: floor_shift from the harvested pivots, then
    the refactorisation of Sigma + f I) gives the recorded status floor counts, x and b."""
    want = np.load(os.path.join(GOLDEN, "hyper_stats_vvh17.npz"))
    got = vvh17_floor_run()
    assert np.sum((want["status"] & _abi.STATUS_FLOOR) != 0) >= C // 2   # the pass is taken
    for k in ("status", "x", "b"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


if __name__ == "__main__":
    np.savez(sys.argv[1], **vvh17_floor_run())
