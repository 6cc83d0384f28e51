"""Launch-boundary invariants of the persistent kernel: no hidden cross-sweep state.

A chain's state between sweeps is, by the reference's semantics (gibbs.py:354-380), exactly
(x, b, z, alpha, pout, theta, nu) -- what the records hold.  The persistent kernel keeps
more than that across the sweeps of one launch (y = r - T b and the z bits in registers, the
published column, junk rows, the parked timing-model factor and stage scratch in LDS /
global scratch).  If any of it leaked from one sweep into the next, a launch of S sweeps
would differ from S launches of one sweep each, where every sweep starts from fresh LDS and
registers.  So: one launch of S sweeps must equal S one-sweep launches BITWISE, records
and final state, for every build the host can pick (one chain per SIMD, two chains per
SIMD with the fair-priority counter, two waves per chain).
"""
import numpy as np
import pytest

from gpu_support import (builds, launch_records, open_sampler, single_sweep_differences,
                         torch)
from gibbs_student_t_amd import _abi
from gibbs_student_t_amd.native import STATE_KEYS as KEYS
from golden_io import load_ref, sweep_state
from support import prior_box, rel, start_state, states_at

pytestmark = pytest.mark.gpu

# (+ the general white-noise instances: two backends with ECORR, one backend with ECORR,
# J1713+0747 with two backends and no ECORR)
FIXTURES = ("beta_efac_fixed", "c3_beta_fixed", "tm22_beta_fixed", "vvh17_prior",
            "ecb_beta_fixed", "ecq_t_fixed", "jb_uniform_fixed")


def _native(ref, C, waves=None):
    return open_sampler(ref, C, "persistent", waves, skip_if_no_instance=True)


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("build", ("occ1", "pair", "occ2"))
def test_one_launch_equals_single_sweep_launches(name, build):
    label, (C, waves) = build, builds()[build]
    ref = load_ref(name)
    S, seed, sweep0 = 100, 11, 5
    init = start_state(ref, C, 21)

    ns = _native(ref, C, waves)
    ns.set_state(**init)
    rec, long_state = launch_records(ns, S, seed=seed, sweep0=sweep0)

    ns = _native(ref, C, waves)
    ns.set_state(**init)
    bad = single_sweep_differences(ns, rec, long_state, S, seed, sweep0)
    assert not bad, f"{label}: first difference (sweep, array) {bad[:4]}"


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("build", ("occ1", "pair", "occ2"))
def test_poisoned_lds_and_scratch_change_nothing(name, build):
    """GST_DEBUG_POISON overwrites every chain's LDS (S0 / stage scratch, published columns,
    junk rows, MH variates, phi^-1) and its parked timing-model factor with NaN at the start
    of every sweep.  The chains must be bitwise those of an ordinary launch: no sweep reads
    a word it did not write itself (the stale-LDS hypothesis)."""
    label, (C, waves) = build, builds()[build]
    ref = load_ref(name)
    S, seed, sweep0 = 100, 12, 9
    init = start_state(ref, C, 22)
    outs = []
    for poison in (False, True):
        ns = _native(ref, C, waves)
        ns.set_debug(poison=poison)
        ns.set_state(**init)
        outs.append(launch_records(ns, S, seed=seed, sweep0=sweep0))
    (r0, s0), (r1, s1) = outs
    for k in KEYS:
        assert torch.equal(r0[k], r1[k]), f"{label}: record {k} differs under poisoning"
    for k in KEYS + ("status",):
        assert torch.equal(s0[k], s1[k]), f"{label}: final {k} differs under poisoning"


@pytest.mark.parametrize("name", ["beta_fixed", "t_prior", "uniform_fixed", "beta_efac_fixed",
                                  "ecq_beta_fixed", "ecq_t_fixed", "jb_beta_fixed"])
def test_low_rank_gram_matches_mfma_gram(name):
    """The persistent kernel's low-rank Gram (one noise class on J1713: the class Gram plus a
    rank-1 update per flagged TOA) against its MFMA Gram
    (GST_DEBUG_MFMA_GRAM) at every state the reference recorded: both likelihoods within
    1e-11 relative (the Gram feeds only the marginal one), and 40 sweeps of 64 chains from
    the same Philox stream make the same MH, z and nu decisions with b, alpha, pout within
    1e-8 relative."""
    ref = load_ref(name)
    S = int(ref["niter"])
    init, ss = states_at(ref, range(S))
    got = []
    for mfma in (False, True):
        ns = _native(ref, S)
        ns.set_debug(mfma_gram=mfma)
        ns.set_state(x=ref["chain"][:S], theta=np.array([s["theta"] for s in ss]),
                     nu=np.array([s["nu"] for s in ss]), **init)
        got.append(ns.eval_lnlike())
        ns.close()
    assert np.all(rel(got[0][1], got[1][1]) <= 1e-11), rel(got[0][1], got[1][1]).max()
    np.testing.assert_array_equal(got[0][0], got[1][0])
    C, n = 64, ref["pta"].n
    st0 = start_state(ref, C, 2)
    out = []
    for mfma in (False, True):
        ns = _native(ref, C)
        ns.set_debug(mfma_gram=mfma)
        ns.set_state(**st0)
        ns.sweep(40, seed=17, sweep0=1)
        out.append(ns.get_state())
        ns.close()
    a, b = out
    same = np.all(a["x"] == b["x"], axis=1) & np.all(a["z"][:, :n] == b["z"][:, :n], axis=1) \
        & (a["nu"] == b["nu"])
    assert same.mean() >= 0.95, same.mean()
    for k in ("b", "alpha", "pout", "theta"):
        r = rel(a[k][same], b[k][same])
        assert np.all(r <= 1e-8), f"{k}: {r.max():.3e}"


@pytest.mark.parametrize("alpha,path", [(30.0, "low_rank"), (1e8, "mfma")])
def test_low_rank_gram_alpha_gate_and_path_counts(alpha, path):
    """The low-rank Gram subtracts c_k (1 - 1 / alpha_t) of a class Gram's share per flagged
    TOA, so a direction fixed by flagged TOAs alone keeps an absolute error ~eps c_k |row|^2
    against its true size c_k |row|^2 / alpha_t.  The kernel takes it only while
    every flagged alpha is <= 2^20.  Ten flagged TOAs of J1713 (one noise class): at alpha =
    30 the Gram runs low-rank, at 1e8 (vvh17's fixed alpha is 1e10) on the MFMA -- counted by
    gst_gram_counts over a GST_STAGE_GRAM launch -- and the likelihoods at 64 prior draws
    agree with the forced MFMA Gram to 1e-11 relative (bitwise at 1e8: the same MFMA Gram)."""
    ref = load_ref("beta_fixed")
    C, n = 64, ref["pta"].n
    lo, hi = prior_box(ref["pta"])
    s0 = sweep_state(ref, 0)
    z = np.zeros((C, n))
    z[:, 7:130:13] = 1.0
    al = np.where(z > 0, alpha, 1.0)
    st0 = dict(x=np.random.default_rng(4).uniform(lo, hi, size=(C, len(lo))),
               b=np.tile(s0["b"], (C, 1)), z=z, alpha=al, pout=np.zeros((C, n)),
               theta=np.full(C, 0.05), nu=np.full(C, 4.0))
    got, counts = [], []
    for mfma in (False, True):
        ns = _native(ref, C)
        ns.set_debug(mfma_gram=mfma)
        ns.set_state(**st0)
        got.append(ns.eval_lnlike())
        ns.gram_counts(reset=True)
        ns.sweep(1, seed=3, mask=_abi.STAGE_GRAM)
        counts.append(ns.gram_counts(reset=True))
        ns.close()
    assert counts[1] == {"low_rank": 0, "mfma": C, "large_mfma": 0}, counts[1]
    want = {"low_rank": C, "mfma": 0} if path == "low_rank" else {"low_rank": 0, "mfma": C}
    assert counts[0] == dict(want, large_mfma=0), counts[0]
    np.testing.assert_array_equal(got[0][0], got[1][0])
    if path == "mfma":
        np.testing.assert_array_equal(got[0][1], got[1][1])
    else:
        assert np.all(rel(got[0][1], got[1][1]) <= 1e-11), rel(got[0][1], got[1][1]).max()
