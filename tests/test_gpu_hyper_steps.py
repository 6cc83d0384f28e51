"""The one-wave hyper MH loop's step sequencing against the CPU oracle.

Between two factorisations the loop takes the verdict of one proposal, skips the proposals
that fall outside the prior (rejected without a likelihood, gibbs.py:100-104) and sets up the
next one; after the last step it reuses the factor in registers for the b draw or refactors at
x.  Which of these paths a step takes depends on where the next in-prior proposal lies on the
accept and on the reject side.  The golden fixtures' wide priors hardly ever reject a proposal
by its prior, so these tests narrow the prior on log10_A / gamma around the start until a
large share of the proposals falls outside it, and replay 16 chains x 30 sweeps of a tape drawn
here on the smallest persistent instances: (8, 2, 2, 56) for a synthetic pulsar of 100 TOAs
with 10 components, (8, 2, 2, 62) of the general white-noise model for the ``ecb`` dataset (two
backends with ECORR, 72 TOAs; its two log10_ecorr parameters are hyper parameters too and get
the same narrow prior, or half of the proposals could never leave it).  The seed and the prior
widths were searched on the CPU with the oracle until every sequencing event below occurred;
the tests count them again from the oracle's replay and require each to occur.

Tolerances are tests/test_gpu_parity.py's (assert_replay_matches): x, z, theta, nu exact; b
normwise and alpha / pout elementwise <= 1e-10 relative, the long-double mean arbitrating b.
"""
import warnings
from collections import Counter

import numpy as np
import pytest
import scipy.linalg as sl

from gibbs_student_t_amd._abi import STATUS_ERRORS
from gibbs_student_t_amd.native import STATE_KEYS, pack_tape
from oracle.gibbs_oracle import (MH_PROBS, MH_SIZES, ChainState, Oracle, OutlierModel,
                                 TapeVariates, choice_from_uniform)
from support import MIXTURE_KW as KW, assert_replay_matches, narrowed_prior_model, prior_box
C, S = 16, 30
EVENTS = ("next_out_on_accept_only", "next_out_on_reject_only", "two_consecutive_out",
          "last_in_prior_accepted", "last_in_prior_rejected", "all_ten_out")
# (seed, half-width of the log10_A prior, of the gamma prior): found on the CPU (module doc)
CASES = {"classic": (2, 0.03, 0.03), "general": (2, 0.03, 0.03)}


class _DrawnTape(TapeVariates):
    """One sweep's variates drawn from a generator and kept in tape layout: the uniform and
    normal ones up front, the state-dependent ones (Beta, gamma) as the oracle asks."""

    def __init__(self, rng, n, hind, wind):
        t = {}
        for stage, ns, ind in (("white", 20, wind), ("hyper", 10, hind)):
            t[f"{stage}_u"] = rng.uniform(size=ns)
            t[f"{stage}_idx"] = rng.choice(ind, size=ns).astype(np.float64)
            t[f"{stage}_xi"] = rng.standard_normal(ns)
            t[f"{stage}_acc"] = rng.uniform(size=ns)
        t["z_u"] = rng.uniform(size=n)
        t["df_u"] = rng.uniform()
        t["gamma"] = np.ones(n)
        t["beta"] = 0.0
        t["b_delta"] = None
        self.rng = rng
        super().__init__(t)

    def beta(self, a, b):
        self.t["beta"] = float(self.rng.beta(a, b))
        return self.t["beta"]

    def gamma(self, shape):
        self.t["gamma"] = self.rng.gamma(shape)
        return self.t["gamma"]


class _DrawingOracle(Oracle):
    """The oracle, drawing the b draw's term U^-1 xi (Sigma + f I = U^T U) into the tape and
    then taking the tape-mode draw (mean + recorded term) the kernel is pinned to."""

    def draw_b(self, st, x, src, mean="floor_delta"):
        Sigma, d = self.sigma_matrix(st, x)
        f = self.floor_shift(Sigma)
        cf = sl.cho_factor(Sigma + f * np.eye(len(d)) if f > 0.0 else Sigma)
        src.t["b_delta"] = sl.solve_triangular(np.triu(cf[0]), src.rng.standard_normal(len(d)),
                                               lower=False)
        return super().draw_b(st, x, src, mean="floor_delta")


def _hyper_events(orc, t, hlog, ev):
    """Count the hyper block's sequencing events of one sweep from its tape and the oracle's
    log of likelihood evaluations ([(x, l0)] + [(q_s, l1_s)], gibbs.py:80-111)."""
    nh = len(orc.hind)
    x, l0 = hlog[0]
    p0 = orc.lnprior(x)
    dl = np.zeros((10, len(x)))
    for s in range(10):
        dl[s, int(t["hyper_idx"][s])] = t["hyper_xi"][s] * (0.05 * nh) * \
            choice_from_uniform(MH_SIZES, MH_PROBS, t["hyper_u"][s])

    def inside(v):
        return np.isfinite(orc.lnprior(v))

    run_out, any_in = 0, False
    for s in range(10):
        q, l1 = hlog[s + 1]
        if not inside(q):
            run_out += 1
            ev["two_consecutive_out"] += run_out == 2
            continue
        run_out, any_in = 0, True
        p1 = orc.lnprior(q)
        acc = (l1 + p1) - (l0 + p0) > np.log(t["hyper_acc"][s])
        in_a = [inside(q + dl[k]) for k in range(s + 1, 10)]
        in_r = [inside(x + dl[k]) for k in range(s + 1, 10)]
        if s + 1 < 10:
            ev["next_out_on_accept_only"] += (not in_a[0]) and in_r[0]
            ev["next_out_on_reject_only"] += in_a[0] and not in_r[0]
        if acc:
            ev["last_in_prior_accepted"] += not any(in_a)
            x, l0, p0 = q, l1, p1
        else:
            ev["last_in_prior_rejected"] += not any(in_r)
    ev["all_ten_out"] += not any_in


def make_case(kind):
    """The model, C start points, the drawn tape ([C][S] per field), the oracle's records
    ([C][S] per key, the state at each sweep's start) and the event counts."""
    seed, wA, wg = CASES[kind]
    pta, x0 = narrowed_prior_model(kind, wA, wg)
    orc = _DrawingOracle(pta, OutlierModel(**KW))
    rng = np.random.default_rng(seed)
    n, m = len(orc.r), pta.get_basis()[0].shape[1]
    lo, hi = prior_box(pta)
    hyp = np.zeros(len(x0), bool)
    hyp[orc.hind] = True
    ev = Counter({k: 0 for k in EVENTS})
    tapes, recs, starts = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in range(C):
            # the hyper parameters anywhere in their (narrowed) box, the white ones at x0
            x = np.where(hyp & (hi - lo < 1.0), rng.uniform(lo, hi), x0)
            z = (rng.uniform(size=n) < 0.1).astype(np.float64)
            st = ChainState(b=np.zeros(m), z=z, alpha=np.where(z > 0, 5.0, 1.0),
                            pout=np.zeros(n), theta=0.05, nu=4.0)
            starts.append(dict(x=x.copy(), b=st.b.copy(), z=st.z.copy(), alpha=st.alpha.copy(),
                               pout=st.pout.copy(), theta=st.theta, nu=st.nu))
            rec = {k: [] for k in STATE_KEYS}
            tp = []
            for _ in range(S):
                for k, v in (("x", x), ("b", st.b), ("z", np.asarray(st.z, float)),
                             ("alpha", st.alpha), ("pout", st.pout), ("theta", st.theta),
                             ("nu", float(st.nu))):
                    rec[k].append(np.array(v, dtype=np.float64, copy=True))
                src = _DrawnTape(rng, n, orc.hind, orc.wind)
                trace = {}
                x = orc.sweep(st, x, src, b_mean="floor_delta", trace=trace)
                if src.t["b_delta"] is None:        # no b draw this sweep (gibbs.py:373)
                    src.t["b_delta"] = np.zeros(m)
                _hyper_events(orc, src.t, trace["hyper_log"], ev)
                tp.append({k: v for k, v in src.t.items()})
            tapes.append({k: np.stack([np.asarray(t[k], float) for t in tp]) for k in tp[0]})
            recs.append({k: np.stack(v) for k, v in rec.items()})
    return dict(pta=pta, starts=starts, tapes=tapes, recs=recs, events=ev)


_CACHE = {}


def case(kind):
    if kind not in _CACHE:
        _CACHE[kind] = make_case(kind)
    return _CACHE[kind]


def _gpu():
    """The device gate, taken per test: this module's CPU test must run without a device."""
    import gpu_support
    return gpu_support


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", [("classic", (8, 2, 2, 56)), ("general", (8, 2, 2, 62))])
def test_narrowed_prior_replay_matches_oracle(kind, shape):
    """16 chains x 30 sweeps in tape mode under the narrowed hyper prior: every sequencing
    event occurs in the oracle's replay, and the kernel's records are the oracle's (x, z,
    theta, nu exact; b, alpha, pout within test_gpu_parity.py's tolerances)."""
    gpu = _gpu()
    cs = case(kind)
    print(kind, dict(cs["events"]))
    for k in EVENTS:
        assert cs["events"][k] > 0, (k, dict(cs["events"]))
    ns = gpu.open_sampler(dict(pta=cs["pta"], kw=KW), C, "persistent")
    ns.set_state(**{k: np.stack([np.asarray(s[k], float) for s in cs["starts"]])
                    for k in STATE_KEYS})
    rows = np.stack([pack_tape(t, np.arange(S), ns.n, ns.m, ns.stride) for t in cs["tapes"]])
    rec = ns.alloc_records(S)
    ns.sweep(S, records=rec, tape=gpu.upload_tape(ns, rows))
    got = {k: v.cpu().numpy() for k, v in rec.items()}
    status = ns.get_state()["status"]
    ns.close()
    assert np.all((status & STATUS_ERRORS) == 0)
    for c in range(C):
        ref = dict(pta=cs["pta"], kw=KW, tape=cs["tapes"][c])
        assert_replay_matches({k: v[c] for k, v in got.items()}, cs["recs"][c], ref,
                              f"{kind} chain {c}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["classic", "general"])
def test_philox_launch_same_records_on_both_builds(kind):
    """64 chains x 20 sweeps with the kernel's own variates on the same data and narrowed
    prior: the one-chain-per-SIMD and the two-chains-per-SIMD builds give bitwise-equal
    records and final states.  The two-chains-per-SIMD build is picked for launches of more
    chains than SIMDs, so its 64 chains are the first of such a launch (chains are keyed by
    their global index: the others do not touch them)."""
    gpu = _gpu()
    seed, wA, wg = CASES[kind]
    pta, x0 = narrowed_prior_model(kind, wA, wg)
    C2, S2 = 64, 20
    simds = 4 * gpu.ncu()
    outs = []
    for Cl in (C2, simds + C2):
        ns = gpu.NativeSampler(pta, KW, 0, path="persistent")
        ns.set_waves(1)
        ns.alloc(Cl)
        ns.set_state(x=np.tile(x0, (Cl, 1)), z=np.zeros((Cl, ns.n)), alpha=np.ones((Cl, ns.n)),
                     theta=np.full(Cl, 0.05), nu=np.full(Cl, 4.0))
        rec = ns.alloc_records(S2)
        ns.sweep(S2, records=rec, seed=17)
        out = {f"rec_{k}": v[:C2].cpu().numpy() for k, v in rec.items()}
        out.update({k: v[:C2] for k, v in ns.get_state().items()})
        ns.close()
        outs.append(out)
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)


def test_event_search_is_reproducible():
    """The fixed seed and prior widths give every sequencing event in the oracle's replay (no
    GPU: the choice of inputs itself)."""
    for kind in CASES:
        ev = case(kind)["events"]
        for k in EVENTS:
            assert ev[k] > 0, (kind, k, dict(ev))
