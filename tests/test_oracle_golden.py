"""Pin the CPU oracle against golden vectors produced by running the reference itself.

Fixtures: tests/golden/ref_*.npz (tools/gen_golden.py; reference gibbs.py:8-385 run with
the build's model, seeded, with every variate recorded).
"""
import warnings

import numpy as np
import pytest

from golden_io import CHAIN_KEYS, fixture_names, load_ref, sweep_state, sweep_tape
from oracle.gibbs_oracle import (ChainState, LegacyNumpyVariates, Oracle, OutlierModel,
                                 TapeVariates, bernoulli_from_uniform, choice_from_uniform,
                                 initial_state)

NAMES = fixture_names()


def _oracle(ref):
    return Oracle(ref["pta"], OutlierModel(**ref["kw"]))


@pytest.mark.parametrize("name", NAMES)
def test_legacy_stream_reproduces_reference_bit_exact(name):
    """Same seed, same RNG calls in the same order -> identical chains (gibbs.py:342-385)."""
    ref = load_ref(name)
    orc = _oracle(ref)
    np.random.seed(int(ref["seed"]))
    if int(ref["prior_draw"]):
        xs = ref["pta"].sample_params()
    else:
        xs = ref["xs"]
    np.testing.assert_array_equal(xs, ref["xs"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, st, x = orc.run(xs, int(ref["niter"]))
    for k in CHAIN_KEYS:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(st.b, ref["final_b"])
    np.testing.assert_array_equal(st.alpha, ref["final_alpha"])


@pytest.mark.parametrize("name", NAMES)
def test_tape_replay_per_sweep(name):
    """Each sweep re-run from the recorded start state with the recorded variates."""
    ref = load_ref(name)
    orc = _oracle(ref)
    niter = int(ref["niter"])
    for i in range(niter):
        s0, s1 = sweep_state(ref, i), sweep_state(ref, i + 1)
        st = ChainState(b=s0["b"].copy(), z=s0["z"].copy(), alpha=s0["alpha"].copy(),
                        pout=s0["pout"].copy(), theta=s0["theta"], nu=s0["nu"])
        trace = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x1 = orc.sweep(st, s0["x"], TapeVariates(sweep_tape(ref, i)), trace=trace)
        tape = sweep_tape(ref, i)
        np.testing.assert_array_equal(trace["x_white"], tape["x_white"])
        if i + 1 < niter:
            np.testing.assert_array_equal(x1, ref["chain"][i + 1])
        np.testing.assert_array_equal(st.b, s1["b"])
        np.testing.assert_array_equal(np.asarray(st.z, float), s1["z"])
        np.testing.assert_array_equal(st.alpha, s1["alpha"])
        np.testing.assert_array_equal(st.pout, s1["pout"])
        assert st.theta == s1["theta"] and float(st.nu) == s1["nu"]
        wl = np.array([v for _, v in trace["white_log"]])
        hl = np.array([v for _, v in trace["hyper_log"]])
        np.testing.assert_array_equal(wl, tape["white_lnl"])
        np.testing.assert_array_equal(hl, tape["hyper_lnl"])


def test_initial_state_matches_reference_layout():
    ref = load_ref("beta_fixed")
    st = initial_state(ref["pta"], OutlierModel(**ref["kw"]))
    s0 = sweep_state(ref, 0)
    np.testing.assert_array_equal(st.z, s0["z"])
    np.testing.assert_array_equal(st.alpha, s0["alpha"])
    assert st.theta == s0["theta"] and st.nu == s0["nu"]


def test_choice_mapping_matches_numpy():
    rs = np.random.RandomState(7)
    p = np.array([0.1, 0.15, 0.5, 0.15, 0.1])
    a = [0.1, 0.5, 1.0, 3.0, 10.0]
    for _ in range(2000):
        st = rs.get_state()
        v = rs.choice(a, p=p)
        rs.set_state(st)
        u = rs.random_sample()
        assert choice_from_uniform(a, p, u) == v


def test_bernoulli_mapping_matches_numpy():
    rs = np.random.RandomState(11)
    q = np.concatenate([rs.random_sample(3000), [0.0, 1.0, 0.5, 1e-300, 1 - 1e-16]])
    st = rs.get_state()
    z = rs.binomial(1, q)
    rs.set_state(st)
    for qi, zi in zip(q, z):
        u = rs.random_sample() if qi != 0.0 else np.nan
        assert bernoulli_from_uniform(qi, u) == zi


# the b draw at the SVD noise floor (Oracle.floor_shift; the HIP path draws the same)
FLOOR_FIXTURES = [n for n in NAMES if "vvh17" in n]


def _floor_sweeps(name):
    import warnings

    import scipy.linalg as sl

    from oracle.gibbs_oracle import ChainState
    ref = load_ref(name)
    t, S = ref["tape"], int(ref["niter"])
    orc = Oracle(ref["pta"], OutlierModel(**ref["kw"]))
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in np.flatnonzero(~np.isnan(t["b_cond"])):
            if i + 1 >= S:
                continue
            s = sweep_state(ref, i)
            st = ChainState(b=s["b"], z=s["z"], alpha=s["alpha"], pout=s["pout"],
                            theta=s["theta"], nu=s["nu"])
            orc.cache = None
            Sigma, d = orc.sigma_matrix(st, ref["chain"][i + 1])
            f = orc.floor_shift(Sigma)
            bf = sl.cho_solve(sl.cho_factor(Sigma + f * np.eye(len(d))), d) + t["b_delta"][i]
            out.append((i, f, Sigma, d, bf, t))
    return out


def test_floor_gate_only_where_the_reference_floors():
    """Gate placement (smallest TM-first pivot < 2^-52 x the largest).  It never opens on a
    non-vvh17 fixture.  On the ill-conditioned vvh17 sweeps it leaves shut (cond > 1e12),
    the exact mean cho_solve(Sigma, d) is closer to the reference's own SVD mean than the
    floor mean (round 4's 1e-14 gate) would be on most sweeps and in total -- e.g.
    vvh17_fixed sweeps 0-5, where LAPACK still resolves the eigenvalues: exact ~1e-6, floor
    2e-2..2e-1 from the reference."""
    import scipy.linalg as sl
    closer = farther = 0
    e_exact = e_floor = 0.0
    for name in NAMES:
        for i, f, Sigma, d, bf, t in _floor_sweeps(name):
            if "vvh17" not in name:
                assert f == 0.0, (name, i)
                continue
            if f > 0.0 or not t["b_cond"][i] > 1e12:
                continue
            piv = np.diag(np.linalg.cholesky(Sigma)) ** 2
            fh = 0.75 * 2.0 ** -52 * piv.max()
            m_floor = sl.cho_solve(sl.cho_factor(Sigma + fh * np.eye(len(d))), d)
            m_svd = t["b_mean_svd"][i]
            a = np.linalg.norm(t["b_mean_chol"][i] - m_svd) / np.linalg.norm(m_svd)
            b = np.linalg.norm(m_floor - m_svd) / np.linalg.norm(m_svd)
            closer += a <= b
            farther += a > b
            e_exact += a
            e_floor += b
    print(f"gate shut, cond > 1e12: exact mean closer to the reference's on {closer}, the "
          f"floor mean on {farther}; summed relative error {e_exact:.3f} vs {e_floor:.3f}")
    assert closer > 2 * farther and e_exact < e_floor


@pytest.mark.parametrize("name", FLOOR_FIXTURES)
def test_floor_draw_against_the_reference_draw(name):
    """Per draw, on every floor sweep of the vvh17 fixtures: the floor rule's b (mean of
    Sigma + f I plus the reference's draw term) is no further from the reference's own SVD b
    (b_ref) than the exact draw is, or f is within the reference's own SVD error
    ||U S U^T - Sigma||_2 on that sweep (the recomputed SVD is bitwise the fixture's)."""
    import scipy.linalg as sl
    n_fwd = n_bwd = 0
    for i, f, Sigma, d, bf, t in _floor_sweeps(name):
        if f == 0.0:
            continue
        b_ref = t["b_ref"][i]
        e_floor = np.linalg.norm(bf - b_ref)
        e_exact = np.linalg.norm(t["b_mean_chol"][i] + t["b_delta"][i] - b_ref)
        if e_floor <= e_exact:
            n_fwd += 1
            continue
        u, sv, _ = sl.svd(Sigma)
        np.testing.assert_array_equal(u @ ((u.T @ d) / sv), t["b_mean_svd"][i])
        ld = np.longdouble
        E = (u.astype(ld) * sv.astype(ld)) @ u.T.astype(ld) - Sigma.astype(ld)
        e_svd = np.linalg.norm(E.astype(np.float64), 2)
        assert f <= e_svd, (i, f, e_svd)
        n_bwd += 1
    print(f"{name}: floor draws closer to b_ref than the exact draw: {n_fwd}; within the "
          f"SVD's own error: {n_bwd}")
